"""The float64 definitions of tests/_loss_reference.py checked without a GPU: against ATen in float64 (binary_cross_entropy_with_logits,
smooth_l1_loss, cross_entropy and their autograd), the CPU oracle (sigmoid_focal_loss, BoxCoder.encode_single, fastrcnn_loss), the
python-loop reduction form of test_third_party_pins.py and torch.optim.Adam; the tolerances against mutants (every subtly wrong copy of a
definition must miss the tolerance at least tenfold ON THE INPUTS THE GPU TEST USES) and against the fp32 emulations they were derived from;
and the branch populations the input builders promise."""
import math

import pytest
import torch
import torch.nn.functional as F

import _loss_reference as L

close = lambda a, b, rtol=1e-12, atol=1e-14: torch.allclose(a, b, rtol=rtol, atol=atol)


# ------------------------------------------------------------------------------------------------------------------ definitions
@pytest.mark.parametrize("T,n_mode", [(257, "tensor"), (257, "zero"), (65537, "tensor")])
def test_ref_rpn_loss_equals_aten_in_float64(T, n_mode):
    d, ref = L.rpn_case(T, n_mode)
    x = d["obj"].double().flatten().requires_grad_(True)
    dl = d["deltas"].double().requires_grad_(True)
    n = max(1, 0 if n_mode == "zero" else d["n_sampled"])
    lo = F.binary_cross_entropy_with_logits(x[d["samp"]], d["labels"].double()[d["samp"]], reduction="sum") / n
    lb = F.smooth_l1_loss(dl[d["pos"]], d["reg_t"].double()[d["pos"]], beta=L.f32(L.BETA9), reduction="sum") / n
    (L.f32(L.G2[0]) * lo + L.f32(L.G2[1]) * lb).backward()
    assert close(ref["losses"], torch.stack([lo, lb]).detach())
    assert close(ref["d_obj"].flatten(), x.grad) and close(ref["d_deltas"], dl.grad)
    assert bool((ref["bce_mag"] >= ref["bce"] * (1 - 1e-9)).all()) and bool((ref["l1_mag"] >= ref["l1"] * (1 - 1e-9)).all())
    assert bool((ref["d_obj_mag"] >= ref["d_obj"].flatten().abs() * (1 - 1e-9)).all())
    assert bool((ref["d_deltas_mag"] >= ref["d_deltas"].abs() * (1 - 1e-9)).all())


def test_ref_rpn_loss_equals_the_python_loop_reduction_form():
    """test_third_party_pins.py's float64 loops (torchvision's rpn.py compute_loss restated) on the T = 255 inputs."""
    d, ref = L.rpn_case(255)
    beta = L.f32(L.BETA9)
    sl1 = lambda v: 0.5 * v * v / beta if abs(v) < beta else abs(v) - 0.5 * beta
    lo = lb = 0.0
    for j in torch.nonzero(d["samp"]).flatten().tolist():
        x, y = float(d["obj"][j, 0]), float(d["labels"][j])
        lo += max(x, 0.0) - x * y + math.log1p(math.exp(-abs(x)))
    for j in torch.nonzero(d["pos"]).flatten().tolist():
        lb += sum(sl1(float(d["deltas"][j, k]) - float(d["reg_t"][j, k])) for k in range(4))
    n = d["n_sampled"]
    assert abs(float(ref["losses"][0]) - lo / n) <= 1e-12 * lo / n and abs(float(ref["losses"][1]) - lb / n) <= 1e-12 * lb / n


@pytest.mark.parametrize("R,K,padding,masked", [(257, 2, "none", False), (300, 91, "none", False), (257, 2, "some", True), (300, 91, "some", True),
                                                (5, 1, "none", False), (257, 2, "all", True)])
def test_ref_fastrcnn_loss_equals_aten_and_the_oracle(R, K, padding, masked):
    from oracle import detection as od
    d, ref = L.frcnn_case(R, K, padding, masked)
    lg = d["logits"].double().requires_grad_(True)
    br = d["breg"].double().requires_grad_(True)
    lab, rt = d["labels"], d["reg_t"].double()
    n = max(1, d["n_valid"]) if masked else R
    valid, fg = lab >= 0, lab > 0
    lc = F.cross_entropy(lg[valid], lab[valid], reduction="sum") / n
    picked = br.reshape(R, K, 4)[torch.nonzero(fg).flatten(), lab[fg]]
    lb = F.smooth_l1_loss(picked, rt[fg], beta=L.f32(L.BETA9), reduction="sum") / n
    (L.f32(L.G2[0]) * lc + L.f32(L.G2[1]) * lb).backward()
    assert close(ref["losses"], torch.stack([lc, lb]).detach())
    assert close(ref["d_logits"], lg.grad) and close(ref["d_breg"], br.grad)
    assert bool((ref["ce_mag"] >= ref["ce"] * (1 - 1e-9)).all()) and bool((ref["d_logits_mag"] >= ref["d_logits"].abs() * (1 - 1e-9)).all())
    assert bool((ref["d_breg_mag"] >= ref["d_breg"].abs() * (1 - 1e-9)).all())
    if padding == "none":          # the oracle has no padding rows; its beta is the double 1/9, 3e-9 from the fp32 value the kernel takes
        oc, ob = od.fastrcnn_loss(d["logits"].double(), d["breg"].double(), [lab], [rt])
        assert close(ref["losses"], torch.stack([oc, ob]), rtol=1e-7)
    if padding == "all":
        assert not bool(ref["losses"].any()) and not bool(ref["d_logits"].any()) and not bool(ref["d_breg"].any())


@pytest.mark.parametrize("ci,pi,variant", [(0, 0, 0), (1, 0, 0), (1, 1, 1), (3, 2, 0), (5, 1, 1), (4, 1, 0)])
def test_ref_retinanet_loss_equals_the_oracle_pieces_composed_per_image(ci, pi, variant):
    """compute_retinanet_loss as the reference states it: per image the focal sum over the counted anchors and the smooth-L1 sum over the
    foreground against BoxCoder.encode_single, each / max(1, nfg), then the mean -- composed here from the oracle's two functions."""
    from oracle import detection as od
    from oracle import retinanet as orn
    d, ref = L.retina_case(ci, pi, variant)
    alpha, gamma, beta, weights = L.RETINA_PARAMS[pi]
    B, A, K = d["cls"].shape
    x = d["cls"].double().requires_grad_(True)
    br = d["breg"].double().requires_grad_(True)
    coder = od.BoxCoder(tuple(L.f32(w) for w in weights))
    lc = lr = 0.0
    for b in range(B):
        m = d["matched"][b]
        fg, counted = m >= 0, m != -2
        t = torch.zeros(A, K, dtype=torch.float64)
        t[fg, d["glab"][b][m[fg]]] = 1.0
        nfg = max(1, int(fg.sum()))
        lc = lc + orn.sigmoid_focal_loss(x[b][counted], t[counted], alpha=L.f32(alpha), gamma=gamma, reduction="sum") / nfg
        tgt = coder.encode_single(d["gt"][b].double()[m[fg]], d["anchors"].double()[fg])
        lr = lr + F.smooth_l1_loss(br[b][fg], tgt, beta=L.f32(beta), reduction="sum") / nfg
        assert float(ref["nfg"][b]) == nfg
    lc, lr = lc / B, lr / B
    (L.f32(L.G2[0]) * lc + L.f32(L.G2[1]) * lr).backward()
    assert close(ref["losses"], torch.stack([lc, lr]).detach(), rtol=1e-11)
    assert close(ref["d_cls"], x.grad, rtol=1e-10, atol=1e-16) and close(ref["d_breg"], br.grad)
    for k in ("focal", "l1", "d_cls", "d_breg"):
        assert bool((ref[k + "_mag"] >= ref[k].abs() * (1 - 1e-9)).all()), k


@pytest.mark.parametrize("alpha,gamma", [p[:2] for p in L.RETINA_PARAMS])
def test_ref_focal_elem_equals_the_oracle_and_its_autograd(alpha, gamma):
    from oracle import retinanet as orn
    d = L.focal_case(257)
    x = d["x"].double().requires_grad_(True)
    want = orn.sigmoid_focal_loss(x, d["t"].double(), alpha=L.f32(alpha), gamma=gamma)
    if gamma == 0:          # autograd of u**0 at u = 0 is 0*inf; with gamma = 0 (and no alpha) the focal loss IS the cross-entropy
        assert alpha < 0
        want = F.binary_cross_entropy_with_logits(x, d["t"].double(), reduction="none")
    want.backward(d["gout"].double())
    assert close(L.ref_focal_elem(d["x"], d["t"], alpha, gamma)["out"], want.detach(), atol=1e-300)
    assert close(L.ref_focal_elem(d["x"], d["t"], alpha, gamma, d["gout"])["out"], x.grad, rtol=1e-10, atol=1e-300)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clip,inv", [(0.5, 1.0 / 8), (0.0, 1.0)])
def test_ref_adam_equals_torch_optim_adam_over_five_steps(wd, clip, inv):
    """Steps 1..5 from zero moments.  torch.optim.Adam runs on float64 parameters with the hyper-parameters' fp32 values; the gradients are
    unscaled and clamped by hand before step().  The one difference left is that the bias corrections reach the kernel rounded to fp32:
    2^-24 relative on each step's update; m and v see it only through weight_decay * p (under 1e-11 here), not at all without decay."""
    h = {k: L.f32(v) for k, v in L.ADAM_HYPER.items()}
    n = 1023
    p0 = L.adam_case(n)["p"].double()
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=L.f32(wd))
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = L.adam_inputs(n, 70 + step)["g"]
        gr = g.double() * L.f32(inv)
        q.grad = gr.clamp(-clip, clip) if clip > 0 else gr
        opt.step()
        r = L.ref_adam(p, g, m, v, h["lr"], h["beta1"], h["beta2"], h["eps"], wd, clip, inv, step)
        p, m, v = r["p"], r["m"], r["v"]
        st = opt.state[q]
        mv_atol = 1e-11 if wd else 1e-15
        assert close(m, st["exp_avg"], atol=mv_atol) and close(v, st["exp_avg_sq"], atol=mv_atol), step
        moved = float((q.detach() - p0).abs().max())
        assert float((p - q.detach()).abs().max()) <= 4 * L.U32 * moved and moved > 0, step


def test_ref_check_finite_is_isfinite():
    nan = float("nan")
    for v, want in ((1.0, False), (L.FLT_MAX, False), (-L.FLT_MAX, False), (3.2e38, False), (1e-45, False), (-0.0, False),
                    (float("inf"), True), (-float("inf"), True), (nan, True), (-nan, True)):
        g = torch.zeros(5)
        g[3] = v
        assert L.ref_check_finite(g) is want, v


# ------------------------------------------------------------------------------------------------------------------ builder conditions
def test_builders_keep_their_promises():
    for T in L.RPN_T + (L.RPN_T_BWD_CAP,):
        L.check_rpn_conditions(L.rpn_case(T)[0])
    for R, K in L.FRCNN_CASES:
        for padding, masked in (("none", False), ("some", True), ("all", True)):
            L.check_frcnn_conditions(L.frcnn_case(R, K, padding, masked)[0])
    for ci in range(len(L.RETINA_CASES)):
        kinds = set()
        for pi in range(len(L.RETINA_PARAMS)):
            for variant in L.retina_variants(ci):
                d = L.retina_case(ci, pi, variant)[0]
                L.check_retina_conditions(d)
                kinds |= set(d["promise"]["kinds"])
        assert L.RETINA_CASES[ci][0] == 1 or kinds == set(L.IMAGE_KINDS), (ci, kinds)      # every batch of 2+ meets all three image kinds
    for n in L.FOCAL_N:
        L.check_focal_conditions(L.focal_case(n))
    assert len(L.beta_edges(L.BETA9)) == 6 == len(set(L.beta_edges(L.BETA9))) and L.beta_edges(L.BETA9)[0] == L.f32(L.BETA9)


# ------------------------------------------------------------------------------------------------------------------ mutants
RED = 10.0          # a mutant must miss the tolerance by at least this factor


def _ratios(bad, ref, keys):
    out = {"losses": L.worst_ratio(bad["losses"], ref["losses"], ref["loss_tol"])}
    for k in keys:
        out[k] = L.worst_ratio(bad[k], ref[k], ref["tol_" + k])
    return out


def _rpn(T, n_mode, mutant):
    d, ref = L.rpn_case(T, n_mode)
    n = 0 if n_mode == "zero" else d["n_sampled"]
    bad = L.ref_rpn_loss(d["obj"], d["deltas"], d["labels"], d["reg_t"], d["pos"], d["samp"], n, L.BETA9, L.G2, mutant=mutant)
    return _ratios(bad, ref, ("d_obj", "d_deltas"))


def _frcnn(R, K, padding, masked, mutant):
    d, ref = L.frcnn_case(R, K, padding, masked)
    bad = L.ref_fastrcnn_loss(d["logits"], d["breg"], d["labels"], d["reg_t"], L.BETA9, d["n_valid"] if masked else None, L.G2, mutant=mutant)
    return _ratios(bad, ref, ("d_logits", "d_breg"))


def _retina(ci, pi, variant, mutant):
    d, ref = L.retina_case(ci, pi, variant)
    alpha, gamma, beta, weights = L.RETINA_PARAMS[pi]
    bad = L.ref_retinanet_loss(d["cls"], d["breg"], d["matched"], d["gt"], d["glab"], d["anchors"], weights, alpha, gamma, beta, L.G2, mutant=mutant)
    return _ratios(bad, ref, ("d_cls", "d_breg"))


ADAM_MUTANT_ARGS = (1e-2, 0.5, 1.0 / 8, 3)          # a point of ADAM_GRID: weight decay, clip, inv_scale, step


def _adam(n, mutant):
    d, h = L.adam_case(n), L.ADAM_HYPER
    args = (d["p"], d["g"], d["m"], d["v"], h["lr"], h["beta1"], h["beta2"], h["eps"]) + ADAM_MUTANT_ARGS
    ref, bad = L.ref_adam(*args), L.ref_adam(*args, mutant=mutant)
    return {k: L.worst_ratio(bad[k], ref[k], ref["tol_" + k]) for k in ("p", "m", "v")}


def _focal_elem(n, alpha, gamma, mutant):
    d = L.focal_case(n)
    out = {}
    for name, gout in (("value", None), ("grad", d["gout"])):
        ref = L.ref_focal_elem(d["x"], d["t"], alpha, gamma, gout)
        out[name] = L.worst_ratio(L.ref_focal_elem(d["x"], d["t"], alpha, gamma, gout, mutant=mutant)["out"], ref["out"], ref["tol"])
    return out


# mutant -> [(what runs it, the outputs that must be red)]; every case is one of the GPU test's own
MUTANT_TABLE = {
    "second_trip_dropped": [(lambda m: _rpn(65537, "tensor", m), ("losses", "d_obj", "d_deltas")),
                            (lambda m: _frcnn(65537, 2, "none", False, m), ("losses", "d_logits", "d_breg")),
                            (lambda m: _retina(3, 0, 0, m), ("losses", "d_cls", "d_breg"))],
    "denominator_unclamped": [(lambda m: _rpn(257, "zero", m), ("losses", "d_obj", "d_deltas")),
                              (lambda m: _frcnn(257, 2, "all", True, m), ("losses",)),
                              (lambda m: _retina(1, 0, 0, m), ("losses", "d_cls"))],
    "ignored_counted_as_background": [(lambda m: _retina(1, 0, 0, m), ("losses", "d_cls")), (lambda m: _retina(4, 1, 0, m), ("losses", "d_cls"))],
    "nfg_shared_across_images": [(lambda m: _retina(1, 0, 0, m), ("losses", "d_cls")), (lambda m: _retina(1, 1, 1, m), ("losses", "d_cls", "d_breg"))],
    "background_rows_regress": [(lambda m: _frcnn(257, 2, "none", False, m), ("losses", "d_breg"))],
    "padding_rows_counted": [(lambda m: _frcnn(257, 2, "some", True, m), ("losses", "d_logits"))],
    "l1_grad_unscaled": [(lambda m: _rpn(257, "tensor", m), ("d_deltas",)), (lambda m: _frcnn(257, 2, "none", False, m), ("d_breg",)),
                         (lambda m: _retina(1, 1, 0, m), ("d_breg",))],
    "linear_branch_offset": [(lambda m: _rpn(257, "tensor", m), ("losses",)), (lambda m: _frcnn(257, 2, "none", False, m), ("losses",)),
                             (lambda m: _retina(1, 1, 0, m), ("losses",))],
    "alpha_swapped": [(lambda m: _retina(1, 0, 0, m), ("losses", "d_cls")), (lambda m: _focal_elem(257, 0.25, 2.0, m), ("value", "grad")),
                      (lambda m: _focal_elem(257, 0.6, 1.5, m), ("value", "grad"))],
    "decay_before_clip": [(lambda m: _adam(4097, m), ("p", "m", "v"))],
    "bc2_not_rooted": [(lambda m: _adam(4097, m), ("p",))],
    "tail_element_dropped": [(lambda m: _adam(n, m), ("p", "m", "v")) for n in (1, 5, 7, 4097)],
}


def test_every_required_mutant_has_a_row():
    assert set(MUTANT_TABLE) == set(L.MUTANTS)


@pytest.mark.parametrize("mutant", L.MUTANTS)
def test_mutants_are_rejected_tenfold_on_the_gpu_tests_inputs(mutant):
    for run, hit in MUTANT_TABLE[mutant]:
        ratios = run(mutant)
        print("loss-reference mutant %s %s" % (mutant, {k: "%.3g" % v for k, v in ratios.items()}))
        for k in hit:
            assert ratios[k] >= RED, (mutant, k, ratios)


def test_unmutated_definitions_have_ratio_zero_against_themselves():
    """The harness itself: a second evaluation of the definition is not red."""
    d, ref = L.rpn_case(257)
    again = L.ref_rpn_loss(d["obj"], d["deltas"], d["labels"], d["reg_t"], d["pos"], d["samp"], d["n_sampled"], L.BETA9, L.G2)
    assert _ratios(again, ref, ("d_obj", "d_deltas")) == {"losses": 0.0, "d_obj": 0.0, "d_deltas": 0.0}


# ------------------------------------------------------------------------------------------------------------------ emulations
def _reproduces(name, worst, const):
    top = max(v[0] for v in worst.values())
    print("loss-reference %s emulation worst %s" % (name, {k: "%.3g at %s" % v for k, v in worst.items()}))
    assert 4 * top <= const <= 4 * top * 1.1, (name, top, const)          # four times the worst case, rounded up by under a tenth


def test_sl1_rtol_is_four_times_the_fp32_emulation():
    _reproduces("smooth-L1", L.derive_sl1_rtol(), L.SL1_RTOL)


def test_ce_rtol_is_four_times_the_fp32_emulation():
    _reproduces("cross-entropy", L.derive_ce_rtol(), L.CE_RTOL)


def test_adam_rtol_is_four_times_the_fp32_emulation():
    _reproduces("Adam", L.derive_adam_rtol(), L.ADAM_RTOL)


def test_adam_emulation_lies_within_a_quarter_of_the_tolerance():
    """The harness of derive_adam_rtol on one case: the fp32 emulation of the kernel's statements is inside ADAM_RTOL / 4 of the float64
    definition, element by element, while the same case's decay_before_clip mutant (test above) is far outside."""
    d, h = L.adam_case(4097), L.ADAM_HYPER
    args = (d["p"], d["g"], d["m"], d["v"], h["lr"], h["beta1"], h["beta2"], h["eps"]) + ADAM_MUTANT_ARGS
    ref = L.ref_adam(*args)
    for k, v in zip(("p", "m", "v"), L.emu_adam_f32(*args)):
        assert L.worst_ratio(torch.from_numpy(v), ref[k], ref["tol_" + k]) <= 0.25, k
