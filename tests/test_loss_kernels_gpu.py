"""The kernels of csrc/losses.hip (hd_rpn_loss, hd_fastrcnn_loss, hd_fastrcnn_loss_masked, hd_retinanet_loss, hd_sigmoid_focal_loss and their
backward entry points) and csrc/optim.hip (hd_adam_step, hd_check_finite) against the float64 definitions of tests/_loss_reference.py,
called through the wrappers the product uses, at the loop edges of each kernel: one thread, the 256-thread block edge, exactly one trip of
the fixed forward grids (65 536 anchors / rows, 8 192 anchors per image) and one element more, the backward grids' caps (524 288 elements,
65 536 anchors per image), Adam's 4 194 304-element trip and its three scalar-tail lengths, check_finite's wave and trip edges.  Inputs carry
smooth-L1 differences at +-beta and its fp32 neighbours, logits where expf overflows and the sigmoid saturates, images without
foreground and with nothing counted, padding rows, K = 1 and K = 91.  Tolerances: _loss_reference's docstring; no element is left out.

Every test prints `loss-kernels ratio <kernel> <largest error / tolerance>` (pytest -s shows it)."""
import types

import pytest
import torch

import _loss_reference as L

pytestmark = pytest.mark.gpu


def note(kernel, ratio):
    print("loss-kernels ratio %s %.4g" % (kernel, ratio))
    return ratio


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ RPN
def run_rpn(dev, d, n_sampled):
    import hallucidet_amd.models.detection as D
    obj, dl = d["obj"].to(dev).requires_grad_(True), d["deltas"].to(dev).requires_grad_(True)
    st = dict(labels=d["labels"].to(dev), reg_t=d["reg_t"].to(dev), pos_f=d["pos"].to(dev), samp_f=d["samp"].to(dev), n_sampled=n_sampled)
    lo, lb = D.rpn_loss_from_samples(st, obj, dl)
    go, gd = torch.autograd.grad(L.G2[0] * lo + L.G2[1] * lb, (obj, dl))
    return torch.stack([lo.detach(), lb.detach()]).cpu(), go.cpu(), gd.cpu()


def rpn_ratios(name, got, ref):
    return (note(name + ".values", L.worst_ratio(got[0], ref["losses"], ref["loss_tol"])),
            note(name + ".d_objectness", L.worst_ratio(got[1], ref["d_obj"], ref["tol_d_obj"])),
            note(name + ".d_deltas", L.worst_ratio(got[2], ref["d_deltas"], ref["tol_d_deltas"])))


@pytest.mark.parametrize("T", L.RPN_T + (L.RPN_T_BWD_CAP,))
def test_rpn_loss_and_gradients(dev, T):
    d, ref = L.rpn_case(T)
    L.check_rpn_conditions(d)
    n = d["n_sampled"]
    got = run_rpn(dev, d, torch.tensor(n, dtype=torch.int64, device=dev))
    assert max(rpn_ratios("rpn_loss[T=%d]" % T, got, ref)) <= 1.0
    assert same(got, run_rpn(dev, d, n))                                                          # host int == device int64
    assert same(got, run_rpn(dev, d, torch.tensor(n, dtype=torch.int64, device=dev)))             # two runs are bit-identical
    assert not bool(got[1].flatten()[~d["samp"]].any()) and not bool(got[2][~d["pos"]].any())     # exact zeros outside samp / pos
    assert float(got[1].abs().max()) > 0 and float(got[2].abs().max()) > 0
    zero = run_rpn(dev, d, 0)                                                                     # divisor clamped to 1
    assert max(rpn_ratios("rpn_loss[T=%d,n_sampled=0]" % T, zero, L.rpn_case(T, "zero")[1])) <= 1.0
    assert same(zero, run_rpn(dev, d, torch.tensor(0, dtype=torch.int64, device=dev)))


# ------------------------------------------------------------------------------------------------------------------ Fast R-CNN
def run_frcnn(dev, d, masked):
    import hallucidet_amd.models.detection as D
    lg, br = d["logits"].to(dev).requires_grad_(True), d["breg"].to(dev).requires_grad_(True)
    nv = torch.tensor(d["n_valid"], dtype=torch.int64, device=dev) if masked else None
    lc, lb = D.fastrcnn_loss_flat(lg, br, d["labels"].to(dev), d["reg_t"].to(dev), nv)
    g1, g2 = torch.autograd.grad(L.G2[0] * lc + L.G2[1] * lb, (lg, br))
    return torch.stack([lc.detach(), lb.detach()]).cpu(), g1.cpu(), g2.cpu()


def frcnn_ratios(name, got, ref):
    return (note(name + ".values", L.worst_ratio(got[0], ref["losses"], ref["loss_tol"])),
            note(name + ".d_logits", L.worst_ratio(got[1], ref["d_logits"], ref["tol_d_logits"])),
            note(name + ".d_box_regression", L.worst_ratio(got[2], ref["d_breg"], ref["tol_d_breg"])))


@pytest.mark.parametrize("R,K", L.FRCNN_CASES)
def test_fastrcnn_loss_and_gradients(dev, R, K):
    d, ref = L.frcnn_case(R, K)
    L.check_frcnn_conditions(d)
    got = run_frcnn(dev, d, False)
    assert max(frcnn_ratios("fastrcnn_loss[R=%d,K=%d]" % (R, K), got, ref)) <= 1.0
    assert same(got, run_frcnn(dev, d, False))
    assert d["n_valid"] == R and same(got, run_frcnn(dev, d, True))          # n_valid == R, no padding: the masked entry is the unmasked one
    assert K == 1 or float(got[2].abs().max()) > 0
    assert K > 1 or (float(got[0][0]) == 0.0 and float(got[0][1]) == 0.0 and not bool(got[1].any()) and not bool(got[2].any()))


@pytest.mark.parametrize("R,K", L.FRCNN_CASES)
def test_fastrcnn_loss_masked(dev, R, K):
    d, ref = L.frcnn_case(R, K, "some", True)
    L.check_frcnn_conditions(d)
    assert R < 257 or 0 < d["n_valid"] < R
    got = run_frcnn(dev, d, True)
    assert max(frcnn_ratios("fastrcnn_loss_masked[R=%d,K=%d]" % (R, K), got, ref)) <= 1.0
    pad = d["labels"] < 0
    assert not bool(got[1][pad].any()) and not bool(got[2][pad].any())        # padding rows: exactly zero gradient
    d0, ref0 = L.frcnn_case(R, K, "all", True)                                # every row padding, n_valid = 0
    L.check_frcnn_conditions(d0)
    got0 = run_frcnn(dev, d0, True)
    assert d0["n_valid"] == 0 and not bool(got0[0].any()) and not bool(got0[1].any()) and not bool(got0[2].any())
    assert max(frcnn_ratios("fastrcnn_loss_masked[R=%d,K=%d,all padding]" % (R, K), got0, ref0)) == 0.0


# ------------------------------------------------------------------------------------------------------------------ RetinaNet
def run_retina(dev, d, alpha, gamma, beta, gt=None, glab=None):
    from hallucidet_amd.models import retinanet as R
    model = types.SimpleNamespace(box_coder=types.SimpleNamespace(weights=d["weights"]))
    cls, breg = d["cls"].to(dev).requires_grad_(True), d["breg"].to(dev).requires_grad_(True)
    gt, glab = (d["gt"] if gt is None else gt), (d["glab"] if glab is None else glab)
    out = R.retinanet_loss_batched(model, d["anchors"].to(dev), gt.to(dev), glab.to(dev), None, cls, breg, matched=d["matched"].to(dev), alpha=alpha,
                                   gamma=gamma, beta=beta)
    lc, lr = out["classification"], out["bbox_regression"]
    g1, g2 = torch.autograd.grad(L.G2[0] * lc + L.G2[1] * lr, (cls, breg))
    return torch.stack([lc.detach(), lr.detach()]).cpu(), g1.cpu(), g2.cpu()


def retina_ratios(name, got, ref):
    return (note(name + ".values", L.worst_ratio(got[0], ref["losses"], ref["loss_tol"])),
            note(name + ".d_cls_logits", L.worst_ratio(got[1], ref["d_cls"], ref["tol_d_cls"])),
            note(name + ".d_bbox_regression", L.worst_ratio(got[2], ref["d_breg"], ref["tol_d_breg"])))


@pytest.mark.parametrize("pi", range(len(L.RETINA_PARAMS)), ids=lambda i: "a%g-g%g-b%.3g" % L.RETINA_PARAMS[i][:3])
@pytest.mark.parametrize("ci", range(len(L.RETINA_CASES)), ids=lambda i: "B%d-A%d-K%d-G%d" % L.RETINA_CASES[i])
def test_retinanet_loss_and_gradients(dev, ci, pi):
    B, A, K, G = L.RETINA_CASES[ci]
    alpha, gamma, beta, weights = L.RETINA_PARAMS[pi]
    for variant in L.retina_variants(ci):
        d, ref = L.retina_case(ci, pi, variant)
        L.check_retina_conditions(d)
        kinds = d["promise"]["kinds"]
        got = run_retina(dev, d, alpha, gamma, beta)
        name = "retinanet_loss[%s,%s,a=%g,g=%g,b=%.3g]" % ("x".join(map(str, (B, A, K, G))), "+".join(kinds), alpha, gamma, beta)
        assert max(retina_ratios(name, got, ref)) <= 1.0
        assert same(got, run_retina(dev, d, alpha, gamma, beta))                                  # two runs are bit-identical
        m = d["matched"]
        assert not bool(got[1][m == -2].any()) and not bool(got[2][m < 0].any())                  # exact zeros: ignored anchors, off foreground
        for b, kind in enumerate(kinds):
            if kind == "mixed":          # anchor 0, component 0 sits at +beta: its gradient is g_reg / (nfg_b * B) and nothing else
                nfg = L.f32(L.G2[1]) / (B * float(got[2][b, 0, 0]))
                assert abs(nfg - float(ref["nfg"][b])) <= 4 * L.U32 * float(ref["nfg"][b]), (b, nfg, float(ref["nfg"][b]))
                assert float(got[1][b].abs().max()) > 0
            elif kind == "nofg":         # nothing to regress; the classification gradient is divided by the clamped 1
                assert float(ref["nfg"][b]) == 1.0 and not bool(got[2][b].any()) and float(got[1][b].abs().max()) > 0
            else:
                assert not bool(got[1][b].any()) and not bool(got[2][b].any())


@pytest.mark.parametrize("pi", range(len(L.RETINA_PARAMS)), ids=lambda i: "a%g-g%g-b%.3g" % L.RETINA_PARAMS[i][:3])
def test_retinanet_loss_without_any_ground_truth_takes_the_dummy_row(dev, pi):
    """gt.shape[1] == 0: retinanet_loss_batched substitutes one never-matched row; the losses are those of the same batch with G = 1."""
    alpha, gamma, beta, weights = L.RETINA_PARAMS[pi]
    d = L.retina_inputs(2, 300, 2, 1, 3900 + pi, ("nofg", "ignored"), beta, weights)
    L.check_retina_conditions(d)
    ref = L.ref_retinanet_loss(d["cls"], d["breg"], d["matched"], d["gt"], d["glab"], d["anchors"], weights, alpha, gamma, beta, L.G2)
    got = run_retina(dev, d, alpha, gamma, beta, gt=torch.zeros(2, 0, 4), glab=torch.zeros(2, 0, dtype=torch.int64))
    assert max(retina_ratios("retinanet_loss[no ground truth,a=%g,g=%g]" % (alpha, gamma), got, ref)) <= 1.0
    assert float(got[0][0]) > 0 and float(got[0][1]) == 0.0 and not bool(got[2].any()) and not bool(got[1][1].any())


# ------------------------------------------------------------------------------------------------------------------ element-wise focal
@pytest.mark.parametrize("alpha,gamma", [p[:2] for p in L.RETINA_PARAMS])
@pytest.mark.parametrize("n", L.FOCAL_N)
def test_sigmoid_focal_loss_elementwise(dev, n, alpha, gamma):
    from hallucidet_amd.utils import eval_forward_retinanet as G
    d = L.focal_case(n)
    L.check_focal_conditions(d)
    x = d["x"].to(dev).requires_grad_(True)
    out = G.sigmoid_focal_loss(x, d["t"].to(dev), alpha=alpha, gamma=gamma, reduction="none")
    out.backward(d["gout"].to(dev))
    ref_v, ref_g = L.ref_focal_elem(d["x"], d["t"], alpha, gamma), L.ref_focal_elem(d["x"], d["t"], alpha, gamma, d["gout"])
    r_v = note("sigmoid_focal_loss[n=%d,a=%g,g=%g].value" % (n, alpha, gamma), L.worst_ratio(out.detach().cpu(), ref_v["out"], ref_v["tol"]))
    r_g = note("sigmoid_focal_loss[n=%d,a=%g,g=%g].grad" % (n, alpha, gamma), L.worst_ratio(x.grad.cpu(), ref_g["out"], ref_g["tol"]))
    assert max(r_v, r_g) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ Adam
def run_adam(dev, d, wd, clip, inv, step, found):
    from hallucidet_amd import ops
    P, G, M, V = (d[k].clone().to(dev) for k in ("p", "g", "m", "v"))
    h = L.ADAM_HYPER
    ops.adam_step(P, G, M, V, lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], weight_decay=wd, clip_value=clip, inv_scale=inv, step=step,
                  found_inf=found)
    return P.cpu(), M.cpu(), V.cpu()


def adam_ref(d, wd, clip, inv, step):
    h = L.ADAM_HYPER
    return L.ref_adam(d["p"], d["g"], d["m"], d["v"], h["lr"], h["beta1"], h["beta2"], h["eps"], wd, clip, inv, step)


@pytest.mark.parametrize("n", L.ADAM_N)
def test_adam_step(dev, n):
    """Every point of weight_decay x clip_value x inv_scale x step (n = 4 194 309, one past the 4 096-block trip plus a 5-element remainder:
    the grid's two opposite corners), found_inf alternating between absent and a zero flag."""
    d = L.adam_case(n)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, (wd, clip, inv, step) in enumerate(L.adam_grid(n)):
        found = torch.zeros(1, device=dev) if i % 2 else None
        got = run_adam(dev, d, wd, clip, inv, step, found)
        ref = adam_ref(d, wd, clip, inv, step)
        for k, v in zip(("p", "m", "v"), got):
            r = L.worst_ratio(v, ref[k], ref["tol_" + k])
            assert r <= 1.0, (n, wd, clip, inv, step, k, r)
            worst[k] = max(worst[k], r)
            if n > L.ADAM_TRIP:          # the elements past the trip: a vector of four in the second trip, then the one-element scalar tail
                tail = note("adam_step[n=%d,wd=%g,clip=%g,step=%d].%s[-5:]" % (n, wd, clip, step, k), L.worst_ratio(v[-5:], ref[k][-5:], ref["tol_" + k][-5:]))
                assert tail <= 1.0 and not torch.equal(v[-5:], d[k][-5:])
        assert found is None or float(found) == 0.0
    for k, r in worst.items():
        note("adam_step[n=%d].%s" % (n, k), r)


@pytest.mark.parametrize("n", [1, 7, 4097])
def test_adam_step_skips_on_the_flag_and_rests_on_zero_gradients(dev, n):
    d = L.adam_case(n)
    flag = torch.ones(1, device=dev)
    got = run_adam(dev, d, 1e-2, 0.5, 1.0 / 8, 3, flag)
    assert torch.equal(got[0], d["p"]) and torch.equal(got[1], d["m"]) and torch.equal(got[2], d["v"]) and float(flag) == 1.0
    z = {"p": d["p"], "g": torch.zeros(n), "m": torch.zeros(n), "v": torch.zeros(n)}
    for clip in (0.0, 0.5):
        got = run_adam(dev, z, 0.0, clip, 1.0, 1, None)          # g = 0, m = v = 0, no decay: 0 / (0 + eps) = 0, p does not move
        assert torch.equal(got[0], d["p"]) and not bool(got[1].any()) and not bool(got[2].any())


def test_adam_step_refuses_a_misaligned_view(dev):
    """A view offset by one float fails hd_adam_step's 16-byte alignment check on the host: an exception, nothing is launched."""
    from hallucidet_amd import _abi, ops
    base = [torch.zeros(12, device=dev) for _ in range(4)]
    h = L.ADAM_HYPER
    kw = dict(lr=h["lr"], beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], weight_decay=0.0, clip_value=0.0, inv_scale=1.0, step=1)
    for which in range(4):
        args = [t[1:9] if i == which else t[:8] for i, t in enumerate(base)]
        assert args[which].data_ptr() % 16 == 4
        with pytest.raises(_abi.HipCallError):
            ops.adam_step(*args, **kw)
    assert not any(bool(t.any()) for t in base)


# ------------------------------------------------------------------------------------------------------------------ check_finite
def _bits(pattern):
    return torch.tensor([pattern - (1 << 32) if pattern >= (1 << 31) else pattern], dtype=torch.int32).view(torch.float32)


BAD = {"+inf": _bits(0x7F800000), "-inf": _bits(0xFF800000), "+nan": _bits(0x7FC00000), "-nan": _bits(0xFFC00000)}


@pytest.mark.parametrize("n", L.FINITE_N)
def test_check_finite_reports_every_non_finite_value_at_every_edge(dev, n):
    """One bad value at the first, a middle and the last index (the last partial wave, the element past the 524 288-element trip)."""
    from hallucidet_amd import ops
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dev)
    flag = torch.zeros(1, device=dev)
    ops.check_finite(g, flag)
    assert float(flag) == 0.0
    for name, bad in BAD.items():
        assert L.ref_check_finite(bad) and (torch.isnan(bad).item() == ("nan" in name)) and (torch.signbit(bad).item() == (name[0] == "-"))
        for idx in sorted({0, n // 2, n - 1}):
            keep = g[idx].clone()
            g[idx] = bad.to(dev)[0]
            assert L.ref_check_finite(g)
            flag.zero_()
            ops.check_finite(g, flag)
            assert float(flag) == 1.0, (n, name, idx)
            g[idx] = keep
    flag.zero_()
    ops.check_finite(g, flag)
    assert float(flag) == 0.0 and not L.ref_check_finite(g)


@pytest.mark.parametrize("n", L.FINITE_N)
def test_check_finite_follows_isfinite_on_large_finite_values(dev, n):
    """+-FLT_MAX, +-3.2e38, denormals and -0.0 are finite: the flag stays 0 (torch.isfinite, GradScaler's rule); a flag that is already 1
    stays 1 on clean data, the kernel only ever sets it."""
    from hallucidet_amd import ops
    special = torch.tensor([L.FLT_MAX, -L.FLT_MAX, 3.2e38, -3.2e38, 1e-45, -1e-45, 1.1e-38, -0.0], dtype=torch.float32)
    g = special[torch.arange(n) % special.numel()].to(dev)          # the first and the last index carry one of them at every n
    assert not L.ref_check_finite(g) and float(g.abs().max()) == L.FLT_MAX
    flag = torch.zeros(1, device=dev)
    ops.check_finite(g, flag)
    assert float(flag) == 0.0, n
    flag.fill_(1.0)
    ops.check_finite(g, flag)
    assert float(flag) == 1.0
