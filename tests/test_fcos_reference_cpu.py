"""The float64 FCOS definitions of tests/_fcos_reference.py checked without a GPU: against torch's group_norm and its autograd, against
the CPU oracle (oracle/fcos.py) on random data, on the matcher's hand-written edge table; the tolerances against mutants (subtly
wrong copies of the definitions must be rejected) and against fp32 emulations of the kernels (the single-pass variance that
groupnorm8_fwd_kernel used to form must fail the rstd tolerance, the centred form it forms now must pass)."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fcos_reference as R


# ------------------------------------------------------------------------------------------------------------------ definitions
def _gn_double(N, HW, C, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {"x": rnd(N, HW, C) * 1.5 + 0.7, "gamma": rnd(C), "beta": rnd(C) * 0.5, "dy": rnd(N, HW, C)}


def _nchw(t):
    return t.permute(0, 2, 1).unsqueeze(-1)          # [N, HW, C] -> [N, C, HW, 1]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("scale,accumulate", [(1.0, False), (1.0 / 256, True)])
def test_groupnorm_definitions_match_torch_group_norm_and_autograd(relu, scale, accumulate):
    N, HW, C = 3, 11, 24
    d = _gn_double(N, HW, C, 1)
    x = d["x"].clone().requires_grad_(True)
    gamma, beta = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    want = F.group_norm(_nchw(x), C // 8, gamma, beta, R.GN_EPS)
    if relu:
        want = torch.relu(want)
    (want * _nchw(d["dy"])).sum().backward()
    st = R.ref_gn_stats(d["x"])
    stat = torch.stack([st["mean"], st["rstd"]], -1)          # float64: the definitions themselves, no fp32 rounding of the statistics
    eps32 = R.f32(R.GN_EPS)
    xg = d["x"].reshape(N, HW, C // 8, 8)
    assert torch.allclose(st["mean"], xg.mean((1, 3)), rtol=0, atol=1e-12)
    assert torch.allclose(st["rstd"], 1 / torch.sqrt(xg.var((1, 3), unbiased=False) + eps32), rtol=1e-12, atol=0)
    y, mag = R.ref_gn_apply(d["x"], d["gamma"], d["beta"], stat, relu)
    assert torch.allclose(_nchw(y), want.detach(), rtol=0, atol=1e-7)          # 1e-5 vs f32(1e-5) in eps
    assert bool((mag >= y.abs() - 1e-12).all())
    b = R.ref_gn_bwd(d["dy"], d["x"], y, d["gamma"], stat, relu)
    assert torch.allclose(b["dx"], x.grad, rtol=0, atol=1e-7)
    assert bool((b["mag"] >= b["dx"].abs() - 1e-12).all())
    prior = (torch.arange(C, dtype=torch.float64) - 3.0, torch.arange(C, dtype=torch.float64) * 0.5)
    p = R.ref_gn_param_grad(d["dy"], d["x"], y if relu else None, stat, scale, accumulate, prior)
    wg, wb = scale * gamma.grad, scale * beta.grad
    if accumulate:
        wg, wb = wg + prior[0], wb + prior[1]
    assert torch.allclose(p["dgamma"], wg, rtol=0, atol=1e-7) and torch.allclose(p["dbeta"], wb, rtol=0, atol=1e-10)


def test_ref_match_equals_the_oracle_on_random_boxes():
    from oracle import fcos as ofc
    me = types.SimpleNamespace(center_sampling_radius=R.RADIUS)
    n_fg = 0
    for seed in range(4):
        d = R.match_random_inputs(None, 5, seed)
        got = R.ref_match(d["anchors"], d["gt"], d["gvalid"], d["first_n"], d["last_start"], R.RADIUS)
        A = d["anchors"].shape[0]
        napl = [d["first_n"], d["last_start"] - d["first_n"], A - d["last_start"]]
        for b in range(2):
            keep = d["gvalid"][b].bool()
            om = ofc.FCOS.match(me, d["anchors"], {"boxes": d["gt"][b][keep]}, napl)
            slot = torch.nonzero(keep).flatten()                                  # the oracle indexes the valid boxes only
            want = torch.where(om >= 0, slot[om.clamp(min=0)], torch.full_like(om, -1))
            assert torch.equal(got[b], want), (seed, b)
            n_fg += int((om >= 0).sum())
    assert n_fg > 100


@pytest.mark.parametrize("K,g3", [(1, (1.0, 1.0, 1.0)), (3, (0.7, 1.3, 2.1))])
def test_ref_fcos_losses_equal_the_oracle_and_its_autograd(K, g3):
    from oracle import fcos as ofc
    d = R.loss_inputs(2, 600, K, 5)
    d["cls"] = d["cls"].clamp(-12, 12)                # the oracle works in fp32: keep it away from saturation (non-edge data)
    d["ctr"] = d["ctr"].clamp(-12, 12)
    ref = R.ref_fcos_losses(d["cls"], d["reg"], d["ctr"], d["matched"], d["gt"], d["glab"], d["anchors"], 0.25, 2.0, g3)
    c, r, t = (v.double().clone().requires_grad_(True) for v in (d["cls"], d["reg"], d["ctr"]))
    head = types.SimpleNamespace(box_coder=ofc.BoxLinearCoder(normalize_by_size=True))
    tg = [{"boxes": d["gt"][b], "labels": d["glab"][b]} for b in range(2)]          # fp32: the oracle casts the predictions to it
    lo = ofc.FCOSHead.compute_loss(head, tg, {"cls_logits": c, "bbox_regression": r, "bbox_ctrness": t[..., None]},
                                   [d["anchors"].double()] * 2, [d["matched"][b] for b in range(2)])
    w = [R.f32(v) for v in g3]                        # the upstream gradients reach the kernel as fp32
    (w[0] * lo["classification"] + w[1] * lo["bbox_regression"] + w[2] * lo["bbox_ctrness"]).backward()
    assert ref["nfg"] == 80.0
    for i, k in enumerate(("classification", "bbox_regression", "bbox_ctrness")):
        assert abs(float(lo[k].detach()) - float(ref["losses"][i])) <= 1e-6 * abs(float(ref["losses"][i])), k      # the oracle's GIoU is fp32
    assert torch.allclose(c.grad, ref["d_cls"], rtol=1e-9, atol=1e-12)
    assert torch.allclose(t.grad, ref["d_ctr"], rtol=1e-9, atol=1e-12)
    assert torch.allclose(r.grad, ref["d_reg"], rtol=1e-4, atol=1e-7) and float(ref["d_reg"].abs().max()) > 0
    for k in ("focal", "giou", "bce", "d_cls", "d_reg", "d_ctr"):
        assert bool((ref[k + "_mag"] >= ref[k].abs() * (1 - 1e-9)).all()), k          # a magnitude bounds its value


@pytest.mark.parametrize("alpha,gamma", [(0.25, 2.0), (0.6, 1.5), (-1.0, 0.0)])
def test_focal_term_equals_the_oracle_for_general_alpha_gamma(alpha, gamma):
    from oracle import retinanet as orn
    d = R.loss_inputs(2, 300, 3, 6)
    x = d["cls"].clamp(-12, 12)
    ref = R.ref_fcos_losses(x, d["reg"], d["ctr"], d["matched"], d["gt"], d["glab"], d["anchors"], alpha, gamma)
    _, lab, _ = R._gather_targets(d["matched"], d["gt"], d["glab"])
    t = (lab[..., None] == torch.arange(3)).double()
    want = orn.sigmoid_focal_loss(x.double(), t, alpha=alpha, gamma=gamma)
    assert torch.allclose(ref["focal"], want, rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------ matcher edges
def test_match_edge_table_gives_the_hand_written_indices():
    for c in R.match_edge_cases():
        got = R.ref_match(c["anchors"], c["gt"], c["gvalid"], c["first_n"], c["last_start"], R.RADIUS)
        for (b, a), want in c["expect"].items():
            assert int(got[b, a]) == want, (c["name"], b, a, int(got[b, a]))
        if c["name"] == "zero_width_and_no_valid":
            assert bool((got[1] == -1).all())


def test_fp32_area_tie_discriminates():
    """float32(1e8 - 1001) == float32(1e8 - 1000): slot 0 wins the tie; with the subtraction in float64 slot 1 (the smaller box) wins."""
    assert np.float32(1e8) - np.float32(1001) == np.float32(1e8) - np.float32(1000)
    c = [c for c in R.match_edge_cases() if c["name"] == "fp32_area_tie"][0]
    args = (c["anchors"], c["gt"], c["gvalid"], c["first_n"], c["last_start"], R.RADIUS)
    assert int(R.ref_match(*args)[0, 0]) == 0
    assert int(R.ref_match(*args, area_dtype=np.float64)[0, 0]) == 1


@pytest.mark.parametrize("mutant", R.MATCH_MUTANTS)
def test_matcher_mutants_are_rejected(mutant):
    caught = []
    for c in R.match_edge_cases():
        args = (c["anchors"], c["gt"], c["gvalid"], c["first_n"], c["last_start"], R.RADIUS)
        if not torch.equal(R.ref_match(*args, mutant=mutant), R.ref_match(*args)):
            caught.append(c["name"])
    assert caught, mutant


# ------------------------------------------------------------------------------------------------------------------ GroupNorm mutants
GN_MUTANT_SHAPES = [(3, 33, 256), (3, 1025, 8)]          # one pixel past one trip of the PL lanes


def _gn_case(N, HW, C, dtype=torch.float16):
    d = R.gn_inputs(N, HW, C, dtype, 11)
    st = R.ref_gn_stats(d["x"])
    d["st"], d["stat"] = st, R.stat_tensor(st)
    y, _ = R.ref_gn_apply(d["x"], d["gamma"], d["beta"], d["stat"], True)
    d["y"] = y.to(dtype)
    return d


def _pixel_weights(kind, n, PL):
    w = torch.ones(n, dtype=torch.float64)
    if kind == "last_dropped":
        w[-1] = 0.0
    else:
        w[PL] = 2.0
    return w


@pytest.mark.parametrize("N,HW,C", GN_MUTANT_SHAPES)
@pytest.mark.parametrize("kind", ["last_dropped", "pixel_PL_twice"])
def test_groupnorm_pixel_mutants_are_rejected(N, HW, C, kind):
    d = _gn_case(N, HW, C)
    PL = R.GB // (C // 8)
    w = _pixel_weights(kind, HW, PL)
    st, bad = d["st"], R.ref_gn_stats(d["x"], _w=w)
    assert R.worst_ratio(bad["mean"], st["mean"], R.mean_rtol(HW, C) * st["absmean"]) > 1
    assert R.worst_ratio(bad["rstd"], st["rstd"], R.RSTD_RTOL * st["rstd"]) > 1
    for relu in (False, True):
        b = R.ref_gn_bwd(d["dy"], d["x"], d["y"], d["gamma"], d["stat"], relu)
        assert R.worst_ratio(R.ref_gn_bwd(d["dy"], d["x"], d["y"], d["gamma"], d["stat"], relu, _w=w)["dx"], b["dx"],
                             R.gn_bwd_tol(b, torch.float16)) > 1
    wf = _pixel_weights(kind, N * HW, R.GB if N * HW > R.GB else PL)          # the parameter gradient strides the flat pixels by the block
    p = R.ref_gn_param_grad(d["dy"], d["x"], d["y"], d["stat"], 1.0, False)
    q = R.ref_gn_param_grad(d["dy"], d["x"], d["y"], d["stat"], 1.0, False, _w=wf)
    assert R.worst_ratio(q["dgamma"], p["dgamma"], p["tol_dgamma"]) > 1 and R.worst_ratio(q["dbeta"], p["dbeta"], p["tol_dbeta"]) > 1


def test_groupnorm_statistics_and_mask_mutants_are_rejected():
    N, HW, C = 3, 33, 256
    d = _gn_case(N, HW, C)
    f16 = torch.float16
    y, mag = R.ref_gn_apply(d["x"], d["gamma"], d["beta"], d["stat"], True)
    neighbour = torch.roll(d["stat"], 1, dims=1)
    assert R.worst_ratio(R.ref_gn_apply(d["x"], d["gamma"], d["beta"], neighbour, True)[0], y, R.elem_tol(y, mag, f16)) > 1
    assert R.worst_ratio(R.ref_gn_apply(d["x"], d["gamma"], d["beta"], torch.roll(d["stat"], 1, dims=0), True)[0], y,
                         R.elem_tol(y, mag, f16)) > 1                                             # another image's statistics
    b = R.ref_gn_bwd(d["dy"], d["x"], d["y"], d["gamma"], d["stat"], True)
    tol = R.gn_bwd_tol(b, f16)
    assert R.worst_ratio(R.ref_gn_bwd(d["dy"], d["x"], d["y"], d["gamma"], neighbour, True)["dx"], b["dx"], tol) > 1
    assert R.worst_ratio(R.ref_gn_bwd(d["dy"], d["x"], d["y"], d["gamma"], d["stat"], False)["dx"], b["dx"], tol) > 1      # mask ignored
    prior = (torch.randn(C, generator=torch.Generator().manual_seed(3)) * 4, torch.randn(C, generator=torch.Generator().manual_seed(4)) * 4)
    p = R.ref_gn_param_grad(d["dy"], d["x"], d["y"], d["stat"], 1.0 / 256, True, prior)

    def rejected(q):
        return R.worst_ratio(q["dgamma"], p["dgamma"], p["tol_dgamma"]) > 1 and R.worst_ratio(q["dbeta"], p["dbeta"], p["tol_dbeta"]) > 1
    assert R.worst_ratio(R.ref_gn_param_grad(d["dy"], d["x"], d["y"], neighbour, 1.0 / 256, True, prior)["dgamma"], p["dgamma"],
                         p["tol_dgamma"]) > 1                                                      # dbeta does not read the statistics
    nxt = ((torch.arange(N * HW) + 1) // HW).clamp(max=N - 1)                                      # n = (i + 1) / HW
    assert R.worst_ratio(R.ref_gn_param_grad(d["dy"], d["x"], d["y"], d["stat"], 1.0 / 256, True, prior, _img=nxt)["dgamma"], p["dgamma"],
                         p["tol_dgamma"]) > 1
    assert rejected(R.ref_gn_param_grad(d["dy"], d["x"], None, d["stat"], 1.0 / 256, True, prior))          # mask ignored
    s = R.f32(1.0 / 256)
    scaled_prior = {k: p[k] - prior[i].double() + s * prior[i].double() for i, k in enumerate(("dgamma", "dbeta"))}
    assert rejected(scaled_prior)                                                                  # scale applied to the prior too


# ------------------------------------------------------------------------------------------------------------------ loss mutants
@pytest.mark.parametrize("mutant", R.LOSS_MUTANTS)
def test_loss_mutants_are_rejected(mutant):
    ci = 4 if mutant == "nfg_unclamped" else 3          # the batch without foreground; K = 3 with all three losses upstream
    B, A, K, alpha, gamma, _, fgd = R.LOSS_CASES[ci]
    g3 = (0.7, 1.3, 2.1)
    d = R.loss_inputs(B, A, K, 100 + ci, fgd)
    args = (d["cls"], d["reg"], d["ctr"], d["matched"], d["gt"], d["glab"], d["anchors"], alpha, gamma, g3)
    ref, bad = R.ref_fcos_losses(*args), R.ref_fcos_losses(*args, mutant=mutant)
    ratios = {"losses": R.worst_ratio(bad["losses"], ref["losses"], ref["loss_tol"])}
    for k in ("d_cls", "d_reg", "d_ctr"):
        ratios[k] = R.worst_ratio(bad[k], ref[k], R.loss_tol(ref[k + "_mag"]))
    hit = {"label_image0": ("losses", "d_cls"), "nfg_per_image": ("losses", "d_cls", "d_reg", "d_ctr"), "nfg_unclamped": ("losses", "d_cls"),
           "giou_tie_one_side": ("d_reg",)}[mutant]
    for k in hit:
        assert ratios[k] > 1, (mutant, k, ratios)


# ------------------------------------------------------------------------------------------------------------------ emulations
def test_rstd_tolerance_is_four_times_the_centred_emulation_and_within_the_format():
    worst = R.derive_rstd_rtol(centred=True)
    print("fcos-reference rstd emulation worst %.3g" % worst)
    assert 4 * worst <= R.RSTD_RTOL <= 2.0 ** -13, worst


def test_loss_tolerance_is_four_times_the_fp32_emulation():
    worst = R.derive_loss_rtol()
    print("fcos-reference loss emulation worst", {k: "%.3g" % v for k, v in worst.items()})
    assert 4 * max(worst.values()) <= R.LOSS_RTOL, worst


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["float16", "float32"])
@pytest.mark.parametrize("N,HW,C", R.GN_CONDITIONING)
def test_single_pass_variance_fails_the_rstd_tolerance_and_the_centred_form_passes(N, HW, C, dtype):
    d, ratio = R.gn_conditioning_inputs(N, HW, C, dtype, 7)
    st = R.ref_gn_stats(d["x"])
    assert float(st["rstd"][ratio == -1]) == 1.0 / math.sqrt(R.f32(R.GN_EPS))          # constant at 100.125: variance 0

    def ratios(centred):
        mean, rstd = R.emu_gn_stats_f32(d["x"], centred=centred)
        rel = (torch.from_numpy(rstd).double() - st["rstd"]).abs() / (R.RSTD_RTOL * st["rstd"])
        mr = R.worst_ratio(torch.from_numpy(mean), st["mean"], R.mean_rtol(HW, C) * st["absmean"])
        return rel, mr
    rel, mr = ratios(True)
    print("fcos-reference centred rstd ratio %.3g mean ratio %.3g" % (float(rel.max()), mr))
    assert float(rel.max()) <= 0.25 and mr <= 1.0
    rel, _ = ratios(False)
    print("fcos-reference single-pass rstd ratio at 256: %.3g, at 64: %.3g, constant group: %.3g"
          % (float(rel[ratio == 256].min()), float(rel[ratio == 64].max()), float(rel[ratio == -1])))
    assert float(rel[ratio == 256].min()) > 1.0          # EVERY group at |mean|/std = 256 is out of tolerance
    assert float(rel[ratio == 64].max()) > 1.0
    if C == 256:                                         # (C = 8: the lone constant group's sums happen to be exact in fp32)
        assert float(rel[ratio == -1]) > 1.0
