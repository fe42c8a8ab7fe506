"""The seven kernels of csrc/fcos.hip (hd_groupnorm8_relu, hd_groupnorm8_relu_bwd, hd_groupnorm8_param_grad and their _f32 twins,
hd_fcos_match, hd_fcos_loss = forward + finish, hd_fcos_loss_bwd) against the float64 definitions of tests/_fcos_reference.py, at the
loop edges of each kernel: GroupNorm's PL = 1024 / (C/8) pixel lanes with no pixel, exactly one trip and one pixel of a second trip,
one channel vector and 128 of them, the parameter gradient's 1 024-pixel stride across image boundaries, the matcher's strict
inequalities and tie rules, the loss forward's 16 384-location trip and the backward's 65 536-location trip.  Tolerances:
_fcos_reference's docstring.  Exact-integer inputs are asserted with torch.equal.

Every test prints `fcos-kernels ratio <kernel> <largest error / tolerance>` (pytest -s shows it)."""
import functools
import math

import pytest
import torch

import _fcos_reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.float32]
_id = lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


def note(kernel, ratio):
    print("fcos-kernels ratio %s %.4g" % (kernel, ratio))
    return ratio


def nhwc(t):
    return t.reshape(t.shape[0], t.shape[1], 1, t.shape[2])          # [N, HW, C] -> the [N, H, W, C] the wrappers take


# ------------------------------------------------------------------------------------------------------------------ GroupNorm forward
def check_forward(dev, d, dtype, relu, HW, C):
    """(a) the returned statistics against the two-pass float64 ones, (b) y against the definition evaluated WITH the returned
    statistics -> the three ratios."""
    from hallucidet_amd import ops
    y, stat = ops.groupnorm8_relu(nhwc(d["x"]).to(dev), d["gamma"].to(dev), d["beta"].to(dev), R.GN_EPS, relu=relu)
    stat = stat.cpu()
    st = R.ref_gn_stats(d["x"])
    r_mean = R.worst_ratio(stat[..., 0], st["mean"], R.mean_rtol(HW, C) * st["absmean"])
    r_rstd = R.worst_ratio(stat[..., 1], st["rstd"], R.RSTD_RTOL * st["rstd"])
    want, mag = R.ref_gn_apply(d["x"], d["gamma"], d["beta"], stat, relu)
    r_y = R.worst_ratio(y.cpu().reshape(d["x"].shape), want, R.elem_tol(want, mag, dtype))
    return r_mean, r_rstd, r_y, stat


@pytest.mark.parametrize("C,hws", R.GN_TABLE, ids=lambda v: str(v) if isinstance(v, int) else None)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_groupnorm_forward(dev, dtype, relu, C, hws):
    worst = [0.0, 0.0, 0.0]
    for HW in hws:
        for N in (1, 3):
            d = R.gn_inputs(N, HW, C, dtype, N * 100000 + HW * 10 + C)
            r = check_forward(dev, d, dtype, relu, HW, C)[:3]
            assert max(r) <= 1.0, (N, HW, C, r)
            worst = [max(a, b) for a, b in zip(worst, r)]
            if relu:
                below = float((R.ref_gn_apply(d["x"], d["gamma"], d["beta"], R.stat_tensor(R.ref_gn_stats(d["x"])), False)[0] < 0).double().mean())
                assert HW * N * C < 4096 or 0.3 < below < 0.7, below          # about half the outputs lie under the ReLU
    for name, r in zip(("mean", "rstd", "y"), worst):
        note("groupnorm8_relu[%s,C=%d].%s" % (_id(dtype), C, name), r)


@pytest.mark.parametrize("N,HW,C", R.GN_CONDITIONING)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_groupnorm_forward_conditioning(dev, dtype, relu, N, HW, C):
    """Groups with |mean| / std in {0, 8, 64, 256}, one constant at 100.125 (rstd = 1/sqrt(f32(eps))), one constant at 0.  A variance
    formed as E[x^2] - mean^2 in fp32 misses RSTD_RTOL by 1e1 .. 1e4 at ratio 256 and by 4e5 on the constant group
    (test_fcos_reference_cpu.py)."""
    d, ratio = R.gn_conditioning_inputs(N, HW, C, dtype, 7)
    r_mean, r_rstd, r_y, stat = check_forward(dev, d, dtype, relu, HW, C)
    st = R.ref_gn_stats(d["x"])
    rel = (stat[..., 1].double() - st["rstd"]).abs() / (R.RSTD_RTOL * st["rstd"])
    for v in R.RATIOS + (-1.0, -2.0):
        note("groupnorm8_relu[%s,C=%d,|mean|/std=%g].rstd" % (_id(dtype), C, v), float(rel[ratio == v].max()))
    note("groupnorm8_relu[%s,C=%d,conditioning].mean" % (_id(dtype), C), r_mean)
    note("groupnorm8_relu[%s,C=%d,conditioning].y" % (_id(dtype), C), r_y)
    assert float(st["rstd"][ratio == -1]) == 1.0 / math.sqrt(R.f32(R.GN_EPS)) and float(st["rstd"][ratio == -2]) == float(st["rstd"][ratio == -1])
    assert float(stat[..., 0][ratio == -1]) == 100.125 and float(stat[..., 0][ratio == -2]) == 0.0
    assert r_mean <= 1.0 and r_rstd <= 1.0 and r_y <= 1.0, (r_mean, r_rstd, r_y)


# ------------------------------------------------------------------------------------------------------------------ GroupNorm data gradient
def bwd_inputs(N, HW, C, dtype, seed):
    """The reference's own statistics (rounded to fp32) and its own forward output (rounded to storage): the kernel is isolated from the
    forward kernel."""
    d = R.gn_inputs(N, HW, C, dtype, seed)
    d["stat"] = R.stat_tensor(R.ref_gn_stats(d["x"]))
    d["y"] = R.ref_gn_apply(d["x"], d["gamma"], d["beta"], d["stat"], True)[0].to(dtype)
    return d


@pytest.mark.parametrize("C,hws", R.GN_TABLE, ids=lambda v: str(v) if isinstance(v, int) else None)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_groupnorm_data_gradient(dev, dtype, relu, C, hws):
    from hallucidet_amd import ops
    worst = 0.0
    for HW in hws:
        for N in (1, 3):
            d = bwd_inputs(N, HW, C, dtype, N * 100000 + HW * 10 + C + 1)
            dx = ops.groupnorm8_relu_bwd(nhwc(d["dy"]).to(dev), nhwc(d["x"]).to(dev), nhwc(d["y"]).to(dev) if relu else None, d["gamma"].to(dev),
                                         d["stat"].to(dev), relu=relu)
            b = R.ref_gn_bwd(d["dy"], d["x"], d["y"], d["gamma"], d["stat"], relu)
            r = R.worst_ratio(dx.cpu().reshape(d["x"].shape), b["dx"], R.gn_bwd_tol(b, dtype))
            assert r <= 1.0, (N, HW, C, r)
            worst = max(worst, r)
    note("groupnorm8_relu_bwd[%s,C=%d]" % (_id(dtype), C), worst)


@pytest.mark.parametrize("N,HW,C", [(3, 32, 256), (1, 128, 8), (3, 8, 1024)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_groupnorm_data_gradient_exact(dev, dtype, N, HW, C):
    """Integer dy and x, integer mean, rstd 0.5, gamma in powers of two, HW*8 a power of two: both group means and every term of dx are
    exact in fp32, so the stored result is the correctly rounded float64 one."""
    from hallucidet_amd import ops
    d = R.gn_integer_inputs(N, HW, C, dtype, HW + C)
    dx = ops.groupnorm8_relu_bwd(nhwc(d["dy"]).to(dev), nhwc(d["x"]).to(dev), None, d["gamma"].to(dev), d["stat"].to(dev), relu=False)
    want = R.ref_gn_bwd(d["dy"], d["x"], None, d["gamma"], d["stat"], False)["dx"]
    assert torch.equal(want.to(dtype).double(), want) or dtype == torch.float16          # fp32 holds it exactly
    assert torch.equal(dx.cpu().reshape(want.shape), want.to(dtype))


# ------------------------------------------------------------------------------------------------------------------ GroupNorm parameter gradient
PARAM_SHAPES = [(1, 1), (1, 1023), (1, 1024), (1, 1025), (3, 341), (3, 683)]      # N*HW = 1, 1023, 1024, 1025, 1023, 2049


def run_param_grad(dev, d, relu, scale, accumulate, prior):
    from hallucidet_amd import ops
    C = d["x"].shape[2]
    if accumulate:
        dg, db = prior[0].clone().to(dev), prior[1].clone().to(dev)
    else:
        dg, db = (torch.full((C,), float("nan"), device=dev) for _ in range(2))
    ops.groupnorm8_param_grad(nhwc(d["dy"]).to(dev), nhwc(d["x"]).to(dev), nhwc(d["y"]).to(dev) if relu else None, d["stat"].to(dev), dg, db, scale,
                              relu=relu, accumulate=accumulate)
    return dg.cpu(), db.cpu()


@pytest.mark.parametrize("C", [8, 256])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_groupnorm_param_grad(dev, dtype, relu, C):
    worst = 0.0
    for N, HW in PARAM_SHAPES:
        d = bwd_inputs(N, HW, C, dtype, N * 100000 + HW * 10 + C + 2)
        g = torch.Generator().manual_seed(HW)
        prior = (torch.randn(C, generator=g) * 3, torch.randn(C, generator=g) * 3)
        for accumulate, scale in ((True, 1.0 / 256), (False, 1.0), (True, 1.0), (False, 1.0 / 256)):
            dg, db = run_param_grad(dev, d, relu, scale, accumulate, prior)
            p = R.ref_gn_param_grad(d["dy"], d["x"], d["y"] if relu else None, d["stat"], scale, accumulate, prior)
            r = max(R.worst_ratio(dg, p["dgamma"], p["tol_dgamma"]), R.worst_ratio(db, p["dbeta"], p["tol_dbeta"]))
            assert r <= 1.0, (N, HW, C, accumulate, scale, r)
            worst = max(worst, r)
    note("groupnorm8_param_grad[%s,C=%d]" % (_id(dtype), C), worst)


@pytest.mark.parametrize("N,HW,C", [(3, 683, 8), (1, 1025, 256), (3, 341, 256)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_groupnorm_param_grad_exact(dev, dtype, N, HW, C):
    """Integer data, integer mean, rstd 0.5, scale 0.5, integer prior: every sum is below 2^24 halves, so any order of additions is exact."""
    d = R.gn_integer_inputs(N, HW, C, dtype, HW + C + 1)
    prior = (torch.arange(C, dtype=torch.float32) - 7.0, 3.0 - torch.arange(C, dtype=torch.float32))
    for relu in (True, False):
        for accumulate in (True, False):
            dg, db = run_param_grad(dev, d, relu, 0.5, accumulate, prior)
            p = R.ref_gn_param_grad(d["dy"], d["x"], d["y"] if relu else None, d["stat"], 0.5, accumulate, prior)
            assert torch.equal(dg.double(), p["dgamma"]) and torch.equal(db.double(), p["dbeta"]), (relu, accumulate)


# ------------------------------------------------------------------------------------------------------------------ matcher
def gpu_match(dev, anchors, gt, gvalid, first_n, last_start, radius=R.RADIUS):
    from hallucidet_amd import _abi
    an, g, gv = anchors.contiguous().float().to(dev), gt.contiguous().float().to(dev), gvalid.contiguous().to(torch.uint8).to(dev)
    B, G, A = g.shape[0], g.shape[1], an.shape[0]
    m = torch.full((B, A), -7, dtype=torch.int64, device=dev)
    _abi.check(_abi.load().hd_fcos_match(_abi.ptr(an), _abi.ptr(g), _abi.ptr(gv), B, A, G, int(first_n), int(last_start), float(radius), _abi.ptr(m),
                                         torch.cuda.current_stream().cuda_stream), "hd_fcos_match")
    return m.cpu()


def test_match_edge_table(dev):
    for c in R.match_edge_cases():
        got = gpu_match(dev, c["anchors"], c["gt"], c["gvalid"], c["first_n"], c["last_start"])
        for (b, a), want in c["expect"].items():
            assert int(got[b, a]) == want, (c["name"], b, a, int(got[b, a]))
        assert torch.equal(got, R.ref_match(c["anchors"], c["gt"], c["gvalid"], c["first_n"], c["last_start"], R.RADIUS)), c["name"]


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("A", [1, 255, 256, 257, None], ids=lambda a: "full" if a is None else str(a))
def test_match_block_edges(dev, A, G):
    """One location, one short of a 256-thread block, exactly one, one more, and the whole three-level pyramid (336 locations)."""
    n_fg = 0
    for seed in range(3):
        d = R.match_random_inputs(A, G, seed * 10 + G)
        got = gpu_match(dev, d["anchors"], d["gt"], d["gvalid"], d["first_n"], d["last_start"])
        assert torch.equal(got, R.ref_match(d["anchors"], d["gt"], d["gvalid"], d["first_n"], d["last_start"], R.RADIUS)), seed
        n_fg += int((got >= 0).sum())
    assert A == 1 or n_fg > 0


def test_match_one_level_pyramid(dev):
    d = R.match_random_inputs(None, 5, 3, levels=((32, 8),))
    assert d["first_n"] == d["anchors"].shape[0] == 64 and d["last_start"] == 0
    got = gpu_match(dev, d["anchors"], d["gt"], d["gvalid"], d["first_n"], d["last_start"])
    assert torch.equal(got, R.ref_match(d["anchors"], d["gt"], d["gvalid"], d["first_n"], d["last_start"], R.RADIUS)) and int((got >= 0).sum()) > 0


# ------------------------------------------------------------------------------------------------------------------ losses
@functools.lru_cache(maxsize=None)
def loss_case(ci):
    """Inputs and float64 reference of LOSS_CASES[ci]: computed once, shared, never modified."""
    B, A, K, alpha, gamma, g3, fgd = R.LOSS_CASES[ci]
    d = R.loss_inputs(B, A, K, 100 + ci, fgd)
    return d, R.ref_fcos_losses(d["cls"], d["reg"], d["ctr"], d["matched"], d["gt"], d["glab"], d["anchors"], alpha, gamma, g3)


@pytest.mark.parametrize("ci", range(len(R.LOSS_CASES)), ids=lambda i: "B%dxA%d-K%d-a%g-g%g-%s%s" % (R.LOSS_CASES[i][:5] + (
    "".join("%g," % v for v in R.LOSS_CASES[i][5]), "" if R.LOSS_CASES[i][6] else "-nofg")))
def test_fcos_losses_and_gradients(dev, ci):
    from hallucidet_amd.models import fcos as F_
    B, A, K, alpha, gamma, g3, fgd = R.LOSS_CASES[ci]
    d, ref = loss_case(ci)
    flat_fg = torch.nonzero(d["matched"].flatten() >= 0).flatten()
    if fgd:
        assert int((d["matched"][0] >= 0).sum()) == 40 == int((d["matched"][1] >= 0).sum()) and ref["nfg"] == 80.0
        assert B * A <= 16384 or int(flat_fg.max()) >= 16384              # foreground in the forward's second trip
        assert B * A <= 65536 or int(flat_fg.max()) >= 65536              # ... and in the backward's
        assert not torch.equal(d["gt"][0], d["gt"][1]) and (K == 1 or not torch.equal(d["glab"][0], d["glab"][1]))
    else:
        assert flat_fg.numel() == 0 and ref["nfg"] == 1.0
    for v in (30.0, -30.0, 100.0, -100.0):
        assert bool((d["cls"] == v).any())
    cg, rg, tg = (d[k].to(dev).requires_grad_(True) for k in ("cls", "reg", "ctr"))
    got = F_.fcos_loss_batched(d["anchors"].to(dev), d["gt"].to(dev), d["glab"].to(dev),
                               {"cls_logits": cg, "bbox_regression": rg, "bbox_ctrness": tg[..., None]}, d["matched"].to(dev), alpha=alpha, gamma=gamma)
    keys = ("classification", "bbox_regression", "bbox_ctrness")
    (g3[0] * got[keys[0]] + g3[1] * got[keys[1]] + g3[2] * got[keys[2]]).backward()
    losses = torch.stack([got[k].detach() for k in keys]).cpu()
    r_val = note("fcos_loss[%d].values" % ci, R.worst_ratio(losses, ref["losses"], ref["loss_tol"]))
    r_cls = note("fcos_loss_bwd[%d].d_cls_logits" % ci, R.worst_ratio(cg.grad.cpu(), ref["d_cls"], R.loss_tol(ref["d_cls_mag"])))
    r_reg = note("fcos_loss_bwd[%d].d_bbox_regression" % ci, R.worst_ratio(rg.grad.cpu(), ref["d_reg"], R.loss_tol(ref["d_reg_mag"])))
    r_ctr = note("fcos_loss_bwd[%d].d_bbox_ctrness" % ci, R.worst_ratio(tg.grad.cpu(), ref["d_ctr"], R.loss_tol(ref["d_ctr_mag"])))
    assert max(r_val, r_cls, r_reg, r_ctr) <= 1.0, (r_val, r_cls, r_reg, r_ctr)
    if not fgd:          # no foreground: the denominator is clamped to 1, the box and centre-ness branches are exactly zero, the focal one is not
        assert float(losses[0]) > 0 and float(losses[1]) == 0.0 and float(losses[2]) == 0.0
        assert not bool(rg.grad.any()) and not bool(tg.grad.any()) and float(cg.grad.abs().max()) > 0
    if g3[1] == 0.0:
        assert not bool(rg.grad.any())
    elif fgd:
        assert float(rg.grad.abs().max()) > 0
