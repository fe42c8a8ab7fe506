"""The BatchNorm kernel chain of csrc/elementwise.hip (hd_bn_finalize, hd_bn_eval_scale_shift, hd_bn_apply, hd_bn_bwd_reduce,
hd_bn_bwd_apply = coefficient launch + apply launch) and the reductions beside it (hd_colsum, hd_rowsum, hd_channel_sum_f16) against
the float64 definitions of tests/_bn_reference.py, at the loop edges of each kernel: the unrolled r + 192 < rows loop and its
stride-64 tail, the 4096 / 2048-block grid caps, one channel vector and 256 of them, blocks shorter than one 4-pixel trip, empty
blocks.  Tolerances: _bn_reference's docstring.  Exact-integer inputs are asserted with torch.equal.

Every test prints `bn-chain ratio <kernel> <largest error / tolerance>` (pytest -s shows it)."""
import math

import pytest
import torch

import _bn_reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.float32]
_id = lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


def note(kernel, ratio):
    print("bn-chain ratio %s %.4g" % (kernel, ratio))
    return ratio


def to_dev(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def randint(seed, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed))


def scalar_ok(got, want, what):
    r = note(what, R.worst_ratio(got, want, R.SCALAR_RTOL * want.abs()))
    assert r <= 1.0, (what, r)


def sum_ok(got, want, mag, what):
    r = note(what, R.worst_ratio(got, want, R.SCALAR_RTOL * mag))
    assert r <= 1.0, (what, r)


# ------------------------------------------------------------------------------------------------------------------ colsum / rowsum
COLSUM_CASES = [(r, 65) for r in (1, 4, 5, 32, 33, 47, 512, 513, 1000)] + [(r, w) for r in (33, 513) for w in (1, 63, 64, 65, 130)]


@pytest.mark.parametrize("rows,W", sorted(set(COLSUM_CASES)))
def test_colsum(dev, rows, W):
    from hallucidet_amd import ops
    xi = randint(rows * 1000 + W, -1000, 1000, rows, W).float()
    assert torch.equal(ops.colsum(xi.to(dev)).cpu().double(), xi.double().sum(0)), "integer data"
    xr = rand(rows * 1000 + W + 1, rows, W) * 3 + 0.5
    r = note("colsum", R.worst_ratio(ops.colsum(xr.to(dev)), xr.double().sum(0), R.COLSUM_RTOL * xr.double().abs().sum(0)))
    assert r <= 1.0, r


@pytest.mark.parametrize("out_rows", [1, 7, 50])
def test_rowsum_each_output_row_is_its_own_slice(dev, out_rows):
    from hallucidet_amd import ops
    rows, W = 50, 65
    per = -(-rows // out_rows)
    for kind, x in (("integer", randint(out_rows, -1000, 1000, rows, W).float()), ("random", rand(out_rows + 100, rows, W) * 3 + 0.5)):
        got = ops.rowsum(x.to(dev), out_rows).cpu()
        for o in range(out_rows):
            sl = x[o * per:min(rows, (o + 1) * per)].double()
            if kind == "integer":
                assert torch.equal(got[o].double(), sl.sum(0)), (kind, o)
            else:
                r = note("rowsum", R.worst_ratio(got[o], sl.sum(0), R.COLSUM_RTOL * sl.abs().sum(0)))
                assert r <= 1.0, (kind, o, r)


# ------------------------------------------------------------------------------------------------------------------ channel_sum
# shapes (storage, C, npix, rows) whose longest fp32 addition chain needs the worst-case bound instead of 1e-6 (test_channel_sum)
CHANNEL_SUM_WORST_CASE = {(torch.float32, 2048, 1000, 1)}


@pytest.mark.parametrize("C", [8, 16, 64, 256, 2048])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_channel_sum(dev, dtype, C):
    """Integer data: exact.  Random data: 1e-6 * sum|x|, except (float32, C 2048, 1000 pixels, 1 row): there plan = 1, so ONE lane adds
    all 1000 pixels of its channel in a serial fp32 chain, and fp32-stored values fill the whole mantissa (f16-stored ones leave 13 bits
    free, so most of their additions are exact: the same shape measures 3.0e-7).  Measured on the GPU 1.52e-6 * sum|x|; a CPU emulation
    of the kernel's lane order in fp32 gives the same 1.52e-6; its exact-integer twin passes.  That shape alone takes the worst-case
    bound (L + 8) * u32 * sum|x| with L = ceil(ceil(npix / rows) / plan) + plan = 1001 additions in the longest chain (6.0e-5)."""
    from hallucidet_amd import ops
    plan = 256 // (C // 8)
    worst = worst_wc = 0.0
    for npix in sorted({n for n in (1, plan - 1, plan, plan + 1, 1000) if n >= 1}):
        xi = R.integer_inputs(npix, C, dtype, npix + C)["y"]
        xr = R.random_inputs(npix, C, dtype, npix + C + 1)["y"]
        xi_d, xr_d = xi.to(dev), xr.to(dev)
        for rows in (1, 3, 64):
            assert torch.equal(ops.channel_sum(xi_d, rows=rows).cpu().double(), xi.double().sum(0)), ("integer", npix, rows)
            rtol = R.REDUCE_RTOL
            if (dtype, C, npix, rows) in CHANNEL_SUM_WORST_CASE:
                per = -(-npix // rows)                              # pixels per block; each lane adds ceil(per / plan) of them,
                rtol = (-(-per // plan) + plan + 8) * R.U32         # then one thread adds the plan lanes
            r = R.worst_ratio(ops.channel_sum(xr_d, rows=rows), xr.double().sum(0), rtol * xr.double().abs().sum(0))
            assert r <= 1.0, ("random", npix, rows, r)
            if rtol == R.REDUCE_RTOL:
                worst = max(worst, r)
            else:
                worst_wc = max(worst_wc, r)
    note("channel_sum[%s]" % _id(dtype), worst)
    if worst_wc:
        note("channel_sum[%s,worst-case-bound]" % _id(dtype), worst_wc)


# ------------------------------------------------------------------------------------------------------------------ bn_finalize
def finalize_data(rows, C, seed):
    """A real f16 activation tensor whose per-channel |mean| ~ std (the variance is then no ill-conditioned difference), cut into `rows`
    slices; affine parameters and running statistics of mixed sign / size."""
    npix = rows + max(3, rows // 7)
    mu = torch.where(rand(seed, C) < 0, -1.0, 1.0) * (0.75 + 0.5 * torch.rand(C, generator=torch.Generator().manual_seed(seed + 1)))
    y = (rand(seed + 2, npix, C) + mu).half()
    return {"y": y, "npix": npix, "part": R.sliced_stat_rows(y, rows), "gamma": rand(seed + 3, C) + 0.25, "beta": rand(seed + 4, C),
            "rm": rand(seed + 5, C), "rv": torch.rand(C, generator=torch.Generator().manual_seed(seed + 6)) + 0.5}


def check_finalize(dev, part, count, gamma, beta, rm, rv, momentum, eps, what):
    from hallucidet_amd import ops
    d = lambda t: None if t is None else t.clone().to(dev)
    rm_d, rv_d = d(rm), d(rv)
    mean, invstd, scale, shift = ops.bn_finalize(part.to(dev), count, d(gamma), d(beta), rm_d, rv_d, momentum, eps)
    f = R.ref_finalize(part, count, gamma, beta, rm, rv, momentum, eps)
    scalar_ok(mean, f["mean"], what + ".mean")
    scalar_ok(invstd, f["invstd"], what + ".invstd")
    scalar_ok(scale, f["scale"], what + ".scale")
    sum_ok(shift, f["shift"], f["shift_mag"], what + ".shift")
    if rm is not None:
        sum_ok(rm_d, f["running_mean"], f["running_mean_mag"], what + ".running_mean")
        sum_ok(rv_d, f["running_var"], f["running_var_mag"], what + ".running_var")
    return f, (mean, invstd, scale, shift)


FINALIZE_CASES = [(r, c) for r in (1, 2, 63, 64, 65, 192, 193, 256, 257, 449, 1000, 4097) for c in (6, 64)] + [(193, 2048)]


@pytest.mark.parametrize("rows,C", FINALIZE_CASES)
def test_bn_finalize_rows(dev, rows, C):
    """The partial rows are slices of a real f16 tensor, summed in float64 and rounded to fp32; the reference takes those fp32 rows.
    rows = 4097 goes through ops.bn_finalize's rowsum(part, 1024) pre-reduction, which rounds 1024 intermediate rows to fp32: each is
    one rounding on ~1/1024 of the total, so even all-aligned they add one u32 on sum|rows|, and finalize_data keeps sum|y| / |sum y|
    below 1.2 and (s2/count) / var near 2 -- inside the four-rounding bound."""
    c = finalize_data(rows, C, rows * 10 + C)
    check_finalize(dev, c["part"], c["npix"], c["gamma"], c["beta"], c["rm"], c["rv"], 0.1, 1e-5, "bn_finalize")


def test_bn_finalize_optional_arguments(dev):
    c = finalize_data(70, 64, 5)
    check_finalize(dev, c["part"], c["npix"], None, None, c["rm"], c["rv"], 0.1, 1e-5, "bn_finalize[no-affine]")
    check_finalize(dev, c["part"], c["npix"], c["gamma"], c["beta"], None, None, 0.1, 1e-5, "bn_finalize[no-running]")
    f, _ = check_finalize(dev, c["part"], c["npix"], c["gamma"], c["beta"], c["rm"], c["rv"], 1.0, 1e-5, "bn_finalize[momentum-1]")
    assert torch.allclose(f["running_mean"], f["mean"], rtol=1e-12, atol=0)        # momentum 1 forgets the old statistics
    # the [rows, 2, C] and the [2C] forms of the partial rows
    from hallucidet_amd import ops
    one = R.sliced_stat_rows(c["y"], 1)
    a = ops.bn_finalize(one.to(dev).view(1, 2, 64), c["npix"], None, None, None, None, 0.1, 1e-5)
    b = ops.bn_finalize(one.to(dev).view(-1), c["npix"], None, None, None, None, 0.1, 1e-5)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_bn_finalize_count_one(dev):
    """count == 1 keeps the biased variance in running_var (count / (count - 1) would be a division by zero)."""
    C = 6
    part = torch.cat([torch.ones(C), torch.full((C,), 1.5)]).reshape(1, -1)      # m = 1, var = 0.5
    f, _ = check_finalize(dev, part, 1, rand(1, C), rand(2, C), rand(3, C), rand(5, C).abs() + 0.5, 0.1, 1e-5, "bn_finalize[count-1]")
    assert torch.equal(f["var"], torch.full((C,), 0.5, dtype=torch.float64))
    y = rand(4, 1, 64).half()                                                     # a real one-pixel batch: var == 0 exactly
    f, _ = check_finalize(dev, R.sliced_stat_rows(y, 1), 1, rand(1, 64), rand(2, 64), rand(3, 64), rand(5, 64).abs() + 0.5, 0.1, 1e-5,
                          "bn_finalize[one-pixel]")
    assert torch.equal(f["var"], torch.zeros(64, dtype=torch.float64))


def test_bn_finalize_negative_variance_and_constant_channel(dev):
    """Channel 0: hand-made rows with s2/count < m^2 (the clamp: invstd == 1/sqrt(eps)).  Channel 1: a constant 3.0 (var == 0 exactly).
    Channel 2: a constant 0.1 in f16 (rows rounded to fp32: var is rounding noise of either sign, ~1e-9 against eps 1e-5)."""
    rows, npix, C, eps = 5, 35, 8, 1e-5
    y = rand(7, npix, C).half()
    y[:, 1] = 3.0
    y[:, 2] = 0.1
    part = R.sliced_stat_rows(y, rows)
    part[:, 0] = 7 * 1.5                       # each row: 7 pixels of mean 1.5 ...
    part[:, C + 0] = 7 * (1.5 * 1.5 - 0.01)    # ... and a sum of squares below 7 * 1.5^2
    f, (mean, invstd, scale, shift) = check_finalize(dev, part, npix, rand(8, C), rand(9, C), rand(10, C), rand(11, C).abs() + 0.5, 0.1, eps,
                                                     "bn_finalize[clamp]")
    assert float(f["var"][0]) == 0.0 and float(f["var"][1]) == 0.0
    want = 1.0 / math.sqrt(R.f32(eps))
    assert abs(float(invstd[0]) - want) <= R.SCALAR_RTOL * want and abs(float(invstd[1]) - want) <= R.SCALAR_RTOL * want
    assert bool(torch.isfinite(torch.stack([mean, invstd, scale, shift])).all())


# ------------------------------------------------------------------------------------------------------------------ bn_eval_scale_shift
@pytest.mark.parametrize("C", [1, 63, 64, 65, 2048])
@pytest.mark.parametrize("affine", [True, False])
def test_bn_eval_scale_shift(dev, C, affine):
    from hallucidet_amd import ops
    gamma, beta = (rand(C, C) + 0.25, rand(C + 1, C)) if affine else (None, None)
    rm, rv = rand(C + 2, C), torch.rand(C, generator=torch.Generator().manual_seed(C + 3)) + 0.1
    d = lambda t: None if t is None else t.to(dev)
    scale, shift = ops.bn_eval_scale_shift(d(gamma), d(beta), d(rm), d(rv), 1e-5)
    f = R.ref_eval_scale_shift(gamma, beta, rm, rv, 1e-5)
    scalar_ok(scale, f["scale"], "bn_eval.scale")
    sum_ok(shift, f["shift"], f["shift_mag"], "bn_eval.shift")


# ------------------------------------------------------------------------------------------------------------------ bn_apply
def check_apply(dev, dtype, npix, C):
    from hallucidet_amd import ops
    d = R.random_inputs(npix, C, dtype, npix + C, with_res=True)
    scale = (rand(C, C) + torch.where(rand(C + 1, C) < 0, -1.5, 1.5)).float()        # mixed signs, |scale| mostly in [0.5, 2.5]
    shift = rand(C + 2, C).float()                                                     # a wrong channel is an O(1) error
    y_d, res_d, sc_d, sh_d = d["y"].to(dev), d["res"].to(dev), scale.to(dev), shift.to(dev)
    worst = 0.0
    for with_res in (False, True):
        for relu in (False, True):
            z = ops.bn_apply(y_d, sc_d, sh_d, res=res_d if with_res else None, relu=relu)
            assert z.dtype == dtype and z.shape == y_d.shape
            want, mag = R.ref_apply(d["y"], scale, shift, d["res"] if with_res else None, relu)
            r = R.worst_ratio(z, want, R.elem_tol(want, mag, dtype))
            assert r <= 1.0, (with_res, relu, r)
            worst = max(worst, r)
    note("bn_apply[%s]" % _id(dtype), worst)


@pytest.mark.parametrize("npix,C", [(1, 8), (255, 8), (257, 8), (33, 64), (5, 2048)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bn_apply_small(dev, dtype, npix, C):
    check_apply(dev, dtype, npix, C)


@pytest.mark.parametrize("npix,C", [(1049349, 8), (16385, 512), (4099, 2048)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bn_apply_past_the_grid_cap(dev, dtype, npix, C):
    """Just past 4096 blocks x 256 threads = 1 048 576 vectors of eight: the second grid-stride trip (768 vectors at (4099, 2048))
    reuses the coefficients each thread loaded for its first vector."""
    assert npix * C // 8 > 4096 * 256
    check_apply(dev, dtype, npix, C)


# ------------------------------------------------------------------------------------------------------------------ bn_bwd_reduce
def launch_reduce(d, rows, mode, fill=float("nan")):
    """hd_bn_bwd_reduce through _abi (ops.bn_backward keeps the slab to itself) into a slab pre-filled with NaN."""
    from hallucidet_amd import _abi
    from hallucidet_amd._abi import ptr
    y = d["y"]
    npix, C = y.shape
    part = torch.full((rows, 2 * C), fill, dtype=torch.float32, device=y.device)
    z = d["z"] if mode == "z" else None
    _abi.check(_abi.fn("hd_bn_bwd_reduce", y)(ptr(d["dz"]), ptr(z), ptr(y), ptr(d["mean"]), ptr(d["invstd"]), ptr(d.get("gamma")),
                                              ptr(d.get("beta")), ptr(part), rows, npix, C, 0 if mode == "none" else 1,
                                              torch.cuda.current_stream().cuda_stream), "hd_bn_bwd_reduce")
    return part


REDUCE_SHAPES = {
    8: [(n, 1) for n in (1, 255, 256, 257, 1023, 1024, 1025, 2049)] + [(1000, 7), (9, 4), (5, 4), (3, 8)],
    64: [(n, 1) for n in (31, 32, 33, 127, 128, 129, 1000)] + [(1000, 7)],
    256: [(n, 1) for n in (7, 8, 9, 31, 32, 33, 500)],
    2048: [(n, 1) for n in (1, 3, 4, 5, 9, 300)],
}


@pytest.mark.parametrize("mode", ["none", "z", "recompute"])
@pytest.mark.parametrize("C", sorted(REDUCE_SHAPES))
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bn_bwd_reduce(dev, dtype, C, mode):
    """Mask modes: no ReLU, ReLU from the saved z, ReLU recomputed from y.  Integer data: the slab's rows add up EXACTLY to the
    float64 sums.  Random data: within 1e-6 * sum|terms| (no shape here needed the worst-case fallback).  Blocks that own no pixel
    (rows * ceil(npix / rows) > npix) must still write zero rows over the NaN the slab was filled with."""
    worst = 0.0
    for npix, rows in REDUCE_SHAPES[C]:
        for kind, build in (("integer", R.integer_inputs), ("random", R.random_inputs)):
            d = build(npix, C, dtype, npix * 3 + rows, with_z=(mode == "z"))
            if kind == "random":
                assert R.mask_margin_violations(d) == 0
            part = launch_reduce(to_dev(d, dev), rows, mode).cpu()
            s = R.ref_bwd_sums(d["dz"], d.get("z") if mode == "z" else None, d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"],
                               mode != "none")
            got, want = part.double().sum(0), torch.cat([s["sg"], s["sgx"]])
            if kind == "integer":
                assert torch.equal(got, want), (kind, npix, rows, (got - want).abs().max())
            else:
                r = R.worst_ratio(got, want, R.REDUCE_RTOL * torch.cat([s["abs_sg"], s["abs_sgx"]]))
                assert r <= 1.0, (kind, npix, rows, r)
                worst = max(worst, r)
            per = -(-npix // rows)
            if rows * per > npix:
                first_empty = -(-npix // per)
                assert torch.equal(part[first_empty:], torch.zeros(rows - first_empty, 2 * C)), (kind, npix, rows)
    note("bn_bwd_reduce[%s,%s]" % (_id(dtype), mode), worst)


# ------------------------------------------------------------------------------------------------------------------ bn_bwd_apply
COEF_CASES = [(r, c) for r in (1, 15, 16, 17, 63, 64, 65, 192, 193, 257, 449, 1000) for c in (8, 64)] + [(193, 2048)]


@pytest.mark.parametrize("rows,C", COEF_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bn_bwd_coefficients_sum_any_number_of_rows(dev, dtype, rows, C):
    """Hand-made INTEGER partial rows: dgamma / dbeta are exact for power-of-two gscale, with and without accumulation (pre-filled with
    small integers when accumulating, with NaN when not), and dy follows the same sums."""
    from hallucidet_amd import ops
    npix = 3
    d = R.integer_inputs(npix, C, dtype, rows + C)
    part = randint(rows * 7 + C, -8, 8, rows, 2 * C).float()
    dd, part_d = to_dev(d, dev), part.to(dev)
    for gscale in (1.0, 0.5, 2.0 ** -7):
        for accumulate in (False, True):
            old_g, old_b = randint(rows, -9, 9, C).float(), randint(rows + 1, -9, 9, C).float()
            dg = old_g.to(dev) if accumulate else torch.full((C,), float("nan"), device=dev)
            db = old_b.to(dev) if accumulate else torch.full((C,), float("nan"), device=dev)
            dy, _, dg2, db2 = ops.bn_backward(dd["dz"], None, dd["y"], dd["mean"], dd["invstd"], dd["gamma"], dd["beta"], relu=True,
                                              gscale=gscale, dgamma=dg, dbeta=db, accumulate=accumulate, part=part_d)
            assert dg2 is dg and db2 is db
            want = R.ref_bwd_apply(d["dz"], None, d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], part, True, gscale,
                                   old_g if accumulate else None, old_b if accumulate else None)
            assert torch.equal(dg.cpu().double(), want["dgamma"]), (gscale, accumulate)
            assert torch.equal(db.cpu().double(), want["dbeta"]), (gscale, accumulate)
            r = R.worst_ratio(dy, want["dy"], R.elem_tol(want["dy"], want["dy_mag"], dtype))
            assert r <= 1.0, (gscale, accumulate, r)


VARIANTS = [(False, False, False), (False, False, True), (True, True, False), (True, True, True), (True, False, False),
            (True, False, True)]          # (ReLU, mask from z, dres wanted)


def cpu_rows(d, z, relu, rows):
    """[rows, 2C] fp32: the backward sums over `rows` contiguous pixel slices, taken in float64 and rounded to fp32."""
    s = R.ref_bwd_sums(d["dz"], z, d["y"], d["mean"], d["invstd"], d.get("gamma"), d.get("beta"), relu)
    npix, C = d["y"].shape
    seg = (torch.arange(npix) * rows) // npix
    out = torch.zeros(rows, 2 * C, dtype=torch.float64)
    out[:, :C].index_add_(0, seg, s["gk"])
    out[:, C:].index_add_(0, seg, s["gk"] * ((d["y"].double() - d["mean"].double()) * d["invstd"].double()))
    return out.float(), s


def check_backward(dev, dtype, d, variants, rows, what, exact_sums):
    """ops.bn_backward(part=P) with P made here, against ref_bwd_apply on the same P: dy inside the element tolerance, dres EQUAL to the
    masked dz, dgamma / dbeta within the reduction tolerance of the float64 sums (equal on integer data)."""
    from hallucidet_amd import ops
    dd = to_dev(d, dev)
    worst = 0.0
    for relu, usez, want_dres in variants:
        z = d["z"] if usez else None
        part, s = cpu_rows(d, z, relu, rows)
        dy, dres, dgamma, dbeta = ops.bn_backward(dd["dz"], dd["z"] if usez else None, dd["y"], dd["mean"], dd["invstd"], dd.get("gamma"),
                                                  dd.get("beta"), relu=relu, want_dres=want_dres, part=part.to(dev))
        want = R.ref_bwd_apply(d["dz"], z, d["y"], d["mean"], d["invstd"], d.get("gamma"), d.get("beta"), part, relu)
        assert dy.dtype == dtype and (dres is None) == (not want_dres)
        r = R.worst_ratio(dy, want["dy"], R.elem_tol(want["dy"], want["dy_mag"], dtype))
        assert r <= 1.0, (what, relu, usez, want_dres, r)
        worst = max(worst, r)
        if want_dres:
            assert torch.equal(dres.cpu().double(), want["dres"]), (what, relu, usez)
        if exact_sums:
            assert torch.equal(dgamma.cpu().double(), s["sgx"]) and torch.equal(dbeta.cpu().double(), s["sg"]), (what, relu, usez)
        else:
            rg = R.worst_ratio(dgamma, s["sgx"], R.REDUCE_RTOL * s["abs_sgx"])
            rb = R.worst_ratio(dbeta, s["sg"], R.REDUCE_RTOL * s["abs_sg"])
            assert rg <= 1.0 and rb <= 1.0, (what, relu, usez, rg, rb)
    return worst


@pytest.mark.parametrize("npix,C", [(1, 8), (257, 8), (100, 64), (5, 2048)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bn_backward_elements(dev, dtype, npix, C):
    """All six (ReLU, mask from z, dres) variants.
    part=P: random data with ONE float64-summed row (the coefficient launch then adds nothing, and the element tolerance's "fewer than
    16 roundings on the terms" holds as derived), integer data with three rows (their fp32 sum is exact).
    rows=r: ops.bn_backward runs the reduction itself.  On integer data (r = 3) the sums are exact whatever the order, so the SAME
    reference applies unchanged.  On random data r = 1, and the reference takes the slab the same deterministic reduction launch
    writes when it is called on its own -- again the very fp32 row the coefficient launch reads; that row is pinned to the float64
    sums by test_bn_bwd_reduce, and dgamma / dbeta are compared with the float64 sums here."""
    from hallucidet_amd import ops
    rnd = R.random_inputs(npix, C, dtype, npix + C, with_z=True)
    itg = R.integer_inputs(npix, C, dtype, npix + C + 1, with_z=True)
    assert R.mask_margin_violations(rnd) == 0
    worst = check_backward(dev, dtype, rnd, VARIANTS, 1, "random", False)
    worst = max(worst, check_backward(dev, dtype, itg, VARIANTS, min(3, npix), "integer", True))
    for kind, d, rows in (("integer", itg, 3), ("random", rnd, 1)):
        dd = to_dev(d, dev)
        for relu, usez, want_dres in VARIANTS:
            z = d["z"] if usez else None
            mode = "none" if not relu else ("z" if usez else "recompute")
            dy, dres, dgamma, dbeta = ops.bn_backward(dd["dz"], dd["z"] if usez else None, dd["y"], dd["mean"], dd["invstd"], dd["gamma"],
                                                      dd["beta"], relu=relu, want_dres=want_dres, rows=rows)
            s = R.ref_bwd_sums(d["dz"], z, d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], relu)
            if kind == "integer":
                part = torch.cat([s["sg"], s["sgx"]]).reshape(1, -1).float()
                assert torch.equal(dgamma.cpu().double(), s["sgx"]) and torch.equal(dbeta.cpu().double(), s["sg"]), (kind, relu, usez)
            else:
                part = launch_reduce(dd, rows, mode).cpu()
                assert R.worst_ratio(dgamma, s["sgx"], R.REDUCE_RTOL * s["abs_sgx"]) <= 1.0, (kind, relu, usez)
                assert R.worst_ratio(dbeta, s["sg"], R.REDUCE_RTOL * s["abs_sg"]) <= 1.0, (kind, relu, usez)
            want = R.ref_bwd_apply(d["dz"], z, d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], part, relu)
            r = R.worst_ratio(dy, want["dy"], R.elem_tol(want["dy"], want["dy_mag"], dtype))
            assert r <= 1.0, (kind, "rows=%d" % rows, relu, usez, r)
            worst = max(worst, r)
            if want_dres:
                assert torch.equal(dres.cpu().double(), want["dres"]), (kind, relu, usez)
    note("bn_bwd_apply.dy[%s]" % _id(dtype), worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bn_backward_without_affine(dev, dtype):
    """gamma = beta = NULL (1 and 0) in the reduction, the coefficient launch and the recomputed mask."""
    d = R.random_inputs(100, 64, dtype, 11, with_z=True, affine=False)
    assert d["gamma"] is None and R.mask_margin_violations(d) == 0
    part = launch_reduce(to_dev(d, dev), 3, "recompute").cpu()
    s = R.ref_bwd_sums(d["dz"], None, d["y"], d["mean"], d["invstd"], None, None, True)
    r = R.worst_ratio(part.double().sum(0), torch.cat([s["sg"], s["sgx"]]), R.REDUCE_RTOL * torch.cat([s["abs_sg"], s["abs_sgx"]]))
    assert r <= 1.0, r
    note("bn_bwd_apply.dy[%s,no-affine]" % _id(dtype), check_backward(dev, dtype, d, VARIANTS, 1, "no affine", False))


@pytest.mark.parametrize("npix,C", [(524588, 8), (2049, 2048)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bn_backward_past_the_grid_cap(dev, dtype, npix, C):
    """Just past 2048 blocks x 256 threads = 524 288 vectors of eight: the second grid-stride trip of the apply launch."""
    assert npix * C // 8 > 2048 * 256
    d = R.random_inputs(npix, C, dtype, npix + C, with_z=True)
    assert R.mask_margin_violations(d) == 0
    worst = check_backward(dev, dtype, d, [(True, False, True), (True, True, False), (False, False, True)], 1, "past cap", False)
    note("bn_bwd_apply.dy[%s,past-cap]" % _id(dtype), worst)
