"""The pooling, resampling and layout kernels of csrc/elementwise.hip (max-pool and its three backward forms, stride-2 subsample,
nearest resize in and out of NHWC with its adjoint, upsample_add and its adjoint, the decoder's 2x2 sum-pool / slice / concat
gradients, the casts, relu_bwd, scale_store, sigmoid_bwd) against the float64 / exact definitions of tests/_glue_reference.py
(proven against ATen in test_glue_reference_cpu.py), through hallucidet_amd.ops, in both storage types.

Grid data (multiples of 2^-6: every fp32 sum is exact) is asserted with torch.equal; wild data with _glue_reference's bound, every
element checked.  Output buffers the caller supplies are pre-filled with NaN for the non-accumulating forms, so a skipped element
shows.  The last section sizes one case per kernel to 4096 * 256 work items plus a few hundred: the grid-stride loops' second trip,
ending inside a block."""
import functools

import pytest
import torch

import _glue_reference as G

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.float32]
_id = lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None
NAN = float("nan")


def eq(got, want, what):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = ~((got == want) | (got.isnan() & want.isnan())) if got.is_floating_point() else got != want
        at = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.numel(), at, got[tuple(at)].item(), want[tuple(at)].item()))


def within(got, ref, tol, what):
    r = G.worst_ratio(got, ref, tol)
    print("glue ratio %s %.4g" % (what, r))
    assert r <= 1.0, (what, r)


def nan_like(shape, dtype, dev):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def _mixed(pairs):
    """(a_in, a_out, b_in, b_out): each pair on the H axis with the next one on the W axis."""
    return [(a[0], a[1], b[0], b[1]) for a, b in zip(pairs, pairs[1:] + pairs[:1])]


# ------------------------------------------------------------------------------------------------------------------ max-pool
POOL_HW = [(1, 1), (1, 8), (2, 3), (5, 4), (3, 2), (4, 7), (7, 5), (16, 3), (2, 16), (16, 16)]


def pool_inputs(seed, shape, dtype):
    yield "negative", G.grid_inputs(seed, shape, dtype, negative=True)
    yield "ties", G.grid_inputs(seed + 1, shape, dtype, levels=4)
    yield "ties-negative", G.grid_inputs(seed + 2, shape, dtype, levels=3, negative=True)
    yield "relu", torch.relu(G.grid_inputs(seed + 3, shape, dtype))
    lowest = torch.full(shape, -65504.0, dtype=dtype)          # mostly the lowest finite fp16: whole windows of it
    keep = torch.rand(shape, generator=torch.Generator().manual_seed(seed + 4)) < 0.15
    yield "lowest", torch.where(keep, G.grid_inputs(seed + 5, shape, dtype), lowest)
    yield "wild", G.wild_inputs(seed + 6, shape, dtype)


@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_maxpool_forward_indices_and_three_backward_forms(dev, dtype, C):
    from hallucidet_amd import ops
    for i, (H, W) in enumerate(POOL_HW):
        N = 3 if i % 2 else 1
        for kind, x in pool_inputs(1000 * H + 10 * W + C, (N, H, W, C), dtype):
            what = (kind, N, H, W)
            y_ref, pos = G.ref_maxpool(x)
            if kind == "lowest" and x.numel() >= 64:
                assert bool((y_ref == -65504).any()), what
            xd = x.to(dev)
            eq(ops.maxpool3x3s2(xd), y_ref, ("maxpool",) + what)
            y2, idx = ops.maxpool3x3s2_idx(xd)
            eq(y2, y_ref, ("maxpool_idx y",) + what)
            eq(idx, pos, ("maxpool_idx idx",) + what)
            # exact: grid gradients
            dy = G.grid_inputs(H * W + C, y_ref.shape, dtype)
            add = G.grid_inputs(H * W + C + 1, x.shape, dtype)
            want = G.ref_maxpool_bwd(pos, dy, H, W)
            dx1 = ops.maxpool3x3s2_bwd(xd, dy.to(dev))
            dx2 = ops.maxpool3x3s2_bwd_idx(idx, dy.to(dev), (H, W))
            eq(dx1, want, ("maxpool_bwd",) + what)
            eq(dx2, want, ("maxpool_bwd_idx",) + what)
            assert torch.equal(dx1, dx2), what
            eq(ops.maxpool3x3s2_bwd_idx(idx, dy.to(dev), (H, W), add=add.to(dev)), G.ref_maxpool_bwd(pos, dy, H, W, add=add),
               ("maxpool_bwd_idx add",) + what)
        # wild gradients, routed by the wild input's winners (the last of pool_inputs): at most 4 windows route into one pixel (k = 4),
        # plus `add` (k = 5, and the documented storage rounding of the routed sum); |values| <= 8192 keeps five of them inside fp16
        assert kind == "wild"
        dyw = G.wild_inputs(H * W + C + 2, y_ref.shape, dtype, max_abs=8192.0)
        addw = G.wild_inputs(H * W + C + 3, x.shape, dtype, max_abs=8192.0)
        s, a = G.ref_maxpool_bwd_terms(pos, dyw, H, W)
        within(ops.maxpool3x3s2_bwd(xd, dyw.to(dev)), s, G.sum_tol(s, a, 4, dtype), "maxpool_bwd wild")
        within(ops.maxpool3x3s2_bwd_idx(idx, dyw.to(dev), (H, W)), s, G.sum_tol(s, a, 4, dtype), "maxpool_bwd_idx wild")
        sa, aa = s + addw.double(), a + addw.double().abs()
        within(ops.maxpool3x3s2_bwd_idx(idx, dyw.to(dev), (H, W), add=addw.to(dev)), sa, G.sum_tol(sa, aa, 5, dtype, extra=s),
               "maxpool_bwd_idx add wild")


def test_maxpool_add_form_rounds_the_routed_sum_before_it_adds(dev):
    """Pixel (1, 1) wins four windows whose gradients sum to 2049, a tie of fp16's spacing-2 range: f16(f16(2049) + 1) = 2048,
    f16(2049 + 1) = 2050.  Odd sums above 2048 on random grid data are rare; this one is built."""
    from hallucidet_amd import ops
    x = torch.zeros(1, 3, 3, 8, dtype=torch.float16)
    x[0, 1, 1] = 1.0
    dy = torch.tensor([1024.0, 1024.0, 1.0, 0.0], dtype=torch.float16).view(1, 2, 2, 1).expand(1, 2, 2, 8).contiguous()
    add = torch.ones(1, 3, 3, 8, dtype=torch.float16)
    y_ref, pos = G.ref_maxpool(x)
    want = G.ref_maxpool_bwd(pos, dy, 3, 3, add=add)
    assert float(want[0, 1, 1, 0]) == 2048.0
    _, idx = ops.maxpool3x3s2_idx(x.to(dev))
    eq(ops.maxpool3x3s2_bwd_idx(idx, dy.to(dev), (3, 3), add=add.to(dev)), want, "two roundings")


# ------------------------------------------------------------------------------------------------------------------ subsample
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_subsample2_and_its_gradient(dev, dtype):
    from hallucidet_amd import ops
    sizes = (1, 2, 5, 10)
    for H in sizes:
        for W in sizes:
            for N, C in ((1, 8), (2, 24)):
                x = G.wild_inputs(H * 100 + W + C, (N, H, W, C), dtype)
                eq(ops.subsample2(x.to(dev)), G.ref_subsample2(x), ("subsample2", N, H, W, C))
                dy = G.grid_inputs(H * 100 + W + C + 1, (N, G.pool_out(H), G.pool_out(W), C), dtype)
                dx = nan_like(x.shape, dtype, dev)
                ops.subsample2_bwd(dy.to(dev), dx, accumulate=False)
                eq(dx, G.ref_subsample2_bwd(dy, H, W), ("subsample2_bwd", N, H, W, C))
                prev = G.grid_inputs(H * 100 + W + C + 2, x.shape, dtype)
                dx = prev.to(dev)
                ops.subsample2_bwd(dy.to(dev), dx, accumulate=True)
                eq(dx, G.ref_subsample2_bwd(dy, H, W, prev), ("subsample2_bwd accumulate", N, H, W, C))


# ------------------------------------------------------------------------------------------------------------------ resize in / out of NHWC
RESIZE_CASES = _mixed(G.RESIZE_PAIRS)          # (H, Ho, W, Wo)
CHANNELS = [(1, 8), (3, 8), (8, 8), (1, 16), (3, 16), (8, 16), (16, 16)]
_case_id = lambda c: "%dto%d_%dto%d" % c


def image_inputs(seed, shape):
    """fp32 NCHW pixels: wild values, some beyond fp16's range (-> inf in fp16 storage) and some that round to fp16 subnormals."""
    x = G.wild_inputs(seed, shape, torch.float32)
    g = torch.Generator().manual_seed(seed + 1)
    pick = torch.randint(0, 40, tuple(shape), generator=g)
    x = torch.where(pick == 0, torch.full_like(x, 70000.0), x)
    x = torch.where(pick == 1, torch.full_like(x, -1e30), x)
    return torch.where(pick == 2, x * 2.0 ** -20, x)


@pytest.mark.parametrize("case", RESIZE_CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_nchw_to_nhwc_resize_follows_the_fp32_index_rule(dev, dtype, case):
    from hallucidet_amd import ops
    H, Ho, W, Wo = case
    N = 2
    for Cr, Cp in CHANNELS:
        x = image_inputs(H * W + Cr + Cp, (N, Cr, H, W))
        want = G.ref_resize_fwd(x, Ho, Wo, Cp, dtype)
        assert not want[..., Cr:].any()
        eq(ops.nchw_to_nhwc_resize(x.to(dev), Ho, Wo, Cp, dtype=dtype), want, ("contiguous", Cr, Cp))
        # image stride > Cr*H*W: the first N images and Cr channels of a larger buffer
        big = image_inputs(H * W + Cr + Cp + 1, (N + 1, Cr + 2, H, W))
        view = big.to(dev)[:N, :Cr]
        assert not view.is_contiguous() and view.stride(0) > Cr * H * W
        eq(ops.nchw_to_nhwc_resize(view, Ho, Wo, Cp, dtype=dtype), G.ref_resize_fwd(big[:N, :Cr], Ho, Wo, Cp, dtype), ("image stride", Cr, Cp))
        # out= a slice of a larger NHWC buffer: the rows around it stay untouched
        buf = nan_like((N + 2, Ho, Wo, Cp), dtype, dev)
        ops.nchw_to_nhwc_resize(x.to(dev), Ho, Wo, Cp, out=buf[1:N + 1])
        eq(buf[1:N + 1], want, ("out=", Cr, Cp))
        assert bool(buf[0].isnan().all()) and bool(buf[N + 1].isnan().all()), ("out= wrote outside its slice", Cr, Cp)
    # the one-plane batch as a stride-0 three-channel view
    for Cp in (8, 16):
        one = image_inputs(H * W + Cp, (N + 1, 1, H, W))
        view = one.to(dev)[:N].expand(-1, 3, -1, -1)
        assert view.stride(1) == 0
        eq(ops.nchw_to_nhwc_resize(view, Ho, Wo, Cp, dtype=dtype), G.ref_resize_fwd(one[:N].expand(-1, 3, -1, -1), Ho, Wo, Cp, dtype),
           ("stride-0 channels", Cp))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_nhwc_to_nchw(dev, dtype):
    from hallucidet_amd import ops
    for H, W in ((1, 1), (5, 1), (7, 22), (33, 46)):
        for Cr, Cp in CHANNELS:
            x = G.wild_inputs(H * W + Cr + Cp, (2, H, W, Cp), dtype)
            eq(ops.nhwc_to_nchw(x.to(dev), Cr), G.ref_nhwc_to_nchw(x, Cr), ("nhwc_to_nchw", H, W, Cr, Cp))
    x = G.wild_inputs(3, (2, 4, 5, 8), dtype)
    eq(ops.nhwc_to_nchw(x.to(dev)), G.ref_nhwc_to_nchw(x, 8), "Cr defaults to Cp")


@pytest.mark.parametrize("case", RESIZE_CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_nchw_to_nhwc_resize_bwd_is_the_adjoint_under_the_fp32_rule(dev, dtype, case):
    from hallucidet_amd import ops
    H, Ho, W, Wo = case
    N = 2
    k = G.max_preimage(Ho, H) * G.max_preimage(Wo, W)
    for Cr, Cp in [(1, 8), (3, 8), (8, 8), (1, 16), (3, 16), (8, 16)]:
        dy = G.grid_inputs(Ho * Wo + Cr + Cp, (N, Ho, Wo, Cp), dtype)          # (channels >= Cr hold values too: they must be ignored)
        for gs in (1.0, 0.5):
            eq(ops.nchw_to_nhwc_resize_bwd(dy.to(dev), N, Cr, H, W, gscale=gs), G.ref_resize_bwd(dy, N, Cr, H, W, gs), ("grid", Cr, Cp, gs))
        dyw = G.wild_inputs(Ho * Wo + Cr + Cp + 1, (N, Ho, Wo, Cp), dtype)
        s, a = G.ref_resize_bwd_terms(dyw, N, Cr, H, W, 1.0 / 3.0)
        within(ops.nchw_to_nhwc_resize_bwd(dyw.to(dev), N, Cr, H, W, gscale=1.0 / 3.0), s, G.sum_tol(s, a, k, torch.float32),
               "resize_bwd wild k=%d" % k)


# ------------------------------------------------------------------------------------------------------------------ upsample_add
UPSAMPLE_CASES = _mixed(G.UPSAMPLE_PAIRS)      # (Hb, H, Wb, W)


@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=_case_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_upsample_add_and_its_adjoint(dev, dtype, case):
    from hallucidet_amd import ops
    Hb, H, Wb, W = case
    k = G.max_preimage(H, Hb) * G.max_preimage(W, Wb)
    for N, C in ((2, 8), (1, 24)):
        a, b = G.grid_inputs(H * W + C, (N, H, W, C), dtype), G.grid_inputs(Hb * Wb + C, (N, Hb, Wb, C), dtype)
        eq(ops.upsample_add(a.to(dev), b.to(dev)), G.ref_upsample_add(a, b), ("upsample_add", C))
        dy = G.grid_inputs(H * W + C + 1, (N, H, W, C), dtype)
        db = nan_like(b.shape, dtype, dev)
        ops.upsample_add_bwd(dy.to(dev), db, accumulate=False)
        eq(db, G.ref_upsample_add_bwd(dy, Hb, Wb), ("upsample_add_bwd", C))
        prev = G.grid_inputs(H * W + C + 2, b.shape, dtype)
        db = prev.to(dev)
        ops.upsample_add_bwd(dy.to(dev), db, accumulate=True)
        eq(db, G.ref_upsample_add_bwd(dy, Hb, Wb, prev), ("upsample_add_bwd accumulate", C))
        # wild data (|values| <= 65504 / (k + 1) rounded down to a power of two: the sums stay inside fp16)
        lim = 2.0 ** 15
        while lim * (k + 1) > 65504:
            lim /= 2
        dyw, prevw = G.wild_inputs(H * W + C + 3, dy.shape, dtype, max_abs=lim), G.wild_inputs(H * W + C + 4, b.shape, dtype, max_abs=lim)
        db = prevw.to(dev)
        ops.upsample_add_bwd(dyw.to(dev), db, accumulate=True)
        s, mag = G.ref_upsample_add_bwd_terms(dyw, Hb, Wb, prevw)
        within(db, s, G.sum_tol(s, mag, k + 1, dtype), "upsample_add_bwd wild k=%d" % (k + 1))


# ------------------------------------------------------------------------------------------------------------------ decoder gradients
@pytest.mark.parametrize("c_off", [0, 8, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_upsample2_bwd_and_slice_channels_at_a_channel_offset(dev, dtype, c_off):
    from hallucidet_amd import ops
    for N, Hl, Wl, C in ((1, 1, 1, 8), (2, 1, 1, 24), (2, 3, 5, 8), (1, 11, 13, 24), (3, 2, 1, 16)):
        Ctot = c_off + C + 8                                                   # channels on both sides of the slice (c_off > 0)
        dy = G.grid_inputs(Hl * Wl + C + c_off, (N, 2 * Hl, 2 * Wl, Ctot), dtype)
        what = (N, Hl, Wl, C, Ctot)
        dx = nan_like((N, Hl, Wl, C), dtype, dev)
        ops.upsample2_bwd(dy.to(dev), dx, c_off, accumulate=False)
        eq(dx, G.ref_upsample2_bwd(dy, c_off, C), ("upsample2_bwd",) + what)
        prev = G.grid_inputs(Hl * Wl + C + c_off + 1, (N, Hl, Wl, C), dtype)
        dx = prev.to(dev)
        ops.upsample2_bwd(dy.to(dev), dx, c_off, accumulate=True)
        eq(dx, G.ref_upsample2_bwd(dy, c_off, C, prev), ("upsample2_bwd accumulate",) + what)
        out = nan_like((N, 2 * Hl, 2 * Wl, C), dtype, dev)
        ops.slice_channels(dy.to(dev), out, c_off, accumulate=False)
        eq(out, G.ref_slice(dy, c_off, C), ("slice_channels",) + what)
        prev = G.grid_inputs(Hl * Wl + C + c_off + 2, out.shape, dtype)
        out = prev.to(dev)
        ops.slice_channels(dy.to(dev), out, c_off, accumulate=True)
        eq(out, G.ref_slice(dy, c_off, C, prev), ("slice_channels accumulate",) + what)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_concat_up_bwd_against_the_reference_itself(dev, dtype):
    """(1, 11, 13, 24, 16): 429 low-resolution vectors, so block 1 holds the end of the sum-pool half and the start of the copy half."""
    from hallucidet_amd import ops
    for N, Hl, Wl, Cup, Cskip in ((1, 1, 1, 8, 0), (2, 3, 5, 8, 0), (2, 3, 5, 8, 8), (1, 11, 13, 24, 16), (2, 2, 1, 16, 24), (1, 1, 1, 8, 8)):
        dcat = G.grid_inputs(Hl * Wl + Cup + Cskip, (N, 2 * Hl, 2 * Wl, Cup + Cskip), dtype)
        da, ds = ops.concat_up_bwd(dcat.to(dev), Cup)
        want_a, want_s = G.ref_concat_up_bwd(dcat, Cup)
        eq(da, want_a, ("concat_up_bwd low", N, Hl, Wl, Cup, Cskip))
        if Cskip:
            eq(ds, want_s, ("concat_up_bwd skip", N, Hl, Wl, Cup, Cskip))
        else:
            assert ds is None and want_s is None
    assert (1 * 11 * 13 * 3) % 256 != 0


# ------------------------------------------------------------------------------------------------------------------ element-wise
VECTOR_COUNTS = [1, 255, 256, 257]
SCALAR_COUNTS = [1, 7, 1000] + [8 * v for v in VECTOR_COUNTS]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_add_and_relu_bwd(dev, dtype):
    from hallucidet_amd import ops
    for v in VECTOR_COUNTS:
        n = 8 * v
        a, b = G.grid_inputs(n, (n,), dtype), G.grid_inputs(n + 1, (n,), dtype)
        eq(ops.add_f16(a.to(dev), b.to(dev)), G.ref_add(a, b), ("add", v))
        out = nan_like((n,), dtype, dev)
        ops.add_f16(a.to(dev), b.to(dev), out=out)
        eq(out, G.ref_add(a, b), ("add out=", v))
        aw, bw = G.wild_inputs(n, (n,), dtype, max_abs=16384.0), G.wild_inputs(n + 1, (n,), dtype, max_abs=16384.0)
        s = aw.double() + bw.double()
        within(ops.add_f16(aw.to(dev), bw.to(dev)), s, G.sum_tol(s, aw.double().abs() + bw.double().abs(), 2, dtype), "add wild")
        # relu_bwd: the gradient passes where z > 0 and nowhere else (-0, +0, the smallest subnormal, negatives, wild values)
        dy = G.wild_inputs(n + 2, (n,), dtype)
        z = G.wild_inputs(n + 3, (n,), dtype)
        z[0::8] = -0.0
        if n >= 8:
            z[1::8], z[2::8], z[3::8] = 0.0, 2.0 ** -24, -2.0 ** -24
        want = G.ref_relu_bwd(dy, z)
        eq(ops.relu_bwd(dy.to(dev), z.to(dev)), want, ("relu_bwd", v))
        assert not want[0::8].any() and torch.equal(want[2::8], dy[2::8])


def cast_inputs(n):
    """fp32 values around every edge of the fp16 format: exact ties of fp16's rounding, values that land in its subnormals (also
    after the 2.0 scale), values above 65504, plus wild ones."""
    x = G.wild_inputs(n, (n,), torch.float32)
    edge = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 1.5 * 2.0 ** -24,
                         -2.5 * 2.0 ** -24, 2.0 ** -15 + 2.0 ** -25, 65504.0, 65519.0, 65520.0, 70000.0, -1e6, 32760.0, 3e-9], dtype=torch.float32)
    m = min(n, edge.numel())
    x[:m] = edge[:m]
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_casts(dev, dtype):
    from hallucidet_amd import ops
    for n in SCALAR_COUNTS:
        x = cast_inputs(n)
        for scale in (1.0, 2.0, 0.5):
            eq(ops.f32_to_f16(x.to(dev), scale, dtype=dtype), G.ref_f32_to_f16(x, scale, dtype), ("f32_to_f16", n, scale))
        # a scale that is no power of two: the fp32 product rounds, and the compiler may fold the multiply into the conversion (gfx950 has
        # a fused multiply-convert that rounds the exact product once) -- as with scale_store's multiply-add, either rounding is the
        # kernel's `(f16)(x * scale)`; nothing else is.  Measured: the library does fold it, 1.5 * 2^-24 * f32(1/3) comes back as 2^-24.
        got = ops.f32_to_f16(x.to(dev), 1.0 / 3.0, dtype=dtype).cpu()
        two, one = G.ref_f32_to_f16(x, 1.0 / 3.0, dtype), G.ref_f32_to_f16_fused(x, 1.0 / 3.0, dtype)
        assert got.dtype == dtype and bool(((got == two) | (got == one)).all()), ("f32_to_f16", n, "1/3")
        h = G.wild_inputs(n + 1, (n,), dtype)
        for scale in (1.0, 2.0, 0.5, 1.0 / 3.0):
            eq(ops.f16_to_f32(h.to(dev), scale), G.ref_f16_to_f32(h, scale), ("f16_to_f32", n, scale))
    if dtype == torch.float16:
        x = cast_inputs(1000)
        want = G.ref_f32_to_f16(x, 2.0, dtype)
        assert bool(want.isinf().any()) and bool(((want != 0) & (want.abs() < 2.0 ** -14)).any())


def test_scale_store(dev):
    from hallucidet_amd import ops
    for n in SCALAR_COUNTS:
        src, prev = G.grid_inputs(n, (n,), torch.float32), G.grid_inputs(n + 1, (n,), torch.float32)
        for scale in (1.0, 0.25, -8.0):
            dst = nan_like((n,), torch.float32, dev)
            ops.scale_store(src.to(dev), dst, scale, accumulate=False)
            eq(dst, G.ref_scale_store_terms(src, scale)[0].float(), ("scale_store", n, scale))
            dst = prev.to(dev)
            ops.scale_store(src.to(dev), dst, scale, accumulate=True)
            eq(dst, G.ref_scale_store_terms(src, scale, prev)[0].float(), ("scale_store accumulate", n, scale))
        srcw, prevw = G.wild_inputs(n + 2, (n,), torch.float32), G.wild_inputs(n + 3, (n,), torch.float32)
        for scale in (1.0 / 3.0, -0.7):
            dst = nan_like((n,), torch.float32, dev)
            ops.scale_store(srcw.to(dev), dst, scale, accumulate=False)
            eq(dst, G.ref_f16_to_f32(srcw, scale), ("scale_store wild", n, scale))               # one fp32 multiply: exact definition
            dst = prevw.to(dev)
            ops.scale_store(srcw.to(dev), dst, scale, accumulate=True)
            s, mag = G.ref_scale_store_terms(srcw, scale, prevw)
            within(dst, s, 2 * G.U32 * mag, "scale_store accumulate wild")                     # the compiler may contract the multiply-add


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_sigmoid_bwd_nchw_to_nhwc(dev, dtype):
    from hallucidet_amd import ops
    for H, W in ((1, 1), (5, 7), (19, 31)):
        for Cr, Cp in [(1, 8), (3, 8), (8, 8), (1, 16), (3, 16), (8, 16)]:
            g = torch.Generator().manual_seed(H * W + Cr + Cp)
            s = torch.rand((2, Cr, H, W), generator=g)
            pick = torch.randint(0, 8, s.shape, generator=g)
            for j, v in enumerate((0.0, 1.0, 0.5)):
                s = torch.where(pick == j, torch.full_like(s, v), s)
            dy = G.wild_inputs(H * W + Cr + Cp + 1, s.shape, torch.float32, max_abs=8192.0)       # |4 * dy * s * (1 - s)| <= 8192: finite in fp16
            ref = G.ref_sigmoid_bwd(dy, s, Cp, 4.0)
            got = ops.sigmoid_bwd_nchw_to_nhwc(dy.to(dev), s.to(dev), Cp, gscale=4.0, dtype=dtype)
            assert got.dtype == dtype
            u = G.U16 if dtype == torch.float16 else G.U32
            within(got, ref, u * ref.abs() + 8 * G.U32 * ref.abs() + 2.0 ** -25, "sigmoid_bwd")
            assert not got[..., Cr:].cpu().any(), ("padding channels", Cr, Cp)
    assert s.numel() > 1000 and bool((s == 0).any()) and bool((s == 1).any()) and bool((s == 0.5).any())


# ------------------------------------------------------------------------------------------------------------------ past the grid cap
# grid_for() caps every launch at 4096 blocks of 256 threads.  Each case below has 4096 * 256 work items (vectors of 8 channels for the
# vector kernels, pixels for the resize / layout kernels, elements for the scalar casts) plus a few hundred: a second trip of the
# grid-stride loop that ends inside a block.  fp16, 16 channels, grid data, torch.equal.
CAP = 4096 * 256
P_VEC = (607, 864)          # 607 * 864 pixels * 2 vectors = CAP + 320
P_PIX = (607, 1728)         # 607 * 1728 pixels = CAP + 320
assert P_VEC[0] * P_VEC[1] * 2 == CAP + 320 and P_PIX[0] * P_PIX[1] == CAP + 320
F16 = torch.float16


@functools.lru_cache(maxsize=None)
def _pool():
    """One flat tensor of grid data that every case below cuts its inputs from (read-only): 1 000 003 values (a prime, so the period
    lines up with no row, plane or vector stride), repeated."""
    need = 1214 * 1728 * 16
    return G.grid_inputs(99, (1000003,), F16).repeat(need // 1000003 + 1)[:need].contiguous()


def cut(shape, offset=0):
    n = 1
    for s in shape:
        n *= s
    return _pool()[offset:offset + n].view(shape)


def test_cap_maxpool_forward(dev):
    from hallucidet_amd import ops
    H, W = 2 * P_VEC[0] - 1, 2 * P_VEC[1] - 1
    x = cut((1, H, W, 16))
    assert (G.pool_out(H), G.pool_out(W)) == P_VEC
    y_ref, pos = G.ref_maxpool(x)
    xd = x.to(dev)
    eq(ops.maxpool3x3s2(xd), y_ref, "maxpool")
    y, idx = ops.maxpool3x3s2_idx(xd)
    eq(y, y_ref, "maxpool_idx y")
    eq(idx, pos, "maxpool_idx idx")


def test_cap_maxpool_backward(dev):
    from hallucidet_amd import ops
    H, W = P_VEC
    x = G.grid_inputs(5, (1, H, W, 16), F16, levels=64)                        # ties in most windows
    y_ref, pos = G.ref_maxpool(x)
    dy, add = cut(y_ref.shape), cut(x.shape, 1000)
    xd, dyd = x.to(dev), dy.to(dev)
    _, idx = ops.maxpool3x3s2_idx(xd)
    eq(idx, pos, "idx")
    want = G.ref_maxpool_bwd(pos, dy, H, W)
    eq(ops.maxpool3x3s2_bwd(xd, dyd), want, "maxpool_bwd")
    eq(ops.maxpool3x3s2_bwd_idx(idx, dyd, (H, W)), want, "maxpool_bwd_idx")
    eq(ops.maxpool3x3s2_bwd_idx(idx, dyd, (H, W), add=add.to(dev)), G.ref_maxpool_bwd(pos, dy, H, W, add=add), "maxpool_bwd_idx add")


def test_cap_subsample2_and_gradient(dev):
    from hallucidet_amd import ops
    H, W = 2 * P_VEC[0] - 1, 2 * P_VEC[1]
    x = cut((1, H, W, 16))
    eq(ops.subsample2(x.to(dev)), G.ref_subsample2(x), "subsample2")
    H, W = P_VEC
    dy, prev = cut((1, G.pool_out(H), G.pool_out(W), 16)), cut((1, H, W, 16), 500)
    dx = nan_like(prev.shape, F16, dev)
    ops.subsample2_bwd(dy.to(dev), dx, accumulate=False)
    eq(dx, G.ref_subsample2_bwd(dy, H, W), "subsample2_bwd")
    dx = prev.to(dev)
    ops.subsample2_bwd(dy.to(dev), dx, accumulate=True)
    eq(dx, G.ref_subsample2_bwd(dy, H, W, prev), "subsample2_bwd accumulate")


def test_cap_resize_and_layout(dev):
    from hallucidet_amd import ops
    Ho, Wo = P_PIX
    x = cut((1, 3, 303, 864)).float()
    eq(ops.nchw_to_nhwc_resize(x.to(dev), Ho, Wo, 16, dtype=F16), G.ref_resize_fwd(x, Ho, Wo, 16, F16), "nchw_to_nhwc_resize")
    dy = cut((1, Ho, 1800, 16))                                                # dx [1, 3, 607, 1728]: CAP + 320 pixels
    eq(ops.nchw_to_nhwc_resize_bwd(dy.to(dev), 1, 3, Ho, Wo, gscale=0.5), G.ref_resize_bwd(dy, 1, 3, Ho, Wo, 0.5), "nchw_to_nhwc_resize_bwd")
    xl = cut((1, Ho, Wo, 16))
    eq(ops.nhwc_to_nchw(xl.to(dev), 3), G.ref_nhwc_to_nchw(xl, 3), "nhwc_to_nchw")
    g = torch.Generator().manual_seed(7)
    s = torch.randint(0, 65, (1, 3, Ho, Wo), generator=g).float() / 64.0      # s, 1 - s, dy: few-bit values, the fp32 product is exact
    d = cut((1, 3, Ho, Wo), 77).float()
    ref = G.ref_sigmoid_bwd(d, s, 16, 4.0)
    eq(ops.sigmoid_bwd_nchw_to_nhwc(d.to(dev), s.to(dev), 16, gscale=4.0, dtype=F16), ref.half(), "sigmoid_bwd_nchw_to_nhwc")


def test_cap_upsample_add_and_adjoint(dev):
    from hallucidet_amd import ops
    H, W = P_VEC
    a, b = cut((1, H, W, 16)), cut((1, 304, 432, 16), 4000)
    eq(ops.upsample_add(a.to(dev), b.to(dev)), G.ref_upsample_add(a, b), "upsample_add")
    dy, prev = cut((1, H, 2 * W - 1, 16)), cut((1, H, W, 16), 123)               # db [1, 607, 864, 16]: CAP + 320 vectors
    db = nan_like(prev.shape, F16, dev)
    ops.upsample_add_bwd(dy.to(dev), db, accumulate=False)
    eq(db, G.ref_upsample_add_bwd(dy, H, W), "upsample_add_bwd")
    db = prev.to(dev)
    ops.upsample_add_bwd(dy.to(dev), db, accumulate=True)
    eq(db, G.ref_upsample_add_bwd(dy, H, W, prev), "upsample_add_bwd accumulate")


def test_cap_decoder_gradients(dev):
    from hallucidet_amd import ops
    Hl, Wl = P_VEC
    dy = cut((1, 2 * Hl, 2 * Wl, 16))
    dx = nan_like((1, Hl, Wl, 16), F16, dev)
    ops.upsample2_bwd(dy.to(dev), dx, 0, accumulate=False)
    eq(dx, G.ref_upsample2_bwd(dy, 0, 16), "upsample2_bwd")
    x = cut((1, Hl, Wl, 32))
    out = nan_like((1, Hl, Wl, 16), F16, dev)
    ops.slice_channels(x.to(dev), out, 16, accumulate=False)
    eq(out, G.ref_slice(x, 16, 16), "slice_channels")
    # concat_up_bwd: 56 * 1873 low-resolution pixels * 2 vectors + four times as many skip pixels * 2 vectors = CAP + 304
    Hl, Wl = 56, 1873
    assert Hl * Wl * 2 * 5 == CAP + 304
    dcat = cut((1, 2 * Hl, 2 * Wl, 32))
    da, ds = ops.concat_up_bwd(dcat.to(dev), 16)
    want_a, want_s = G.ref_concat_up_bwd(dcat, 16)
    eq(da, want_a, "concat_up_bwd low")
    eq(ds, want_s, "concat_up_bwd skip")


def test_cap_elementwise(dev):
    from hallucidet_amd import ops
    n = (CAP + 300) * 8
    a, b = cut((n,)), cut((n,), 8)
    eq(ops.add_f16(a.to(dev), b.to(dev)), G.ref_add(a, b), "add")
    eq(ops.relu_bwd(a.to(dev), b.to(dev)), G.ref_relu_bwd(a, b), "relu_bwd")
    n = CAP + 300
    x = cut((n,), 16).float() + 2.0 ** -12                                     # (not representable in fp16: the cast rounds)
    eq(ops.f32_to_f16(x.to(dev), 2.0, dtype=F16), G.ref_f32_to_f16(x, 2.0, F16), "f32_to_f16")
    h = cut((n,), 24)
    eq(ops.f16_to_f32(h.to(dev), 0.5), G.ref_f16_to_f32(h, 0.5), "f16_to_f32")
