"""The definitions of tests/_glue_reference.py are the operations they claim to be: checked here, without a GPU, against ATen's own
max_pool2d / interpolate(mode='nearest') / cat and their float64 autograd, at the shapes and size pairs test_glue_kernels_gpu.py uses."""
import pytest
import torch
import torch.nn.functional as F

import _glue_reference as G

POOL_HW = [(1, 1), (1, 8), (2, 3), (5, 4), (3, 2), (4, 7), (7, 5), (16, 3), (2, 16), (16, 16)]


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def pool_inputs(seed, shape):
    yield "negative", G.grid_inputs(seed, shape, torch.float16, negative=True)
    yield "ties", G.grid_inputs(seed + 1, shape, torch.float16, levels=4)
    yield "ties-negative", G.grid_inputs(seed + 2, shape, torch.float16, levels=3, negative=True)
    yield "relu", torch.relu(G.grid_inputs(seed + 3, shape, torch.float16))
    yield "wild", G.wild_inputs(seed + 4, shape, torch.float16)


def aten_positions(ind, H, W):
    """ATen's flat h*W + w argmax of each 3x3 / stride-2 / pad-1 window (NCHW) -> the window position kh*3 + kw (NHWC)."""
    N, C, Ho, Wo = ind.shape
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    kh, kw = ind // W - (2 * ho - 1), ind % W - (2 * wo - 1)
    assert int(kh.min()) >= 0 and int(kh.max()) <= 2 and int(kw.min()) >= 0 and int(kw.max()) <= 2
    return nhwc(kh * 3 + kw).to(torch.uint8)


@pytest.mark.parametrize("hw", POOL_HW, ids=lambda v: "%dx%d" % v)
def test_ref_maxpool_is_atens_max_pool2d_values_indices_and_gradient(hw):
    H, W = hw
    for C in (8, 24):
        for kind, x in pool_inputs(100 * H + W + C, (2, H, W, C)):
            xv = nchw(x.double()).requires_grad_(True)
            want, ind = F.max_pool2d(xv, 3, 2, 1, return_indices=True)
            y, pos = G.ref_maxpool(x)
            assert y.dtype == x.dtype and torch.equal(y.double(), nhwc(want.detach())), (kind, C)
            assert torch.equal(pos, aten_positions(ind, H, W)), (kind, C)
            dy = G.grid_inputs(H + W, y.shape, torch.float16)
            want.backward(nchw(dy.double()))
            routed, mag = G.ref_maxpool_bwd_terms(pos, dy, H, W)
            assert torch.equal(routed, nhwc(xv.grad)), (kind, C)
            assert torch.equal(mag.sum(), dy.double().abs().sum())
            add = G.grid_inputs(H + W + 1, x.shape, torch.float16)
            assert torch.equal(G.ref_maxpool_bwd(pos, dy, H, W), routed.half())
            assert torch.equal(G.ref_maxpool_bwd(pos, dy, H, W, add=add), (routed.half().double() + add.double()).half())


def test_two_roundings_of_the_add_form_differ_from_one():
    """A case that tells f16(f16(routed) + add) from f16(routed + add): one pixel wins four windows whose gradients sum to 2049, a tie
    of fp16's spacing-2 range."""
    x = torch.zeros(1, 3, 3, 8, dtype=torch.float16)
    x[0, 1, 1] = 1.0                                                    # pixel (1, 1) wins all four windows
    y, pos = G.ref_maxpool(x)
    dy = torch.tensor([1024.0, 1024.0, 1.0, 0.0], dtype=torch.float16).view(1, 2, 2, 1).expand(1, 2, 2, 8).contiguous()
    add = torch.full((1, 3, 3, 8), 1.0, dtype=torch.float16)
    got = G.ref_maxpool_bwd(pos, dy, 3, 3, add=add)
    assert float(got[0, 1, 1, 0]) == 2048.0                             # f16(2049) = 2048 (tie to even), f16(2048 + 1) = 2048
    assert float(torch.tensor(2049.0 + 1.0, dtype=torch.float64).half()) == 2050.0


@pytest.mark.parametrize("pair", sorted(set(G.ALL_PAIRS)), ids=lambda p: "%dto%d" % p)
def test_nn_index_is_what_interpolate_picks(pair):
    """float32 images: ATen's CPU forward forms the scale in the image's own type, so on SOME shapes a float64 image is resized by a
    float64 scale (the exact index at these sizes) while ATen's backward, and every float32 call, use the fp32 rule the kernels claim."""
    inp, out = pair
    img = torch.arange(inp, dtype=torch.float32).view(1, 1, inp, 1)
    got = F.interpolate(img, size=(out, 1), mode="nearest").view(-1).long()
    assert torch.equal(got, G.nn_index(out, inp))
    got_w = F.interpolate(img.view(1, 1, 1, inp), size=(1, out), mode="nearest").view(-1).long()
    assert torch.equal(got_w, G.nn_index(out, inp))
    both = F.interpolate((img * 4096 + img.view(1, 1, 1, inp)).expand(2, 3, inp, inp).contiguous(), size=(out, out), mode="nearest")[1, 2].long()
    assert torch.equal(both, G.nn_index(out, inp).view(-1, 1) * 4096 + G.nn_index(out, inp).view(1, -1))


@pytest.mark.parametrize("pair", G.DIVERGENT_PAIRS, ids=lambda p: "%dto%d" % p)
def test_divergent_pairs_really_diverge(pair):
    inp, out = pair
    assert not torch.equal(G.nn_index(out, inp), G.exact_index(out, inp))


def test_identity_and_integer_factor_pairs_do_not_diverge():
    for inp, out in [(7, 7), (5, 10), (1, 3), (1, 5), (5, 1), (6, 6)]:
        assert torch.equal(G.nn_index(out, inp), G.exact_index(out, inp)), (inp, out)


def _mixed(pairs):
    """(H, Ho, W, Wo): each pair on the H axis with the next one on the W axis."""
    return [(a[0], a[1], b[0], b[1]) for a, b in zip(pairs, pairs[1:] + pairs[:1])]


@pytest.mark.parametrize("case", _mixed(G.RESIZE_PAIRS), ids=lambda c: "%dto%d_%dto%d" % c)
def test_ref_resize_and_its_adjoint_are_interpolate_and_its_autograd(case):
    H, Ho, W, Wo = case
    for Cr, Cp in [(1, 8), (3, 8), (8, 8), (3, 16)]:
        x = G.grid_inputs(H + W + Cr, (2, Cr, H, W), torch.float32)
        want = F.interpolate(x, size=(Ho, Wo), mode="nearest")                  # float32: see test_nn_index_is_what_interpolate_picks
        y = G.ref_resize_fwd(x, Ho, Wo, Cp, torch.float16)
        assert torch.equal(y[..., :Cr].double(), nhwc(want).double()) and not y[..., Cr:].any()
        dy = G.grid_inputs(Ho + Wo + Cr, (2, Ho, Wo, Cp), torch.float16)
        xv = x.double().requires_grad_(True)
        F.interpolate(xv, size=(Ho, Wo), mode="nearest").backward(nchw(dy.double())[:, :Cr])
        for gs in (1.0, 0.5):
            dx, mag = G.ref_resize_bwd_terms(dy, 2, Cr, H, W, gs)
            assert torch.equal(dx, gs * xv.grad), (Cr, Cp, gs)
            assert torch.equal(mag.sum(), gs * dy[..., :Cr].double().abs().sum())
        assert torch.equal(G.ref_nhwc_to_nchw(y, Cr), want)


@pytest.mark.parametrize("case", _mixed(G.UPSAMPLE_PAIRS), ids=lambda c: "%dto%d_%dto%d" % c)
def test_ref_upsample_add_and_its_adjoint(case):
    Hb, H, Wb, W = case
    a, b = G.grid_inputs(H + W, (2, H, W, 8), torch.float16), G.grid_inputs(Hb + Wb, (2, Hb, Wb, 8), torch.float16)
    up = F.interpolate(nchw(b.float()), size=(H, W), mode="nearest")            # float32: see test_nn_index_is_what_interpolate_picks
    assert torch.equal(G.ref_upsample_add(a, b), (a.double() + nhwc(up).double()).half())
    dy = G.grid_inputs(H * W, (2, H, W, 8), torch.float16)
    bv = nchw(b.double()).requires_grad_(True)
    F.interpolate(bv, size=(H, W), mode="nearest").backward(nchw(dy.double()))
    s, mag = G.ref_upsample_add_bwd_terms(dy, Hb, Wb)
    assert torch.equal(s, nhwc(bv.grad)) and torch.equal(mag.sum(), dy.double().abs().sum())
    prev = G.grid_inputs(Hb * Wb, (2, Hb, Wb, 8), torch.float16)
    assert torch.equal(G.ref_upsample_add_bwd(dy, Hb, Wb, prev), (nhwc(bv.grad) + prev.double()).half())


@pytest.mark.parametrize("shape", [(1, 1, 1, 8, 0), (2, 3, 5, 8, 8), (1, 11, 13, 24, 16), (2, 2, 1, 16, 24)])
def test_ref_concat_up_bwd_is_the_autograd_of_interpolate_and_cat(shape):
    N, Hl, Wl, Cup, Cskip = shape
    a = torch.zeros(N, Cup, Hl, Wl, dtype=torch.float64, requires_grad=True)
    skip = torch.zeros(N, Cskip, 2 * Hl, 2 * Wl, dtype=torch.float64, requires_grad=True)
    cat = torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), skip], dim=1)
    dcat = G.grid_inputs(Hl * Wl + Cup, (N, 2 * Hl, 2 * Wl, Cup + Cskip), torch.float16)
    cat.backward(nchw(dcat.double()))
    da, ds = G.ref_concat_up_bwd(dcat, Cup)
    assert torch.equal(da.double(), nhwc(a.grad).half().double())
    if Cskip:
        assert torch.equal(ds.double(), nhwc(skip.grad))
    else:
        assert ds is None
    # the pieces it is made of, at a channel offset and accumulating
    prev = G.grid_inputs(7, da.shape, torch.float16)
    assert torch.equal(G.ref_upsample2_bwd(dcat, 0, Cup, prev), (nhwc(a.grad) + prev.double()).half())
    if Cskip:
        prev = G.grid_inputs(8, ds.shape, torch.float16)
        assert torch.equal(G.ref_slice(dcat, Cup, Cskip, prev), (nhwc(skip.grad) + prev.double()).half())


def test_ref_subsample2_is_a_strided_slice_and_its_autograd():
    for H, W in [(1, 1), (1, 2), (2, 5), (5, 10), (10, 1)]:
        x = G.grid_inputs(H * W, (2, H, W, 8), torch.float16)
        xv = x.double().requires_grad_(True)
        y = xv[:, ::2, ::2]
        assert torch.equal(G.ref_subsample2(x).double(), y.detach())
        dy = G.grid_inputs(H + W, y.shape, torch.float16)
        y.backward(dy.double())
        assert torch.equal(G.ref_subsample2_bwd(dy, H, W).double(), xv.grad)
        prev = G.grid_inputs(H + W + 1, x.shape, torch.float16)
        assert torch.equal(G.ref_subsample2_bwd(dy, H, W, prev), (xv.grad + prev.double()).half())


def test_ref_sigmoid_bwd_is_the_autograd_of_sigmoid():
    logit = torch.randn(2, 3, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(0), requires_grad=True)
    s = torch.sigmoid(logit)
    dy = torch.randn(2, 3, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    (s * dy).sum().backward()
    got = G.ref_sigmoid_bwd(dy, s.detach(), 8, 4.0)
    assert torch.allclose(got[..., :3], 4.0 * nhwc(logit.grad), rtol=1e-12, atol=0) and not got[..., 3:].any()


@pytest.mark.parametrize("k", [9, 17, 170])
def test_grid_sums_are_exact_in_fp32_in_any_order(k):
    """The claim behind torch.equal on grid data: a serial fp32 sum of k grid values, forwards and backwards, is the float64 sum."""
    for dtype in (torch.float16, torch.float32):
        for kw in ({}, {"levels": 4}, {"negative": True}):
            t = G.grid_inputs(k, (4096, k), dtype, **kw)
            assert torch.equal(t.double() * 64, (t.double() * 64).round()) and float(t.abs().max()) <= 16.0
            fwd = torch.zeros(4096, dtype=torch.float32)
            rev = torch.zeros(4096, dtype=torch.float32)
            for j in range(k):
                fwd = fwd + t[:, j].float()
                rev = rev + t[:, k - 1 - j].float()
            want = t.double().sum(1)
            assert torch.equal(fwd.double(), want) and torch.equal(rev.double(), want)


def test_fused_cast_reference_rounds_the_exact_product_once():
    x = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -23, 1.5 * 2.0 ** -24, 3.0, 210000.0], dtype=torch.float32)
    # 1 + 2^-11 + 2^-23 lies above fp16's tie, and stays there in fp32: both roundings give 1 + 2^-10 at scale 1
    assert torch.equal(G.ref_f32_to_f16_fused(x, 1.0, torch.float16), G.ref_f32_to_f16(x, 1.0, torch.float16))
    assert torch.equal(G.ref_f32_to_f16_fused(x, 2.0, torch.float16), G.ref_f32_to_f16(x, 2.0, torch.float16))
    # 1.5 * 2^-24 * f32(1/3) = 2^-25 * (1 + 2^-25): above the tie between 0 and 2^-24 exactly, ON it after the fp32 rounding
    one, two = G.ref_f32_to_f16_fused(x, 1.0 / 3.0, torch.float16), G.ref_f32_to_f16(x, 1.0 / 3.0, torch.float16)
    assert float(one[1]) == 2.0 ** -24 and float(two[1]) == 0.0 and torch.equal(one[2:], two[2:]) and bool(one[3].isinf())
    assert torch.equal(G.ref_f32_to_f16_fused(x, 1.0 / 3.0, torch.float32), G.ref_f32_to_f16(x, 1.0 / 3.0, torch.float32))


def test_grid_levels_and_negative_options():
    t = G.grid_inputs(3, (1000,), torch.float16, levels=4)
    assert t.unique().numel() <= 4
    n = G.grid_inputs(3, (1000,), torch.float16, negative=True)
    assert float(n.max()) < 0 and float(n.min()) >= -16


def test_wild_inputs_hold_the_values_they_promise():
    for dtype in (torch.float16, torch.float32):
        t = G.wild_inputs(5, (4000,), dtype)
        assert bool(torch.isfinite(t).all())
        d = t.double()
        assert bool(((d != 0) & (d.abs() < 2.0 ** -14)).any()), "fp16 subnormals"
        assert bool((d == 0).any()) and bool((d == 65504).any()) and bool((d == -65504).any())
        assert bool((d > 0).any()) and bool((d < 0).any())
        assert float(G.wild_inputs(5, (4000,), dtype, max_abs=2048.0).abs().max()) == 2048.0
