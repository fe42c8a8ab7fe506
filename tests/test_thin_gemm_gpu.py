"""gemm_thin.hip -- the LDS-free streaming kernels for the detector's thin 1x1 problems -- against the implicit-GEMM routes they replace
(hd_thin_gemm_mode(0)): every output BIT FOR BIT (same MFMA instruction, same chunk order, the same rounding points), at the loop
edges of both kernels; one case against an fp64 product; one small training step, eager and as a hipGraph replay."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

M_EDGES = (1, 31, 32, 33, 95)          # below / at / past one 32-row group, three groups with a ragged last one


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


@pytest.fixture
def thin(dev):
    from hallucidet_amd import ops
    try:
        yield ops
    finally:
        ops.thin_gemm_mode(-1)


def _route_family(ops, x, w, cout, nchw):
    import ctypes as C
    from hallucidet_amd import _abi
    N, H, W, K = x.shape
    P = 0x1000
    a = _abi.ConvArgs(P, None, P, P, None, None, P, None, N, H, W, H, W, K, 0, H, W, cout, 1, 1, 1, 0, 0, 1, 0, 1 if nchw else 2, None, None, 0, 0)
    out = (C.c_int32 * 8)()
    ops.check(_abi.load().hd_conv2d_route(C.byref(a), out), "hd_conv2d_route")
    return out[0]


def _heads(ops, x, ws, biases, couts, nchw):
    kws = [dict(bias=b, cout=c, **({"out_nchw_f32": True} if nchw else {"out_nhwc_f32": True})) for b, c in zip(biases, couts)]
    return ops.conv2d_multi([(x, w, 1, 1, kw) for w, kw in zip(ws, kws)])


def test_forward_pairs_and_single_heads_bit_for_bit(thin, dev):
    """M at the 32-row edges, K with a half chunk (8, 24, 72), a tail that is no multiple of 64 and the long chain (1024), the channel pairs of
    the RPN head and the predictor and the fullest pair (15 + 16 = 32 rows), with / without bias, NHWC fp32 and the Ho * Wo = 1 NCHW form."""
    ops = thin
    checked = 0
    for K in (8, 24, 64, 72, 256, 1024):
        for ca, cb in ((1, 4), (2, 8), (3, 12), (15, 16)):
            wa = rnd(ca, K, scale=1.0 / math.sqrt(K), seed=K + ca).to(dev)
            wb = rnd(cb, K, scale=1.0 / math.sqrt(K), seed=K + cb + 100).to(dev)
            ba, bb = torch.randn(ca, generator=torch.Generator().manual_seed(4)).to(dev), torch.randn(cb, generator=torch.Generator().manual_seed(5)).to(dev)
            for M in M_EDGES:
                for nchw in (False, True):
                    x = rnd(M, 1, 1, K, seed=M + K).to(dev) if nchw else rnd(1, 1, M, K, seed=M + K).to(dev)
                    for bias in (True, False):
                        bs = [ba, bb] if bias else [None, None]
                        ops.thin_gemm_mode(0)
                        assert _route_family(ops, x, wa, ca, nchw) == 8
                        ref = _heads(ops, x, [wa, wb], bs, [ca, cb], nchw)
                        ops.thin_gemm_mode(-1)
                        assert _route_family(ops, x, wa, ca, nchw) == 10
                        got = _heads(ops, x, [wa, wb], bs, [ca, cb], nchw)
                        one = ops.conv2d(x, wb, 1, 1, bias=bs[1], cout=cb, out_nchw_f32=nchw, out_nhwc_f32=not nchw)      # a single unpaired head
                        for g, r in zip(got, ref):
                            assert g.dtype == torch.float32 and g.shape == r.shape
                            assert torch.equal(g, r), (M, K, ca, cb, nchw, bias, float((g - r).abs().max()))
                        assert torch.equal(one, ref[1]), (M, K, cb, nchw, bias)
                        checked += 1
    assert checked == 6 * 4 * 5 * 2 * 2


def test_forward_pair_that_does_not_fit_one_operand_and_relu(thin, dev):
    """16 + 16 + 12 channels over one input: the first two share an operand (32 rows), the third runs unpaired in the same grid; ReLU in the
    epilogue; a member the kernel does not implement (f16 output) keeps its route inside the same hd_conv2d_multi call."""
    ops = thin
    K, M = 72, 95
    x = rnd(1, 5, 19, K, seed=1).to(dev)
    ws = [rnd(c, K, scale=0.2, seed=c + i).to(dev) for i, c in enumerate((16, 16, 12))]
    bs = [torch.randn(c, generator=torch.Generator().manual_seed(7 + i)).to(dev) for i, c in enumerate((16, 16, 12))]
    w16 = rnd(16, K, scale=0.2, seed=9).to(dev)

    def run():
        calls = [(x, w, 1, 1, dict(bias=b, act=1, out_nhwc_f32=True)) for w, b in zip(ws, bs)] + [(x, w16, 1, 1, dict(bias=bs[0]))]
        return ops.conv2d_multi(calls)
    ops.thin_gemm_mode(0)
    ref = run()
    ops.thin_gemm_mode(1)
    got = run()
    assert got[3].dtype == torch.float16 and M == x.shape[1] * x.shape[2]
    for g, r in zip(got, ref):
        assert torch.equal(g, r)
    assert float(got[0].min()) == 0.0 and float(got[0].max()) > 0


def test_forward_five_levels_in_one_grid(thin, dev):
    """[cls] * 5 + [box] * 5 over five maps of 2 images (13^2 .. 1^2: problems smaller than one 32-row group) as hd_conv2d_multi pairs them."""
    ops = thin
    K = 256
    wa, wb = rnd(8, K, scale=1.0 / 16, seed=2).to(dev), rnd(16, K, scale=1.0 / 16, seed=3).to(dev)
    ba, bb = torch.randn(3, generator=torch.Generator().manual_seed(4)).to(dev), torch.randn(12, generator=torch.Generator().manual_seed(5)).to(dev)
    xs = [rnd(2, s, s, K, seed=10 + s).to(dev) for s in (13, 7, 4, 2, 1)]

    def run():
        calls = [(x, wa, 1, 1, dict(bias=ba, cout=3, out_nhwc_f32=True)) for x in xs] + [(x, wb, 1, 1, dict(bias=bb, cout=12, out_nhwc_f32=True)) for x in xs]
        return ops.conv2d_multi(calls)
    ops.thin_gemm_mode(0)
    ref = run()
    ops.thin_gemm_mode(-1)
    got = run()
    assert len(got) == 10
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def _pair_reference(ops, ga, gb, wda, wdb, mask):
    """today's route: two pad-and-casts, the first head's data gradient, the second's with `res` and `mask`"""
    n, H, W, _ = ga.shape
    a16 = ops.pad_cast_f32_f16(ga, wda.shape[1], dtype=torch.float16)
    b16 = ops.pad_cast_f32_f16(gb, wdb.shape[1], dtype=torch.float16)
    d = ops.conv2d(a16, wda, 1, 1, cout=wda.shape[0])
    return ops.conv2d(b16, wdb, 1, 1, cout=wdb.shape[0], res=d, mask=mask), a16, b16


@pytest.mark.parametrize("C", [32, 256, 1024])
def test_gradient_pair_bit_for_bit(thin, dev, C):
    """(Ka, Kb) of the predictor and of the RPN head, with / without the mask, M at the 32-row edges (one image of M pixels, and M images of
    one pixel: the predictor's form), fp32 gradients and the already padded f16 variant."""
    ops = thin
    ops.thin_gemm_mode(0)          # the reference launches are those of the implicit-GEMM family
    for Ka, Kb in ((2, 8), (3, 12)):
        Kap, Kbp = (Ka + 7) // 8 * 8, (Kb + 7) // 8 * 8
        wda, wdb = rnd(C, Kap, scale=0.3, seed=C + Ka).to(dev), rnd(C, Kbp, scale=0.3, seed=C + Kb).to(dev)
        for M in M_EDGES:
            for shape in ((1, 1, M), (M, 1, 1)):
                ga = torch.randn(*shape, Ka, generator=torch.Generator().manual_seed(M + Ka)).to(dev)
                gb = torch.randn(*shape, Kb, generator=torch.Generator().manual_seed(M + Kb + 50)).to(dev)
                for use_mask in (True, False):
                    mask = (torch.rand(*shape, C, generator=torch.Generator().manual_seed(6)) > 0.4).half().to(dev) if use_mask else None
                    ref, a16, b16 = _pair_reference(ops, ga, gb, wda, wdb, mask)
                    got = ops.thin_dgrad_pair_many([(ga, gb, wda, wdb, mask)])[0]
                    got16 = ops.thin_dgrad_pair_many([(a16, b16, wda, wdb, mask)])[0]
                    assert got.dtype == torch.float16 and got.shape == ref.shape
                    assert torch.equal(got, ref), (C, Ka, Kb, M, shape, use_mask, float((got.float() - ref.float()).abs().max()))
                    assert torch.equal(got16, ref), (C, Ka, Kb, M, shape, use_mask)


def test_gradient_pair_slices_zero_rows_and_levels_in_one_grid(thin, dev):
    """Gradients as the [:n_active] slice of a larger buffer (image stride > H * W * K), rows that are all zero (the label -1 padding rows),
    and five levels in one launch against the per-level reference."""
    ops = thin
    ops.thin_gemm_mode(0)
    C, Ka, Kb = 256, 3, 12
    wda, wdb = rnd(C, 8, scale=0.3, seed=1).to(dev), rnd(C, 16, scale=0.3, seed=2).to(dev)
    calls, refs = [], []
    for s in (13, 7, 4, 2, 1):
        big_a = torch.randn(3, s * s * Ka + 5 * Ka, generator=torch.Generator().manual_seed(s)).to(dev)
        big_b = torch.randn(3, s * s * Kb + 5 * Kb, generator=torch.Generator().manual_seed(s + 20)).to(dev)
        ga = big_a[:2, :s * s * Ka].view(2, s, s, Ka)
        gb = big_b[:2, :s * s * Kb].view(2, s, s, Kb)
        ga[1, s // 2] = 0
        gb[1, s // 2] = 0
        assert s == 1 or (ga.stride(0) > s * s * Ka and not ga.is_contiguous())
        mask = (torch.rand(2, s, s, C, generator=torch.Generator().manual_seed(6 + s)) > 0.5).half().to(dev)
        refs.append(_pair_reference(ops, ga, gb, wda, wdb, mask)[0])
        calls.append((ga, gb, wda, wdb, mask))
    got = ops.thin_dgrad_pair_many(calls)
    for g, r in zip(got, refs):
        assert torch.equal(g, r)
    assert float(got[0][1, 13 // 2].abs().max()) == 0.0 and float(got[0].abs().max()) > 0


def test_against_fp64_products_of_the_rounded_operands(thin, dev):
    """Forward: fp32 output of a K = 1024 chain against the fp64 product of the f16 operands -- the fp32 accumulation error bound K * 2^-24
    * sum |x w| (each of the K additions rounds once, relative 2^-24).  Gradient pair: the output is ONE f16 rounding of the exact sum
    apart from the first product's own f16 rounding, so |got - exact| <= 2^-11 |exact| + 2^-11 |first| + 2^-24 (subnormal step), plus the
    (negligible, K <= 16) accumulation term bounded the same way."""
    ops = thin
    ops.thin_gemm_mode(1)
    M, K = 95, 1024
    x, w = rnd(1, 1, M, K, seed=1).to(dev), rnd(8, K, scale=1.0 / 32, seed=2).to(dev)
    b = torch.randn(8, generator=torch.Generator().manual_seed(3)).to(dev)
    got = ops.conv2d(x, w, 1, 1, bias=b, out_nhwc_f32=True).double().view(M, 8)
    xd, wd = x.double().view(M, K), w.double()
    want = xd @ wd.t() + b.double()
    bound = K * 2.0 ** -24 * (xd.abs() @ wd.abs().t() + b.double().abs()) + 1e-30
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())

    C, Ka, Kb = 256, 3, 12
    wda, wdb = rnd(C, 8, scale=0.3, seed=1).to(dev), rnd(C, 16, scale=0.3, seed=2).to(dev)
    ga = torch.randn(1, 1, M, Ka, generator=torch.Generator().manual_seed(4)).to(dev)
    gb = torch.randn(1, 1, M, Kb, generator=torch.Generator().manual_seed(5)).to(dev)
    got = ops.thin_dgrad_pair_many([(ga, gb, wda, wdb, None)])[0].double().view(M, C)
    a16, b16 = ga.half().double().view(M, Ka), gb.half().double().view(M, Kb)
    first = a16 @ wda.double()[:, :Ka].t()
    second = b16 @ wdb.double()[:, :Kb].t()
    want = first + second
    mag = a16.abs() @ wda.double()[:, :Ka].abs().t() + b16.abs() @ wdb.double()[:, :Kb].abs().t()
    bound = 2.0 ** -11 * want.abs() + 2.0 ** -11 * first.abs() + 2.0 ** -24 + 16 * 2.0 ** -24 * mag
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())


def _lit(seed=5):
    from hallucidet_amd import synthetic
    return synthetic.make_module(seed=seed, device="cuda", precision=16, detector_name="fasterrcnn")


def _step_outputs(lit, batch, graph):
    lit.use_detector_graph = graph
    lit.encoder_decoder.train()
    torch.manual_seed(77)
    imgs_rgb, targets_rgb, imgs_ir, targets_ir = batch
    out = lit.forward_step(imgs_rgb, targets_rgb, imgs_ir, targets_ir, 0, step='train')
    r = lit.encoder_decoder.runner
    r.flat_grads.zero_()
    lit.scaler.scale(out['loss']['total']).backward()
    got = {"total": out['loss']['total'].detach().clone(), "grads": r.flat_grads.clone()}
    for k in ('det_regression', 'det_classification', 'det_objectness', 'det_rpn_box_reg'):
        v = out['loss'][k]
        got[k] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(float(v))
    for name in ("hall", "rgb", "ir"):
        for i, d in enumerate(lit._last_detections[name]):
            for kk in ("boxes", "scores", "labels"):
                got["%s%d_%s" % (name, i, kk)] = d[kk].clone()
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("graph", [False, True])
def test_training_step_is_unchanged(thin, dev, graph):
    """One two-image Faster R-CNN training step at 128 x 160 with the thin kernels off and on: losses, the gradient that reaches the U-Net's
    parameters through the image, and the three passes' detections equal -- issued eagerly and as the detector hipGraph's replay."""
    from hallucidet_amd import synthetic
    ops = thin
    batch = synthetic.make_batch(2, 128, 160, seed=9, device="cuda")
    outs = []
    for mode in (0, -1):
        ops.thin_gemm_mode(mode)
        assert ops.thin_gemm_on() == (mode != 0)
        lit = _lit()
        if graph:
            _step_outputs(lit, batch, True)          # captures after two eager warm-up runs
            g = lit._detector_graph()
            assert g is not None and g.usable and g.captures == 1
        outs.append(_step_outputs(lit, batch, graph))
        if graph:
            assert g.captures == 1 and g.replays == 2
    a, b = outs
    assert set(a) == set(b) and float(b["grads"].abs().max()) > 0 and bool(torch.isfinite(b["grads"]).all())
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
