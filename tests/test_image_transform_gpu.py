"""hd_image_resample / hd_image_resample_bwd (csrc/image_transform.hip; --detector-resize) on the GPU: the pin to the existing nearest
kernels, run-to-run bits, forward and gradient against float64 references with bounds derived from the arithmetic, the transform class,
and a training step in the antialiased mode (graph replay == eager, the U-Net's gradient == the gradient kernel's)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hallucidet_amd import resample
from hallucidet_amd.resample import resample_taps

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SMALL = [(7, 9, 5, 4), (4, 5, 9, 11), (37, 53, 30, 30), (1, 1, 3, 3)]          # H, W -> Ho, Wo, batches of 2
BIG = (512, 640, 300, 300)
SHAPES = SMALL + [BIG]
SHAPE_IDS = ["%dx%dto%dx%d" % s for s in SHAPES]
STATS = {"trivial": (None, None), "imagenet": (resample.IMAGENET_MEAN, resample.IMAGENET_STD)}
_INPUTS = {}


def _f32(v, default):
    """The statistics as the C boundary receives them: fp32, then exact in float64."""
    return np.array([default] * 3 if v is None else v, dtype=np.float32).astype(np.float64)


def _input(shape, planes):
    """A float32 [2, planes, H, W] batch in [0, 1) (built once per shape, never modified)."""
    key = (shape, planes)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * shape[0] + shape[1] + planes)
        _INPUTS[key] = torch.rand(2, planes, shape[0], shape[1], generator=g)
    return _INPUTS[key]


def _reference(x, shape, mode, stats):
    """float64 on the CPU: normalise, then interpolate.  -> (ref [2, Ho, Wo, 3], bound [2, Ho, Wo, 3]); see test_forward for the bound."""
    H, W, Ho, Wo = shape
    mean, std = _f32(stats[0], 0.0), _f32(stats[1], 1.0)
    xn = (x.double().expand(-1, 3, -1, -1) - torch.from_numpy(mean).view(1, 3, 1, 1)) / torch.from_numpy(std).view(1, 3, 1, 1)
    if mode == "nearest":
        ref = F.interpolate(xn, size=(Ho, Wo), mode="nearest")
    else:
        ref = F.interpolate(xn, size=(Ho, Wo), mode="bilinear", align_corners=False, antialias=(mode == "bilinear_aa"))
    ty, tx = resample_taps(H, Ho, mode), resample_taps(W, Wo, mode)
    a = xn.abs().numpy()
    amax = np.zeros((2, 3, Ho, Wo))
    for i in range(ty.T):
        rows = np.minimum(ty.start + i, H - 1)
        for j in range(tx.T):
            cols = np.minimum(tx.start + j, W - 1)
            live = (i < ty.count)[:, None] & (j < tx.count)[None, :]
            amax = np.maximum(amax, np.where(live, a[:, :, rows][:, :, :, cols], 0.0))
    taps = (ty.count[:, None] * tx.count[None, :]).astype(np.float64)
    ref = ref.permute(0, 2, 3, 1).numpy()
    bound = U * np.abs(ref) + (taps[:, :, None] + 8.0) * 2.0 ** -44 * amax.transpose(0, 2, 3, 1)
    return ref, bound


def _check_forward(y, ref, bound, what):
    assert y.shape[-1] == 8 and (y[..., 3:] == 0).all() and not np.signbit(y[..., 3:].astype(np.float64)).any(), what      # pad channels: +0
    got = y[..., :3]
    if got.dtype == np.float32:
        err = np.abs(got.astype(np.float64) - ref)
        print("%s: max err %.3e, max err / bound %.3f" % (what, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), what
        return
    r = ref.astype(np.float16)                                   # round to nearest even
    rf = r.astype(np.float64)
    lo = np.where(rf <= ref, r, np.nextafter(r, np.float16(-np.inf)))
    hi = np.where(rf >= ref, r, np.nextafter(r, np.float16(np.inf)))
    off = ~((got == lo) | (got == hi))
    if off.any():
        print("%s: %d of %d values are not an fp16 neighbour of the reference; largest |ref| among them %.3e, their bound up to %.3e"
              % (what, off.sum(), off.size, np.abs(ref[off]).max(), bound[off].max()))
    assert not off.any(), what                                   # one of the reference's two fp16 neighbours
    mid = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
    far = (np.abs(ref - mid) > bound) | (lo == hi)
    print("%s: %d of %d values within the bound of a rounding midpoint" % (what, (~far).sum(), far.size))
    assert (got[far] == r[far]).all(), what                      # the correctly rounded one wherever the fp32 error cannot cross a midpoint


def _layouts(x1, x3, dev):
    """name -> (device input, planes of the CPU input it equals)."""
    return {"contiguous": x3.to(dev), "ir_stride0": x1.to(dev).expand(-1, 3, -1, -1)}


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("mode", resample.MODES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_forward_against_float64(dev, dtype, mode, shape):
    """fp32 storage: |y - ref| <= B = 2^-24 * |ref| + (T + 8) * 2^-44 * max |x_norm| over the T = count_y * count_x taps of the pixel.
    The kernel carries every quantity as an unevaluated pair of floats h + l (fp32 instructions, no contraction, fused multiply-adds
    spelled out) and adds the terms in row-major tap order onto -0.  Per term: the weight pair is the float64 weight to 2^-48 (its
    low part is rounded once); the product of two pairs (error-free product of the high parts by one fused multiply-add, the three cross
    terms in fp32) has a relative error below 8 * 2^-48; x - mean is exact (two-sum); the quotient by std is fl(d * fl(1 / std)) plus
    one correction step from the exact remainder, relative error below 4 * 2^-48; a pair addition errs by at most 3 * 2^-48 of the
    magnitudes added.  With non-negative weights that sum to 1 all of it is below (3 T + 24) * 2^-48 * max |x_norm| <
    (T + 8) * 2^-44 * max |x_norm|, the second summand.  What is stored is the high part, which is the pair rounded to fp32: half a unit
    in the last place of the result, at most 2^-24 * |ref| (the first summand; the slack of the second covers ref against the pair).  This is
    far inside the (T + 8) * 2^-24 * max |x_norm| a plain fp32 sum over an fp32 table would need.  The statistics of the reference are the
    fp32 values the C boundary receives.
    fp16 storage: the stored value is fp16(high part), so it is one of the reference's two fp16 neighbours -- down to fp16 subnormals,
    because B is then below 2^-25 (half their spacing) as soon as |ref| < 1 -- and the correctly rounded one wherever the reference is
    farther than B from the midpoint between them."""
    from hallucidet_amd import ops
    H, W, Ho, Wo = shape
    x1, x3 = _input(shape, 1), _input(shape, 3)
    for sname, stats in STATS.items():
        refs = {3: _reference(x3, shape, mode, stats), 1: _reference(x1, shape, mode, stats)}
        for lname, xd in _layouts(x1, x3, dev).items():
            ref, bound = refs[1 if lname == "ir_stride0" else 3]
            if True:                                                  # (one storage type per case)
                what = "%s %s %s %s %s" % (mode, shape, sname, lname, dtype)
                y = ops.image_resample(xd, Ho, Wo, mode, stats[0], stats[1], dtype=dtype)
                assert y.dtype == dtype and tuple(y.shape) == (2, Ho, Wo, 8)
                again = ops.image_resample(xd, Ho, Wo, mode, stats[0], stats[1], dtype=dtype)
                assert torch.equal(y, again), what                                            # the same bits from run to run
                _check_forward(y.cpu().numpy(), ref, bound, what)
                # out=: a slice of a larger batch, its neighbours untouched
                big = torch.full((4, Ho, Wo, 8), 7.0, dtype=dtype, device=dev)
                ops.image_resample(xd, Ho, Wo, mode, stats[0], stats[1], out=big[1:3])
                assert torch.equal(big[1:3], y) and (big[0] == 7).all() and (big[3] == 7).all(), what


def _adjoint(ay, g, ax):
    """ay^T g ax per image and channel: g [N, Ho, Wo, C] -> [N, C, H, W] (float64)."""
    return np.matmul(np.matmul(ay.T, g.transpose(0, 3, 1, 2)), ax)


def _dy(shape, dtype):
    Ho, Wo = shape[2], shape[3]
    g = torch.Generator().manual_seed(77 + Ho * 31 + Wo)
    dy = torch.randn(2, Ho, Wo, 8, generator=g).to(dtype)
    dy[0, 0, 0, :] = 0                                              # a pixel that contributes nothing
    return dy


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("mode", resample.MODES)
def test_gradient_against_float64(dev, mode, shape):
    """dx[n, c, h, w] = fl(acc * fl(gscale * fl(1 / std[c]))), acc = sum_k fl(fl(wy * wx) * g_k) over the F = fan_y[h] * fan_x[w]
    contributing outputs in (output row, output column) order onto acc = 0, g the stored dy taken as exact.  Against
    (gscale / std) * sum_k Wy Wx g_k with the float64 weights a term carries seven roundings (wy, wx, their product; the term; the
    reciprocal, the coefficient, the final scaling) and the F - 1 rounding additions add (F - 1) * 2^-24 of the sum of magnitudes:
    |dx - ref| <= B = (F + 8) * 2^-24 * |gscale / std[c]| * sum_k Wy Wx |g_k|  (the transposed sum of |dy|).  An input pixel no output
    reads gets exactly zero."""
    from hallucidet_amd import ops
    H, W, Ho, Wo = shape
    ty, tx = resample_taps(H, Ho, mode), resample_taps(W, Wo, mode)
    ay, ax = ty.dense(np.float64), tx.dense(np.float64)                                   # [Ho, H], [Wo, W]
    fan = np.diff(ty.rstart)[:, None].astype(np.float64) * np.diff(tx.rstart)[None, :]
    gscale = 0.375
    for dtype in (torch.float16, torch.float32):
        dy = _dy(shape, dtype)
        g64 = dy[..., :3].double().numpy()
        t, tabs = _adjoint(ay, g64, ax), _adjoint(ay, np.abs(g64), ax)
        dyd = dy.to(dev)
        for sname, stats in STATS.items():
            std = _f32(stats[1], 1.0)
            coef = (gscale / std).reshape(1, 3, 1, 1)
            ref, bound = t * coef, (fan + 8.0) * U * np.abs(coef) * tabs
            what = "%s %s %s %s" % (mode, shape, sname, dtype)
            dx = ops.image_resample_bwd(dyd, 2, 3, H, W, mode, stats[1], gscale)
            assert dx.dtype == torch.float32 and tuple(dx.shape) == (2, 3, H, W)
            assert torch.equal(dx, ops.image_resample_bwd(dyd, 2, 3, H, W, mode, stats[1], gscale)), what
            got = dx.cpu().numpy().astype(np.float64)
            err = np.abs(got - ref)
            print("%s: max err %.3e, max err / bound %.3f" % (what, err.max(), (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), what
            assert (got[:, :, fan == 0] == 0).all(), what
        # one channel (the IR plane): the same sums
        dx1 = ops.image_resample_bwd(dyd, 2, 1, H, W, mode, None, gscale)
        assert torch.equal(dx1[:, 0], ops.image_resample_bwd(dyd, 2, 3, H, W, mode, None, gscale)[:, 0])


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_nearest_is_the_existing_kernel_bit_for_bit(dev, shape):
    """mode 'nearest', mean 0 / std 1 through the new pair == ops.nchw_to_nhwc_resize / _bwd, forward and gradient, both storage types,
    contiguous and stride-0 input, with and without explicit trivial statistics."""
    from hallucidet_amd import ops
    H, W, Ho, Wo = shape
    x1, x3 = _input(shape, 1), _input(shape, 3)
    for lname, xd in _layouts(x1, x3 * 2 - 1, dev).items():                 # signed values too
        for dtype in (torch.float16, torch.float32):
            want = ops.nchw_to_nhwc_resize(xd, Ho, Wo, 8, dtype=dtype)
            assert torch.equal(ops.image_resample(xd, Ho, Wo, "nearest", dtype=dtype), want), (lname, dtype)
            assert torch.equal(ops.image_resample(xd, Ho, Wo, "nearest", [0.0], [1.0, 1.0, 1.0], dtype=dtype), want), (lname, dtype)
    for dtype in (torch.float16, torch.float32):
        dyd = _dy(shape, dtype).to(dev)
        for gscale in (1.0, 0.5, 1.0 / 1024):
            want = ops.nchw_to_nhwc_resize_bwd(dyd, 2, 3, H, W, gscale)
            assert torch.equal(ops.image_resample_bwd(dyd, 2, 3, H, W, "nearest", None, gscale), want), (dtype, gscale)
            assert torch.equal(ops.image_resample_bwd(dyd, 2, 3, H, W, "nearest", [1.0], gscale), want), (dtype, gscale)


def test_more_than_three_channels(dev):
    """The eight-channel instance: 5 real channels against the three-channel one run on channel triples."""
    from hallucidet_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 5, 37, 53, generator=g).to(dev)
    y = ops.image_resample(x, 30, 30, "bilinear_aa", dtype=torch.float32)
    assert torch.equal(y[..., :3], ops.image_resample(x[:, :3].contiguous(), 30, 30, "bilinear_aa", dtype=torch.float32)[..., :3])
    assert torch.equal(y[..., 3:5], ops.image_resample(x[:, 3:].contiguous(), 30, 30, "bilinear_aa", dtype=torch.float32)[..., :2])
    assert (y[..., 5:] == 0).all()
    dy = torch.randn(2, 30, 30, 8, generator=g).half().to(dev)
    dx = ops.image_resample_bwd(dy, 2, 5, 37, 53, "bilinear_aa")
    assert torch.equal(dx[:, :3], ops.image_resample_bwd(dy, 2, 3, 37, 53, "bilinear_aa"))


def test_a_new_table_inside_a_capture_is_refused(dev):
    from hallucidet_amd import ops
    x = torch.rand(1, 3, 23, 29, device=dev)
    y = torch.empty(1, 11, 13, 8, dtype=torch.float16, device=dev)
    marker = torch.zeros(8, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="stream capture"):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            marker.add_(1.0)
            ops.image_resample(x, 11, 13, "bilinear", out=y)
    torch.cuda.synchronize()
    want = ops.image_resample(x, 11, 13, "bilinear", dtype=torch.float16)          # eagerly: uploads the tables
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        ops.image_resample(x, 11, 13, "bilinear", out=y)                           # now capturable
    y.zero_()
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)


# ------------------------------------------------------------------------------------------------------------ the class
def _transform(mode, stats=(None, None), size=(30, 24)):
    from hallucidet_amd.models.custom_generalized_transform import CustomGeneralizedRCNNTransform as T
    return T(min_size=30, max_size=30, image_mean=[0.0] if stats[0] is None else list(stats[0]),
             image_std=[1.0] if stats[1] is None else list(stats[1]), size_divisible=1, fixed_size=size, interpolation=mode)


@pytest.mark.parametrize("mode", resample.MODES)
def test_transform_class_runs_the_pair(dev, mode):
    from hallucidet_amd import ops
    stats = STATS["imagenet"]
    t, near = _transform(mode, stats), _transform("nearest")
    Wo, Ho = t.fixed_size
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 37, 53, generator=g).to(dev).requires_grad_(True)
    ir = torch.rand(2, 1, 37, 53, generator=g).to(dev).expand(-1, 3, -1, -1)
    targets = [{"boxes": torch.tensor([[1.0, 2.0, 30.0, 20.0], [4.0, 4.0, 50.0, 36.0]], device=dev), "labels": torch.ones(2, dtype=torch.int64, device=dev)}
               for _ in range(2)]
    il, tg = t(x, targets)
    want = ops.image_resample(x.detach(), Ho, Wo, mode, stats[0], stats[1])
    assert il.tensors.dtype == torch.float16 and torch.equal(il.tensors, want) and il.image_sizes == [(Ho, Wo)] * 2
    _, tg_near = near(x.detach(), targets)
    for a, b in zip(tg, tg_near):
        assert torch.equal(a["boxes"], b["boxes"])                   # the ratio does not depend on the mode
    dy = torch.randn(il.tensors.shape, generator=g).half().to(dev)
    il.tensors.backward(dy)
    assert torch.equal(x.grad, ops.image_resample_bwd(dy, 2, 3, 37, 53, mode, stats[1], 1.0))
    # several batches into one tensor; only the batch that requires a gradient gets one
    x2 = x.detach().clone().requires_grad_(True)
    rgb = torch.rand(2, 3, 37, 53, generator=g).to(dev)
    ilb, tgb = t.forward_batches([x2, rgb, ir], targets * 3)
    assert tuple(ilb.tensors.shape) == (6, Ho, Wo, 8)
    assert torch.equal(ilb.tensors[0:2], want)
    assert torch.equal(ilb.tensors[2:4], ops.image_resample(rgb, Ho, Wo, mode, stats[0], stats[1]))
    assert torch.equal(ilb.tensors[4:6], ops.image_resample(ir, Ho, Wo, mode, stats[0], stats[1]))
    assert len(tgb) == 6 and all(torch.equal(a["boxes"], tg_near[0]["boxes"]) for a in tgb)
    dyb = torch.randn(ilb.tensors.shape, generator=g).half().to(dev)
    ilb.tensors.backward(dyb)
    assert torch.equal(x2.grad, ops.image_resample_bwd(dyb[0:2].contiguous(), 2, 3, 37, 53, mode, stats[1], 1.0))


def test_default_transform_launches_the_kernels_it_always_did(dev, monkeypatch):
    from hallucidet_amd import ops
    t = _transform("nearest")
    monkeypatch.setattr(ops, "image_resample", lambda *a, **k: pytest.fail("the default transform reached hd_image_resample"))
    monkeypatch.setattr(ops, "image_resample_bwd", lambda *a, **k: pytest.fail("the default transform reached hd_image_resample_bwd"))
    x = torch.rand(2, 3, 37, 53, device=dev, requires_grad=True)
    il, _ = t(x, None)
    assert torch.equal(il.tensors, ops.nchw_to_nhwc_resize(x.detach(), 24, 30, 8))
    il.tensors.backward(torch.ones_like(il.tensors))
    ilb, _ = t.forward_batches([x.detach(), x.detach()], None)
    assert torch.equal(ilb.tensors[2:], il.tensors)


# ------------------------------------------------------------------------------------------------------------ a step
H, W = 128, 160


@pytest.fixture(scope="module")
def aa_lit():
    from hallucidet_amd import synthetic
    return synthetic.make_module(seed=5, device="cuda", precision=16, detector_name="fasterrcnn", resize_mode="bilinear_aa")


def _step_outputs(lit, batch):
    lit.use_detector_graph = True
    lit.encoder_decoder.train()
    torch.manual_seed(77)
    imgs_rgb, targets_rgb, imgs_ir, targets_ir = batch
    out = lit.forward_step(imgs_rgb, targets_rgb, imgs_ir, targets_ir, 0, step='train')
    r = lit.encoder_decoder.runner
    r.flat_grads.zero_()
    lit.scaler.scale(out['loss']['total']).backward()
    got = {"total": out['loss']['total'].detach().clone(), "grads": r.flat_grads.clone()}
    for name in ("hall", "rgb", "ir"):
        for i, d in enumerate(lit._last_detections[name]):
            for kk in ("boxes", "scores", "labels"):
                got["%s%d_%s" % (name, i, kk)] = d[kk].clone()
    torch.cuda.synchronize()
    return got


def test_step_in_the_antialiased_mode_replay_equals_eager(dev, aa_lit, monkeypatch):
    """The training step with resize_mode='bilinear_aa' (2 x 128 x 160): the detector graph is keyed by the mode, its replay equals the
    eagerly issued section bit for bit (as tests/test_det_graph_gpu.py asserts for the default), the loss is finite, and the gradient
    handed to the U-Net is hd_image_resample_bwd of the step's own dy -- non-zero on every pixel whose transposed rows meet a non-zero dy."""
    from hallucidet_amd import ops, synthetic
    lit = aa_lit
    assert lit.resize_mode == "bilinear_aa" and lit.detector.transform.interpolation == "bilinear_aa"
    batch = synthetic.make_batch(2, H, W, seed=9, device="cuda")
    _step_outputs(lit, batch)                                      # eager warm-up (uploads the tables), capture, first replay
    g = lit._detector_graph()
    assert g is not None and g.usable and g.captures == 1 and g.replays == 1
    assert any(isinstance(k, tuple) and k and k[0] == "resize" and k[1] == "bilinear_aa" for key in g.entries for k in key if isinstance(k, tuple))
    b = _step_outputs(lit, batch)
    assert g.captures == 1 and g.replays == 2
    assert torch.isfinite(b["total"]).all()
    # the same section eagerly, on the graph's staged targets; the gradient kernel's calls are recorded
    calls = []
    real_bwd = ops.image_resample_bwd

    def recording_bwd(dy, *a, **k):
        dx = real_bwd(dy, *a, **k)
        calls.append((dy.clone(), a, k, dx))
        return dx
    monkeypatch.setattr(ops, "image_resample_bwd", recording_bwd)
    e = next(iter(g.entries.values()))
    lit.use_detector_graph = False
    lit.encoder_decoder.train()
    torch.manual_seed(77)
    imgs_rgb, targets_rgb, imgs_ir, targets_ir = batch
    ir3 = imgs_ir.expand(-1, 3, -1, -1)
    hall = lit.encoder_decoder(ir3)
    handed = []
    hall.register_hook(lambda gr: handed.append(gr.clone()))
    N = hall.shape[0]
    t = [{"boxes": e.tb[i], "labels": e.tl[i], "_rows": e.live[i]} for i in range(3 * N)]
    losses, total, dets = lit._detector_section(hall, imgs_rgb, ir3, t[N:2 * N], t[:N], 'train', False, targets_ir_pass=t[2 * N:])
    r = lit.encoder_decoder.runner
    r.flat_grads.zero_()
    lit.scaler.scale(total).backward()
    torch.cuda.synchronize()
    assert torch.equal(total, b["total"]) and torch.isfinite(total).all()
    assert torch.isfinite(r.flat_grads).all() and float(r.flat_grads.abs().max()) > 0
    assert torch.equal(r.flat_grads, b["grads"])
    for name, dd in zip(("hall", "rgb", "ir"), dets):
        for i, d in enumerate(dd):
            for kk in ("boxes", "scores", "labels"):
                assert torch.equal(d[kk], b["%s%d_%s" % (name, i, kk)]), (name, i, kk)
    # one gradient launch (the hallucinated batch alone requires one), its result is what reaches the U-Net
    assert len(calls) == 1 and len(handed) == 1
    dy, a, k, dx = calls[0]
    assert tuple(dy.shape) == (N, 300, 300, 8) and a[:4] == (N, 3, H, W) and a[4] == "bilinear_aa"
    monkeypatch.setattr(ops, "image_resample_bwd", real_bwd)
    assert torch.equal(handed[0], dx) and torch.equal(dx, ops.image_resample_bwd(dy, N, 3, H, W, "bilinear_aa", None, 1.0))
    # coverage: wherever the transposed rows meet a non-zero dy the gradient is non-zero
    ty, tx = resample_taps(H, 300, "bilinear_aa"), resample_taps(W, 300, "bilinear_aa")
    my, mx = (ty.dense(np.float32) != 0).astype(np.float64), (tx.dense(np.float32) != 0).astype(np.float64)
    nz = (dy[..., :3] != 0).double().cpu().numpy()
    reach = _adjoint(my, nz, mx) > 0
    got = dx.cpu().numpy()
    assert reach.any() and (got[reach] != 0).all()
    assert (got[~reach] == 0).all()
    print("share of pixels with a detector gradient: %.2f %%" % (100.0 * (got != 0).mean()))


@pytest.mark.parametrize("mode", resample.MODES)
def test_detector_lit_validation_step_runs_in_each_mode(dev, mode):
    from hallucidet_amd import synthetic
    from hallucidet_amd.models.detector import Detector
    from hallucidet_amd.train_detector import DetectorLit
    torch.manual_seed(41)
    det = Detector(name="fasterrcnn", pretrained=False, n_classes=2, size=300).detector.to(dev)
    rgb, trgb, _, _ = synthetic.make_batch(2, H, W, seed=9, device=str(dev))
    lit = DetectorLit(batch_size=2, lr=1e-4, detector_name="fasterrcnn", pretrained=False, detector=det, device=str(dev), modality="rgb",
                      resize_mode=mode, image_mean=list(resample.IMAGENET_MEAN), image_std=list(resample.IMAGENET_STD))
    assert lit.resize_mode == mode and lit.detector.transform.interpolation == mode and not lit.detector.transform._legacy
    il, _ = lit.detector.transform(rgb, None)
    lit.detector.backbone.calibrate_(il.tensors)
    lit.prepare()
    loss = lit.validation_step((rgb, trgb), 0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


def test_scripts_take_the_flags(dev, tmp_path, capsys, monkeypatch):
    """--detector-resize / --detector-norm reach the running modules: one epoch of train_hallucidet.py in the antialiased mode and of
    train_detector.py with ImageNet statistics on a synthetic LLVIP tree."""
    import os
    import sys
    from _synth_llvip import make_tree
    from hallucidet_amd import ops
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    monkeypatch.chdir(tmp_path)
    root = make_tree(tmp_path, n_train=2, n_test=2, hw=(64, 96), extra_objects=False)
    import train_detector
    import train_hallucidet
    modes = []
    real = ops.image_resample
    monkeypatch.setattr(ops, "image_resample", lambda x, Ho, Wo, mode, mean=None, std=None, **k: (modes.append((mode, mean)), real(x, Ho, Wo, mode, mean, std, **k))[1])
    common = ["--dataset", "llvip", "--train", root, "--test", root, "--ext", ".jpg", "--batch", "2", "--num-workers", "0", "--seed", "3"]
    train_hallucidet.main(common + ["--detector", "fasterrcnn", "--epochs", "1", "--precision", "16", "--wandb-name", "r1", "--detector-resize", "bilinear_aa"])
    out = capsys.readouterr().out
    assert "HalluciDet   on IR  AP@50:" in out and modes and all(m == ("bilinear_aa", (0.0, 0.0, 0.0)) for m in modes)
    del modes[:]
    train_detector.main(common + ["--detector", "fasterrcnn", "--modality", "rgb", "--epochs", "1", "--wandb-name", "r2", "--detector-norm", "imagenet"])
    out = capsys.readouterr().out
    assert "test:" in out and modes and all(m == ("nearest", resample.IMAGENET_MEAN) for m in modes)
