"""The IR pre-processing baselines on the GPU (hd_ir_preprocess, csrc/ir_preprocess.hip) against the torch-CPU oracle
(tests/_ir_preprocess_oracle.py, itself pinned to the reference's own output by tests/test_ir_preprocess_cpu.py).

What "equal" means here:
  * invert, equalization and their chains are single IEEE fp32 operations on exact integer statistics: bit-equal to the oracle on
    every input;
  * stretching: the two neighbours the quantile interpolates between must be the exact sorted input elements, so q lies inside
    [s_lo, s_hi] and equals them bit for bit when they tie (as nearly all do on k/255 images of more than a few hundred pixels; q
    and the image must be the oracle's bits there); where they differ, ATen's CPU lerp is not reproducible to the bit (fused or not,
    either branch), every form being two roundings from the exact value: q within 2 ulp of torch.quantile.  The image is always the
    reference's arithmetic evaluated with the REPORTED quantiles, bit for bit;
  * blur: nine products and eight sums at 2^-24 relative each is <= 1.0e-6 per side, summation order free on both sides:
    |kernel - F.conv2d| <= 2e-6 * max(1, max|input|) against the conv of the kernel's own (separately verified) input stage."""
import os

import numpy as np
import pytest
import torch

import _ir_preprocess_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 3, 512, 640), (8, 1, 512, 640), (2, 3, 127, 161), (1, 3, 2, 2)]
EXACT = ("invert", "equalization", "invert_equalization", "parallel")
STRETCH = (("stretching", False), ("invert_stretching", True))
BLUR = ("blur", "invert_stretching_blur", "invert_equalization_blur")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _preset(x, name):
    from hallucidet_amd.models.cnnBasedThermalInfraredDA import CnnBasedThermalInfraredDA as M
    return M.apply_preset(x, name)


def _stages(name):
    from hallucidet_amd.models.cnnBasedThermalInfraredDA import IR_PREPROCESS
    return IR_PREPROCESS[name]


def _fixture_inputs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ir_preprocess.npz"))
    return [torch.from_numpy(g["in_" + k])[None] for k in ("skewed", "narrow", "const")]


def _inputs(kind, shape, seed):
    return (O.batch_u8 if kind == "u8" else O.batch_float)(*shape, seed=seed)


def _neighbours(xin):
    """[N, C, 2] sorted elements below and above each of the two quantile ranks (the rank model of torch.quantile, formed in fp32)"""
    n, c = xin.shape[:2]
    p = xin.shape[2] * xin.shape[3]
    srt = xin.reshape(n, c, p).sort(dim=2).values
    lo, hi = [], []
    for q in (O.BETA, 1 - O.BETA):
        rank = torch.tensor(q, dtype=torch.float32) * torch.tensor(float(p - 1), dtype=torch.float32)
        l = int(torch.floor(rank))
        lo.append(srt[:, :, l])
        hi.append(srt[:, :, min(l + 1, p - 1)])
    return torch.stack(lo, dim=2), torch.stack(hi, dim=2)


def _check_stretch(dev, x, invert_first, expect_ties):
    from hallucidet_amd import ops
    name = "invert_stretching" if invert_first else "stretching"
    n, c = x.shape[:2]
    q = torch.full((n, c, 2), float("nan"), device=dev)
    got = ops.ir_preprocess(x.to(dev), _stages(name), q_out=q).cpu()
    q = q.cpu()
    xin = O.invert(x) if invert_first else x
    s_lo, s_hi = _neighbours(xin)
    tq = O.quantiles(xin)
    ties = s_lo == s_hi
    print(name, tuple(x.shape), "tied ranks %d / %d" % (int(ties.sum()), ties.numel()),
          "max ulp distance to torch.quantile %d" % int((_bits(q) - _bits(tq)).abs().max()))
    assert bool(((q >= s_lo) & (q <= s_hi)).all()), (name, tuple(x.shape))
    assert int((_bits(q) - _bits(tq)).abs().max()) <= 2
    assert torch.equal(_bits(q)[ties], _bits(s_lo)[ties]) and torch.equal(_bits(q)[ties], _bits(tq)[ties])
    assert _same(got, O.stretch_with(xin, q)), (name, tuple(x.shape), int((_bits(got) != _bits(O.stretch_with(xin, q))).sum()))
    if expect_ties:            # k/255 images of some size: (nearly) every rank ties, and the result is the oracle's bit for bit
        assert int(ties.sum()) * 10 >= ties.numel() * 9 and _same(q, tq) and _same(got, O.ORACLE[name](x))
    return got


def _check_blur(dev, x, name):
    from hallucidet_amd import ops
    xd = x.to(dev)
    st = _stages(name)
    pre = ops.ir_preprocess(xd, st[:-1]).cpu() if len(st) > 1 else x
    got = ops.ir_preprocess(xd, st).cpu()
    want = O.blur(pre)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (name, tuple(x.shape))
    scale = max(1.0, float(pre[~torch.isnan(pre)].abs().max())) if bool((~torch.isnan(pre)).any()) else 1.0
    err = float((got[~nan] - want[~nan]).abs().max()) if bool((~nan).any()) else 0.0
    print(name, tuple(x.shape), "max |kernel - conv2d| %.3g (bound %.3g)" % (err, 2e-6 * scale))
    assert err <= 2e-6 * scale, (name, tuple(x.shape), err)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_u8_derived_inputs_equal_the_oracle(dev, shape):
    x = _inputs("u8", shape, seed=shape[0] + shape[2])
    xd = x.to(dev)
    names = EXACT + (("parallel_per_channel",) if shape[1] == 3 else ())
    for name in names:
        got = _preset(xd, name)
        assert got.data_ptr() != xd.data_ptr() and _same(got, O.ORACLE[name](x)), (name, shape, int((_bits(got) != _bits(O.ORACLE[name](x))).sum()))
    for _, inv in STRETCH:
        _check_stretch(dev, x, inv, expect_ties=shape[2] * shape[3] >= 1000)
    for name in BLUR:
        _check_blur(dev, x, name)


def test_fixture_inputs_equal_the_reference_output(dev):
    """the kernel against what the reference's own file wrote (tests/golden/ir_preprocess.npz), the constant plane included"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "ir_preprocess.npz"))
    for key in ("skewed", "narrow", "const"):
        x = torch.from_numpy(g["in_" + key])
        for name in EXACT + tuple(n for n, _ in STRETCH):
            got = _preset(x.to(dev), name).cpu()             # [C, H, W], as the reference takes it
            assert _same(got, torch.from_numpy(g["%s_%s" % (name, key)])), (name, key)
        for name in BLUR:
            got, want = _preset(x.to(dev), name).cpu(), torch.from_numpy(g["%s_%s" % (name, key)])
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, key)
            ok = ~torch.isnan(want)
            assert not bool(ok.any()) or float((got[ok] - want[ok]).abs().max()) <= 2e-6, (name, key)
            _check_blur(dev, x[None], name)


@pytest.mark.parametrize("shape", [(8, 3, 512, 640), (2, 3, 127, 161), (4, 1, 96, 100)], ids=lambda s: "x".join(map(str, s)))
def test_generic_float_inputs(dev, shape):
    x = _inputs("float", shape, seed=7)
    xd = x.to(dev)
    for name in EXACT + ("parallel_per_channel",) * (shape[1] == 3):
        assert _same(_preset(xd, name), O.ORACLE[name](x)), (name, shape)
    for _, inv in STRETCH:
        _check_stretch(dev, x, inv, expect_ties=False)
    for name in BLUR:
        _check_blur(dev, x, name)


def test_constant_plane_is_nan_exactly_where_the_oracle_has_nan(dev):
    x = O.batch_u8(2, 3, 64, 80, seed=3)
    x[1, 1] = 128.0 / 255.0
    x[0, 2] = 0.0
    for name, inv in STRETCH:
        got = _check_stretch(dev, x, inv, expect_ties=True)
        want = O.ORACLE[name](x)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got[1, 1]).all()) and bool(torch.isnan(got[0, 2]).all())
        assert int(torch.isnan(got).sum()) == 2 * 64 * 80
    _check_blur(dev, x, "invert_stretching_blur")
    assert _same(_preset(x.to(dev), "equalization"), O.equalization(x))        # one level: step == 0, the quantised plane itself


def test_one_plane_view_equals_three_planes(dev):
    from hallucidet_amd.models.cnnBasedThermalInfraredDA import IR_PREPROCESS
    from hallucidet_amd.utils.utils import Utils
    x1 = O.batch_u8(3, 1, 60, 84, seed=9).to(dev)
    view = Utils.expand_one_channel_to_output_channels(x1, 3)
    assert view.stride(1) == 0
    for name in IR_PREPROCESS:
        got, full = _preset(view, name), _preset(view.contiguous(), name)
        assert tuple(got.shape) == (3, 3, 60, 84) and _same(got, full), name
        assert (got.stride(1) == 0) == (name != "parallel_per_channel"), name
    assert _same(_preset(view, "parallel_per_channel"), O.parallel_per_channel(view.cpu()))


def test_method_surface(dev):
    """the reference's static method names and keyword signatures, [C, H, W] and [N, C, H, W], a new tensor every time"""
    from hallucidet_amd.models.cnnBasedThermalInfraredDA import CnnBasedThermalInfraredDA as M
    x = O.batch_u8(2, 3, 40, 52, seed=4)
    xd = x.to(dev)
    for name in O.METHODS:
        fn = getattr(M, O.REFERENCE_NAME[name])
        if name in BLUR:
            continue
        for inp, ref in ((xd, x), (xd[0], x[0])):
            got = fn(inp) if name == "parallel" else fn(inp, channels=[0, 1, 2])
            assert got.shape == inp.shape and _same(got, O.ORACLE[name](ref)), name
        assert _same(xd, x)                                                    # the input is never written
    assert _same(M.paralel_combination(xd, channel_op=["invert", "none", "bogus"]), O.invert(x))
    assert _same(M.paralel_combination(xd, channel_op=["none"]), x)
    assert _same(M.paralel_combination(xd, channel_op=["invert", "equalization", "invert", "equalization", "invert"]),
                 O.parallel(x, ("invert", "equalization", "invert", "equalization", "invert")))
    only1 = M.basic_preprocessing_histogram_stretching(xd, channels=[1])      # stretching honours `channels`
    assert _same(only1[:, 0::2], x[:, 0::2]) and _same(only1[:, 1:2], O.stretching(x[:, 1:2]))
    assert _same(M.basic_preprocessing_blur(xd, kernel_size=(3, 3), sigma=None), M.apply_preset(xd, "blur"))


def test_runs_are_bit_identical_and_every_preset_is_capturable(dev):
    """a capture forbids host synchronisation and freezes the launch list: the replay on NEW data must equal the eager bits"""
    from hallucidet_amd import ops
    from hallucidet_amd.models.cnnBasedThermalInfraredDA import IR_PREPROCESS
    a, b = O.batch_u8(4, 3, 128, 160, seed=1).to(dev), O.batch_float(4, 3, 128, 160, seed=2).to(dev)
    for name, st in IR_PREPROCESS.items():
        e1, e2 = ops.ir_preprocess(a, st), ops.ir_preprocess(a, st)
        assert _same(e1, e2), name
        eb = ops.ir_preprocess(b, st)
        x, out = a.clone(), torch.empty_like(a)
        q = torch.zeros(4, 3, 2, device=dev)
        ws = torch.empty(ops.ir_preprocess_ws_bytes(a.shape, len(st)), dtype=torch.uint8, device=dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.ir_preprocess(x, st, out=out, q_out=q, ws=ws)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.ir_preprocess(x, st, out=out, q_out=q, ws=ws)
        out.zero_()
        g.replay()
        assert _same(out, e1), name
        x.copy_(b)
        g.replay()
        assert _same(out, eb), name


def test_argument_errors_raise(dev):
    from hallucidet_amd import _abi, ops
    x = torch.rand(2, 3, 16, 20, device=dev)
    inv = ops.irp_stage(ops.IRP_INVERT)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.ir_preprocess(x[:, :, :, ::2], [inv])
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.ir_preprocess(x.half(), [inv])
    with pytest.raises(ValueError, match="C in"):
        ops.ir_preprocess(x[:, :2].contiguous(), [inv])
    with pytest.raises(ValueError, match="stages"):
        ops.ir_preprocess(x, [inv] * 5)
    with pytest.raises(ValueError, match="stages"):
        ops.ir_preprocess(x, [])
    with pytest.raises(ValueError, match="H, W >= 2"):
        ops.ir_preprocess(x[:, :, :1].contiguous(), [inv])
    for bad in (4 | 7 << 8, ops.IRP_BLUR, -1, inv | 1 << 11):
        with pytest.raises(ValueError, match="stage"):
            ops.ir_preprocess(x, [bad])
    with pytest.raises(ValueError, match="not the input itself"):
        ops.ir_preprocess(x, [inv], out=x)
    with pytest.raises(ValueError, match="ws must be"):
        ops.ir_preprocess(x, [inv, ops.irp_stage(ops.IRP_BLUR)], ws=torch.empty(64, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="q_out"):
        ops.ir_preprocess(x, [inv], q_out=torch.empty(2, 3, device=dev))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ir_preprocess(x.cpu(), [inv])
    # the C boundary itself: a status code and a message
    lib = _abi.load()
    import ctypes
    out = torch.empty_like(x)
    ws = torch.empty(ops.ir_preprocess_ws_bytes(x.shape, 1), dtype=torch.uint8, device=dev)
    st = (ctypes.c_int * 1)(7)
    assert lib.hd_ir_preprocess(x.data_ptr(), 2, 3, 16, 20, st, 1, out.data_ptr(), None, ws.data_ptr(), None) == -1
    assert b"stage 0" in lib.hd_last_error()


def _record(monkeypatch, obj, attr, static=False):
    calls = []
    orig = getattr(obj, attr)

    def wrapper(*a, **k):
        calls.append([v.clone() if torch.is_tensor(v) else v for v in a])
        return orig(*a, **k)
    monkeypatch.setattr(obj, attr, staticmethod(wrapper) if static else wrapper)
    return calls


def _dets(d):
    return [{k: v.clone() for k, v in x.items()} for x in d]


def _dets_equal(a, b):
    return len(a) == len(b) and all(set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


def test_encoder_decoder_lit_preprocesses_the_ir_pass_only(dev, monkeypatch):
    from hallucidet_amd import ops, synthetic
    from hallucidet_amd.utils.utils import Utils
    on = synthetic.make_module(seed=5, device="cuda", precision=16, ir_preprocess="invert_equalization")
    off = synthetic.make_module(seed=5, device="cuda", precision=16)
    assert on.ir_preprocess == "invert_equalization" and off.ir_preprocess == "none"
    batch = synthetic.make_batch(2, 128, 160, seed=9, device="cuda")
    want_ir = O.invert_equalization(Utils.expand_one_channel_to_output_channels(batch[2].cpu(), 3))
    res = {}
    for key, lit in (("on", on), ("off", off)):
        calls = _record(monkeypatch, lit, "_detector_section")
        lit.eval()
        torch.manual_seed(21)
        loss, d = lit.test_step(batch, 0)
        torch.cuda.synchronize()
        assert len(calls) == 1
        res[key] = dict(args=calls[0], loss=loss.clone(), dets={k: _dets(v) for k, v in d.items()})
    a_on, a_off = res["on"]["args"], res["off"]["args"]
    assert _same(a_on[2], want_ir)                                   # the IR pass reads the pre-processed batch
    assert _same(a_off[2], Utils.expand_one_channel_to_output_channels(batch[2], 3))
    assert _same(a_on[0], a_off[0]) and _same(a_on[1], a_off[1])     # the hallucinated (so: the U-Net input) and RGB batches: untouched
    assert torch.equal(res["on"]["loss"], res["off"]["loss"])
    assert _dets_equal(res["on"]["dets"]["hall"], res["off"]["dets"]["hall"]) and _dets_equal(res["on"]["dets"]["rgb"], res["off"]["dets"]["rgb"])
    assert sum(x["boxes"].shape[0] for x in res["off"]["dets"]["ir"]) > 0
    assert not _dets_equal(res["on"]["dets"]["ir"], res["off"]["dets"]["ir"])
    # validation takes the same path
    calls = _record(monkeypatch, on, "_detector_section")
    torch.manual_seed(21)
    on.validation_step(batch, 0)
    assert _same(calls[0][2], want_ir)

    # a training step with the option on launches nothing new: same loss, same parameter gradients
    def boom(*a, **k):
        raise AssertionError("hd_ir_preprocess reached in a training step")
    monkeypatch.setattr(ops, "ir_preprocess", boom)
    grads = {}
    for key, lit in (("on", on), ("off", off)):
        lit.train()
        lit.encoder_decoder.runner.flat_grads.zero_()
        torch.manual_seed(33)
        out = lit.forward_step(*batch, 0, step="train")
        lit.scaler.backward(out["loss"]["total"])
        torch.cuda.synchronize()
        grads[key] = (out["loss"]["total"].detach().clone(), lit.encoder_decoder.runner.flat_grads.clone())
    assert torch.equal(grads["on"][0], grads["off"][0]) and torch.equal(grads["on"][1], grads["off"][1])
    assert bool(torch.isfinite(grads["on"][1]).all()) and float(grads["on"][1].abs().max()) > 0


def test_detector_lit_trains_on_the_preprocessed_batch(dev, monkeypatch):
    from hallucidet_amd import synthetic
    from hallucidet_amd.models.detector import Detector
    from hallucidet_amd.train_detector import DetectorLit
    from hallucidet_amd.utils.utils import Utils
    torch.manual_seed(41)
    det = Detector(name="fasterrcnn", pretrained=False, n_classes=2, size=300).detector.to(dev)
    rgb, _, ir, tir = synthetic.make_batch(2, 128, 160, seed=9, device=str(dev))
    il, _ = det.transform(rgb, None)
    det.backbone.calibrate_(il.tensors)
    lit = DetectorLit(batch_size=2, lr=1e-4, detector_name="fasterrcnn", pretrained=False, detector=det, device=str(dev), modality="ir",
                      ir_preprocess="invert_equalization").prepare()
    want = O.invert_equalization(Utils.expand_one_channel_to_output_channels(ir.cpu(), 3))
    calls = _record(monkeypatch, Detector, "calculate_loss", static=True)
    loss = lit.fit_step((ir, tir))
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and len(calls) == 1 and _same(calls[0][1], want)
    lit.validation_step((ir, tir), 0)
    lit.test_step((ir, tir), 0)
    assert len(calls) == 3 and _same(calls[1][1], want) and _same(calls[2][1], want)
    plain = DetectorLit(batch_size=2, detector_name="fasterrcnn", pretrained=False, detector=det, device=str(dev), modality="ir")
    imgs, _ = plain._unpack((ir, tir))
    assert _same(imgs, Utils.expand_one_channel_to_output_channels(ir, 3))
