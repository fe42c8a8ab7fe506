"""hd_media_render on the GPU against tests/_media_oracle.py, byte for byte: the grid layout, both pixel modes at their rounding
boundaries, the outline rule at every clipping case, the score filter at the threshold's fp32 neighbours, the caps, determinism, graph
capture, and the writer inside the evaluation steps of EncoderDecoderLit and DetectorLit."""
import os

import numpy as np
import pytest
import torch

import _media_cases as K
import _media_oracle as O

pytestmark = pytest.mark.gpu


def _gpu(dev, x, mode, outputs=None, targets=None, threshold=0.5, nrow=8, box_dtype=torch.float32, extra=3):
    from hallucidet_amd import ops
    det = gt = None
    if outputs is not None:
        det, gt = K.padded(outputs, targets, extra=extra, box_dtype=box_dtype)
        det, gt = tuple(t.to(dev) for t in det), tuple(t.to(dev) for t in gt)
    xd = x[:, :1].to(dev).expand(-1, 3, -1, -1) if x.stride(1) == 0 else x.to(dev)      # a stride-0 view stays one on the device
    assert tuple(xd.stride()) == tuple(x.stride())
    out = ops.media_render(xd, mode, det=det, gt=gt, threshold=threshold, nrow=nrow)
    assert out.dtype == torch.uint8 and tuple(out.shape) == ops.media_canvas_shape(x.shape, nrow)
    return out.cpu().numpy()


def _diff(got, want):
    return "shape %s / %s, %d bytes differ" % (got.shape, want.shape, int((got != want).sum()) if got.shape == want.shape else -1)


@pytest.mark.parametrize("N,H,W,nrow", K.SHAPES)
def test_quantise_equals_the_oracle(dev, N, H, W, nrow):
    cases = dict(uniform=K.uniform(N, H, W), levels=K.levels(N, H, W), outside=K.uniform(N, H, W, 3, lo=-0.5, hi=1.5),
                 view=K.one_plane_view(N, H, W))
    for name, x in cases.items():
        got, want = _gpu(dev, x, "quantise", nrow=nrow), O.render(x, "quantise", nrow=nrow)
        assert np.array_equal(got, want), (name, _diff(got, want))
    x = cases["view"]
    assert np.array_equal(_gpu(dev, x, "quantise", nrow=nrow), _gpu(dev, x.contiguous(), "quantise", nrow=nrow))


@pytest.mark.parametrize("threshold", [0.5, 0.3])
@pytest.mark.parametrize("N,H,W,nrow", K.SHAPES)
def test_normalise_with_boxes_equals_the_oracle(dev, N, H, W, nrow, threshold):
    outputs, targets = K.boxes(N, H, W, threshold)
    cases = dict(uniform=K.uniform(N, H, W), special=K.special_channels(N, H, W), view=K.one_plane_view(N, H, W))
    for name, x in cases.items():
        want = O.render(x, "normalise", outputs, targets, threshold, nrow)
        got = _gpu(dev, x, "normalise", outputs, targets, threshold, nrow)
        assert np.array_equal(got, want), (name, _diff(got, want))
    x = cases["view"]
    assert np.array_equal(_gpu(dev, x.contiguous(), "normalise", outputs, targets, threshold, nrow),
                          O.render(x, "normalise", outputs, targets, threshold, nrow))
    x = cases["uniform"]                                          # detections given as float64 boxes: the same corners
    assert np.array_equal(_gpu(dev, x, "normalise", outputs, targets, threshold, nrow, box_dtype=torch.float64),
                          O.render(x, "normalise", outputs, targets, threshold, nrow))


def test_no_boxes_in_every_spelling(dev):
    from hallucidet_amd import ops
    N, H, W = 3, 37, 53
    x = K.special_channels(N, H, W)
    want = O.render(x, "normalise")
    assert np.array_equal(_gpu(dev, x, "normalise"), want)
    assert not want[2:2 + H, 2:2 + W, 1].any() and set(np.unique(want[2:2 + H, 2:2 + W, 2])) == {0, 255}
    xd = x.to(dev)
    zero = torch.zeros(N, dtype=torch.int32, device=dev)
    det0 = (torch.zeros(N, 0, 4, device=dev), torch.zeros(N, 0, device=dev), zero)
    gt0 = (torch.zeros(N, 0, 4, dtype=torch.float64, device=dev), zero)
    assert np.array_equal(ops.media_render(xd, "normalise", det=det0, gt=gt0).cpu().numpy(), want)            # P = 0, Q = 0
    outputs, targets = K.boxes(N, H, W, 0.5)
    det, gt = K.padded(outputs, targets)
    det = (det[0].to(dev), det[1].to(dev), zero)
    gt = (gt[0].to(dev), zero)
    assert np.array_equal(ops.media_render(xd, "normalise", det=det, gt=gt).cpu().numpy(), want)              # count = 0
    # the overlap of a ground truth and a detection is red, and both colours are present otherwise
    drawn = _gpu(dev, x, "normalise", outputs, targets)
    assert (drawn == np.array(O.RED, dtype=np.uint8)).all(-1).any() and (drawn == np.array(O.YELLOW, dtype=np.uint8)).all(-1).any()
    yy, xx = 2 + int(H / 4), 2 + int(W / 4) + 3                   # on the top side of image 0's shared box
    assert tuple(drawn[yy, xx]) == O.RED


def test_full_caps_on_a_small_image(dev):
    P, Q, H, W = 1024, 512, 64, 64
    g = torch.Generator().manual_seed(7)
    x = K.uniform(2, H, W, seed=8)

    def rnd(n):
        return torch.rand(n, 4, generator=g) * 80 - 8
    outputs = [{"boxes": rnd(P), "scores": torch.rand(P, generator=g)} for _ in range(2)]
    targets = [{"boxes": rnd(Q).double()} for _ in range(2)]
    got = _gpu(dev, x, "normalise", outputs, targets, 0.5, extra=0)
    assert np.array_equal(got, O.render(x, "normalise", outputs, targets, 0.5))


def test_caps_raise_on_the_host_before_any_launch(dev, monkeypatch):
    from hallucidet_amd import _abi, ops
    lib = _abi.load()

    class NoLaunch:
        def __getattr__(self, name):
            if name == "hd_media_render":
                raise AssertionError("hd_media_render reached")
            return getattr(lib, name)
    monkeypatch.setattr(_abi, "_lib", NoLaunch())
    with pytest.raises(ValueError, match="1499"):
        ops.media_render(torch.zeros(1, 3, 4, 1500, device=dev), "normalise")
    with pytest.raises(ValueError, match="1499"):
        ops.media_render(torch.zeros(1, 3, 1500, 4, device=dev), "quantise")
    x = torch.zeros(1, 3, 8, 8, device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="1024"):
        ops.media_render(x, "normalise", det=(torch.zeros(1, 1025, 4, device=dev), torch.zeros(1, 1025, device=dev), one))
    with pytest.raises(ValueError, match="512"):
        ops.media_render(x, "normalise", gt=(torch.zeros(1, 513, 4, dtype=torch.float64, device=dev), one))
    with pytest.raises(ValueError, match="dense"):
        ops.media_render(torch.zeros(1, 3, 8, 16, device=dev)[:, :, :, ::2], "quantise")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.media_render(torch.zeros(1, 3, 8, 8), "quantise")
    monkeypatch.setattr(_abi, "_lib", lib)
    # the C boundary itself: a status code and a message
    out = torch.empty(8, 1500, 3, dtype=torch.uint8, device=dev)
    big = torch.zeros(1, 3, 8, 1500, device=dev)
    assert lib.hd_media_render(big.data_ptr(), 36000, 12000, 1, 8, 1500, 8, 0, None, 0, None, None, 0, 0.5, None, None, 0, out.data_ptr(),
                               None, None) == -1
    assert b"1499" in lib.hd_last_error()


def test_two_calls_agree_and_a_captured_call_follows_its_inputs(dev):
    from hallucidet_amd import ops
    N, H, W = 9, 32, 64
    xs = [K.uniform(N, H, W, seed=s, lo=-1.0, hi=2.0) for s in (11, 12)]
    sets = [K.boxes(N, H, W, 0.5), K.boxes(N, H - 5, W - 9, 0.5)]
    padded = [K.padded(o, t) for o, t in sets]
    x = xs[0].to(dev)
    det = tuple(t.to(dev) for t in padded[0][0])
    gt = tuple(t.to(dev) for t in padded[0][1])
    a = ops.media_render(x, "normalise", det=det, gt=gt)
    b = ops.media_render(x, "normalise", det=det, gt=gt)
    assert torch.equal(a, b)
    out = torch.empty_like(a)
    ws = torch.empty(ops.media_ws_bytes(N), dtype=torch.uint8, device=dev)
    graph = torch.cuda.CUDAGraph()                                # the two eager calls above were the warm-up
    with torch.cuda.graph(graph):
        ops.media_render(x, "normalise", det=det, gt=gt, out=out, ws=ws)
    graph.replay()
    assert torch.equal(out, a)
    x.copy_(xs[1])                                                # new inputs in place: the replay renders them
    for dst, src in zip(det + gt, padded[1][0] + padded[1][1]):
        dst.copy_(src)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = O.render(xs[1], "normalise", sets[1][0], sets[1][1], 0.5)
    assert np.array_equal(out.cpu().numpy(), want), _diff(out.cpu().numpy(), want)


def test_plot_each_image_on_the_gpu(dev):
    from hallucidet_amd.utils.utils import Utils
    H, W = 23, 31
    outputs, targets = K.boxes(1, H, W, 0.3)
    image = K.special_channels(1, H, W)[0]
    got = Utils.plot_each_image(image.to(dev), {k: v.to(dev) for k, v in outputs[0].items()}, {k: v.to(dev) for k, v in targets[0].items()},
                                threshold=0.3)
    want = O.plot_each_image(image, outputs[0], targets[0], 0.3)
    assert got.shape == (3, H, W) and np.array_equal(got, want.transpose(2, 0, 1) / 255.0)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def _cpu_dets(d):
    return [{k: v.detach().cpu().clone() for k, v in x.items()} for x in d]


def _hallucidet_module(media):
    from hallucidet_amd import synthetic
    from hallucidet_amd.train_hallucidet import EncoderDecoderLit
    torch.manual_seed(5)
    lit = EncoderDecoderLit(batch_size=2, model_name="resnet18", detector_name="fasterrcnn", precision=16, device="cuda", media=media)
    lit.prepare()
    with torch.no_grad():
        il, _ = lit.detector.transform(synthetic.make_batch(2, 64, 64, seed=6, device="cuda")[0], None)
        lit.detector.backbone.calibrate_(il.tensors)
    lit.eval()
    return lit


def test_encoder_decoder_lit_writes_the_six_panels(dev, tmp_path):
    from hallucidet_amd import synthetic
    from hallucidet_amd.utils.media import MediaWriter
    thr = 0.05
    writer = MediaWriter(str(tmp_path / "media"), every=1, offset=0, threshold=thr)
    on, off = _hallucidet_module(writer), _hallucidet_module(None)
    on.current_epoch = off.current_epoch = 3
    halls = []
    fwd = on.forward_step

    def recording(*a, **k):
        r = fwd(*a, **k)
        halls.append(r["output"]["imgs_hallucinated"].float().cpu().clone())
        return r
    on.forward_step = recording
    batches = [synthetic.make_batch(2, 64, 64, seed=20 + i, device="cuda") for i in range(2)]
    losses, dets = {"on": [], "off": []}, []
    for key, lit in (("on", on), ("off", off)):
        for i, batch in enumerate(batches):
            torch.manual_seed(21 + i)
            loss, d = lit.test_step(batch, i)
            losses[key].append(loss.detach().clone())
            if key == "on":
                dets.append({k: _cpu_dets(v) for k, v in d.items()})
    writer.close()
    names = ("input_ir", "input_rgb", "output_hal", "output_hal_det", "output_rgb_det", "output_ir_det")
    assert sorted(os.listdir(tmp_path / "media" / "test")) == sorted("epoch003_batch%05d_%s.png" % (i, n) for i in range(2) for n in names)
    drawn = 0
    for i, (rgb, t_rgb, ir, t_ir) in enumerate(batches):
        hall = halls[i]
        ir3 = ir.cpu().expand(-1, 3, -1, -1)
        t_rgb, t_ir = _cpu_dets(t_rgb), _cpu_dets(t_ir)
        want = {"input_ir": O.render(ir3, "quantise"), "input_rgb": O.render(rgb, "quantise"), "output_hal": O.render(hall, "quantise"),
                "output_hal_det": O.render(hall, "normalise", dets[i]["hall"], t_ir, thr),
                "output_rgb_det": O.render(rgb, "normalise", dets[i]["rgb"], t_rgb, thr),
                "output_ir_det": O.render(ir3, "normalise", dets[i]["ir"], t_ir, thr)}
        for n in names:
            got = _read_png(tmp_path / "media" / "test" / ("epoch003_batch%05d_%s.png" % (i, n)))
            assert np.array_equal(got, want[n]), (i, n, _diff(got, want[n]))
        assert (want["output_hal_det"] == np.array(O.YELLOW, dtype=np.uint8)).all(-1).any()
        drawn += sum(int((x["scores"] > thr).sum()) for k in dets[i] for x in dets[i][k])
    print("detections above the threshold drawn over the two steps:", drawn)
    # the writer changes nothing the step computes: the same loss bits, the same mAP
    assert all(torch.equal(a, b) for a, b in zip(losses["on"], losses["off"]))
    m_on, m_off = on.on_test_epoch_end(), off.on_test_epoch_end()
    assert m_on.keys() == m_off.keys()
    for k in m_on:
        assert all(torch.equal(torch.as_tensor(m_on[k][q]), torch.as_tensor(m_off[k][q])) for q in m_on[k]), k


def test_detector_lit_writes_its_two_panels(dev, tmp_path):
    from hallucidet_amd import synthetic
    from hallucidet_amd.models.detector import Detector
    from hallucidet_amd.train_detector import DetectorLit
    from hallucidet_amd.utils.media import MediaWriter
    thr = 0.05
    torch.manual_seed(41)
    det = Detector(name="fasterrcnn", pretrained=False, n_classes=2, size=300).detector.to(dev)
    batches = [synthetic.make_batch(2, 64, 64, seed=30 + i, device=str(dev)) for i in range(2)]
    with torch.no_grad():
        il, _ = det.transform(batches[0][0], None)
        det.backbone.calibrate_(il.tensors)
    det.eval()
    writer = MediaWriter(str(tmp_path / "media"), every=1, offset=0, threshold=thr)
    # --map-device cuda: the evaluator and the writer both take the step's padded tensors (LazyDetections.padded), nothing is sliced first
    kw = dict(batch_size=2, detector_name="fasterrcnn", pretrained=False, detector=det, device=str(dev), modality="rgb", map_device="cuda")
    on, off = DetectorLit(media=writer, **kw), DetectorLit(**kw)
    res = {"on": [], "off": []}
    for key, lit in (("on", on), ("off", off)):
        for i, (rgb, t_rgb, _, _) in enumerate(batches):
            torch.manual_seed(51 + i)
            res[key].append(_cpu_dets(lit.test_step((rgb, t_rgb), i)))
    writer.close()
    assert sorted(os.listdir(tmp_path / "media" / "test")) == sorted("epoch000_batch%05d_%s.png" % (i, n) for i in range(2)
                                                                     for n in ("input", "output_det"))
    for i, (rgb, t_rgb, _, _) in enumerate(batches):
        got = _read_png(tmp_path / "media" / "test" / ("epoch000_batch%05d_input.png" % i))
        assert np.array_equal(got, O.render(rgb, "quantise"))
        got = _read_png(tmp_path / "media" / "test" / ("epoch000_batch%05d_output_det.png" % i))
        want = O.render(rgb, "normalise", res["on"][i], _cpu_dets(t_rgb), thr)
        assert np.array_equal(got, want), (i, _diff(got, want))
    for a, b in zip(res["on"], res["off"]):
        assert len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in x)
    m_on, m_off = on.on_test_epoch_end(), off.on_test_epoch_end()
    assert all(torch.equal(torch.as_tensor(m_on[k]), torch.as_tensor(m_off[k])) for k in m_on)
