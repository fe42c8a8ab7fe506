"""Host-side checks of the detection media (hallucidet_amd/utils/media.py): the numpy twin of the kernel against the oracle on the GPU
tests' shapes, the writer's cadence, file names, PNG contents and error reporting, the flags, the module keywords, plot_each_image."""
import os

import numpy as np
import pytest
import torch

import _media_cases as K
import _media_oracle as O


def _host(x, mode, outputs=None, targets=None, threshold=0.5, nrow=8, box_dtype=torch.float32):
    from hallucidet_amd import ops
    det = gt = None
    if outputs is not None:
        det, gt = K.padded(outputs, targets, box_dtype=box_dtype)
    return ops.media_render_host(x, mode, det=det, gt=gt, threshold=threshold, nrow=nrow).numpy()


@pytest.mark.parametrize("N,H,W,nrow", K.SHAPES)
def test_host_quantise_equals_the_oracle(N, H, W, nrow):
    for x in (K.uniform(N, H, W), K.levels(N, H, W), K.uniform(N, H, W, 3, lo=-0.5, hi=1.5), K.one_plane_view(N, H, W)):
        got, want = _host(x, "quantise", nrow=nrow), O.render(x, "quantise", nrow=nrow)
        assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize("threshold", [0.5, 0.3])
@pytest.mark.parametrize("N,H,W,nrow", K.SHAPES)
def test_host_normalise_with_boxes_equals_the_oracle(N, H, W, nrow, threshold):
    outputs, targets = K.boxes(N, H, W, threshold)
    for x in (K.uniform(N, H, W), K.special_channels(N, H, W), K.one_plane_view(N, H, W)):
        got = _host(x, "normalise", outputs, targets, threshold, nrow)
        want = O.render(x, "normalise", outputs, targets, threshold, nrow)
        assert got.shape == want.shape and np.array_equal(got, want)
    x = K.special_channels(N, H, W)
    assert np.array_equal(_host(x, "normalise", nrow=nrow), O.render(x, "normalise", nrow=nrow))          # no boxes at all
    got = _host(x, "normalise", nrow=nrow)
    pad = 0 if N == 1 else 2
    assert not got[pad:pad + H, pad:pad + W, 1].any()                                                     # the constant channel is 0


def test_host_caps_raise():
    from hallucidet_amd import ops
    with pytest.raises(ValueError, match="1499"):
        ops.media_render_host(torch.zeros(1, 3, 2, 1500), "quantise")
    x = torch.zeros(1, 3, 4, 4)
    det = (torch.zeros(1, 1025, 4), torch.zeros(1, 1025), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="1024"):
        ops.media_render_host(x, "normalise", det=det)
    gt = (torch.zeros(1, 513, 4, dtype=torch.float64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="512"):
        ops.media_render_host(x, "normalise", gt=gt)
    assert ops.media_canvas_shape((9, 3, 32, 64)) == (2 * 34 + 2, 8 * 66 + 2, 3) and ops.media_canvas_shape((1, 3, 5, 7)) == (5, 7, 3)


def _panels(i, N=3, H=12, W=20):
    x = K.uniform(N, H, W, seed=100 + i)
    outputs, targets = K.boxes(N, H, W, 0.5)
    return {"input": (x, "quantise", None, None), "output_det": (x, "normalise", outputs, targets)}


def _read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"))


def test_writer_cadence_names_and_png_contents(tmp_path):
    from hallucidet_amd.utils.media import MediaWriter
    w = MediaWriter(str(tmp_path / "m"), every=3, offset=1, threshold=0.5)
    logged = []
    for i in range(8):
        if w.wants(i):
            w.log("val", 2, i, _panels(i))
            logged.append(i)
    w.close()
    assert logged == [1, 4, 7]
    want = sorted("epoch002_batch%05d_%s.png" % (i, p) for i in logged for p in ("input", "output_det"))
    assert sorted(os.listdir(tmp_path / "m" / "val")) == want and os.listdir(tmp_path / "m") == ["val"]
    for i in logged:
        for name, (x, mode, outputs, targets) in _panels(i).items():
            got = _read_png(tmp_path / "m" / "val" / ("epoch002_batch%05d_%s.png" % (i, name)))
            assert np.array_equal(got, O.render(x, mode, outputs, targets, 0.5))
    w.close()                                                        # idempotent


def test_writer_media_max_rank_and_every_one(tmp_path):
    from hallucidet_amd.utils.media import MediaWriter
    w = MediaWriter(str(tmp_path / "a"), every=1, offset=1, max_batches=2)          # the scripts' offset: every=1 still selects every batch
    for epoch in (0, 1):
        for i in range(4):
            assert w.wants(i)
            w.log("test", epoch, i, {"input": _panels(i)["input"]})
    w.close()
    assert sorted(os.listdir(tmp_path / "a" / "test")) == ["epoch%03d_batch%05d_input.png" % (e, i) for e in (0, 1) for i in (0, 1)]
    other = MediaWriter(str(tmp_path / "b"), every=1, offset=0, rank=1)
    assert not other.wants(0)
    other.log("test", 0, 0, _panels(0))
    other.close()
    assert not (tmp_path / "b").exists()
    ref = MediaWriter(str(tmp_path / "c"))
    assert [i for i in range(250) if ref.wants(i)] == [1, 101, 201]                 # the reference's batch_idx % 100 == 1


def test_writer_reports_worker_errors(tmp_path):
    from hallucidet_amd.utils.media import MediaWriter
    blocker = tmp_path / "file"
    blocker.write_text("not a directory")
    w = MediaWriter(str(blocker), every=1, offset=0)
    w.log("val", 0, 0, {"input": _panels(0)["input"]})
    with pytest.raises(RuntimeError, match="encoder thread failed"):
        w.close()
    w2 = MediaWriter(str(blocker), every=1, offset=0)
    w2.log("val", 0, 0, {"input": _panels(0)["input"]})
    w2.flush()                                                       # the panel has been tried by now
    with pytest.raises(RuntimeError, match="encoder thread failed"):
        w2.log("val", 0, 1, {"input": _panels(1)["input"]})           # ... and the next log() says so
    w2.close()


def test_flags_defaults_and_module_keywords(tmp_path):
    from hallucidet_amd.config import Config
    a = Config.argument_parser([])
    assert a.save_media is None and a.media_every == 100 and a.media_max is None
    a = Config.argument_parser(["--save-media", str(tmp_path), "--media-every", "7", "--media-max", "3", "--threshold", "0.3"])
    assert a.save_media == str(tmp_path) and a.media_every == 7 and a.media_max == 3 and a.threshold == 0.3
    import train_hallucidet
    assert train_hallucidet.media_writer(Config.argument_parser([])) is None
    w = train_hallucidet.media_writer(a)
    assert (w.every, w.offset, w.max_batches, w.threshold, w.nrow) == (7, 1, 3, 0.3, 8)
    w.close()
    for script in ("train_hallucidet.py", "eval_hallucidet.py", "train_detector.py"):
        src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), script)).read()
        assert "media" in src and ".close()" in src, script
    from hallucidet_amd.train_detector import DetectorLit
    from hallucidet_amd.train_hallucidet import EncoderDecoderLit
    lit = EncoderDecoderLit(model_name="resnet18", device="cpu", media=None)
    assert lit.media is None and EncoderDecoderLit(model_name="resnet18", device="cpu", media=w).media is w
    det = DetectorLit(detector_name="fasterrcnn", pretrained=False, detector=lit.detector, device="cpu", media=None)
    assert det.media is None


def test_plot_each_image_equals_the_oracle():
    from hallucidet_amd.utils.utils import Utils
    H, W = 23, 31
    outputs, targets = K.boxes(1, H, W, 0.5)
    image = K.special_channels(1, H, W)[0]
    before = image.clone()
    got = Utils.plot_each_image(image, outputs[0], targets[0], threshold=0.5)
    want = O.plot_each_image(image, outputs[0], targets[0], 0.5)
    assert got.shape == (3, H, W) and got.dtype == np.float64 and got.min() >= 0.0 and got.max() <= 1.0
    assert np.array_equal(got, want.transpose(2, 0, 1) / 255.0) and torch.equal(image, before)
    assert (want == np.array(O.RED, dtype=np.uint8)).all(-1).any() and (want == np.array(O.YELLOW, dtype=np.uint8)).all(-1).any()
