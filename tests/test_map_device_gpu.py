"""The device COCO mAP evaluator (hallucidet_amd/metrics/device.py, csrc/coco_map.hip) against the host evaluator
(hallucidet_amd/metrics/metrics.py): every key of compute() bit-identical on the same inputs, plus its own surface (LazyDetections
input without a host sync, reset, the per-image cap, merging) and the modules' `map_device="cuda"` path."""
import numpy as np
import pytest
import torch

from hallucidet_amd.metrics import Detection, DeviceMeanAveragePrecision, MeanAveragePrecision

pytestmark = pytest.mark.gpu


def _box(x, y, w, h):
    return [x, y, x + w, y + h]


def _scene(seed, n_img=24, classes=(1,), big=False):
    """Seeded scenes with the awkward cases of COCO matching: quantised scores (ties within and across images), detections built
    at IoU exactly 0.5 / 0.75 with a ground truth, ground truths of area exactly 32^2 and 96^2, empty and ground-truth-only images,
    a class present only in detections, and images with more than 10 (and, with big=True, more than 100) detections."""
    rng = np.random.default_rng(seed)
    preds, targets = [], []
    det_only = max(classes) + 1
    for i in range(n_img):
        kind = i % 6
        gb, gl, db, ds, dl = [], [], [], [], []
        if kind == 0:                                       # empty image
            pass
        elif kind == 1:                                     # ground truth only
            for _ in range(rng.integers(1, 4)):
                gb.append(_box(*rng.uniform(0, 200, 2), *rng.uniform(5, 120, 2)))
                gl.append(int(rng.choice(classes)))
        else:
            ng = int(rng.integers(1, 9))
            for g in range(ng):
                side = [32.0, 96.0, None][g % 3]
                w, h = (side, side) if side else tuple(rng.uniform(4, 150, 2))
                x, y = rng.uniform(0, 300, 2)
                c = int(rng.choice(classes))
                gb.append(_box(x, y, w, h))
                gl.append(c)
                # exact-IoU partners: 0.5 and 0.75 of the area, same left/top edge
                for frac in (0.5, 0.75):
                    if rng.random() < 0.6:
                        db.append(_box(x, y, w, h * frac))
                        ds.append(float(rng.integers(1, 9)) / 8.0)
                        dl.append(c)
            nd = int(rng.integers(0, 30)) if not big else int(rng.integers(90, 160))
            if kind == 5:
                nd += 12
            for _ in range(nd):
                j = int(rng.integers(0, ng))
                bx = np.asarray(gb[j]) + rng.normal(0, 6, 4)
                bx[2:] = np.maximum(bx[2:], bx[:2] + 1.0)
                db.append(bx.tolist())
                ds.append(float(rng.integers(1, 17)) / 16.0 if rng.random() < 0.5 else float(rng.random()))
                dl.append(gl[j] if rng.random() < 0.8 else int(rng.choice(classes)))
            if rng.random() < 0.3:
                db.append(_box(*rng.uniform(0, 200, 2), 20.0, 20.0))
                ds.append(0.5)
                dl.append(det_only)
        preds.append({"boxes": torch.tensor(db, dtype=torch.float32).reshape(-1, 4), "scores": torch.tensor(ds, dtype=torch.float32),
                      "labels": torch.tensor(dl, dtype=torch.int64)})
        targets.append({"boxes": torch.tensor(gb, dtype=torch.float32).reshape(-1, 4), "labels": torch.tensor(gl, dtype=torch.int64)})
    return preds, targets


def _to(dev, items):
    return [{k: v.to(dev) for k, v in d.items()} for d in items]


def _host(preds, targets, class_metrics=False, chunk=5):
    m = MeanAveragePrecision(class_metrics=class_metrics)
    for i in range(0, len(preds), chunk):
        m.update(preds[i:i + chunk], targets[i:i + chunk])
    return m.compute()


def _device(dev, preds, targets, class_metrics=False, chunk=5):
    m = MeanAveragePrecision(class_metrics=class_metrics).to(dev)
    assert isinstance(m, DeviceMeanAveragePrecision)
    for i in range(0, len(preds), chunk):
        m.update(_to(dev, preds[i:i + chunk]), _to(dev, targets[i:i + chunk]))
    return m.compute()


def _assert_identical(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), (k, got[k], want[k])


@pytest.mark.parametrize("seed,classes,big,class_metrics", [(0, (1,), False, False), (1, (1,), True, False), (2, (1, 2), False, True),
                                                            (3, (1, 2), True, True), (4, (0, 3, 7), False, True)])
def test_bit_identical_to_the_host_evaluator(dev, seed, classes, big, class_metrics):
    preds, targets = _scene(seed, classes=classes, big=big)
    assert max(len(p["scores"]) for p in preds) > (100 if big else 10)
    want = _host(preds, targets, class_metrics)
    got = _device(dev, preds, targets, class_metrics)
    _assert_identical(got, want)
    assert float(want["map"]) > 0.0 and float(want["mar_1"]) <= float(want["mar_100"])


def test_torchmetrics_documented_example(dev):
    pred = [{"boxes": torch.tensor([[258.0, 41.0, 606.0, 285.0]]), "scores": torch.tensor([0.536]), "labels": torch.tensor([0])}]
    target = [{"boxes": torch.tensor([[214.0, 41.0, 562.0, 285.0]]), "labels": torch.tensor([0])}]
    got = _device(dev, pred, target)
    _assert_identical(got, _host(pred, target))
    want = {"map": 0.6, "map_50": 1.0, "map_75": 1.0, "map_small": -1.0, "map_medium": -1.0, "map_large": 0.6,
            "mar_1": 0.6, "mar_10": 0.6, "mar_100": 0.6, "mar_small": -1.0, "mar_medium": -1.0, "mar_large": 0.6}
    for k, v in want.items():
        assert abs(float(got[k]) - v) < 1e-6, (k, float(got[k]), v)


def test_agrees_with_the_oracle(dev):
    from oracle import coco_map
    preds, targets = _scene(7, n_img=12, classes=(1, 2))
    got = _device(dev, preds, targets)
    want = coco_map.evaluate([{k: v.tolist() for k, v in p.items()} for p in preds], [{k: v.tolist() for k, v in t.items()} for t in targets])
    for k, v in want.items():
        assert abs(float(got[k]) - v) < 1e-6, (k, float(got[k]), v)


def test_empty_and_reset(dev):
    m = Detection(device=str(dev)).map
    assert isinstance(m, DeviceMeanAveragePrecision)
    _assert_identical(m.compute(), MeanAveragePrecision().compute())
    preds, targets = _scene(8, n_img=10)
    m.update(_to(dev, preds), _to(dev, targets))
    first = m.compute()
    m.reset()
    _assert_identical(m.compute(), MeanAveragePrecision().compute())
    m.update(_to(dev, preds), _to(dev, targets))
    _assert_identical(m.compute(), first)
    _assert_identical(first, _host(preds, targets))


def _sync_free(dev):
    """Whether this build honours torch.cuda.set_sync_debug_mode("error") (an .item() must raise under it)."""
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.zeros(1, device=dev).item()
        honoured = False
    except RuntimeError:
        honoured = True
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return honoured


def test_lazy_detections_without_materialising_or_syncing(dev):
    from hallucidet_amd.models.detection import LazyDetections
    preds, targets = _scene(9, n_img=8, classes=(1, 2), big=True)
    n, D = len(preds), max(len(p["scores"]) for p in preds)
    b = torch.zeros(n, D, 4)
    s = torch.zeros(n, D)
    lab = torch.zeros(n, D, dtype=torch.int64)
    for i, p in enumerate(preds):
        c = len(p["scores"])
        b[i, :c], s[i, :c], lab[i, :c] = p["boxes"] / 2, p["scores"], p["labels"]
    counts = torch.tensor([len(p["scores"]) for p in preds], dtype=torch.int64)
    lazy = LazyDetections(b.to(dev), s.to(dev), lab.to(dev), counts.to(dev), box_fn=lambda x: x * 2)
    tg = _to(dev, targets)
    m = DeviceMeanAveragePrecision(device=dev, class_metrics=True)
    torch.cuda.synchronize()
    if _sync_free(dev):
        torch.cuda.set_sync_debug_mode("error")
        try:
            m.update(lazy, tg)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    else:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            m.update(lazy, tg)
            torch.cuda.synchronize()
        d2h = [e.name for e in prof.events() if "DtoH" in e.name or "DeviceToHost" in e.name]
        assert not d2h, d2h
    assert list.__len__(lazy) == 0, "update() materialised the detections"
    got = m.compute()
    _assert_identical(got, _host(preds, targets, class_metrics=True))
    # the same detections as a list of dicts (this materialises them)
    m2 = DeviceMeanAveragePrecision(device=dev, class_metrics=True)
    m2.update(list(lazy), tg)
    _assert_identical(m2.compute(), got)


def test_per_image_cap_raises(dev):
    from hallucidet_amd import ops
    n = ops.MAP_DET_CAP + 1
    xy = torch.rand(n, 2) * 100
    pred = [{"boxes": torch.cat([xy, xy + 10], 1), "scores": torch.rand(n), "labels": torch.ones(n, dtype=torch.int64)}]
    target = [{"boxes": torch.tensor([[0.0, 0.0, 10.0, 10.0]]), "labels": torch.tensor([1])}]
    m = DeviceMeanAveragePrecision(device=dev)
    m.update(_to(dev, pred), _to(dev, target))
    with pytest.raises(ValueError, match=str(ops.MAP_DET_CAP)):
        m.compute()
    # at the cap it evaluates, and equals the host
    pred[0] = {k: v[:ops.MAP_DET_CAP] for k, v in pred[0].items()}
    _assert_identical(_device(dev, pred, target), _host(pred, target))


def test_merged_halves_equal_one_evaluator(dev):
    from hallucidet_amd.metrics import device as md
    preds, targets = _scene(10, n_img=30, classes=(1, 2))
    whole = _device(dev, preds, targets, class_metrics=True)
    a = DeviceMeanAveragePrecision(device=dev, class_metrics=True)
    b = DeviceMeanAveragePrecision(device=dev, class_metrics=True)
    a.update(_to(dev, preds[:13]), _to(dev, targets[:13]))
    b.update(_to(dev, preds[13:]), _to(dev, targets[13:]))
    c = DeviceMeanAveragePrecision(device=dev, class_metrics=True)
    c.merge(md.unpack_state(*md.pack_state(b.state())))            # a state that went through the rank payload format
    a.merge(b)
    _assert_identical(a.compute(), whole)
    d = DeviceMeanAveragePrecision(device=dev, class_metrics=True)
    d.update(_to(dev, preds[:13]), _to(dev, targets[:13]))
    d.merge(c)
    _assert_identical(d.compute(), whole)


def test_validation_hooks_with_map_device_cuda_match_the_host_module(dev):
    """validation_step -> on_validation_epoch_end (the pattern of test_step_gpu.test_validation_and_test_hooks_accumulate_map) with
    map_device="cuda": the hooks report exactly what the host module's hooks report for the same detections (host accumulators fed
    the very detection objects each step produced, after the device accumulators consumed them unmaterialised), and test_step /
    on_test_epoch_end and the reset behave as with the host evaluator."""
    from hallucidet_amd import synthetic
    from hallucidet_amd.models.detection import LazyDetections
    from hallucidet_amd.utils.utils import Utils
    lit = synthetic.make_module(seed=5, device=str(dev), precision=16, map_device="cuda")
    assert lit.map_device == "cuda"
    with torch.no_grad():
        lit.detector.roi_heads.box_predictor.cls_score.weight.mul_(30.0)
    lit.detector.invalidate_packs()
    host = {k: MeanAveragePrecision() for k in ("hall", "rgb", "ir")}
    n_det, lazy = 0, 0
    for bi in range(3):
        batch = synthetic.make_batch(2, 128, 160, seed=6 + bi, device=str(dev))
        _, dets = lit.validation_step(batch, bi)
        assert all(isinstance(m, DeviceMeanAveragePrecision) for m in lit._metrics("val").values())
        for k, tg in (("hall", batch[3]), ("rgb", batch[1]), ("ir", batch[3])):
            lazy += isinstance(dets[k], LazyDetections) and list.__len__(dets[k]) == 0
            host[k].update(dets[k], tg)
            n_det += sum(len(d["scores"]) for d in dets[k])
    assert n_det > 0 and lazy > 0, "the scene must contain detections, handed over unmaterialised"
    dev_out = lit.on_validation_epoch_end()
    assert set(dev_out) == {"map_rgb", "map_hall", "map_ir"}
    for k in ("hall", "rgb", "ir"):
        want = Utils.filter_dictionary(host[k].compute(), {"map_50", "map_75", "map"})
        _assert_identical(dev_out["map_" + k], want)
    lit.test_step(batch, 0)
    assert set(lit.on_test_epoch_end()) == set(dev_out)
    assert all(float(t) == -1.0 for t in lit.on_validation_epoch_end()["map_hall"].values())
