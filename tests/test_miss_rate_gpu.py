"""The log-average miss rate on the device (hd_mr_accumulate in csrc/coco_map.hip, metrics/device.py) against the host evaluator: every
key of compute() with torch.equal, the integer counts and the curves with np.array_equal, at the scan's chunk edges, past the 10-bit
per-chunk packing of the running counters, at the rank cut and at the fppi == ref boundary; the call's argument checks; the modules'
`miss_rate=True` path and the --miss-rate-curves files."""
import ctypes

import numpy as np
import pytest
import torch

import _miss_rate_oracle as orc
from hallucidet_amd.metrics import DeviceMeanAveragePrecision, MeanAveragePrecision

pytestmark = pytest.mark.gpu

MR_KEYS = {"lamr", "lamr_75", "lamr_small", "lamr_medium", "lamr_large", "mr_fppi01", "lamr_per_class"}


def _to(dev, items):
    return [{k: v.to(dev) for k, v in d.items()} for d in items]


def _host(preds, targets, class_metrics=True):
    m = MeanAveragePrecision(class_metrics=class_metrics, miss_rate=True)
    m.update(preds, targets)
    return m, m.compute()


def _device(dev, preds, targets, class_metrics=True, chunk=7):
    m = MeanAveragePrecision(class_metrics=class_metrics, miss_rate=True).to(dev)
    assert isinstance(m, DeviceMeanAveragePrecision) and m.miss_rate
    for i in range(0, len(preds), chunk):
        m.update(_to(dev, preds[i:i + chunk]), _to(dev, targets[i:i + chunk]))
    return m, m.compute()


def _assert_identical(got, want):
    assert set(got) == set(want) and MR_KEYS <= set(got)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), (k, got[k], want[k])


def _assert_same_counts_and_curves(d, h):
    cd, ch = d.miss_rate_counts(), h.miss_rate_counts()
    assert cd["classes"] == ch["classes"] and cd["n_images"] == ch["n_images"]
    for k in ("hit", "total", "n_gt"):
        assert cd[k].dtype == ch[k].dtype == np.int32 and np.array_equal(cd[k], ch[k]), k
    vd, vh = d.miss_rate_curves(), h.miss_rate_curves()
    assert list(vd) == list(vh)
    for c in vh:
        assert vd[c]["n_images"] == vh[c]["n_images"] and vd[c]["n_gt"] == vh[c]["n_gt"]
        for k in ("score", "fppi", "miss_rate"):
            assert vd[c][k].dtype == np.float64 and np.array_equal(vd[c][k], vh[c][k]), (c, k)


def _check(dev, preds, targets, class_metrics=True):
    h, want = _host(preds, targets, class_metrics)
    d, got = _device(dev, preds, targets, class_metrics)
    _assert_identical(got, want)
    _assert_same_counts_and_curves(d, h)
    return d, h, got


def _alternating(n_img, per_image, tp_per_image):
    """n_img images of `per_image` detections each, the first tp_per_image of every image's odd-even interleave true positives; scores
    quantised so that ties cross images."""
    fl, sc = [], []
    for i in range(n_img):
        f = [j % 2 == 0 and j // 2 < tp_per_image for j in range(per_image[i])]
        fl.append(f)
        sc.append([round(0.95 - 0.009 * ((j * 7 + i) % 100), 3) for j in range(per_image[i])])
    return orc.grid_scene(n_img, [sum(f) for f in fl], fl, scores=sc)


@pytest.mark.parametrize("seed,classes,big", [(0, (1,), False), (1, (1,), True), (4, (0, 3, 7), False)])
def test_seeded_scenes_equal_the_host(dev, seed, classes, big):
    preds, targets = orc.scene(seed, n_img=12 if big else 24, classes=classes, big=big)
    assert max(len(p["scores"]) for p in preds) > (100 if big else 10)          # big: the rank cut at 100 per image and class
    _, _, got = _check(dev, preds, targets)
    assert 0.0 < float(got["lamr"]) <= 1.0 and got["lamr_per_class"].shape == (len(classes) + 1,)


def test_one_image_all_empty_and_no_class_metrics(dev):
    preds, targets = orc.scene(5, n_img=6)
    _check(dev, preds[2:3], targets[2:3])
    empty_p, empty_t = orc.grid_scene(4, [0] * 4, [[]] * 4)
    _, _, got = _check(dev, empty_p, empty_t)
    assert all(float(got[k]) == -1.0 for k in MR_KEYS)
    _, _, got = _check(dev, preds, targets, class_metrics=False)
    assert got["lamr_per_class"].shape == ()
    # ground truths and no detection: exactly 1.0
    none = [{"boxes": torch.zeros(0, 4), "scores": torch.zeros(0), "labels": torch.zeros(0, dtype=torch.int64)} for _ in targets]
    _, _, got = _check(dev, none, targets)
    assert float(got["lamr"]) == 1.0


@pytest.mark.parametrize("kept", [255, 256, 257, 512, 513])
def test_class_segments_at_the_scan_chunk_edges(dev, kept):
    per_image = [100] * (kept // 100) + ([kept % 100] if kept % 100 else [])
    preds, targets = _alternating(len(per_image), per_image, 20)
    d, _, _ = _check(dev, preds, targets)
    assert int(d.miss_rate_counts()["total"][0, 0, 0].sum()) == kept


def test_running_counters_past_the_per_chunk_packing(dev):
    """More than 1 023 true and more than 1 023 false positives in one class: the per-chunk scan packs 10 bits per counter, the running
    totals must not."""
    preds, targets = _alternating(30, [100] * 30, 36)
    d, _, got = _check(dev, preds, targets)
    tp, fp = d.miss_rate_counts()["total"][0, 0, 0].tolist()
    assert tp == 30 * 36 > 1023 and fp == 30 * 64 > 1023
    assert float(got["lamr"]) < 1.0


def test_boundary_equality(dev):
    fl = [False, True] + [False] * 9 + [True] + [False] * 90 + [True] + [False, True]
    preds, targets = orc.grid_scene(100, [sum(fl[:100]), sum(fl[100:])] + [0] * 98, [fl[:100], fl[100:]] + [[]] * 98,
                                    scores=[np.linspace(0.99, 0.5, 100).tolist(), np.linspace(0.4, 0.1, len(fl) - 100).tolist()] + [[]] * 98)
    d, _, _ = _check(dev, preds, targets)
    assert d.miss_rate_counts()["hit"][0, 0, 0].tolist() == [1, 1, 1, 1, 2, 2, 2, 2, 3]


def test_worked_case(dev):
    preds, targets = orc.worked_case()
    d, _, got = _check(dev, preds, targets)
    assert d.miss_rate_counts()["hit"][0, 0, 0].tolist() == [1, 1, 1, 1, 1, 1, 3, 3, 4]
    assert float(got["lamr"]) == np.float32(0.5878937969102396)


def test_padded_lazy_style_input(dev):
    from hallucidet_amd.models.detection import LazyDetections
    preds, targets = orc.scene(9, n_img=8, classes=(1, 2), big=True)
    n, D = len(preds), max(len(p["scores"]) for p in preds)
    b, s, lab = torch.zeros(n, D, 4), torch.zeros(n, D), torch.zeros(n, D, dtype=torch.int64)
    for i, p in enumerate(preds):
        c = len(p["scores"])
        b[i, :c], s[i, :c], lab[i, :c] = p["boxes"] / 2, p["scores"], p["labels"]
    counts = torch.tensor([len(p["scores"]) for p in preds], dtype=torch.int64)
    lazy = LazyDetections(b.to(dev), s.to(dev), lab.to(dev), counts.to(dev), box_fn=lambda x: x * 2)
    m = DeviceMeanAveragePrecision(device=dev, class_metrics=True, miss_rate=True)
    m.update(lazy, _to(dev, targets))
    assert list.__len__(lazy) == 0, "update() materialised the detections"
    h, want = _host(preds, targets)
    _assert_identical(m.compute(), want)
    _assert_same_counts_and_curves(m, h)


def test_option_off_on_the_device_keeps_todays_keys(dev):
    preds, targets = orc.scene(2, n_img=12, classes=(1, 2))
    off = MeanAveragePrecision(class_metrics=True).to(dev)
    off.update(_to(dev, preds), _to(dev, targets))
    off = off.compute()
    _, on = _device(dev, preds, targets)
    assert set(on) - set(off) == MR_KEYS and all(torch.equal(off[k], on[k]) for k in off)


def _captured_call(dev, monkeypatch, preds, targets):
    """The arguments compute() hands ops.mr_accumulate."""
    from hallucidet_amd import ops
    seen, real = {}, ops.mr_accumulate

    def spy(*a, **kw):
        seen["a"], seen["kw"] = a, kw
        return real(*a, **kw)
    monkeypatch.setattr(ops, "mr_accumulate", spy)
    _device(dev, preds, targets)
    monkeypatch.setattr(ops, "mr_accumulate", real)
    return seen["a"], seen["kw"]


def test_two_runs_give_the_same_bits(dev, monkeypatch):
    from hallucidet_amd import ops
    preds, targets = _alternating(6, [100, 100, 100, 100, 100, 13], 20)
    a, kw = _captured_call(dev, monkeypatch, preds, targets)
    assert kw == {"curve_t": 0}
    first = ops.mr_accumulate(*a, **kw)
    second = ops.mr_accumulate(*a, **kw)
    for x, y in zip((first[0], first[1]) + first[2], (second[0], second[1]) + second[2]):
        assert x.dtype == torch.int32 and torch.equal(x, y)
    assert first[2][0].shape == a[0].shape and int(first[2][0].max()) == int(first[1][0, 0, 0, 0]) == 5 * 20 + 7
    # without the curve the counts are the same and no curve comes back
    hit, total, curve = ops.mr_accumulate(*a)
    assert curve is None and torch.equal(hit, first[0]) and torch.equal(total, first[1])
    d1, d2 = _device(dev, preds, targets)[1], _device(dev, preds, targets)[1]
    assert all(torch.equal(d1[k], d2[k]) for k in d1)


def test_mr_accumulate_refuses_null_and_ill_sized_arguments(dev, monkeypatch):
    from hallucidet_amd import _abi, ops
    preds, targets = orc.worked_case()
    (order, class_off, flags, npig, n_eval, n_images, ref), _ = _captured_call(dev, monkeypatch, preds, targets)
    K = n_eval.shape[0]
    with pytest.raises(ValueError, match="class_off"):
        ops.mr_accumulate(order, class_off[:-1].contiguous(), flags, npig, n_eval, n_images, ref)
    with pytest.raises(ValueError, match="npig"):
        ops.mr_accumulate(order, class_off, flags, npig[:, :3].contiguous(), n_eval, n_images, ref)
    with pytest.raises(ValueError, match="ref_fppi"):
        ops.mr_accumulate(order, class_off, flags, npig, n_eval, n_images, ref[:8].contiguous())
    with pytest.raises(ValueError, match="order"):
        ops.mr_accumulate(order.long(), class_off, flags, npig, n_eval, n_images, ref)
    with pytest.raises(ValueError, match="images"):
        ops.mr_accumulate(order, class_off, flags, npig, n_eval, n_images + 1, ref)
    with pytest.raises(ValueError, match="images"):
        ops.mr_accumulate(order, class_off, flags, npig, n_eval, 0, ref)
    with pytest.raises(ValueError, match="curve_t"):
        ops.mr_accumulate(order, class_off, flags, npig, n_eval, n_images, ref, curve_t=10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mr_accumulate(order.cpu(), class_off, flags, npig, n_eval, n_images, ref)
    # the C entry itself: status codes and the library's message, nothing launched
    lib = _abi.load()
    hit = torch.empty((10, K, 4, 9), dtype=torch.int32, device=dev)
    total = torch.empty((10, K, 4, 2), dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = [p(order), p(class_off), p(flags), flags.shape[1], p(npig), p(n_eval), K, n_images, p(ref), p(hit), p(total), -1, None, None, None]
    assert lib.hd_mr_accumulate(*good) == 0
    for i in (1, 2, 4, 5, 8, 9, 10):
        bad = list(good)
        bad[i] = None
        assert lib.hd_mr_accumulate(*bad) == -1 and b"null" in lib.hd_last_error(), i
    for i, v in ((6, -1), (7, 0), (7, -3), (11, 10)):
        bad = list(good)
        bad[i] = v
        assert lib.hd_mr_accumulate(*bad) == -1, (i, v)
    one = torch.empty_like(order)
    bad = list(good)
    bad[11], bad[12] = 0, p(one)
    assert lib.hd_mr_accumulate(*bad) == -1 and b"curve" in lib.hd_last_error()
    torch.cuda.synchronize()


def test_modules_report_the_same_miss_rate_keys_on_both_map_devices_and_write_the_curves(dev, tmp_path):
    """test_step -> on_test_epoch_end with miss_rate=True at the smallest synthetic set-up of the map-device tests: map_device "cuda"
    and "cpu" report what host evaluators fed the very same detections compute, new keys included; --miss-rate-curves writes one
    parseable CSV per stream and class whose last miss rate is 1 - total_tp / n_gt."""
    from hallucidet_amd import synthetic
    from hallucidet_amd.utils.utils import Utils
    out_dir = tmp_path / "curves"
    lit = synthetic.make_module(seed=5, device=str(dev), precision=16, map_device="cuda", miss_rate_curves=str(out_dir))
    assert lit.miss_rate                                            # the curve directory implies the metric
    with torch.no_grad():
        lit.detector.roi_heads.box_predictor.cls_score.weight.mul_(30.0)
    lit.detector.invalidate_packs()
    keys = {"map_50", "map_75", "map", "lamr", "lamr_75", "lamr_small", "lamr_medium", "lamr_large", "mr_fppi01"}
    batches = [synthetic.make_batch(2, 128, 160, seed=6 + bi, device=str(dev)) for bi in range(2)]
    for map_device, kind in (("cuda", DeviceMeanAveragePrecision), ("cpu", MeanAveragePrecision)):
        lit.map_device = map_device
        lit.__dict__.pop("_map_metrics", None)
        host = {k: MeanAveragePrecision(miss_rate=True) for k in ("hall", "rgb", "ir")}
        n_det = 0
        for bi, batch in enumerate(batches):
            _, dets = lit.test_step(batch, bi)
            assert all(type(m) is kind and m.miss_rate for m in lit._metrics("test").values())
            for k, tg in (("hall", batch[3]), ("rgb", batch[1]), ("ir", batch[3])):
                host[k].update(dets[k], tg)
                n_det += sum(len(d["scores"]) for d in dets[k])
        assert n_det > 0
        out = lit.on_test_epoch_end()
        assert set(out) == {"map_rgb", "map_hall", "map_ir"}
        for k in ("hall", "rgb", "ir"):
            want = Utils.filter_dictionary(host[k].compute(), keys)
            assert set(out["map_" + k]) == keys
            for key in keys:
                assert torch.equal(out["map_" + k][key], want[key]), (map_device, k, key)
            cnt = host[k].miss_rate_counts()
            for ki, c in enumerate(cnt["classes"]):
                path = out_dir / ("test_%s_class%d.csv" % (k, c))
                if cnt["n_gt"][ki, 0] == 0:
                    assert not path.exists()
                    continue
                rows = path.read_text().splitlines()
                assert rows[0] == "score,fppi,miss_rate" and len(rows) == 1 + int(cnt["total"][0, ki, 0].sum())
                vals = np.asarray([[float(v) for v in r.split(",")] for r in rows[1:]]).reshape(-1, 3)
                if len(vals):
                    assert vals[-1, 2] == 1.0 - cnt["total"][0, ki, 0, 0] / cnt["n_gt"][ki, 0]
                    assert (np.diff(vals[:, 1]) >= 0).all() and (np.diff(vals[:, 0]) <= 0).all()
                path.unlink()
        assert not list(out_dir.iterdir())
