"""The log-average miss rate of the host evaluator (hallucidet_amd/metrics/metrics.py, `miss_rate=True`) against an independent
restatement of Dollar's procedure (tests/_miss_rate_oracle.py), its hand-worked cases, and the option's surface (keys, curves, the
trainer's "-1 means no data" rule, the scripts' flags and printed lines)."""
import math

import numpy as np
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

import _miss_rate_oracle as orc
from hallucidet_amd.metrics import Detection, MeanAveragePrecision

MR_KEYS = {"lamr", "lamr_75", "lamr_small", "lamr_medium", "lamr_large", "mr_fppi01", "lamr_per_class"}
TODAY = {"map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium",
         "mar_large", "map_per_class", "mar_100_per_class"}


def _host(preds, targets, class_metrics=False, miss_rate=True, chunk=5):
    m = MeanAveragePrecision(class_metrics=class_metrics, miss_rate=miss_rate)
    for i in range(0, len(preds), chunk):
        m.update(preds[i:i + chunk], targets[i:i + chunk])
    return m, m.compute()


def _against_oracle(preds, targets):
    m, out = _host(preds, targets, class_metrics=True)
    want, want_mean = orc.evaluate(preds, targets)
    cnt = m.miss_rate_counts()
    assert cnt["classes"] == sorted(want) and cnt["n_images"] == len(targets)
    per_class = out["lamr_per_class"].reshape(-1).tolist() if want else []
    for k, c in enumerate(cnt["classes"]):
        hit = cnt["hit"][0, k, 0]
        if want[c] is None:
            assert (hit == -1).all() and (cnt["total"][0, k, 0] == -1).all() and per_class[k] == -1.0
            continue
        assert hit.dtype == np.int32 and hit.tolist() == want[c]["hit"], (c, hit.tolist(), want[c]["hit"])
        assert cnt["total"][0, k, 0].tolist() == [want[c]["tp"], want[c]["fp"]] and cnt["n_gt"][k, 0] == want[c]["n_gt"]
        lamr, _ = MeanAveragePrecision.mr_summary(cnt["hit"], cnt["n_gt"])
        assert abs(lamr[0, k, 0] - want[c]["lamr"]) <= 1e-12 * want[c]["lamr"], (c, lamr[0, k, 0], want[c]["lamr"])
        assert per_class[k] == np.float32(lamr[0, k, 0])
    if want_mean < 0:
        assert float(out["lamr"]) == -1.0
    else:
        assert abs(float(out["lamr"]) - want_mean) <= 1e-6 * want_mean          # the key is a float32 tensor
    return m, out, want


@pytest.mark.parametrize("seed,classes,big", [(0, (1,), False), (1, (1,), True), (2, (1, 2), False), (4, (0, 3, 7), False)])
def test_host_equals_the_oracle_on_seeded_scenes(seed, classes, big):
    preds, targets = orc.scene(seed, n_img=12 if big else 24, classes=classes, big=big)
    _, out, want = _against_oracle(preds, targets)
    assert want[max(classes) + 1] is None                       # the detection-only class: undefined, left out of the mean
    assert 0.0 < float(out["lamr"]) <= 1.0


_image = st.tuples(st.integers(0, 3), st.lists(st.tuples(st.booleans(), st.integers(0, 4), st.integers(1, 2)), max_size=8))


@settings(max_examples=60, deadline=None, database=None, derandomize=True)
@given(st.lists(_image, min_size=1, max_size=6))
def test_host_equals_the_oracle_under_hypothesis(images):
    """Random small scenes: per image up to 3 ground truths per class on a grid and up to 8 detections that copy a ground truth, miss
    everything, or duplicate an earlier copy; scores quantised to fifths so that ties abound."""
    preds, targets = [], []
    for ng, dets in images:
        gb = [orc.box(40.0 * g, 0.0, 20.0, 20.0) for g in range(ng)] * 2
        gl = [1] * ng + [2] * ng
        db, ds, dl = [], [], []
        for j, (on_gt, q, lab) in enumerate(dets):
            db.append(orc.box(40.0 * (j % max(ng, 1)), 0.0, 20.0, 20.0) if on_gt and ng else orc.box(40.0 * j, 500.0, 20.0, 20.0))
            ds.append(q / 5.0)
            dl.append(lab)
        p, t = orc.tensors(db, ds, dl, gb, gl)
        preds.append(p)
        targets.append(t)
    _against_oracle(preds, targets)


def test_worked_case():
    preds, targets = orc.worked_case()
    m, out = _host(preds, targets)
    cnt = m.miss_rate_counts()
    assert cnt["n_images"] == 4 and cnt["n_gt"][0, 0] == 5
    assert cnt["hit"][0, 0, 0].tolist() == [1, 1, 1, 1, 1, 1, 3, 3, 4] and cnt["total"][0, 0, 0].tolist() == [4, 5]
    lamr, mr = MeanAveragePrecision.mr_summary(cnt["hit"], cnt["n_gt"])
    assert np.allclose(mr[0, 0, 0], [.8, .8, .8, .8, .8, .8, .4, .4, .2], rtol=0, atol=1e-15)
    assert lamr[0, 0, 0] == pytest.approx(0.5878937969102396, rel=1e-14)
    assert out["lamr"].dtype == torch.float32 and out["lamr"].shape == () and float(out["lamr"]) == np.float32(0.5878937969102396)
    assert float(out["mr_fppi01"]) == np.float32(0.8)
    assert orc.evaluate(preds, targets)[0][1]["hit"] == [1, 1, 1, 1, 1, 1, 3, 3, 4]


def test_perfect_detector_no_detections_and_a_class_without_ground_truth():
    preds, targets = orc.grid_scene(3, [2, 3, 1], [[True] * 2, [True] * 3, [True]])
    m, out = _host(preds, targets)
    lamr, _ = MeanAveragePrecision.mr_summary(m.miss_rate_counts()["hit"], m.miss_rate_counts()["n_gt"])
    assert lamr[0, 0, 0] == pytest.approx(1e-10, rel=1e-12) and lamr[0, 0, 0] == math.exp(math.log(1e-10))
    assert float(out["lamr"]) == np.float32(lamr[0, 0, 0])
    # no detections at all: exactly 1.0
    none = [{"boxes": torch.zeros(0, 4), "scores": torch.zeros(0), "labels": torch.zeros(0, dtype=torch.int64)} for _ in targets]
    m, out = _host(none, targets)
    assert float(out["lamr"]) == 1.0 and float(out["mr_fppi01"]) == 1.0 and float(out["lamr_75"]) == 1.0
    assert (m.miss_rate_counts()["hit"][:, 0, 0] == 0).all() and (m.miss_rate_counts()["total"][:, 0, 0] == 0).all()
    # a class that only detections name has no ground truth: -1, and the mean leaves it out
    extra = [dict(p) for p in preds]
    extra[0] = {"boxes": torch.cat([preds[0]["boxes"], torch.tensor([[300.0, 300.0, 320.0, 320.0]])]),
                "scores": torch.cat([preds[0]["scores"], torch.tensor([0.99])]), "labels": torch.cat([preds[0]["labels"], torch.tensor([9])])}
    m, out = _host(extra, targets, class_metrics=True)
    assert out["lamr_per_class"].tolist() == [float(np.float32(lamr[0, 0, 0])), -1.0]
    assert float(out["lamr"]) == np.float32(lamr[0, 0, 0])
    assert list(m.miss_rate_curves()) == [1]
    # nothing at all
    m = MeanAveragePrecision(miss_rate=True)
    out = m.compute()
    assert all(float(out[k]) == -1.0 for k in MR_KEYS) and m.miss_rate_curves() == {}


def test_boundary_equality_counts_as_not_above():
    """fp / n_img == REF[i] exactly (n_img = 100; fp = 1, 10, 100 against 0.01, 0.1, 1.0): the point at the boundary qualifies."""
    ref = MeanAveragePrecision.REF_FPPI
    assert ref[0] == 1 / 100 and ref[4] == 10 / 100 and ref[8] == 100 / 100 and np.array_equal(ref, np.logspace(-2.0, 0.0, 9))
    # image 0: FP then TP (fp = 1 when the first true positive arrives), 9 more FPs then a TP (fp = 10), 90 more FPs then a TP (fp = 100), an FP, a TP
    fl = [False, True] + [False] * 9 + [True] + [False] * 90 + [True] + [False, True]
    # image 0 holds the first 100 detections of the global order (an image keeps at most 100), image 1 the rest, 98 images are empty
    preds, targets = orc.grid_scene(100, [sum(fl[:100]), sum(fl[100:])] + [0] * 98, [fl[:100], fl[100:]] + [[]] * 98,
                                    scores=[np.linspace(0.99, 0.5, 100).tolist(), np.linspace(0.4, 0.1, len(fl) - 100).tolist()] + [[]] * 98)
    m, _ = _host(preds, targets)
    hit = m.miss_rate_counts()["hit"][0, 0, 0].tolist()
    assert hit == [1, 1, 1, 1, 2, 2, 2, 2, 3], hit
    assert hit == orc.evaluate(preds, targets)[0][1]["hit"]


def test_empty_images_move_fppi_and_lower_lamr():
    preds, targets = orc.worked_case()
    _, base = _host(preds, targets)
    empty_p, empty_t = orc.grid_scene(10, [0] * 10, [[]] * 10)
    m, more = _host(preds + empty_p, targets + empty_t)
    assert m.miss_rate_counts()["n_images"] == 14
    assert float(more["lamr"]) < float(base["lamr"])
    assert float(more["map_50"]) == float(base["map_50"])          # the mAP does not see empty images


@pytest.mark.parametrize("class_metrics", [False, True])
def test_option_off_keeps_todays_keys_and_values(class_metrics):
    preds, targets = orc.scene(2, n_img=12, classes=(1, 2))
    _, off = _host(preds, targets, class_metrics=class_metrics, miss_rate=False)
    _, on = _host(preds, targets, class_metrics=class_metrics, miss_rate=True)
    assert set(off) == TODAY and set(on) == TODAY | MR_KEYS
    for k in TODAY:
        assert off[k].dtype == on[k].dtype and torch.equal(off[k], on[k]), k
    for k in MR_KEYS - {"lamr_per_class"}:
        assert on[k].dtype == torch.float32 and on[k].shape == ()
    assert on["lamr_per_class"].shape == ((3,) if class_metrics else ())
    with pytest.raises(ValueError, match="miss_rate=True"):
        MeanAveragePrecision().miss_rate_curves()


def test_prefix_evaluation_equals_a_matching_per_max_dets():
    """compute() matches once per (image, class, area) at max-dets 100 and cuts the result for 1 and 10; every column of the cut equals
    what _evaluate_img returns when asked for that max-dets directly."""
    preds, targets = orc.scene(3, n_img=12, classes=(1, 2), big=True)
    m = MeanAveragePrecision()
    m.update(preds, targets)
    for rng in m.AREA_RNG.values():
        for i in range(len(targets)):
            top = m._evaluate_img(i, 1, rng, 100)
            for md in (1, 10):
                want = m._evaluate_img(i, 1, rng, md)
                if want is None:
                    assert top is None
                    continue
                got = m._cut(top, md)
                assert got["npos"] == want["npos"] and all(np.array_equal(got[k], want[k]) for k in ("scores", "dtm", "dig"))


def test_curves():
    preds, targets = orc.scene(2, n_img=24, classes=(1, 2))
    m, out = _host(preds, targets)
    curves, cnt = m.miss_rate_curves(), m.miss_rate_counts()
    want, _ = orc.evaluate(preds, targets)
    assert sorted(curves) == [1, 2]
    for k, c in enumerate(cnt["classes"]):
        if c not in curves:
            continue
        cv = curves[c]
        n = int(cnt["total"][0, k, 0].sum())                      # one point per non-ignored detection
        assert cv["n_images"] == 24 and cv["n_gt"] == cnt["n_gt"][k, 0]
        for key in ("score", "fppi", "miss_rate"):
            assert cv[key].dtype == np.float64 and cv[key].shape == (n,)
        assert (np.diff(cv["fppi"]) >= 0).all() and (np.diff(cv["score"]) <= 0).all() and (np.diff(cv["miss_rate"]) <= 0).all()
        assert cv["miss_rate"][-1] == 1.0 - cnt["total"][0, k, 0, 0] / cv["n_gt"]
        # hit, recovered from the curve: the smallest miss rate among the points with fppi <= ref
        hit = [int(round((1.0 - cv["miss_rate"][cv["fppi"] <= r].min()) * cv["n_gt"])) if (cv["fppi"] <= r).any() else 0 for r in m.REF_FPPI]
        assert hit == cnt["hit"][0, k, 0].tolist()
        assert np.allclose(cv["fppi"], want[c]["fppi"], rtol=0, atol=0) and np.allclose(cv["miss_rate"], want[c]["miss_rate"], rtol=1e-15, atol=0)
        assert cv["score"].tolist() == want[c]["score"]
    m.reset()
    assert m.miss_rate_curves() == {}


def test_detection_wrapper_and_to_carry_the_option():
    d = Detection(miss_rate=True, class_metrics=True).map
    assert type(d) is MeanAveragePrecision and d.miss_rate and d.class_metrics and d.to("cpu") is d
    assert not Detection().map.miss_rate


def test_trainer_treats_minus_one_as_no_data_for_the_new_keys():
    from hallucidet_amd.trainer import Trainer
    flat = Trainer._flat({"lamr": torch.tensor(-1.0), "lamr_75": torch.tensor(0.25), "mr_fppi01": torch.tensor(-1.0), "map": torch.tensor(-1.0),
                          "lamr_per_class": torch.tensor([0.1, 0.2])})
    assert set(flat) == {"lamr", "lamr_75", "mr_fppi01", "map"}
    got = Trainer._nanmean_over_ranks(dict(flat, val_loss=(3.0, 2), other=-1.0))
    assert got == {"lamr": -1.0, "lamr_75": 0.25, "mr_fppi01": -1.0, "map": -1.0, "val_loss": 1.5, "other": -1.0}
    assert all(Trainer._no_data(k, -1.0) for k in ("lamr", "lamr_small", "mr_fppi01", "map_hall/lamr", "map_50"))
    assert not Trainer._no_data("other", -1.0) and not Trainer._no_data("lamr", 0.5) and Trainer._no_data("x", float("nan"))


def test_flags_parse_and_the_scripts_print_the_lamr_lines(capsys, tmp_path):
    from hallucidet_amd.config import Config
    import train_hallucidet as script
    a = Config.argument_parser([])
    assert a.miss_rate is False and a.miss_rate_curves is None and Config.miss_rate_kwargs(a) == dict(miss_rate=False, miss_rate_curves=None)
    a = Config.argument_parser(["--miss-rate"])
    assert Config.miss_rate_kwargs(a) == dict(miss_rate=True, miss_rate_curves=None)
    a = Config.argument_parser(["--miss-rate-curves", str(tmp_path)])
    assert Config.miss_rate_kwargs(a) == dict(miss_rate=True, miss_rate_curves=str(tmp_path))           # implies --miss-rate
    maps = {"map_ir": {"map_50": torch.tensor(0.5), "lamr": torch.tensor(0.25)}, "map_rgb": {"map_50": torch.tensor(0.25), "lamr": torch.tensor(0.5)},
            "map_hall": {"map_50": torch.tensor(0.75), "lamr": torch.tensor(0.125)}}
    script.print_ap50(maps)
    assert capsys.readouterr().out == ("RGB Detector on IR  AP@50:  50.0\nRGB Detector on IR  LAMR:  25.0\nRGB Detector on RGB AP@50:  25.0\n"
                                       "RGB Detector on RGB LAMR:  50.0\nHalluciDet   on IR  AP@50:  75.0\nHalluciDet   on IR  LAMR:  12.5\n")
    script.print_ap50({k: {"map_50": v["map_50"]} for k, v in maps.items()})
    assert "LAMR" not in capsys.readouterr().out


def test_curve_files(tmp_path):
    from hallucidet_amd.metrics import write_miss_rate_curves
    preds, targets = orc.worked_case()
    m, _ = _host(preds, targets)
    paths = write_miss_rate_curves(m, str(tmp_path / "curves"), "test", "hall")
    assert [p.split("/")[-1] for p in paths] == ["test_hall_class1.csv"]
    rows = open(paths[0]).read().splitlines()
    assert rows[0] == "score,fppi,miss_rate" and len(rows) == 10
    last = [float(v) for v in rows[-1].split(",")]
    assert last[1] == 5 / 4 and last[2] == 1.0 - 4 / 5
    cv = m.miss_rate_curves()[1]
    assert [float(r.split(",")[2]) for r in rows[1:]] == cv["miss_rate"].tolist()          # repr round-trips float64
