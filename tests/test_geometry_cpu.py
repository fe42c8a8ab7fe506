"""The paired geometric augmentation on the host: `apply_host` against the independent oracle (tests/_geometry_oracle.py) byte for byte
and against a float64 bilinear resize within the fp32 rounding bound; the draw's properties; the box transform; the flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from hypothesis import given, settings
from hypothesis import strategies as st

import _geometry_oracle as O
from _geometry_cases import KINDS, SHAPES, case_rows, image
from _synth_llvip import make_tree
from hallucidet_amd.dataloader import geometry as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ pixels
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hw", SHAPES)
def test_apply_host_equals_the_oracle(hw, kind):
    H, W = hw
    rows = case_rows(H, W)
    base = image(kind, 5, 3, H, W)
    for c in (1, 3):
        x = base[[i % 5 for i in range(rows.shape[0])], :c].contiguous()
        got = G.apply_host(x, rows)
        want = torch.from_numpy(O.batch(x.numpy(), rows.tolist()))
        assert got.dtype == torch.uint8 and got.shape == x.shape
        bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, (hw, kind, c, [rows[i].tolist() for i in bad[:3]])


def _float64_reference(x, row):
    """F.interpolate in float64 of the crop of the (flipped) image; x: uint8 [C, H, W]"""
    flip, x0, y0, x1, y1 = row[:5]
    src = torch.flip(x, dims=[2]) if flip else x
    crop = src[:, y0:y1, x0:x1].double()[None]
    return F.interpolate(crop, size=tuple(x.shape[1:]), mode="bilinear", align_corners=False)[0].numpy()


BOUND = 8 * 2.0 ** -24 * 255          # eight fp32 roundings at magnitude <= 255, first order


def _drawn_rows(H, W, n, seed):
    """n drawn records with crops: one random box per image"""
    g = np.random.RandomState(seed)
    targets = []
    for _ in range(n):
        xa, ya = g.uniform(0, W - 2), g.uniform(0, H - 2)
        targets.append({"boxes": torch.tensor([[xa, ya, g.uniform(xa + 1, W), g.uniform(ya + 1, H)]], dtype=torch.float64)})
    return G.PairedGeometry(p_flip=0.5, p_crop=1.0, min_scale=0.3, seed=seed).params_for([targets], H, W, 0)


# seeded records whose float64 values rarely sit on a half-integer (a 9-row image has too few distinct weights for that: its ties
# exceed the 1 % the test may leave undecided, asserted below)
@pytest.mark.parametrize("hw", [(37, 53), (64, 80), (23, 45)])
def test_agreement_with_the_float64_resize(hw):
    H, W = hw
    rows = torch.cat([_drawn_rows(H, W, 10, seed=H), G.make_row(H=H, W=W)[None], G.make_row(flip=True, H=H, W=W)[None]])
    assert len({tuple(r) for r in rows.tolist()}) >= 10
    x = image("noise", rows.shape[0], 3, H, W, seed=4)
    got = G.apply_host(x, rows).numpy()
    skipped = total = 0
    for n, row in enumerate(rows.tolist()):
        v = G.resample_host_image(x[n].numpy(), row)
        v64 = _float64_reference(x[n], row)
        assert v.dtype == np.float32 and float(np.abs(v.astype(np.float64) - v64).max()) <= BOUND, (hw, row)
        far = np.abs(v64 - np.floor(v64) - 0.5) > BOUND          # farther than the bound from a half-integer: the byte is decided
        assert np.array_equal(got[n][far], np.floor(v64 + 0.5).astype(np.uint8)[far]), (hw, row)
        skipped += int((~far).sum())
        total += far.size
    assert skipped <= 0.01 * total, (skipped, total)


@pytest.mark.parametrize("hw", SHAPES)
def test_identity_row_returns_the_input_and_flip_is_torch_flip(hw):
    H, W = hw
    for c in (1, 3):
        x = image("noise", 2, c, H, W, seed=2)
        ident = torch.stack([G.make_row(H=H, W=W)] * 2)
        assert ident[0].tolist() == [0, 0, 0, W, H, 0, 0, 0]
        assert torch.equal(G.apply_host(x, ident), x)
        flip = torch.stack([G.make_row(flip=True, H=H, W=W)] * 2)
        assert torch.equal(G.apply_host(x, flip), torch.flip(x, dims=[3]))


def test_apply_host_validates():
    x = torch.zeros(1, 3, 8, 16, dtype=torch.uint8)
    for bad in ([0, 0, 0, 17, 8], [0, 4, 0, 4, 8], [0, -1, 0, 4, 8], [2, 0, 0, 16, 8], [0, 0, 0, 16, 9], [0, 0, 5, 16, 5]):
        with pytest.raises(ValueError, match="row 0"):
            G.apply_host(x, torch.tensor([bad + [0, 0, 0]], dtype=torch.int32))
    with pytest.raises(ValueError, match="row 0"):
        G.apply_host(x, torch.tensor([[0, 0, 0, 16, 8, 0, 1, 0]], dtype=torch.int32))
    with pytest.raises(ValueError, match="rows must be"):
        G.apply_host(x, torch.zeros(2, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="images must be"):
        G.apply_host(x.float(), G.make_row(H=8, W=16)[None])


# ------------------------------------------------------------------------------------------------ the draw
def _scene(n, H, W, seed, empty_every=4):
    """n paired targets: RGB and IR boxes differ slightly, some reach outside the image, every `empty_every`-th image has none"""
    g = np.random.RandomState(seed)
    rgb, ir = [], []
    for i in range(n):
        k = 0 if i % empty_every == empty_every - 1 else g.randint(1, 4)
        xa, ya = g.uniform(-3, W - 2, k), g.uniform(-3, H - 2, k)
        b = np.stack([xa, ya, xa + g.uniform(1, W / 2, k), ya + g.uniform(1, H / 2, k)], 1).reshape(-1, 4)
        rgb.append({"boxes": torch.from_numpy(b), "labels": torch.ones(k, dtype=torch.int64)})
        ir.append({"boxes": torch.from_numpy(b + g.uniform(-1, 1, b.shape)), "labels": torch.ones(k, dtype=torch.int64)})
    return rgb, ir


def _check_rows_against_scene(rows, groups, H, W, min_scale):
    mw, mh = math.ceil(min_scale * W), math.ceil(min_scale * H)
    for i, (flip, x0, y0, x1, y1, *rest) in enumerate(rows.tolist()):
        assert rest == [0, 0, 0] and flip in (0, 1)
        assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H and x1 - x0 >= mw and y1 - y0 >= mh
        boxes = torch.cat([g[i]["boxes"].reshape(-1, 4).double() for g in groups])
        if boxes.numel() == 0:
            assert (x0, y0, x1, y1) == (0, 0, W, H)          # an image without boxes is never cropped
            continue
        bx0, bx1 = float(boxes[:, 0].min()), float(boxes[:, 2].max())
        if flip:
            bx0, bx1 = W - bx1, W - bx0
        assert x0 <= max(bx0, 0) and min(bx1, W) <= x1, (i, rows[i].tolist())
        assert y0 <= max(float(boxes[:, 1].min()), 0) and min(float(boxes[:, 3].max()), H) <= y1, (i, rows[i].tolist())


def test_draw_is_a_pure_function_of_its_key_and_the_boxes():
    H, W = 48, 64
    scene = _scene(16, H, W, seed=1)

    def rec(seed=1, epoch=2, rank=3, batch=4, groups=scene):
        a = G.PairedGeometry(p_crop=1.0, seed=seed, rank=rank)
        a.set_epoch(epoch)
        return a.params_for(groups, H, W, batch)
    base = rec()
    assert base.shape == (16, G.ROW) and base.dtype == torch.int32
    assert torch.equal(base, rec())
    assert torch.equal(base, G.PairedGeometry(p_crop=1.0, seed=1, rank=3).params_for(scene, H, W, 4, epoch=2))
    for other in (rec(seed=2), rec(epoch=3), rec(rank=4), rec(batch=5), rec(groups=_scene(16, H, W, seed=2))):
        assert not torch.equal(base, other)
    # independent of the photometric draws of the same key: another generator seed
    from hallucidet_amd.dataloader.augment import ReferenceAugmentation
    assert G.PairedGeometry(seed=1).generator(0).initial_seed() != ReferenceAugmentation(seed=1).generator(0).initial_seed()


@pytest.mark.parametrize("hw,min_scale", [((48, 64), 0.5), ((37, 53), 0.3), ((512, 640), 0.75), ((9, 16), 1.0)])
def test_drawn_crops_are_box_safe(hw, min_scale):
    H, W = hw
    for batch in range(6):
        groups = _scene(32, H, W, seed=batch)
        rows = G.PairedGeometry(p_flip=0.5, p_crop=1.0, min_scale=min_scale, seed=9).params_for(groups, H, W, batch)
        _check_rows_against_scene(rows, groups, H, W, min_scale)
        if min_scale < 1:
            assert any(r[1:5] != [0, 0, W, H] for r in rows.tolist())
    hflip = G.PairedGeometry(p_crop=0.0, seed=9).params_for(_scene(32, H, W, seed=0), H, W, 0)
    assert all(r[1:5] == [0, 0, W, H] for r in hflip.tolist())          # 'hflip': never a crop


box = st.tuples(st.floats(-8, 72), st.floats(-8, 56), st.floats(0.5, 40), st.floats(0.5, 40))


@settings(max_examples=150, deadline=None)
@given(st.lists(st.lists(box, max_size=3), min_size=1, max_size=4), st.integers(0, 10 ** 6), st.floats(0.05, 1.0), st.integers(2, 70),
       st.integers(2, 70))
def test_draw_properties_under_hypothesis(images, key, min_scale, H, W):
    targets = [{"boxes": torch.tensor([[x, y, x + w, y + h] for x, y, w, h in im], dtype=torch.float64).reshape(-1, 4)} for im in images]
    geo = G.PairedGeometry(p_flip=0.5, p_crop=1.0, min_scale=min_scale, seed=key)
    rows = geo.params_for([targets], H, W, key % 7)
    G.check_rows(rows, len(targets), H, W)
    _check_rows_against_scene(rows, [targets], H, W, min_scale)
    assert torch.equal(rows, geo.params_for([targets], H, W, key % 7))


def test_flip_rate():
    geo = G.PairedGeometry(seed=3)
    empty = [{"boxes": torch.zeros(0, 4)}] * 40
    flips = sum(int(geo.params_for([empty], 32, 32, b)[:, 0].sum()) for b in range(100))
    assert abs(flips / 4000 - 0.5) <= 0.04, flips


def test_constructor_validates():
    for kw in (dict(p_flip=1.5), dict(p_crop=-0.1), dict(min_scale=0.0), dict(min_scale=1.5)):
        with pytest.raises(ValueError):
            G.PairedGeometry(**kw)


# ------------------------------------------------------------------------------------------------ boxes
def test_box_edges_land_where_pixel_edges_land():
    H, W = 48, 64
    for flip in (False, True):
        row = G.make_row(flip=flip, x0=8, y0=6, x1=40, y1=30)
        # the crop window as a box of the flipped image = [W - x1, W - x0] of the image when flip
        xs = (W - 40.0, W - 8.0) if flip else (8.0, 40.0)
        t = {"boxes": torch.tensor([[xs[0], 6.0, xs[1], 30.0]], dtype=torch.float64), "labels": torch.tensor([1]), "path_image": "a.jpg"}
        out = G.transform_targets(row[None], [t], H, W)[0]
        assert out["boxes"].tolist() == [[0.0, 0.0, float(W), float(H)]]
        assert out["labels"] is t["labels"] and out["path_image"] == "a.jpg" and list(out) == list(t)
        assert t["boxes"].tolist() == [[xs[0], 6.0, xs[1], 30.0]]           # the input is not modified


def test_flipping_twice_is_the_identity_and_dtypes_are_kept():
    H, W = 48, 64
    flip = G.make_row(flip=True, H=H, W=W)[None]
    for dtype in (torch.float64, torch.float32):
        t = [{"boxes": torch.tensor([[3.0, 5.0, 20.5, 31.0], [10.0, 1.0, 64.0, 48.0]], dtype=dtype), "labels": torch.tensor([1, 1])}]
        once = G.transform_targets(flip, t, H, W)
        assert once[0]["boxes"].dtype == dtype and once[0]["boxes"].tolist() == [[43.5, 5.0, 61.0, 31.0], [0.0, 1.0, 54.0, 48.0]]
        twice = G.transform_targets(flip, once, H, W)
        assert torch.equal(twice[0]["boxes"], t[0]["boxes"]) and twice[0]["boxes"].dtype == dtype
        crop = G.transform_targets(G.make_row(x0=2, y0=1, x1=34, y1=25)[None], t, H, W)[0]["boxes"]
        assert crop.dtype == dtype and crop[0].tolist() == [2.0, 8.0, 37.0, 60.0]
    empty = [{"boxes": torch.zeros(0, 4, dtype=torch.float64), "labels": torch.zeros(0, dtype=torch.int64)}]
    out = G.transform_targets(G.make_row(flip=True, x0=2, y0=1, x1=34, y1=25)[None], empty, H, W)
    assert out[0]["boxes"].shape == (0, 4) and out[0]["boxes"].dtype == torch.float64
    with pytest.raises(ValueError, match="rows for"):
        G.transform_targets(flip, t + t, H, W)


def test_drawn_boxes_stay_inside_the_image():
    H, W = 48, 64
    rgb, ir = _scene(64, H, W, seed=5)
    clip = lambda ts: [{"boxes": t["boxes"].clamp(min=0).clamp(max=torch.tensor([W, H, W, H], dtype=torch.float64))} for t in ts]
    rgb, ir = clip(rgb), clip(ir)
    rows = G.PairedGeometry(p_crop=1.0, seed=2).params_for([rgb, ir], H, W, 0)
    for ts in (rgb, ir):
        for t in G.transform_targets(rows, ts, H, W):
            b = t["boxes"]
            if b.numel():
                assert float(b.min()) >= 0 and float(b[:, [0, 2]].max()) <= W and float(b[:, [1, 3]].max()) <= H


# ------------------------------------------------------------------------------------------------ prefetcher on a CPU device
@pytest.fixture(scope="module")
def llvip(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("geo"), n_train=6, n_test=2, hw=(32, 48), extra_objects=False)


def test_prefetcher_cpu_path(llvip):
    from hallucidet_amd.dataloader import DevicePrefetcher, MultiModalDataModule, SingleModalDataModule
    H, W = 32, 48
    geo = G.PairedGeometry(p_crop=1.0, seed=4)
    dm = MultiModalDataModule("llvip", llvip, llvip, llvip, llvip, batch_size=2, num_workers=0, ext=".jpg")
    loader = dm.test_dataloader()
    raw = list(loader)
    got = list(DevicePrefetcher(loader, device="cpu", geometry=geo))
    assert len(got) == len(raw) == 1
    for b, (r, g) in enumerate(zip(raw, got)):
        rows = geo.params_for([r[1], r[3]], H, W, b)
        assert any(row[1:5] != [0, 0, W, H] for row in rows.tolist())
        for k in (0, 2):
            want = G.apply_host(torch.stack(list(r[k])), rows).float().div_(255.0)
            assert torch.equal(g[k], want)
            for t, w in zip(g[k + 1], G.transform_targets(rows, r[k + 1], H, W)):
                assert torch.equal(t["boxes"], w["boxes"]) and t["boxes"].dtype == torch.float64 and torch.equal(t["labels"], w["labels"])
    sm = SingleModalDataModule("llvip", llvip, llvip, batch_size=2, num_workers=0, ext=".jpg", modality="ir")
    raw = list(sm.test_dataloader())
    got = list(DevicePrefetcher(sm.test_dataloader(), device="cpu", geometry=geo))
    rows = geo.params_for([raw[0][1]], H, W, 0)
    assert torch.equal(got[0][0], G.apply_host(torch.stack(list(raw[0][0])), rows).float().div_(255.0))
    assert got[0][1][0]["path_image"] == raw[0][1][0]["path_image"]
    plain = list(DevicePrefetcher(sm.test_dataloader(), device="cpu"))
    assert torch.equal(plain[0][0], torch.stack(list(raw[0][0])).float().div_(255.0))          # off: what it was


# ------------------------------------------------------------------------------------------------ flags, trainer, C entry
def test_geometry_options(monkeypatch):
    from hallucidet_amd.config import Config
    a = Config.argument_parser([])
    assert a.augment_geometry == "none" and a.geometry_min_scale == 0.5 and Config.train_geometry(a) is None
    a = Config.argument_parser(["--augment-geometry", "hflip", "--seed", "7"])
    g = Config.train_geometry(a, rank=2)
    assert (g.p_flip, g.p_crop, g.min_scale, g.seed, g.rank) == (0.5, 0.0, 0.5, 7, 2)
    g = Config.train_geometry(Config.argument_parser(["--augment-geometry", "hflip_crop", "--geometry-min-scale", "0.8"]))
    assert (g.p_flip, g.p_crop, g.min_scale) == (0.5, 0.5, 0.8)
    with pytest.raises(SystemExit):
        Config.argument_parser(["--augment-geometry", "vflip"])
    monkeypatch.syspath_prepend(ROOT)
    import eval_hallucidet
    import train_hallucidet
    for mode in ("hflip", "hflip_crop"):
        with pytest.raises(SystemExit, match="--augment-geometry %s is an option of the training scripts" % mode):
            eval_hallucidet.main(["--augment-geometry", mode])
    # the photometric set is still rejected for the paired training, in the words it always was
    with pytest.raises(SystemExit, match="--augment reference is an option of train_detector.py"):
        train_hallucidet.main(["--augment", "reference", "--augment-geometry", "hflip_crop"])


def test_training_scripts_pass_the_option_on(monkeypatch):
    """train_hallucidet.py (paired) and train_detector.py (with --augment reference and --cache-dataset hbm) accept the flag: their
    Trainer receives the PairedGeometry.  Data module and model are stand-ins; the scripts are cut short where they build the Trainer."""
    monkeypatch.syspath_prepend(ROOT)
    import train_detector
    import train_hallucidet

    class Stop(Exception):
        pass

    class Model:
        def __init__(self, **kw):
            pass

        def prepare(self):
            pass

    def trainer(**kw):
        raise Stop(kw)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    for mod, dm, lit, extra in ((train_hallucidet, "MultiModalDataModule", "EncoderDecoderLit", []),
                                (train_detector, "SingleModalDataModule", "DetectorLit", ["--augment", "reference", "--cache-dataset", "hbm"])):
        monkeypatch.setattr(mod, dm, lambda *a, **kw: None)
        monkeypatch.setattr(mod, lit, Model)
        monkeypatch.setattr(mod, "Trainer", trainer)
        with pytest.raises(Stop) as e:
            mod.main(["--augment-geometry", "hflip_crop", "--geometry-min-scale", "0.6", "--seed", "5"] + extra)
        g = e.value.args[0]["train_geometry"]
        assert isinstance(g, G.PairedGeometry) and (g.p_crop, g.min_scale, g.seed, g.rank) == (0.5, 0.6, 5, 0)
        with pytest.raises(Stop) as e:
            mod.main(extra)
        assert e.value.args[0]["train_geometry"] is None                     # off by default
        if extra:
            assert e.value.args[0]["train_augment"] is not None


def test_trainer_takes_the_geometry():
    from hallucidet_amd.trainer import Trainer
    geo = G.PairedGeometry()
    assert Trainer(device="cpu", train_geometry=geo).train_geometry is geo and Trainer(device="cpu").train_geometry is None


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hallucidet_amd import _abi
    return _abi.load()


def test_hd_geometry_u8_rejects_bad_arguments(lib):
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.hd_geometry_u8(None, 1, None, None, 1, 3, 8, 8, 0, None, None) == -1 and b"null" in lib.hd_last_error()
    assert lib.hd_geometry_u8(p, 1, None, p, 1, 2, 8, 8, 0, p, None) == -1 and b"C in (1, 3)" in lib.hd_last_error()
    assert lib.hd_geometry_u8(p, 1, None, p, 1, 3, 1, 8, 0, p, None) == -1
    assert lib.hd_geometry_u8(p, 1, None, p, 1, 3, 8, 16385, 0, p, None) == -1 and b"16384" in lib.hd_last_error()
    assert lib.hd_geometry_u8(p, 0, None, p, 0, 3, 8, 8, 0, p, None) == -1
    assert lib.hd_geometry_u8(p, 1, None, p, 65536, 3, 8, 8, 0, p, None) == -1
    assert lib.hd_geometry_u8(p, 2, None, p, 1, 3, 8, 8, 0, p, None) == -1 and b"dense" in lib.hd_last_error()
    assert lib.hd_geometry_u8(p, 0, p, p, 1, 3, 8, 8, 0, p, None) == -1
    assert lib.hd_geometry_u8(p, 1, None, p, 1, 3, 8, 8, 2, p, None) == -1 and b"mode" in lib.hd_last_error()


def test_c_row_validation_agrees_with_the_host_check(lib):
    H, W = 8, 16
    good = [[0, 0, 0, 16, 8], [1, 15, 7, 16, 8], [1, 0, 0, 1, 1]]
    bad = [[0, 0, 0, 17, 8], [0, 4, 0, 4, 8], [0, -1, 0, 4, 8], [2, 0, 0, 16, 8], [0, 0, 0, 16, 9], [0, 0, 5, 16, 5], [0, 5, 0, 4, 8]]
    for r, ok in [(r, True) for r in good] + [(r, False) for r in bad]:
        rows = torch.tensor([good[0] + [0, 0, 0], r + [0, 0, 0]], dtype=torch.int32)
        rc = lib.hd_geometry_check_rows(rows.data_ptr(), 2, H, W)
        assert (rc == 0) == ok, r
        if ok:
            G.check_rows(rows, 2, H, W)
        else:
            assert b"row 1" in lib.hd_last_error()
            with pytest.raises(ValueError, match="row 1"):
                G.check_rows(rows, 2, H, W)
    rows = torch.tensor([[0, 0, 0, 16, 8, 0, 0, 3]], dtype=torch.int32)
    assert lib.hd_geometry_check_rows(rows.data_ptr(), 1, H, W) == -1 and b"reserved" in lib.hd_last_error()
    assert lib.hd_geometry_check_rows(None, 1, H, W) == -1


def test_ops_wrapper_validates(monkeypatch, lib):
    from hallucidet_amd import ops
    x, rows = torch.zeros(2, 3, 8, 16, dtype=torch.uint8), torch.stack([G.make_row(H=8, W=16)] * 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.geometry_u8(x, rows)
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)       # reach the checks without a GPU; no call below passes them
    with pytest.raises(ValueError, match="mode"):
        ops.geometry_u8(x, rows, mode="f32_default")
    with pytest.raises(ValueError, match="src must be"):
        ops.geometry_u8(x.float(), rows)
    with pytest.raises(ValueError, match="C in"):
        ops.geometry_u8(torch.zeros(2, 2, 8, 16, dtype=torch.uint8), rows)
    with pytest.raises(ValueError, match="2 <= H, W"):
        ops.geometry_u8(torch.zeros(2, 1, 1, 16, dtype=torch.uint8), rows)
    with pytest.raises(ValueError, match="rows must be"):
        ops.geometry_u8(x, rows[:1])
    with pytest.raises(ValueError, match="rows must be"):
        ops.geometry_u8(x, rows.long())
    bad = rows.clone()
    bad[1, 3] = 17
    with pytest.raises(ValueError, match="row 1"):
        ops.geometry_u8(x, bad)
    with pytest.raises(IndexError):
        ops.geometry_u8(x, rows, idx=[0, 2])
    with pytest.raises(ValueError, match="idx_host without idx"):
        ops.geometry_u8(x, rows, idx_host=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="out must be"):
        ops.geometry_u8(x, rows, out=torch.zeros(2, 3, 8, 16))
    with pytest.raises(ValueError, match="out must be"):
        ops.geometry_u8(x, rows, mode="f32_ieee", out=torch.zeros(2, 3, 8, 16, dtype=torch.uint8))


def test_constants_agree_with_the_header():
    from hallucidet_amd import ops
    src = open(os.path.join(ROOT, "include", "hallucidet_hip.h")).read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
    assert val("HD_GEOM_ROW") == ops.GEOM_ROW == G.ROW == G.make_row(H=4, W=4).numel()
    assert val("HD_GEOM_MAX_EXTENT") == ops.GEOM_MAX_EXTENT == G.MAX_EXTENT and 2 * G.MAX_EXTENT ** 2 < 2 ** 31
    assert val("HD_GEOM_MAX_BATCH") == ops.GEOM_MAX_BATCH
    assert ops.GEOM_MODES == {"u8": val("HD_GEOM_U8"), "f32_ieee": val("HD_GEOM_F32_IEEE")}
