"""The reference's detector-training augmentation (--augment reference) without a GPU: `apply_host` against Pillow bit for bit, the
parameter draw, the CPU path of DevicePrefetcher, the CLI option, and hd_augment_u8's argument checks at the C boundary."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from _augment_oracle import all_colours, forced_rows, image, pil_apply, pil_hue, single_op_rows, to_pil
from _synth_llvip import make_tree
from hallucidet_amd.dataloader import augment as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(kind, c, 96, 128) for kind in ("uniform", "smooth", "narrow", "const") for c in (3, 1)] + \
        [("twolevel", 3, 64, 80), ("twolevel", 1, 64, 80), ("uniform", 3, 127, 161), ("uniform", 1, 127, 161), ("uniform", 3, 3, 3),
         ("uniform", 1, 3, 3)]


@pytest.mark.parametrize("kind,c,h,w", CASES)
def test_apply_host_equals_pillow_op_by_op(kind, c, h, w):
    x = image(kind, c, h, w, seed=1)[None]
    rows = single_op_rows()
    for f in (0.99, 1.0, 1.01, 1.2):       # the enhance operations over the factor range, 1.2 = the clipping branch of blend
        rows += [A.make_row(order=(op,), brightness=f, contrast=f, saturation=f) for op in range(3)]
    rows += [A.make_row(order=(A.HUE,), hue=hf) for hf in (-0.01, -0.004, 0.0, 0.004, 0.01)]
    rows.append(A.make_row(sharpness=True, sharpness_factor=0.5))
    for r in rows:
        got, want = A.apply_host(x, r[None]), pil_apply(x, r[None])
        assert torch.equal(got, want), (kind, c, r.tolist(), int((got != want).sum()))


@pytest.mark.parametrize("kind,c,h,w", CASES)
def test_apply_host_equals_pillow_on_pipelines(kind, c, h, w):
    x = image(kind, c, h, w, seed=2)[None]
    aug = A.ReferenceAugmentation(p_invert=0.5, p_sharpness=0.5, p_equalize=0.5, seed=7)
    rows = forced_rows() + list(aug.params_for(12, 0))
    for r in rows:
        got, want = A.apply_host(x, r[None]), pil_apply(x, r[None])
        assert torch.equal(got, want), (kind, c, r.tolist(), int((got != want).sum()))


def test_hue_shift_on_every_colour():
    x = all_colours()
    im = to_pil(x[0].numpy())
    hwc = np.ascontiguousarray(x[0].numpy().transpose(1, 2, 0))
    for shift in (-2, 0, 2):
        got = A.hue(hwc, shift)
        want = np.asarray(pil_hue(im, shift))
        assert np.array_equal(got, want), (shift, int((got != want).sum()))


def test_small_images_raise():
    with pytest.raises(ValueError, match="3 x 3"):
        A.apply_host(torch.zeros(1, 3, 2, 5, dtype=torch.uint8), A.make_row()[None])


def test_draw_is_a_pure_function_of_seed_epoch_rank_batch():
    def rec(seed=1, epoch=2, rank=3, batch=4):
        a = A.ReferenceAugmentation(seed=seed, rank=rank)
        a.set_epoch(epoch)
        return a.params_for(16, batch)
    base = rec()
    assert base.shape == (16, A.ROW) and base.dtype == torch.float32
    assert torch.equal(base, rec())
    for kw in (dict(seed=2), dict(epoch=3), dict(rank=4), dict(batch=5)):
        assert not torch.equal(base, rec(**kw)), kw


def test_draw_distribution():
    aug = A.ReferenceAugmentation(seed=11)
    rows = aug.draw(20000, torch.Generator().manual_seed(5))
    b, c, s, h = (rows[:, i].double() for i in (4, 5, 6, 7))
    for v in (b, c, s):
        assert 0.99 <= float(v.min()) and float(v.max()) <= 1.01 and float(v.max() - v.min()) > 0.019
    assert -0.01 <= float(h.min()) and float(h.max()) <= 0.01 and float(h.max() - h.min()) > 0.019
    orders = {tuple(int(o) for o in r) for r in rows[:, 0:4].tolist()}
    assert orders == set(itertools.permutations(range(4)))
    for col in (8, 9, 10):
        assert set(rows[:, col].tolist()) <= {0.0, 1.0}
        assert abs(float(rows[:, col].mean()) - 0.1) <= 0.01, (col, float(rows[:, col].mean()))
    assert torch.all(rows[:, 11] == np.float32(1.2))
    # an operation whose range is zero is left out of the order, as ColorJitter leaves it out
    rows = A.ReferenceAugmentation(hue=0.0).draw(64, torch.Generator().manual_seed(1))
    assert not (rows[:, 0:4] == A.HUE).any() and ((rows[:, 0:4] == -1).sum(1) == 1).all()


@pytest.fixture()
def llvip(tmp_path):
    return make_tree(tmp_path)


def test_prefetcher_cpu_path(llvip):
    from hallucidet_amd.dataloader import DevicePrefetcher, MultiModalDataModule, SingleModalDataModule
    for modality in ("rgb", "ir"):
        dm = SingleModalDataModule("llvip", llvip, llvip, batch_size=2, num_workers=0, ext=".jpg", modality=modality)
        loader = dm.test_dataloader()
        raw = list(loader)
        plain = list(DevicePrefetcher(loader, device="cpu"))
        none = list(DevicePrefetcher(loader, device="cpu", augment=None))
        aug = A.ReferenceAugmentation(p_invert=0.5, p_sharpness=0.5, p_equalize=0.5, seed=3)
        aug.set_epoch(2)
        got = list(DevicePrefetcher(loader, device="cpu", augment=aug))
        assert len(raw) == len(plain) == len(got) == 1
        for i, (rb, pb, nb, gb) in enumerate(zip(raw, plain, none, got)):
            u8 = torch.stack(list(rb[0]))
            assert torch.equal(pb[0], u8.float() / 255.0) and torch.equal(nb[0], pb[0])
            want = A.apply_host(u8, aug.params_for(len(rb[0]), i)).float() / 255.0
            assert torch.equal(gb[0], want) and not torch.equal(gb[0], pb[0])
            for t_raw, t_got in zip(rb[1], gb[1]):
                assert torch.equal(t_raw["boxes"], t_got["boxes"]) and torch.equal(t_raw["labels"], t_got["labels"])
                assert t_raw["path_image"] == t_got["path_image"]
    dm = MultiModalDataModule("llvip", llvip, llvip, llvip, llvip, batch_size=2, num_workers=0, ext=".jpg")
    with pytest.raises(ValueError, match="single-modal"):
        list(DevicePrefetcher(dm.test_dataloader(), device="cpu", augment=A.ReferenceAugmentation()))


def test_augment_option(monkeypatch):
    from hallucidet_amd.config import Config
    assert Config.argument_parser([]).augment == "none"
    assert Config.argument_parser(["--augment", "reference"]).augment == "reference"
    with pytest.raises(SystemExit):
        Config.argument_parser(["--augment", "albumentations"])
    monkeypatch.syspath_prepend(ROOT)
    import eval_hallucidet
    import train_hallucidet
    for mod in (train_hallucidet, eval_hallucidet):
        with pytest.raises(SystemExit, match="--augment reference is an option of train_detector.py"):
            mod.main(["--augment", "reference"])


def test_trainer_takes_the_augmentation():
    from hallucidet_amd.trainer import Trainer
    aug = A.ReferenceAugmentation()
    assert Trainer(device="cpu", train_augment=aug).train_augment is aug and Trainer(device="cpu").train_augment is None


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hallucidet_amd import _abi
    return _abi.load()


def test_hd_augment_u8_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.hd_augment_u8(None, None, 1, 3, 8, 8, None, None, None) == -1 and b"null" in lib.hd_last_error()
    assert lib.hd_augment_u8(p, p, 1, 2, 8, 8, p, p, None) == -1 and b"C in {1, 3}" in lib.hd_last_error()
    assert lib.hd_augment_u8(p, p, 1, 3, 2, 8, p, p, None) == -1
    assert lib.hd_augment_u8(p, p, 1, 3, 8192, 8192, p, p, None) == -1 and b"16843009" in lib.hd_last_error()
    assert lib.hd_augment_u8_ws_bytes(1, 3, 2, 2) == -1
    n = lib.hd_augment_u8_ws_bytes(16, 3, 512, 640)
    assert n >= 16 * 3 * 512 * 640 + 4 * (16 + 16 * 3 * 256) and n % 256 == 0


def test_ops_wrapper_validates(monkeypatch, lib):
    from hallucidet_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.augment_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), A.make_row()[None])
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)       # reach the shape checks without a GPU; no check below passes on
    x, rows = torch.zeros(2, 3, 8, 8, dtype=torch.uint8), A.make_row()[None].repeat(2, 1)
    with pytest.raises(ValueError, match="params"):
        ops.augment_u8(x, rows[:1])
    with pytest.raises(ValueError, match="params"):
        ops.augment_u8(x, rows.double())
    with pytest.raises(ValueError, match="uint8"):
        ops.augment_u8(x.float(), rows)
    with pytest.raises(ValueError, match="H, W >= 3"):
        ops.augment_u8(torch.zeros(2, 3, 2, 8, dtype=torch.uint8), rows)
    with pytest.raises(ValueError, match="out must"):
        ops.augment_u8(x, rows, out=torch.zeros(2, 3, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="ws must"):
        ops.augment_u8(x, rows, ws=torch.zeros(16, dtype=torch.uint8))
    assert ops.augment_ws_bytes((16, 3, 512, 640)) == lib.hd_augment_u8_ws_bytes(16, 3, 512, 640)
    with pytest.raises(ValueError):
        ops.augment_ws_bytes((1, 2, 8, 8))


def test_constants_agree_with_the_header():
    import re
    from hallucidet_amd import ops
    src = open(os.path.join(ROOT, "include", "hallucidet_hip.h")).read()
    row = int(re.search(r"#define HD_AUG_ROW (\d+)", src).group(1))
    pix = int(re.search(r"#define HD_AUG_MAX_PIXELS (\d+)", src).group(1))
    assert row == ops.AUG_ROW == A.ROW == A.make_row().numel()
    assert pix == ops.AUG_MAX_PIXELS and 255 * pix < 2 ** 32 <= 255 * (pix + 1)
