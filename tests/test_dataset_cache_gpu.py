"""The HBM dataset cache on the GPU: hd_batch_gather_u8 against the ATen expressions its modes are named after (torch.equal, no excluded
cases), slot offsets past 2^32 bytes, the host-side index validation, and the cached loaders against the uncached ones batch by batch:
images bit-equal, targets equal with their dtypes, strings equal."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from _synth_llvip import make_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("u8", "f32_default", "f32_ieee")


def _aten(arena, idx, mode):
    """what each mode must equal, evaluated on the GPU from the same bytes"""
    g = arena[idx]
    if mode == "u8":
        return g
    if mode == "f32_default":
        return g.float().div_(255.0)
    return g.float().div_(torch.full((), 255.0, device=arena.device))


def _arena(dev, S, shape):
    """seeded random bytes, no two slots alike; every byte value 0 ... 255 occurs in the first 256 bytes of each slot, or, for slots
    shorter than that, once over the first 256 bytes of the arena (16 slots of 16 bytes)"""
    chw = int(np.prod(shape))
    a = torch.randint(0, 256, (S, chw), generator=torch.Generator().manual_seed(S * 1000 + chw), dtype=torch.uint8)
    if chw >= 256:
        a[:, :256] = ((torch.arange(256)[None] + 37 * torch.arange(S)[:, None]) % 256).to(torch.uint8)
    else:
        a.view(-1)[:256] = torch.arange(256).to(torch.uint8)
    assert a.unique().numel() == 256 and a.unique(dim=0).shape[0] == S
    return a.view((S,) + tuple(shape)).to(dev)


def _check(arena, idx, mode):
    from hallucidet_amd import ops
    dev = arena.device
    want = _aten(arena, torch.tensor(idx, device=dev), mode)
    got = ops.batch_gather(arena, idx, mode)                                   # host indices: validated and uploaded
    assert got.dtype == want.dtype and got.shape == want.shape and got.is_contiguous()
    assert torch.equal(got, want), (tuple(arena.shape), idx, mode, int((got != want).sum()))
    host = torch.tensor(idx, dtype=torch.int64)
    again = ops.batch_gather(arena, host.to(dev), mode, idx_host=host)         # device indices + their host copy
    assert torch.equal(again, want)


# C*H*W = 16: one 16-byte vector per image; 3 x 37 x 53: the byte path, odd slot bases; the IR plane; an RGB image
@pytest.mark.parametrize("shape,S", [((1, 4, 4), 20), ((3, 37, 53), 20), ((1, 512, 640), 17), ((3, 64, 96), 20)])
@pytest.mark.parametrize("mode", MODES)
def test_gather_equals_aten(dev, shape, S, mode):
    arena = _arena(dev, S, shape)
    for idx in ([0], [S - 1],                                  # N = 1: the first and the last slot
                [S - 1, 0], [3, 3],                            # N = 2: descending, duplicates
                [S - 1, 0, 5, 5, 5, 4, 3, 2],                  # N = 8: all of them
                list(range(16))):                              # every byte value passes through the kernel at C*H*W = 16 too
        _check(arena, idx, mode)


# one image is more than one pass of the capped grid (batch_gather.hip: 256 blocks x 256 lanes x 16 bytes = 1 MiB on the vector path,
# 256 x 256 = 65 536 values on the byte path), so the grid-stride loop goes round again
@pytest.mark.parametrize("shape", [(3, 640, 640), (3, 151, 151)])
def test_gather_past_the_grid_cap(dev, shape):
    chw = int(np.prod(shape))
    assert chw > (256 * 256 * 16 if chw % 16 == 0 else 256 * 256)
    arena = _arena(dev, 3, shape)
    for mode in MODES:
        _check(arena, [2, 0], mode)


def test_slot_offsets_past_32_bits(dev):
    """13 200 slots of 1 x 512 x 640 = 4.33 GB, not filled: slot 13 107 straddles byte 2^32, 13 108 and 13 199 lie past it; a 32-bit
    offset would wrap to another slot."""
    from hallucidet_amd import ops
    S, shape = 13200, (1, 512, 640)
    chw = int(np.prod(shape))
    assert 13107 * chw < 2 ** 32 < 13108 * chw
    arena = torch.empty((S,) + shape, dtype=torch.uint8, device=dev)
    slots = [0, 13107, 13108, 13199]
    g = torch.Generator(device=dev).manual_seed(5)
    for s in slots:
        arena[s] = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8, device=dev)
    for mode in MODES:
        want = _aten(arena, torch.tensor(slots, device=dev), mode)
        assert torch.equal(ops.batch_gather(arena, slots, mode), want), mode
    del arena
    torch.cuda.empty_cache()


def test_bad_index_raises_before_any_launch(dev):
    from hallucidet_amd import ops
    S = 6
    arena = _arena(dev, S, (1, 8, 16))
    for mode in MODES:
        out = torch.full((2, 1, 8, 16), 77, dtype=torch.uint8 if mode == "u8" else torch.float32, device=dev)
        for bad in ([0, -1], [S, 0]):
            with pytest.raises(IndexError):
                ops.batch_gather(arena, bad, mode, out=out)
            host = torch.tensor(bad, dtype=torch.int64)
            with pytest.raises(IndexError):
                ops.batch_gather(arena, host.clamp(0, S - 1).to(dev), mode, out=out, idx_host=host)
        with pytest.raises(ValueError, match="host copy"):
            ops.batch_gather(arena, torch.tensor([0, 1], device=dev), mode, out=out)
        torch.cuda.synchronize()
        assert bool((out == 77).all())
        got = ops.batch_gather(arena, torch.tensor([5, 0], device=dev), mode, out=out, validate=False)
        assert got is out and torch.equal(out, _aten(arena, torch.tensor([5, 0], device=dev), mode))


def test_gather_is_capturable_and_repeatable(dev):
    """no host synchronisation: the call records into a graph; a replay reads the index vector's current contents; same bytes run to run"""
    from hallucidet_amd import ops
    arena = _arena(dev, 12, (3, 64, 96))
    idx = torch.tensor([1, 4, 4, 11], device=dev)
    out = torch.zeros((4, 3, 64, 96), device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.batch_gather(arena, idx, "f32_default", out=out, validate=False)          # the library is loaded before the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.batch_gather(arena, idx, "f32_default", out=out, validate=False)
    first = None
    for values in ([1, 4, 4, 11], [0, 11, 3, 3], [1, 4, 4, 11]):
        idx.copy_(torch.tensor(values, device=dev))
        graph.replay()
        assert torch.equal(out, _aten(arena, idx, "f32_default"))
        first = out.clone() if first is None else first
    assert torch.equal(out, first)


# ------------------------------------------------------------------------------------------------ loaders
def _cpu(x):
    if torch.is_tensor(x):
        return x.cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_cpu(v) for v in x]
    return x


def _same(a, b, where=""):
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], where + "/" + str(k))
    elif isinstance(a, list):
        assert isinstance(b, list) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, where + "/%d" % i)
    else:
        assert type(a) is type(b) and a == b, where


def _run(dm, dev, epochs=3, augment=None):
    """every staged batch of `epochs` training epochs, one validation and one test pass, on the host"""
    from hallucidet_amd.dataloader import DevicePrefetcher
    out = []
    for e in range(epochs):
        if augment is not None:
            augment.set_epoch(e)
        out.append([_cpu(b) for b in DevicePrefetcher(dm.train_dataloader(), dev, augment=augment)])
    out.append([_cpu(b) for b in DevicePrefetcher(dm.val_dataloader(), dev)])
    out.append([_cpu(b) for b in DevicePrefetcher(dm.test_dataloader(), dev)])
    return out


def _module(kind, root, dev, cache, rank=0, world=1, batch=2, workers=0, **kw):
    from hallucidet_amd.dataloader import MultiModalDataModule, SingleModalDataModule
    common = dict(batch_size=batch, num_workers=workers, ext=".jpg", seed=3, rank=rank, world_size=world, cache=cache, device=dev, **kw)
    if kind == "multi":
        return MultiModalDataModule("llvip", root, root, root, root, **common)
    return SingleModalDataModule("llvip", root, root, modality=kind, **common)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    return {hw: make_tree(tmp_path_factory.mktemp("tree%dx%d" % hw), n_train=10, n_test=4, hw=hw) for hw in ((64, 96), (37, 53))}


_uncached = {}


def _reference(kind, root, dev, rank, world):
    """the uncached batches: computed once per setting, shared, never modified"""
    key = (kind, root, rank, world)
    if key not in _uncached:
        _uncached[key] = _run(_module(kind, root, dev, "none", rank, world), dev)
    return _uncached[key]


def _assert_cached(dm, n_train=10, n_test=4):
    from hallucidet_amd.dataloader.cache import CachedLoader
    assert all(isinstance(l, CachedLoader) for l in (dm.train_dataloader(), dm.val_dataloader(), dm.test_dataloader()))
    assert dm.caches["train"].decoded == len(dm.caches["train"]) == n_train and dm.caches["test"].decoded == len(dm.caches["test"]) == n_test


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2), (0, 3)])
@pytest.mark.parametrize("hw", [(64, 96), (37, 53)])
@pytest.mark.parametrize("kind", ["multi", "rgb", "ir"])
def test_cached_loaders_yield_the_uncached_batches(dev, trees, kind, hw, rank, world):
    want = _reference(kind, trees[hw], dev, rank, world)
    dm = _module(kind, trees[hw], dev, "hbm", rank, world)
    _assert_cached(dm)
    got = _run(dm, dev)
    # train: 8 samples, batches of 2 over `world` ranks; validation: 2 samples; test: 4
    assert [len(p) for p in got] == [len(p) for p in want] == [8 // (2 * world)] * 3 + [1, 2]
    _same(got, want)
    imgs = got[0][0][0]
    assert imgs.dtype == torch.float32 and tuple(imgs.shape) == (2, 1 if kind == "ir" else 3) + hw
    t = got[0][0][1][0]
    assert t["boxes"].dtype == torch.float64 and t["labels"].dtype == torch.int64
    if kind != "multi":
        assert t["path_image"].endswith(".jpg")
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(got[0], got[1]))          # the epochs are different permutations


@pytest.mark.parametrize("hw", [(64, 96), (37, 53)])
@pytest.mark.parametrize("kind", ["rgb", "ir"])
def test_cached_loader_composes_with_the_gpu_augmentation(dev, trees, kind, hw):
    from hallucidet_amd.dataloader.augment import ReferenceAugmentation

    def aug():
        return ReferenceAugmentation(p_invert=0.5, p_sharpness=0.5, p_equalize=0.5, seed=5, rank=0)
    want = _run(_module(kind, trees[hw], dev, "none"), dev, augment=aug())
    got = _run(_module(kind, trees[hw], dev, "hbm"), dev, augment=aug())
    _same(got, want)
    plain = _reference(kind, trees[hw], dev, 0, 1)
    assert not torch.equal(got[0][0][0], plain[0][0][0])                 # the augmentation did run ...
    _same(got[3:], plain[3:])                                            # ... on the training batches only


@pytest.mark.parametrize("kind,workers", [("multi", 2), ("rgb", 0)])
def test_nothing_is_decoded_after_the_build(dev, trees, kind, workers, monkeypatch):
    from hallucidet_amd.dataloader import dataloader as D
    from hallucidet_amd.dataloader import DevicePrefetcher
    want = _reference(kind, trees[(64, 96)], dev, 0, 1)
    dm = _module(kind, trees[(64, 96)], dev, "hbm", workers=workers)           # workers: the fill's only; the cached loaders have none
    _assert_cached(dm)

    def no_read(self, path, mode):
        raise AssertionError("decoded %s after the cache was built" % path)
    monkeypatch.setattr(D.SingleModalDetectionDataset, "_read", no_read)
    with pytest.raises(AssertionError, match="decoded"):               # the patch bites: the dataset itself can no longer read
        D.SingleModalDetectionDataset("llvip", trees[(64, 96)], modality="rgb", ext=".jpg")[0]
    got = _run(dm, dev)
    _same(got, want)
    assert sum(1 for _ in DevicePrefetcher(dm.test_dataloader(), dev)) == 2
    assert dm.caches["train"].decoded == 10 and dm.caches["test"].decoded == 4


def _module_kw(kind, root, dev, cache, lines, **kw):
    return _module(kind, root, dev, cache, batch=1, log=lines.append, **kw)


@pytest.mark.parametrize("kind", ["multi", "ir"])
def test_a_unit_of_mixed_shapes_stays_on_the_dataloader(dev, tmp_path, kind):
    from hallucidet_amd.dataloader.cache import CachedLoader
    root = make_tree(tmp_path, n_train=10, n_test=4, hw=(64, 96))
    rng = np.random.RandomState(1)
    for mod, shape in (("visible", (48, 96, 3)), ("infrared", (48, 96))):          # one training pair of another height
        Image.fromarray(rng.randint(0, 256, shape, dtype=np.uint8)).save(os.path.join(root, mod, "train", "10007.jpg"), quality=95)
    lines = []
    dm = _module_kw(kind, root, dev, "hbm", lines)
    stays = [l for l in lines if "stays on the DataLoader" in l]
    assert len(stays) == 1 and "train" in stays[0] and "one shape" in stays[0], lines
    assert dm.caches["train"] is None and dm.caches["test"].decoded == 4
    assert isinstance(dm.train_dataloader(), torch.utils.data.DataLoader) and isinstance(dm.val_dataloader(), torch.utils.data.DataLoader)
    assert isinstance(dm.test_dataloader(), CachedLoader)
    _same(_run(dm, dev, epochs=2), _run(_module_kw(kind, root, dev, "none", []), dev, epochs=2))


def test_a_budget_of_one_byte_caches_nothing(dev, trees):
    lines = []
    dm = _module_kw("multi", trees[(37, 53)], dev, "hbm", lines, cache_budget_bytes=1)
    stays = [l for l in lines if "stays on the DataLoader" in l]
    assert len(stays) == 2 and "train" in stays[0] and "test" in stays[1] and all("budget of 1 bytes" in l for l in stays), lines
    assert dm.caches == {"train": None, "test": None}
    assert all(isinstance(l, torch.utils.data.DataLoader) for l in (dm.train_dataloader(), dm.val_dataloader(), dm.test_dataloader()))
    _same(_run(dm, dev, epochs=2), _run(_module_kw("multi", trees[(37, 53)], dev, "none", []), dev, epochs=2))


def test_default_budget_is_half_of_the_free_memory(dev):
    from hallucidet_amd.dataloader import cache as hc
    free = torch.cuda.mem_get_info(dev)[0]
    assert abs(hc.default_budget(dev) - free // 2) <= 1 << 30             # two readings of a live counter


# ------------------------------------------------------------------------------------------------ scripts
def _common(root, name):
    return ["--dataset", "llvip", "--train", root, "--test", root, "--ext", ".jpg", "--batch", "2", "--num-workers", "0", "--seed", "3",
            "--cache-dataset", "hbm", "--precision", "16", "--wandb-name", name]


def test_train_detector_script_with_the_cache(dev, trees, tmp_path, capsys, monkeypatch):
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    import train_detector
    train_detector.main(_common(trees[(64, 96)], "c1") + ["--detector", "fasterrcnn", "--modality", "rgb", "--epochs", "2", "--augment", "reference"])
    out = capsys.readouterr().out
    assert "test:" in out and "map_50" in out and "epoch 1 " in out
    assert "the train unit is in HBM: 10 samples" in out and "the test unit is in HBM: 4 samples" in out


def test_hallucidet_scripts_with_the_cache(dev, trees, tmp_path, capsys, monkeypatch):
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    import eval_hallucidet
    import train_hallucidet
    train_hallucidet.main(_common(trees[(64, 96)], "c2") + ["--detector", "fasterrcnn", "--epochs", "2"])
    out = capsys.readouterr().out
    assert "HalluciDet   on IR  AP@50:" in out and "epoch 1 " in out and "the train unit is in HBM: 10 samples" in out
    maps = eval_hallucidet.main(["--dataset", "llvip", "--test", trees[(64, 96)], "--ext", ".jpg", "--batch", "2", "--num-workers", "0",
                                 "--precision", "16", "--cache-dataset", "hbm", "--cache-budget-gb", "0.5"])
    out = capsys.readouterr().out
    assert out.count("AP@50") == 3 and set(maps) == {"map_rgb", "map_hall", "map_ir"} and "the test unit is in HBM: 4 samples" in out
    assert "train unit" not in out                            # a single pass over the test split: the train unit is not decoded
