"""Host side of the HBM dataset cache (dataloader/cache.py, --cache-dataset hbm): the flags, the batch order of CachedLoader against the
DataLoader it replaces, the budget arithmetic and the build order, and the checks that raise before any GPU work."""
import pytest
import torch

from _synth_llvip import make_tree


def test_parser_defaults_and_choices():
    from hallucidet_amd.config import Config
    a = Config.argument_parser([])
    assert a.cache_dataset == "none" and a.cache_budget_gb is None
    assert Config.cache_kwargs(a, "cuda:0") == dict(cache="none", cache_budget_bytes=None, device="cuda:0")
    a = Config.argument_parser(["--cache-dataset", "hbm", "--cache-budget-gb", "1.5"])
    assert a.cache_dataset == "hbm" and a.cache_budget_gb == 1.5
    assert Config.cache_kwargs(a, "cuda:1") == dict(cache="hbm", cache_budget_bytes=1500000000, device="cuda:1")
    with pytest.raises(SystemExit):
        Config.argument_parser(["--cache-dataset", "host"])


class _Indexed(torch.utils.data.Dataset):
    """sample i = (the image [[[i]]], {'i': i})"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return torch.full((1, 1, 1), i, dtype=torch.uint8), {"i": int(i)}


def _fake_cache(n):
    from hallucidet_amd.dataloader.cache import DeviceDatasetCache
    return DeviceDatasetCache([torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1)], [[{"i": i} for i in range(n)]], decoded=n)


def _order(loader):
    """per batch the sample numbers, read from the images (DataLoader) or from the slots' images (CachedLoader)"""
    from hallucidet_amd.dataloader.cache import IndexBatch
    out = []
    for b in loader:
        if isinstance(b, IndexBatch):
            assert [t["i"] for t in b.targets[0]] == b.indices
            out.append([int(b.cache.arenas[0][i]) for i in b.indices])
        else:
            assert [t["i"] for t in b[1]] == [int(im) for im in b[0]]
            out.append([int(im) for im in b[0]])
    return out


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2), (0, 3), (2, 3)])
def test_cached_loader_yields_the_dataloaders_order(rank, world):
    from hallucidet_amd.dataloader import dataloader as D
    from hallucidet_amd.dataloader.cache import CachedLoader
    n, bs, seed = 23, 2, 7
    base = _Indexed(n)
    tr, va = D.split_dataset(base, split_ratio=0.8, seed=seed)
    cache = _fake_cache(n)
    ref = D._loader(tr, bs, True, 0, seed, rank, world)
    got = D._unit_loader(cache, tr.indices, tr, bs, True, 0, seed, rank, world)
    assert isinstance(got, CachedLoader) and len(got) == len(ref) == len(tr) // (world * bs)
    epochs = [(_order(ref), _order(got)) for _ in range(4)]          # every __iter__ advances the sampler's epoch
    assert all(r == g and len(r) == len(ref) for r, g in epochs)
    assert epochs[0][0] != epochs[1][0]                               # ... so the epochs differ
    ref, got = D._loader(va, bs, False, 0, seed), D._unit_loader(cache, va.indices, va, bs, False, 0, seed)
    assert len(got) == len(ref) == len(va) // bs                      # sequential, drop_last: 5 samples -> 2 batches
    assert _order(ref) == _order(got) == _order(got) and len(_order(got)) == len(ref)
    whole = D._unit_loader(cache, range(n), base, 4, False, 0, seed)
    assert _order(whole) == _order(D._loader(base, 4, False, 0, seed)) == [list(range(b * 4, b * 4 + 4)) for b in range(5)]
    with pytest.raises(IndexError):
        CachedLoader(cache, [0, n], bs)


def test_budget_arithmetic_and_build_order():
    from hallucidet_amd.dataloader import cache as hc
    # LLVIP's train split at full size: 12 025 pairs of 3 + 1 planes of 1024 x 1280 bytes
    assert hc.unit_bytes(12025, [(3, 1024, 1280), (1, 1024, 1280)]) == 12025 * 5242880 == 63045632000
    assert hc.unit_bytes(10, [(1, 37, 53)]) == 19610

    class Fake:
        def __init__(self, nbytes):
            self.nbytes, self.fill_seconds = nbytes, 0.0

        def __len__(self):
            return 1
    calls, lines = [], []

    def build(ds, device, num_workers=0, budget_bytes=None, log=None):
        calls.append((ds, budget_bytes))
        if ds["bytes"] > budget_bytes:
            raise hc.CacheUnavailable("does not fit")
        return Fake(ds["bytes"])
    units = [("train", dict(bytes=600)), ("valid", dict(bytes=500)), ("test", dict(bytes=400))]
    out = hc.build_units(units, "cuda:0", budget_bytes=1000, log=lines.append, build=build)
    # in order, each offered what its predecessors left; the unit that does not fit costs nothing and the next one is still tried
    assert calls == [(units[0][1], 1000), (units[1][1], 400), (units[2][1], 400)]
    assert out["train"].nbytes == 600 and out["valid"] is None and out["test"].nbytes == 400 and list(out) == ["train", "valid", "test"]
    stays = [l for l in lines if "stays on the DataLoader" in l]
    assert len(stays) == 1 and "valid" in stays[0] and "does not fit" in stays[0]


def test_host_transforms_and_cpu_device_raise(tmp_path):
    from hallucidet_amd.dataloader import MultiModalDataModule, SingleModalDataModule
    root = make_tree(tmp_path, n_train=5, n_test=2, hw=(16, 24))
    kw = dict(batch_size=2, num_workers=0, ext=".jpg", cache="hbm")
    for t in ("data_augmentation", "fixed_transformations"):
        with pytest.raises(ValueError, match=t):
            SingleModalDataModule("llvip", root, root, **kw, **{t: lambda x: x})
        with pytest.raises(ValueError, match=t):
            MultiModalDataModule("llvip", root, root, root, root, **kw, **{t: lambda **k: k})
    with pytest.raises(ValueError, match="GPU"):
        SingleModalDataModule("llvip", root, root, device="cpu", **kw)
    with pytest.raises(ValueError, match="GPU"):
        MultiModalDataModule("llvip", root, root, root, root, device=torch.device("cpu"), **kw)
    with pytest.raises(ValueError, match="'none' or 'hbm'"):
        SingleModalDataModule("llvip", root, root, **dict(kw, cache="host"))
    dm = SingleModalDataModule("llvip", root, root, **dict(kw, cache="none"), device="cpu")      # off: today's loaders, no device needed
    assert dm.caches == {} and isinstance(dm.train_dataloader(), torch.utils.data.DataLoader)


def test_batch_gather_checks_raise_before_the_library_is_touched(monkeypatch):
    from hallucidet_amd import _abi, ops

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_abi, "load", no_library)
    arena = torch.zeros(4, 1, 8, 8, dtype=torch.uint8)
    idx = torch.tensor([0, 3])
    with pytest.raises(ValueError, match="mode"):
        ops.batch_gather(arena, idx, "f16")
    for bad in (arena[0], arena.float(), arena[:, :, :, ::2], arena[:0]):
        with pytest.raises(ValueError, match="arena"):
            ops.batch_gather(bad, idx, "u8")
    for bad in (idx.int(), idx.float(), idx.view(1, 2)):
        with pytest.raises(ValueError, match="int64"):
            ops.batch_gather(arena, bad, "u8")
    for bad in ([-1], [4], [0, 1, 7]):
        with pytest.raises(IndexError, match="outside"):
            ops.batch_gather(arena, bad, "f32_default")
    with pytest.raises(ValueError, match="1 <= N"):
        ops.batch_gather(arena, [], "u8")
    for out in (torch.zeros(2, 1, 8, 8), torch.zeros(3, 1, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            ops.batch_gather(arena, idx, "u8", out=out)
    with pytest.raises(ValueError, match="out must be"):
        ops.batch_gather(arena, idx, "f32_ieee", out=torch.zeros(2, 1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):              # well-formed arguments on the CPU: still no library call
        ops.batch_gather(arena, idx, "u8")
    assert torch.equal(ops.check_gather_indices([3, 0, 3], 4), torch.tensor([3, 0, 3]))
