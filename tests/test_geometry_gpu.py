"""hd_geometry_u8 on the GPU: byte for byte the independent oracle (tests/_geometry_oracle.py) on both paths of the kernel, the float
mode, the arena source, `out=`, repeatability and capture; then the prefetcher: paired batches with and without the HBM cache against
the host arithmetic, the composition with the photometric augmentation, and one training step of each module on an augmented batch."""
import numpy as np
import pytest
import torch

import _geometry_oracle as O
from _geometry_cases import KINDS, SHAPES, case_rows, chunks, image
from _synth_llvip import make_tree
from hallucidet_amd.dataloader import geometry as G

pytestmark = pytest.mark.gpu


def _ieee(u8):
    return u8.float().div_(torch.full((), 255.0, device=u8.device))


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hw", SHAPES)
def test_kernel_equals_the_oracle(dev, hw, kind):
    from hallucidet_amd import ops
    H, W = hw
    rows = case_rows(H, W)
    base = image(kind, 5, 3, H, W)
    for c in (1, 3):
        for n in (1, 5):
            for s, part in enumerate(chunks(rows, n)):
                x = base[[(s * n + i) % 5 for i in range(n)], :c].contiguous()
                want = torch.from_numpy(O.batch(x.numpy(), part.tolist()))
                got = ops.geometry_u8(x.to(dev), part)                               # host rows: validated and uploaded
                assert got.dtype == torch.uint8 and got.shape == x.shape and got.is_contiguous()
                bad = (got.cpu() != want).flatten(1).any(1).nonzero().flatten().tolist()
                assert not bad, (hw, kind, c, n, [part[i].tolist() for i in bad[:3]])
                f = ops.geometry_u8(x.to(dev), part.to(dev), mode="f32_ieee")        # device rows
                assert f.dtype == torch.float32 and torch.equal(f, _ieee(got))


@pytest.mark.parametrize("hw", [(9, 1040), (3, 2064)])
def test_images_wider_than_one_tile(dev, hw):
    """W > 1024: a row is cut into column tiles of 1024, the last one 16 wide; each tile stages its own piece of the source rows"""
    from hallucidet_amd import ops
    H, W = hw
    rows = case_rows(H, W)[[0, 7, 8, 11, 12, 17, 20, 23]]
    x = image("noise", rows.shape[0], 1, H, W, seed=5)
    want = torch.from_numpy(O.batch(x.numpy(), rows.tolist()))
    got = ops.geometry_u8(x.to(dev), rows)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.geometry_u8(x.to(dev), rows, mode="f32_ieee"), _ieee(got))


@pytest.mark.parametrize("hw", SHAPES)
def test_identity_row_returns_the_input(dev, hw):
    from hallucidet_amd import ops
    H, W = hw
    for c in (1, 3):
        x = image("noise", 3, c, H, W, seed=6).to(dev)
        ident = torch.stack([G.make_row(H=H, W=W)] * 3)
        assert torch.equal(ops.geometry_u8(x, ident), x)
        assert torch.equal(ops.geometry_u8(x, torch.stack([G.make_row(flip=True, H=H, W=W)] * 3)), torch.flip(x, dims=[3]))


@pytest.mark.parametrize("hw", [(9, 48), (37, 53)])
@pytest.mark.parametrize("c", [1, 3])
def test_arena_source_equals_the_dense_call(dev, hw, c):
    from hallucidet_amd import ops
    H, W = hw
    arena = image("noise", 7, c, H, W, seed=7).to(dev)
    rows = case_rows(H, W)
    for idx in ([6, 5, 4, 3, 2, 1, 0], [3, 3, 0, 6, 3], [6]):
        part = rows[[(5 * k + 7) % rows.shape[0] for k in range(len(idx))]]
        host = torch.tensor(idx, dtype=torch.int64)
        for mode in ("u8", "f32_ieee"):
            want = ops.geometry_u8(arena[host.to(dev)].contiguous(), part, mode=mode)
            assert torch.equal(ops.geometry_u8(arena, part, idx=idx, mode=mode), want)                               # host indices
            assert torch.equal(ops.geometry_u8(arena, part, idx=host.to(dev), idx_host=host, mode=mode), want)      # device + host copy
            assert torch.equal(ops.geometry_u8(arena, part.to(dev), idx=host.to(dev), validate=False, mode=mode), want)
    out = torch.full((2, c, H, W), 77, dtype=torch.uint8, device=dev)
    for bad in ([0, -1], [7, 0]):
        with pytest.raises(IndexError):
            ops.geometry_u8(arena, rows[:2], idx=bad, out=out)
        host = torch.tensor(bad, dtype=torch.int64)
        with pytest.raises(IndexError):
            ops.geometry_u8(arena, rows[:2], idx=host.clamp(0, 6).to(dev), idx_host=host, out=out)
    with pytest.raises(ValueError, match="host copy"):
        ops.geometry_u8(arena, rows[:2], idx=torch.tensor([0, 1], device=dev), out=out)
    with pytest.raises(ValueError, match="row 1"):
        ops.geometry_u8(arena, torch.tensor([[0, 0, 0, W, H, 0, 0, 0], [0, 0, 0, W + 1, H, 0, 0, 0]], dtype=torch.int32), idx=[0, 1], out=out)
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                        # nothing was launched


@pytest.mark.parametrize("hw", [(9, 48), (3, 17)])
def test_out_into_a_slice_of_a_larger_batch(dev, hw):
    from hallucidet_amd import ops
    H, W = hw
    x = image("noise", 2, 3, H, W, seed=8).to(dev)
    rows = case_rows(H, W)[[7, 20]]
    for mode, dtype, fill in (("u8", torch.uint8, 77), ("f32_ieee", torch.float32, -3.0)):
        want = ops.geometry_u8(x, rows, mode=mode)
        big = torch.full((5, 3, H, W), fill, dtype=dtype, device=dev)
        got = ops.geometry_u8(x, rows, mode=mode, out=big[2:4])
        assert got.data_ptr() == big[2].data_ptr() and torch.equal(big[2:4], want)
        assert bool((big[:2] == fill).all()) and bool((big[4:] == fill).all())
    with pytest.raises(ValueError, match="overlaps"):
        ops.geometry_u8(x, rows, out=x)


def test_two_runs_and_a_captured_graph_give_the_same_bytes(dev):
    from hallucidet_amd import ops
    H, W = 64, 80
    arena = image("noise", 6, 3, H, W, seed=9).to(dev)
    rows = case_rows(H, W)[[1, 8, 11, 23]].to(dev)
    idx = torch.tensor([5, 0, 2, 2], device=dev)
    eager = ops.geometry_u8(arena, rows, idx=idx, validate=False, mode="f32_ieee")
    assert torch.equal(ops.geometry_u8(arena, rows, idx=idx, validate=False, mode="f32_ieee"), eager)
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.geometry_u8(arena, rows, idx=idx, validate=False, mode="f32_ieee", out=out)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.geometry_u8(arena, rows, idx=idx, validate=False, mode="f32_ieee", out=out)
    out.zero_()
    graph.replay()
    assert torch.equal(out, eager)
    idx.copy_(torch.tensor([1, 1, 4, 3], device=dev))                      # a replay reads the current indices and rows
    rows.copy_(case_rows(H, W)[[13, 2, 5, 19]].to(dev))
    graph.replay()
    assert torch.equal(out, ops.geometry_u8(arena, rows, idx=idx, validate=False, mode="f32_ieee"))


# ------------------------------------------------------------------------------------------------ the prefetcher
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


def _module(kind, root, dev, cache, rank=0, world=1):
    from hallucidet_amd.dataloader import MultiModalDataModule, SingleModalDataModule
    common = dict(batch_size=2, num_workers=0, ext=".jpg", seed=3, rank=rank, world_size=world, cache=cache, device=dev)
    if kind == "multi":
        return MultiModalDataModule("llvip", root, root, root, root, **common)
    return SingleModalDataModule("llvip", root, root, modality=kind, **common)


def _run(dm, dev, geometry=None, augment=None, epochs=2):
    """every staged batch of `epochs` training epochs, one validation and one test pass, on the host; validation and test are staged
    the way the Trainer stages them: without any augmentation"""
    from hallucidet_amd.dataloader import DevicePrefetcher
    out = []
    for e in range(epochs):
        for a in (geometry, augment):
            if a is not None:
                a.set_epoch(e)
        out.append([_cpu(b) for b in DevicePrefetcher(dm.train_dataloader(), dev, augment=augment, geometry=geometry)])
    out.append([_cpu(b) for b in DevicePrefetcher(dm.val_dataloader(), dev)])
    out.append([_cpu(b) for b in DevicePrefetcher(dm.test_dataloader(), dev)])
    return out


def _geo(rank=0):
    return G.PairedGeometry(p_flip=0.5, p_crop=0.75, min_scale=0.5, seed=5, rank=rank)


def _to_u8(f):
    """the bytes behind an un-augmented staged batch (b * fp32(1/255) on the GPU: within an ulp of b / 255)"""
    v = f.double() * 255.0
    assert float((v - v.round()).abs().max()) < 1e-3
    return v.round().to(torch.uint8)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """(64, 96): the wide path; (37, 53): the byte path"""
    out = {}
    for hw in ((64, 96), (37, 53)):
        out[hw] = make_tree(tmp_path_factory.mktemp("geo%dx%d" % hw), n_train=10, n_test=4, hw=hw, extra_objects=False)
    return out


@pytest.mark.parametrize("hw", [(64, 96), (37, 53)])
def test_paired_batches_with_and_without_the_cache(dev, trees, hw):
    H, W = hw
    plain = _run(_module("multi", trees[hw], dev, "none"), dev)
    got = _run(_module("multi", trees[hw], dev, "none"), dev, geometry=_geo())
    cached = _run(_module("multi", trees[hw], dev, "hbm"), dev, geometry=_geo())
    _same(cached, got)                                         # arena -> floats in one launch == upload + kernel
    _same(got[2:], plain[2:])                                  # validation and test batches are untouched
    geo, cropped = _geo(), 0
    for e in range(2):
        geo.set_epoch(e)
        for b, (p, g) in enumerate(zip(plain[e], got[e])):
            rows = geo.params_for([p[1], p[3]], H, W, b)
            cropped += sum(r[1:5] != [0, 0, W, H] for r in rows.tolist())
            for k in (0, 2):
                want = G.apply_host(_to_u8(p[k]), rows).float().div_(255.0)
                assert g[k].dtype == torch.float32 and torch.equal(g[k], want), (e, b, k)
                _same(g[k + 1], G.transform_targets(rows, p[k + 1], H, W))
                assert g[k + 1][0]["boxes"].dtype == torch.float64
    assert cropped >= 2
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(got[0], plain[0]))


def test_both_modalities_get_the_same_transform(dev):
    """an IR image that is channel 0 of the RGB image stays channel 0 of the augmented RGB image"""
    from hallucidet_amd.dataloader import DevicePrefetcher
    H, W = 64, 96
    rgb = image("noise", 4, 3, H, W, seed=12)
    g = np.random.RandomState(0)
    targets = []
    for _ in range(4):
        xa, ya = g.uniform(0, W - 20), g.uniform(0, H - 20)
        targets.append({"boxes": torch.tensor([[xa, ya, xa + 15, ya + 18]], dtype=torch.float64), "labels": torch.ones(1, dtype=torch.int64)})
    batch = (tuple(rgb), tuple(targets), tuple(rgb[:, :1].contiguous()), tuple(targets))
    geo = G.PairedGeometry(p_flip=0.5, p_crop=1.0, seed=1)
    out, = list(DevicePrefetcher([batch], dev, geometry=geo))
    assert torch.equal(out[2], out[0][:, :1]) and not torch.equal(out[0].cpu(), rgb.float().div_(255.0))
    _same(_cpu(out[1]), _cpu(out[3]))


def test_rows_differ_between_epochs_and_ranks(dev, trees):
    hw = (64, 96)
    base = _run(_module("multi", trees[hw], dev, "none", 0, 2), dev, geometry=_geo(0))
    other = _run(_module("multi", trees[hw], dev, "none", 0, 2), dev, geometry=_geo(1))         # the same samples, another rank's draws
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(base[0], other[0]))
    geo = _geo()
    targets = [[{"boxes": torch.tensor([[4.0, 5.0, 20.0, 30.0]], dtype=torch.float64)}] * 8]
    geo.set_epoch(0)
    e0 = geo.params_for(targets, 64, 96, 0)
    geo.set_epoch(1)
    assert not torch.equal(e0, geo.params_for(targets, 64, 96, 0))
    assert not torch.equal(e0, _geo(1).params_for(targets, 64, 96, 0))


@pytest.mark.parametrize("cache", ["none", "hbm"])
@pytest.mark.parametrize("kind,hw", [("rgb", (64, 96)), ("ir", (37, 53))])
def test_single_modal_with_the_photometric_augmentation(dev, trees, kind, hw, cache):
    """geometry (u8) -> hd_augment_u8 -> IEEE division == the same three steps on the host"""
    from hallucidet_amd.dataloader import augment as A
    H, W = hw

    def aug():
        return A.ReferenceAugmentation(p_invert=0.5, p_sharpness=0.5, p_equalize=0.5, seed=5, rank=0)
    plain = _run(_module(kind, trees[hw], dev, "none"), dev)
    got = _run(_module(kind, trees[hw], dev, cache), dev, geometry=_geo(), augment=aug())
    _same(got[2:], plain[2:])
    geo, a = _geo(), aug()
    for e in range(2):
        geo.set_epoch(e)
        a.set_epoch(e)
        for b, (p, g) in enumerate(zip(plain[e], got[e])):
            rows = geo.params_for([p[1]], H, W, b)
            want = A.apply_host(G.apply_host(_to_u8(p[0]), rows), a.params_for(2, b)).float().div_(255.0)
            assert torch.equal(g[0], want), (e, b)
            _same(g[1], G.transform_targets(rows, p[1], H, W))


# ------------------------------------------------------------------------------------------------ one step of each module
def _host_batch(n, H, W, seed):
    from hallucidet_amd import synthetic
    rgb, trgb, ir, tir = synthetic.make_batch(n, H, W, seed=seed, device="cpu")
    u8 = lambda t: tuple((t * 255.0).round().clamp_(0, 255).to(torch.uint8))
    host = lambda ts: tuple({k: v.cpu() for k, v in t.items()} for t in ts)
    return u8(rgb), host(trgb), u8(ir), host(tir)


def _boxes_inside(targets, H, W):
    for t in targets:
        b = t["boxes"]
        assert b.numel() and float(b.min()) >= 0 and float(b[:, [0, 2]].max()) <= W and float(b[:, [1, 3]].max()) <= H


def test_one_step_of_each_module_on_an_augmented_batch(dev):
    from hallucidet_amd import synthetic
    from hallucidet_amd.dataloader import DevicePrefetcher
    from hallucidet_amd.models.detector import Detector
    from hallucidet_amd.train_detector import DetectorLit
    H, W = 128, 160
    geo = G.PairedGeometry(p_flip=1.0, p_crop=1.0, seed=2)
    paired = _host_batch(2, H, W, seed=4)
    batch, = list(DevicePrefetcher([paired], dev, geometry=geo))
    assert tuple(batch[0].shape) == (2, 3, H, W) and tuple(batch[2].shape) == (2, 1, H, W)
    rows = geo.params_for([paired[1], paired[3]], H, W, 0)
    assert all(r[0] == 1 and r[1:5] != [0, 0, W, H] for r in rows.tolist())
    _boxes_inside(batch[1], H, W)
    _boxes_inside(batch[3], H, W)
    lit = synthetic.make_module(seed=3, device=str(dev), precision=16)
    loss = lit.fit_step(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)

    torch.manual_seed(41)
    det = Detector(name="fasterrcnn", pretrained=False, n_classes=2, size=300).detector.to(dev)
    single, = list(DevicePrefetcher([paired[:2]], dev, geometry=geo))
    assert torch.equal(single[0], batch[0])                    # the same records whatever the number of image groups ...
    _boxes_inside(single[1], H, W)
    il, _ = det.transform(single[0], None)
    det.backbone.calibrate_(il.tensors)
    dlit = DetectorLit(batch_size=2, lr=1e-4, detector_name="fasterrcnn", pretrained=False, detector=det, device=str(dev)).prepare()
    det.set_trainable(True, grad_scale=dlit.loss_scale)
    loss = dlit.fit_step(single)
    torch.cuda.synchronize()
    assert torch.isfinite(torch.as_tensor(loss))
