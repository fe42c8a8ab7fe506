"""The reference's detector-training augmentation on the GPU (hd_augment_u8, csrc/augment.hip): bit for bit Pillow and `apply_host`,
run-to-run identity, independence from the batch, a launch count that depends on nothing, graph capture, the prefetcher and the
training script."""
import math
import os
import sys

import pytest
import torch

from _augment_oracle import all_colours, all_on_row, forced_rows, image, pil_apply
from _synth_llvip import make_tree
from hallucidet_amd.dataloader import augment as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("uniform", "smooth", "narrow", "const", "twolevel")


def _batch(n, c, h, w, seed):
    return torch.stack([image(KINDS[(seed + i) % len(KINDS)] if i % 3 else "uniform", c, h, w, seed=seed * 100 + i) for i in range(n)])


def _check(dev, x, rows):
    from hallucidet_amd import ops
    got = ops.augment_u8(x.to(dev), rows.to(dev)).cpu()
    host = A.apply_host(x, rows)
    pil = pil_apply(x, rows)
    for n in range(x.shape[0]):
        assert torch.equal(got[n], host[n]), ("apply_host", tuple(x.shape), n, rows[n].tolist(), int((got[n] != host[n]).sum()))
        assert torch.equal(got[n], pil[n]), ("Pillow", tuple(x.shape), n, rows[n].tolist(), int((got[n] != pil[n]).sum()))


@pytest.mark.parametrize("n,c,h,w", [(16, 3, 512, 640), (16, 1, 512, 640), (2, 3, 127, 161), (1, 3, 3, 3), (3, 3, 36, 40), (3, 1, 36, 40)])
def test_kernel_equals_pillow_and_host(dev, n, c, h, w):
    rows = forced_rows()                     # each operation alone, the 24 orders, everything at once, nothing
    rows += [rows[-1]] * (-len(rows) % n)
    for b in range(len(rows) // n):
        _check(dev, _batch(n, c, h, w, seed=b), torch.stack(rows[b * n:(b + 1) * n]))
    # a drawn batch at the reference's probabilities: most images have no flag set
    drawn = A.ReferenceAugmentation(seed=5).params_for(n, 0)
    _check(dev, _batch(n, c, h, w, seed=9), drawn)
    if n == 16:
        assert int((drawn[:, 8:11].sum(1) == 0).sum()) >= 4


def test_hue_on_every_colour(dev):
    x = all_colours()
    for hf in (-2.5 / 255, 0.0, 2.5 / 255):      # H shifts -2, 0, 2
        _check(dev, x, A.make_row(order=(A.HUE,), hue=hf)[None])


def test_run_to_run_and_batch_independence(dev):
    from hallucidet_amd import ops
    x = _batch(16, 3, 512, 640, seed=3)
    rows = A.ReferenceAugmentation(p_invert=0.5, p_sharpness=0.5, p_equalize=0.5, seed=2).params_for(16, 1)
    xd, rd = x.to(dev), rows.to(dev)
    a, b = ops.augment_u8(xd, rd), ops.augment_u8(xd, rd)
    assert torch.equal(a, b)
    for k in (0, 5, 15):
        alone = ops.augment_u8(xd[k:k + 1].contiguous(), rd[k:k + 1].contiguous())
        assert torch.equal(alone[0], a[k]), k
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(1)).to(dev)
    assert torch.equal(ops.augment_u8(xd[perm].contiguous(), rd[perm].contiguous()), a[perm])


def _launches(dev, n, row, c=3, h=64, w=96):
    from torch.profiler import ProfilerActivity, profile
    from hallucidet_amd import ops
    x = _batch(n, c, h, w, seed=1).to(dev)
    rows = row[None].repeat(n, 1).to(dev)
    ops.augment_u8(x, rows)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ops.augment_u8(x, rows)
        torch.cuda.synchronize()
    return sorted(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def test_launch_count_depends_on_nothing_and_the_call_is_capturable(dev):
    from hallucidet_amd import ops
    off, on = A.make_row(), all_on_row()
    base = _launches(dev, 1, off)
    print("device activities of one call:", base)
    assert sum("aug_" in name for name in base) == 4, base
    for n, row in ((16, off), (1, on), (16, on)):
        assert _launches(dev, n, row) == base, (n, row.tolist())
    # the other instantiations: one plane; an odd width (one byte per lane); H*W a multiple of 16 with W not one (mixed)
    for c, h, w in ((1, 64, 96), (3, 37, 61), (3, 32, 40)):
        per = [_launches(dev, n, row, c, h, w) for n, row in ((1, off), (16, off), (1, on), (16, on))]
        assert all(p == per[0] for p in per) and len(per[0]) == len(base) and sum("aug_" in name for name in per[0]) == 4, (c, h, w, per)
    x = _batch(4, 3, 64, 96, seed=2).to(dev)
    rows = torch.stack([off, on, A.make_row(equalize=True), on]).to(dev)
    want = ops.augment_u8(x, rows)
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                       # a host synchronisation inside the call would fail the capture
        ops.augment_u8(x, rows, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_prefetcher_on_the_gpu_equals_the_cpu_prefetcher(dev, tmp_path):
    from hallucidet_amd.dataloader import DevicePrefetcher, SingleModalDataModule
    root = make_tree(tmp_path, n_train=10, n_test=6, hw=(48, 64))
    for modality in ("rgb", "ir"):
        dm = SingleModalDataModule("llvip", root, root, batch_size=2, num_workers=0, ext=".jpg", modality=modality)
        aug = A.ReferenceAugmentation(p_invert=0.5, p_sharpness=0.5, p_equalize=0.5, seed=3)
        cpu = list(DevicePrefetcher(dm.test_dataloader(), device="cpu", augment=aug))
        gpu = list(DevicePrefetcher(dm.test_dataloader(), device=dev, augment=aug))
        assert len(cpu) == len(gpu) == 3
        for cb, gb in zip(cpu, gpu):
            g8, c8 = (gb[0].cpu() * 255.0).round(), (cb[0] * 255.0).round()
            print("prefetcher %s: uint8 values differing %d, float values differing %d of %d" % (
                modality, int((g8 != c8).sum()), int((gb[0].cpu() != cb[0]).sum()), cb[0].numel()))
            assert torch.equal(g8, c8)               # the augmented uint8 batch itself
            assert gb[0].is_cuda and gb[0].dtype == torch.float32 and torch.equal(gb[0].cpu(), cb[0])
            for tc, tg in zip(cb[1], gb[1]):
                assert torch.equal(tc["boxes"], tg["boxes"].cpu()) and torch.equal(tc["labels"], tg["labels"].cpu())


def test_train_detector_script_with_the_augmentation(dev, tmp_path, capsys, monkeypatch):
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    root = make_tree(tmp_path, n_train=8, n_test=2, hw=(64, 96), extra_objects=False)
    import train_detector
    from hallucidet_amd import ops
    calls = []
    real = ops.augment_u8
    monkeypatch.setattr(ops, "augment_u8", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    train_detector.main(["--dataset", "llvip", "--train", root, "--test", root, "--ext", ".jpg", "--batch", "2", "--num-workers", "0",
                         "--seed", "3", "--detector", "fasterrcnn", "--modality", "rgb", "--epochs", "1", "--wandb-name", "aug",
                         "--augment", "reference"])
    out = capsys.readouterr().out
    losses = [float(l.split(" loss ")[1].split()[0]) for l in out.splitlines() if l.startswith("epoch 0 step")]
    assert losses and all(math.isfinite(v) for v in losses), out
    assert len(calls) == 3 and all(tuple(s) == (2, 3, 64, 96) for s in calls), calls      # the three training batches, nothing else
    assert "test:" in out and "map_50" in out
