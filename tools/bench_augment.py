"""Cost of the detector-training augmentation (--augment reference, hd_augment_u8).

1. The call at 16x3x512x640 for three records -- every flag off with no jitter (each image is a copy), the drawn mix of the reference's
   probabilities, every operation on for every image -- each next to a `copy_` of the same uint8 batch (the least traffic the call can
   have: the batch read once and written once).  Every timing is a captured graph of REPS back-to-back calls, timed with device
   events, so that host issue cost is not measured.
2. `DetectorLit.fit_step` fed by `DevicePrefetcher` from host uint8 batches, as `Trainer.fit` feeds it, with the augmentation on and
   off: alternating blocks of steps in one process, every step on a batch other than the previous one.
3. The host alternative: the same operations through Pillow on a drawn batch, one thread and 16 threads.

Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

N, C, H, W = 16, 3, 512, 640


def graph_time_us(fn, reps, rounds=7):
    """median over `rounds` of (one replay of a graph holding `reps` calls of fn) / reps, in microseconds"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out)


def records():
    from hallucidet_amd.dataloader import augment as A
    drawn = A.ReferenceAugmentation(seed=123).params_for(N, 0)
    on = drawn.clone()
    on[:, 0:4] = torch.tensor([1.0, 3.0, 0.0, 2.0])
    on[:, 8:11] = 1.0
    return {"all_off": A.make_row()[None].repeat(N, 1), "drawn_mix": drawn, "all_on": on}


def kernel_section(reps):
    from hallucidet_amd import ops
    dev = "cuda"
    x = torch.randint(0, 256, (N, C, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
    out = torch.empty_like(x)
    ws = torch.empty(ops.augment_ws_bytes(x.shape), dtype=torch.uint8, device=dev)
    tc = graph_time_us(lambda: out.copy_(x), reps)
    res = {"batch_bytes": x.numel(), "copy_us": round(tc, 2), "copy_TBps": round(2 * x.numel() / tc / 1e6, 2)}
    for name, rows in records().items():
        rd = rows.to(dev)
        t = graph_time_us(lambda: ops.augment_u8(x, rd, out=out, ws=ws), reps)
        res[name] = {"call_us": round(t, 2), "ratio_to_copy": round(t / tc, 2), "flags_set": int(rows[:, 8:11].sum())}
    return res


def host_batches(k):
    from hallucidet_amd import synthetic
    out = []
    for i in range(k):
        rgb, tg, _, _ = synthetic.make_batch(N, H, W, seed=500 + i, device="cpu")
        out.append((tuple((rgb * 255).to(torch.uint8)), tuple(tg)))
    return out


def step_section(blocks, per_block):
    from hallucidet_amd import synthetic
    from hallucidet_amd.dataloader import DevicePrefetcher
    from hallucidet_amd.dataloader.augment import ReferenceAugmentation
    from hallucidet_amd.models.detector import Detector
    from hallucidet_amd.train_detector import DetectorLit
    dev = "cuda:0"
    torch.manual_seed(1)
    det = Detector(name="fasterrcnn", pretrained=False, n_classes=2, size=300).detector.to(dev)
    il, _ = det.transform(synthetic.make_batch(2, H, W, seed=124, device=dev)[0], None)
    det.backbone.calibrate_(il.tensors)
    lit = DetectorLit(batch_size=N, detector=det, pretrained=False, device=dev).prepare()
    pool = host_batches(6)
    loader = [pool[i % len(pool)] for i in range(per_block)]
    aug = ReferenceAugmentation(seed=123)
    feeds = {"none": None, "reference": aug}
    for a in feeds.values():                                   # warm-up of both feeds
        for i, batch in enumerate(DevicePrefetcher(loader[:4], dev, augment=a)):
            lit.fit_step(batch, i)
    torch.cuda.synchronize()
    times = {"none": [], "reference": []}
    for b in range(blocks):
        aug.set_epoch(b)
        for name in (("none", "reference") if b % 2 == 0 else ("reference", "none")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, batch in enumerate(DevicePrefetcher(loader, dev, augment=feeds[name])):
                loss = lit.fit_step(batch, i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / per_block)
    assert torch.isfinite(loss)
    med = {n: statistics.median(v) for n, v in times.items()}
    return {"ms_per_step_none": round(med["none"], 4), "ms_per_step_reference": round(med["reference"], 4),
            "delta_ms": round(med["reference"] - med["none"], 4), "ratio": round(med["reference"] / med["none"], 4),
            "blocks_none": [round(v, 3) for v in times["none"]], "blocks_reference": [round(v, 3) for v in times["reference"]],
            "steps_per_block": per_block, "batch": N}


def pil_image(hwc, row):
    """the operations of one record through Pillow, as torchvision's PIL backend runs them"""
    from PIL import Image, ImageEnhance, ImageOps
    from hallucidet_amd.dataloader.augment import hue_shift_of
    im = Image.fromarray(hwc, "RGB")
    for op in row[0:4].astype(int):
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(float(row[4]))
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(float(row[5]))
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(float(row[6]))
        elif op == 3:
            h, s, v = im.convert("HSV").split()
            nh = ((np.array(h, dtype=np.uint8).astype(np.int32) + hue_shift_of(row[7])) & 255).astype(np.uint8)
            im = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    if row[8]:
        im = ImageOps.invert(im)
    if row[9]:
        im = ImageEnhance.Sharpness(im).enhance(float(row[11]))
    if row[10]:
        im = ImageOps.equalize(im)
    return np.asarray(im)


def pillow_section(threads=16):
    from concurrent.futures import ThreadPoolExecutor
    rows = records()["drawn_mix"].numpy()
    imgs = [np.random.default_rng(i).integers(0, 256, (H, W, C), dtype=np.uint8) for i in range(N)]
    pil_image(imgs[0], rows[0])
    t0 = time.perf_counter()
    for im, r in zip(imgs, rows):
        pil_image(im, r)
    one = (time.perf_counter() - t0) * 1e3
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(pil_image, imgs, rows))
        t0 = time.perf_counter()
        list(ex.map(pil_image, imgs, rows))
        many = (time.perf_counter() - t0) * 1e3
    return {"batch_ms_1_thread": round(one, 1), "per_image_ms_1_thread": round(one / N, 1), "batch_ms_%d_threads" % threads: round(many, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: no GPU visible (nothing here runs on the CPU)")
    res = {"call_16x3x512x640": kernel_section(a.reps), "pillow_host_16x3x512x640": pillow_section(),
           "fit_step_detector_16x512x640": step_section(a.blocks, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
