"""Cost and gain of the HBM dataset cache (--cache-dataset hbm, hd_batch_gather_u8, dataloader/cache.py).

1. `kernel`: one gather of 8 x 3 x 512 x 640 and of 8 x 1 x 512 x 640, each mode, as a captured graph of back-to-back calls timed with
   device events.  `cold`: an arena of >= 1 GiB and another index vector in every call of the graph (slots of a random permutation), with
   enough calls in the graph (20 for RGB, 60 for IR) that > 256 MiB of traffic lie between two reads of a row: the source is HBM, not the
   Infinity Cache.  `cached`: 16 slots and the same indices every call.  Next to it the ATen chain the kernel replaces on device-resident
   bytes (`arena[idx]` -> `.float()` -> `.div_(255.0)`, same indices: 15 B per value against 5) and a `copy_` of the fp32 batch.
   `TBps` = 5 B per value over the time.
2. `loader`: DevicePrefetcher alone over a synthetic 512 x 640 JPEG tree (the consumer only waits for each batch), cache off at 4 and
   16 workers and cache on; batches/s and the fill time.
3. `step`: EncoderDecoderLit.fit_step, batch 8, fed by the uncached prefetcher, the cached one and one resident batch, in alternating
   blocks in one process; images/s and the spread over the blocks.

Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N, H, W = 8, 512, 640
XML = "<annotation><filename>{name}.jpg</filename><object><name>person</name><bndbox><xmin>{a}</xmin><ymin>{b}</ymin><xmax>{c}</xmax>" \
      "<ymax>{d}</ymax></bndbox></object></annotation>"


def make_tree(root, n_train, n_test, seed=0):
    """LLVIP layout; smooth images with some noise (pure noise decodes slower than a photograph), JPEG quality 90"""
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    root = os.path.join(root, "LLVIP")
    for split, n in (("train", n_train), ("test", n_test)):
        for mod in ("visible", "infrared"):
            os.makedirs(os.path.join(root, mod, split), exist_ok=True)
        os.makedirs(os.path.join(root, "Annotations"), exist_ok=True)
        for i in range(n):
            name = "%s%05d" % ("1" if split == "train" else "9", i)
            for mod, c in (("visible", 3), ("infrared", 1)):
                low = rng.randint(0, 256, (H // 16, W // 16, c), dtype=np.uint8).squeeze()
                img = np.asarray(Image.fromarray(low).resize((W, H), Image.BICUBIC)).astype(np.int16) + rng.randint(-6, 7, (H, W, c)).squeeze()
                Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(os.path.join(root, mod, split, name + ".jpg"), quality=90)
            a, b = int(rng.randint(0, W - 120)), int(rng.randint(0, H - 200))
            with open(os.path.join(root, "Annotations", name + ".xml"), "w") as f:
                f.write(XML.format(name=name, a=a, b=b, c=a + 40 + int(rng.randint(0, 60)), d=b + 90 + int(rng.randint(0, 90))))
    return root


def kernel_section(reps):
    import torch
    from bench_augment import graph_time_us
    from hallucidet_amd import ops
    dev = "cuda"
    res = {}
    for C, mult in ((3, 1), (1, 3)):
        chw, calls = C * H * W, reps * mult
        nval = N * chw
        x = torch.rand(N, C, H, W, device=dev)
        dst = torch.empty_like(x)
        tc = graph_time_us(lambda: dst.copy_(x), reps)
        sec = {"values": nval, "copy_us": round(tc, 2), "copy_TBps": round(8 * nval / tc / 1e6, 2)}
        for label, S in (("cold", -(-(1 << 30) // chw) + 1), ("cached", 16)):
            arena = torch.randint(0, 256, (S, C, H, W), dtype=torch.uint8, device=dev)
            g = torch.Generator().manual_seed(S)
            if label == "cold":
                perm = torch.randperm(S, generator=g)[:calls * N].view(calls, N)
            else:
                perm = torch.randperm(S, generator=g)[:N].repeat(calls, 1)
            idxs = [p.contiguous().to(dev) for p in perm]
            part = {"arena_bytes": arena.numel(), "calls_per_graph": calls, "traffic_between_rereads_MiB": round(5 * nval * calls / 2 ** 20)}
            turn = [0]

            def nxt():
                turn[0] += 1
                return idxs[turn[0] % calls]
            for mode in ops.GATHER_MODES:
                out = torch.empty((N, C, H, W), dtype=torch.uint8 if mode == "u8" else torch.float32, device=dev)
                us = graph_time_us(lambda: ops.batch_gather(arena, nxt(), mode, out=out, validate=False), calls)
                nbytes = nval * (2 if mode == "u8" else 5)
                part[mode] = {"us": round(us, 2), "bytes": nbytes, "TBps": round(nbytes / us / 1e6, 2), "ratio_to_copy": round(us / tc, 2)}
            ua = graph_time_us(lambda: arena[nxt()].float().div_(255.0), calls)
            part["aten_chain"] = {"us": round(ua, 2), "bytes": nval * 15, "TBps": round(nval * 15 / ua / 1e6, 2)}
            part["aten_over_kernel_f32_default"] = round(ua / part["f32_default"]["us"], 2)
            sec[label] = part
            del arena, idxs
            torch.cuda.empty_cache()
        res["%dx%dx%dx%d" % (N, C, H, W)] = sec
    return res


def _module(root, workers, cache):
    from hallucidet_amd.dataloader import MultiModalDataModule
    return MultiModalDataModule("llvip", root, root, root, root, batch_size=N, num_workers=workers, ext=".jpg", seed=123, cache=cache,
                                device="cuda", log=lambda *a: None)


def loader_section(root, epochs):
    import torch
    from hallucidet_amd.dataloader import DevicePrefetcher
    res = {}
    for name, workers, cache in (("off_4_workers", 4, "none"), ("off_16_workers", 16, "none"), ("hbm", 16, "hbm")):
        t0 = time.perf_counter()
        dm = _module(root, workers, cache)
        built = time.perf_counter() - t0
        loader = dm.train_dataloader()
        rates = []
        for e in range(epochs + 1):                    # the first epoch starts the workers: not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for batch in DevicePrefetcher(loader, "cuda"):
                torch.cuda.current_stream().synchronize()
                n += 1
            if e:
                rates.append(n / (time.perf_counter() - t0))
        sec = {"batches_per_epoch": n, "batches_per_s": round(statistics.median(rates), 1), "pairs_per_s": round(statistics.median(rates) * N, 1),
               "per_epoch": [round(r, 1) for r in rates]}
        if cache == "hbm":
            c = dm.caches
            sec.update(fill_s={k: round(v.fill_seconds, 2) for k, v in c.items()}, fill_workers=workers, module_build_s=round(built, 2),
                       cached_pairs={k: len(v) for k, v in c.items()}, cache_bytes={k: v.nbytes for k, v in c.items()})
        res[name] = sec
        del loader, dm
    return res


def step_section(root, blocks, per_block):
    import torch
    from hallucidet_amd import synthetic
    from hallucidet_amd.dataloader import DevicePrefetcher
    lit = synthetic.make_module(seed=123, device="cuda", precision=16)

    def cycle(loader):
        while True:
            for b in DevicePrefetcher(loader, "cuda"):
                yield b
    dms = {"uncached_16_workers": _module(root, 16, "none"), "cached": _module(root, 16, "hbm")}
    feeds = {k: cycle(dm.train_dataloader()) for k, dm in dms.items()}
    one = next(cycle(dms["cached"].train_dataloader()))

    def resident():
        while True:
            yield one
    feeds["resident"] = resident()
    for f in feeds.values():                           # warm-up: the workers, the step's graphs
        for _ in range(4):
            lit.fit_step(next(f))
    torch.cuda.synchronize()
    times = {k: [] for k in feeds}
    for b in range(blocks):
        order = list(feeds) if b % 2 == 0 else list(feeds)[::-1]
        for name in order:
            f = feeds[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(per_block):
                lit.fit_step(next(f), i)
            torch.cuda.synchronize()
            times[name].append(N * per_block / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"images_per_s": {k: round(v, 1) for k, v in med.items()}, "blocks": {k: [round(x, 1) for x in v] for k, v in times.items()},
            "block_spread_images_per_s": {k: round(max(v) - min(v), 1) for k, v in times.items()},
            "cached_minus_resident_images_per_s": round(med["cached"] - med["resident"], 1), "steps_per_block": per_block, "batch": N}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=320, help="training pairs of the synthetic tree (80 percent of them are the train split)")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--sections", default="kernel,loader,step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset_cache: no GPU visible (nothing here runs on the CPU)")
    res, tmp = {}, None

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    try:
        if "kernel" in a.sections:
            res["kernel"] = kernel_section(a.reps)
            flush()
        if "loader" in a.sections or "step" in a.sections:
            tmp = tempfile.mkdtemp(prefix="bench_dataset_cache_")
            t0 = time.perf_counter()
            root = make_tree(tmp, a.pairs, 16)
            res["tree"] = {"train_pairs": a.pairs, "test_pairs": 16, "size": "%dx%d" % (H, W), "written_in_s": round(time.perf_counter() - t0, 1)}
        if "loader" in a.sections:
            res["loader"] = loader_section(root, a.epochs)
            flush()
        if "step" in a.sections:
            res["step"] = step_section(root, a.blocks, a.steps)
            flush()
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
