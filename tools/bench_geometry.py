"""Cost of the paired geometric augmentation (--augment-geometry, hd_geometry_u8, dataloader/geometry.py).

1. `kernel`: one call at 8 x 3 x 512 x 640 and 8 x 1 x 512 x 640 as a captured graph of 20 back-to-back calls timed with device events:
   identity records, flip-only records and the drawn hflip_crop mix; 'u8' and 'f32_ieee'; from a dense batch and from an arena of
   >= 1 GiB with other slots in every call (the `cold` set-up of tools/bench_dataset_cache.py).  Yardsticks: a `copy_` of the fp32
   batch and `ops.batch_gather` in 'f32_default' and 'f32_ieee' on the same arena and indices.  Bytes: 1 B read per source byte a
   tile stages (at most 9/8 of the crop) + 1 B ('u8') or 4 B ('f32_ieee') written per value; the four taps per value come from LDS.
   Next to it the ATen restatement on the same device-resident data: arena[idx] -> per image flip / crop / F.interpolate -> round -> / 255.
2. `step`: EncoderDecoderLit.fit_step (batch 8, 512 x 640, fp16) fed by the prefetcher from the HBM cache, hflip_crop against off in
   alternating blocks of 10 steps in one process; images/s, the difference and the spread of the off blocks.

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


def record_sets(calls):
    """{name: [int32 [N, 8] per call]}; the drawn mix sees one 60 x 140 person box per image, as LLVIP's scenes roughly do"""
    import numpy as np
    import torch
    from hallucidet_amd.dataloader import geometry as G
    ident = torch.stack([G.make_row(H=H, W=W)] * N)
    flip = torch.stack([G.make_row(flip=True, H=H, W=W)] * N)
    geo = G.PairedGeometry(p_flip=0.5, p_crop=0.5, min_scale=0.5, seed=123)
    rng = np.random.RandomState(1)
    drawn = []
    for b in range(calls):
        t = []
        for _ in range(N):
            x, y = rng.uniform(0, W - 60), rng.uniform(0, H - 140)
            t.append({"boxes": torch.tensor([[x, y, x + 60, y + 140]], dtype=torch.float64)})
        drawn.append(geo.params_for([t], H, W, b))
    return {"identity": [ident] * calls, "flip": [flip] * calls, "hflip_crop": drawn}


def aten_chain(arena, idx, rows_host):
    """the same result with ATen calls on the same device-resident bytes (floats within an ulp; the bytes can differ at ties)"""
    import torch
    import torch.nn.functional as F
    g = arena[idx]
    out = torch.empty(g.shape, dtype=torch.float32, device=g.device)
    for n, (flip, x0, y0, x1, y1) in enumerate(rows_host):
        im = g[n]
        if flip:
            im = torch.flip(im, dims=[2])
        v = F.interpolate(im[None, :, y0:y1, x0:x1].float(), size=(H, W), mode="bilinear", align_corners=False)[0]
        out[n] = torch.floor(v + 0.5).div_(255.0)
    return out


def kernel_section(reps):
    import torch
    from bench_augment import graph_time_us
    from hallucidet_amd import ops
    dev = "cuda"
    res = {}
    for C in (3, 1):
        chw, calls = C * H * W, reps
        nval = N * chw
        x = torch.rand(N, C, H, W, device=dev)
        dst = torch.empty_like(x)
        tc = graph_time_us(lambda: dst.copy_(x), reps)
        sec = {"values": nval, "calls_per_graph": calls, "copy_us": round(tc, 2)}
        S = -(-(1 << 30) // chw) + 1
        arena = torch.randint(0, 256, (S, C, H, W), dtype=torch.uint8, device=dev)
        perm = torch.randperm(S, generator=torch.Generator().manual_seed(S))[:calls * N].view(calls, N)
        idxs = [p.contiguous().to(dev) for p in perm]
        dense = arena[:N].clone()
        turn = [0]

        def nxt():
            turn[0] += 1
            return turn[0] % calls
        sec["arena_bytes"] = arena.numel()
        for mode in ("f32_default", "f32_ieee"):
            out = torch.empty((N, C, H, W), dtype=torch.float32, device=dev)
            us = graph_time_us(lambda: ops.batch_gather(arena, idxs[nxt()], mode, out=out, validate=False), calls)
            sec["batch_gather_" + mode] = {"us": round(us, 2), "bytes": 5 * nval, "TBps": round(5 * nval / us / 1e6, 2)}
        for name, rows in record_sets(calls).items():
            dev_rows = [r.to(dev) for r in rows]
            part = {}
            for mode in ("u8", "f32_ieee"):
                out = torch.empty((N, C, H, W), dtype=torch.uint8 if mode == "u8" else torch.float32, device=dev)
                wr = 1 if mode == "u8" else 4

                def arena_call():
                    k = nxt()
                    ops.geometry_u8(arena, dev_rows[k], idx=idxs[k], validate=False, mode=mode, out=out)

                def dense_call():
                    ops.geometry_u8(dense, dev_rows[nxt()], mode=mode, out=out)
                for src, fn in (("arena", arena_call), ("dense", dense_call)):
                    us = graph_time_us(fn, calls)
                    part["%s_%s" % (src, mode)] = {"us": round(us, 2), "written_bytes": wr * nval, "ratio_to_copy": round(us / tc, 2),
                                                   "ratio_to_batch_gather_f32_default": round(us / sec["batch_gather_f32_default"]["us"], 2),
                                                   "ratio_to_batch_gather_f32_ieee": round(us / sec["batch_gather_f32_ieee"]["us"], 2)}
            host = [[tuple(r[:5]) for r in t.tolist()] for t in rows]

            def aten_call():
                k = nxt()
                aten_chain(arena, idxs[k], host[k])
            ua = graph_time_us(aten_call, calls)
            part["aten_chain_us"] = round(ua, 2)
            part["aten_over_kernel_arena_f32_ieee"] = round(ua / part["arena_f32_ieee"]["us"], 2)
            sec[name] = part
        res["%dx%dx%dx%d" % (N, C, H, W)] = sec
        del arena, idxs, dense
        torch.cuda.empty_cache()
    return res


def step_section(root, blocks, per_block):
    import torch
    from hallucidet_amd import synthetic
    from hallucidet_amd.dataloader import DevicePrefetcher, MultiModalDataModule
    from hallucidet_amd.dataloader.geometry import PairedGeometry
    lit = synthetic.make_module(seed=123, device="cuda", precision=16)
    dm = MultiModalDataModule("llvip", root, root, root, root, batch_size=N, num_workers=8, ext=".jpg", seed=123, cache="hbm", device="cuda",
                              log=lambda *a: None)

    def cycle(geometry):
        epoch = 0
        while True:
            if geometry is not None:
                geometry.set_epoch(epoch)
            for b in DevicePrefetcher(dm.train_dataloader(), "cuda", geometry=geometry):
                yield b
            epoch += 1
    feeds = {"off": cycle(None), "hflip_crop": cycle(PairedGeometry(seed=123))}
    for f in feeds.values():
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
            "off_block_spread_images_per_s": round(max(times["off"]) - min(times["off"]), 1),
            "hflip_crop_minus_off_images_per_s": round(med["hflip_crop"] - med["off"], 1), "steps_per_block": per_block, "batch": N}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=160, help="training pairs of the synthetic tree of the step section")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sections", default="kernel,step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry: no GPU visible (nothing here runs on the CPU)")
    res, tmp = {"device": torch.cuda.get_device_name(0), "host": os.uname().nodename}, None

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    try:
        if "kernel" in a.sections:
            res["kernel"] = kernel_section(a.reps)
            flush()
        if "step" in a.sections:
            from bench_dataset_cache import make_tree
            tmp = tempfile.mkdtemp(prefix="bench_geometry_")
            root = make_tree(tmp, a.pairs, 8)
            res["step"] = step_section(root, a.blocks, a.steps)
            flush()
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
