"""Cost of the detection media (--save-media DIR, hd_media_render, utils/media.py).

1. One call at 8x3x512x640 and 8x3x1024x1280, each mode, without boxes and with 100 detections + 8 ground truths per image, next to a
   `copy_` of the same fp32 batch.  Kernel and copy timings are a captured graph of REPS back-to-back calls, timed with device events,
   so that host issue cost is not measured.  The call is bound by bytes: 4 B read + 1 B written per value in quantise mode, a second
   4 B read (the min/max pass) in normalise mode; `TBps` is those bytes over the time, `of_hbm_copy` that against the 6.29 TB/s a
   float4 copy reaches on an MI355X (8.0 TB/s spec).  A replayed 31 / 126 MB batch stays in the 256 MiB Infinity Cache, for the
   kernel and for the copy alike: read the ratio to the copy, not the absolute figure, as a statement about HBM.
2. An evaluation step (EncoderDecoderLit.test_step, 8x512x640) with the writer off, on at every=1 (the worst case: six panels per
   step, their D2H copies and the encoder's back-pressure) and on at every=100 (the batch index runs on across a configuration's
   blocks, so 60 steps log one batch): alternating blocks in one process.
3. `--step-off-only [--tree DIR]`: only the writer-off blocks, of this tree or of another checkout's package (the parent commit, built
   in DIR): run the two alternately as processes to compare the off path with the parent.

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
HBM_COPY_TBPS = 6.29
SHAPES = ((8, 512, 640), (8, 1024, 1280))


def kernel_section(reps):
    import torch
    from bench_augment import graph_time_us
    from hallucidet_amd import ops
    dev = "cuda"
    res = {}
    for N, H, W in SHAPES:
        g = torch.Generator().manual_seed(H)
        x = torch.rand(N, 3, H, W, generator=g).to(dev)
        dst = torch.empty_like(x)
        tc = graph_time_us(lambda: dst.copy_(x), reps)
        nval = x.numel()
        sec = {"batch_bytes": nval * 4, "copy_us": round(tc, 2), "copy_TBps": round(2 * nval * 4 / tc / 1e6, 2)}
        P, Q = 100, 8
        x1 = torch.rand(N, P + Q, generator=g) * (W - 90)
        y1 = torch.rand(N, P + Q, generator=g) * (H - 120)
        b = torch.stack([x1, y1, x1 + 16 + torch.rand(N, P + Q, generator=g) * 64, y1 + 32 + torch.rand(N, P + Q, generator=g) * 80], dim=2)
        det = (b[:, :P].contiguous().to(dev), torch.rand(N, P, generator=g).to(dev), torch.full((N,), P, dtype=torch.int32, device=dev))
        gt = (b[:, P:].double().contiguous().to(dev), torch.full((N,), Q, dtype=torch.int32, device=dev))
        ws = torch.empty(ops.media_ws_bytes(N), dtype=torch.uint8, device=dev)
        out = torch.empty(ops.media_canvas_shape(x.shape), dtype=torch.uint8, device=dev)
        ir = torch.rand(N, 1, H, W, generator=g).to(dev).expand(-1, 3, -1, -1)
        runs = {"quantise": (x, "quantise", None, None, nval * 5), "quantise_one_plane_view": (ir, "quantise", None, None, nval // 3 * 4 + nval),
                "normalise_no_boxes": (x, "normalise", None, None, nval * 9), "normalise_100_det_8_gt": (x, "normalise", det, gt, nval * 9)}
        for name, (xx, mode, d, t, nbytes) in runs.items():
            us = graph_time_us(lambda: ops.media_render(xx, mode, det=d, gt=t, out=out, ws=ws), reps)
            tbps = nbytes / us / 1e6
            sec[name] = {"us": round(us, 2), "ratio_to_copy": round(us / tc, 2), "bytes": nbytes, "TBps": round(tbps, 2),
                         "of_hbm_copy": round(tbps / HBM_COPY_TBPS, 2)}
        res["%dx3x%dx%d" % (N, H, W)] = sec
    return res


def _blocks(lit, batch, configs, blocks, per_block):
    """Alternating blocks; every configuration counts its own batch index on across its blocks, as one evaluation epoch would."""
    import torch
    times = {k: [] for k in configs}
    seen = {k: 0 for k in configs}
    for b in range(blocks):
        order = list(configs) if b % 2 == 0 else list(configs)[::-1]
        for name in order:
            lit.media = configs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(per_block):
                lit.test_step(batch, seen[name] + i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / per_block)
            seen[name] += per_block
    return times


def step_section(blocks, per_block, off_only):
    import torch
    from hallucidet_amd import synthetic
    N, H, W = SHAPES[0]
    lit = synthetic.make_module(seed=123, device="cuda", precision=16)
    lit.eval()
    batch = synthetic.make_batch(N, H, W, seed=123, device="cuda")
    tmp = None
    configs = {"off": None}
    if not off_only:
        from hallucidet_amd.utils.media import MediaWriter
        tmp = tempfile.mkdtemp(prefix="bench_media_")
        configs["every_1"] = MediaWriter(os.path.join(tmp, "e1"), every=1, offset=0)
        configs["every_100"] = MediaWriter(os.path.join(tmp, "e100"), every=100, offset=1)
    try:
        for name, w in configs.items():
            if hasattr(lit, "media"):
                lit.media = w
            for i in range(3):
                lit.test_step(batch, i)
        torch.cuda.synchronize()
        times = _blocks(lit, batch, configs, blocks, per_block)
        written = 0
        for w in configs.values():
            if w is not None:
                w.close()
        if tmp:
            written = sum(len(f) for _, _, f in os.walk(tmp))
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    lit.on_test_epoch_end()
    med = {n: statistics.median(v) for n, v in times.items()}
    out = {"ms_per_step": {n: round(v, 4) for n, v in med.items()}, "blocks": {n: [round(v, 3) for v in t] for n, t in times.items()},
           "off_blocks_spread_ms": round(max(times["off"]) - min(times["off"]), 4), "steps_per_block": per_block, "batch": N}
    if not off_only:
        out["delta_ms_every_1"] = round(med["every_1"] - med["off"], 4)
        out["delta_ms_every_100"] = round(med["every_100"] - med["off"], 4)
        out["png_files_written"] = written
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-off-only", action="store_true")
    ap.add_argument("--tree", default=None, help="with --step-off-only: take the hallucidet_amd package of this checkout")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_media: no GPU visible (nothing here runs on the CPU)")
    if a.step_off_only:
        res = {"tree": os.path.abspath(a.tree) if a.tree else ROOT, "test_step_8x512x640": step_section(a.blocks, a.steps, True)}
    else:
        res = {"call": kernel_section(a.reps), "test_step_8x512x640": step_section(a.blocks, a.steps, False)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
