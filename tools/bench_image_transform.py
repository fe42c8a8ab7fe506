"""Cost of the detector-input resize modes (--detector-resize, hd_image_resample / hd_image_resample_bwd).

1. Per call, forward and gradient, at 8 and 24 x 3 x 512 x 640 -> 300 x 300 and 8 x 3 x 1024 x 1280 -> 300 x 300 (fp16 storage): the three
   modes through the new pair, the existing nearest kernels (hd_nchw_to_nhwc_resize / _bwd) and a `copy_` of the fp32 input batch.
   Every timing is a captured graph of REPS back-to-back calls between device events, so host issue cost is not measured.  Bytes are
   computed from the shapes (input batch + output batch; a resize that skips input pixels moves less than that); the ratios to the
   existing nearest kernels and to the copy are the yardstick.
2. A training step (EncoderDecoderLit.fit_step, 8 x 512 x 640) with resize_mode='bilinear_aa' against 'nearest': two modules, alternating
   blocks in one process; the spread of the nearest blocks is printed next to the difference.

Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_augment import graph_time_us

SIZES = [(8, 512, 640), (24, 512, 640), (8, 1024, 1280)]
OUT = 300
MODES = ("nearest", "bilinear", "bilinear_aa")


def call_section(reps):
    from hallucidet_amd import ops
    dev = "cuda"
    res = {}
    for n, h, w in SIZES:
        x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(n + h)).to(dev)
        xc = torch.empty_like(x)
        y = torch.empty(n, OUT, OUT, 8, dtype=torch.float16, device=dev)
        dy = torch.randn(n, OUT, OUT, 8, generator=torch.Generator().manual_seed(3)).half().to(dev)
        in_b, out_b = x.numel() * 4, y.numel() * 2
        tc = graph_time_us(lambda: xc.copy_(x), reps)
        f0 = graph_time_us(lambda: ops.nchw_to_nhwc_resize(x, OUT, OUT, 8, out=y), reps)
        b0 = graph_time_us(lambda: ops.nchw_to_nhwc_resize_bwd(dy, n, 3, h, w, 1.0), reps)
        sec = {"input_bytes": in_b, "output_bytes": out_b, "copy_us": round(tc, 2), "copy_TBps": round(2 * in_b / tc / 1e6, 2),
               "existing_nearest": {"fwd_us": round(f0, 2), "bwd_us": round(b0, 2)}}
        for m in MODES:
            ops.image_resample(x, OUT, OUT, m, out=y)                # uploads the tables outside the capture
            ops.image_resample_bwd(dy, n, 3, h, w, m)
            f = graph_time_us(lambda: ops.image_resample(x, OUT, OUT, m, out=y), reps)
            b = graph_time_us(lambda: ops.image_resample_bwd(dy, n, 3, h, w, m), reps)
            ty, tx = ops.resample_taps(h, OUT, m), ops.resample_taps(w, OUT, m)
            sec[m] = {"taps": [ty.T, tx.T], "fwd_us": round(f, 2), "bwd_us": round(b, 2),
                      "fwd_over_existing": round(f / f0, 2), "bwd_over_existing": round(b / b0, 2),
                      "fwd_over_copy": round(f / tc, 2), "bwd_over_copy": round(b / tc, 2),
                      "fwd_TBps_in_plus_out": round((in_b + out_b) / f / 1e6, 2), "bwd_TBps_in_plus_out": round((in_b + out_b) / b / 1e6, 2)}
        res["%dx3x%dx%d" % (n, h, w)] = sec
    return res


def step_section(blocks, per_block):
    from hallucidet_amd import synthetic
    lits = {m: synthetic.make_module(seed=123, device="cuda", precision=16, resize_mode=m) for m in ("nearest", "bilinear_aa")}
    batch = synthetic.make_batch(8, 512, 640, seed=123, device="cuda")
    for lit in lits.values():
        for _ in range(4):
            lit.fit_step(batch)
    torch.cuda.synchronize()
    times = {m: [] for m in lits}
    for b in range(blocks):
        for m in (("nearest", "bilinear_aa") if b % 2 == 0 else ("bilinear_aa", "nearest")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_block):
                lits[m].fit_step(batch)
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) * 1e3 / per_block)
    med = {m: statistics.median(v) for m, v in times.items()}
    return {"ms_per_step_nearest": round(med["nearest"], 4), "ms_per_step_bilinear_aa": round(med["bilinear_aa"], 4),
            "delta_ms": round(med["bilinear_aa"] - med["nearest"], 4),
            "nearest_blocks_spread_ms": round(max(times["nearest"]) - min(times["nearest"]), 4),
            "blocks_nearest": [round(v, 3) for v in times["nearest"]], "blocks_bilinear_aa": [round(v, 3) for v in times["bilinear_aa"]],
            "steps_per_block": per_block, "batch": 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_transform: no GPU visible (nothing here runs on the CPU)")
    res = {"call": call_section(a.reps)}
    if not a.no_step:
        res["fit_step_8x512x640"] = step_section(a.blocks, a.steps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
