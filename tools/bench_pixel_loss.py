"""Cost of the pixel reconstruction loss (--pixel, hd_pixel_loss).

1. The kernel at 8x3x512x640 (one-plane IR, as the training step holds it), value-only and gradient mode, each next to a `copy_` that
   moves the same bytes (read + write) in the same process.  Every timing is a captured graph of REPS back-to-back calls, timed with
   device events, so that host issue cost is not measured.
2. Whole `fit_step` times with the option on (mse, both weights 1.0) and off, two modules in one process, alternating blocks of
   steps, every step on a batch other than the previous one (six distinct batches in rotation: each step stages its inputs).

Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


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


def kernel_section(reps):
    from hallucidet_amd import ops
    N, H, W = 8, 512, 640
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    hall = torch.rand(N, 3, H, W, generator=g).to(dev)
    rgb = torch.rand(N, 3, H, W, generator=g).to(dev)
    ir = torch.rand(N, 1, H, W, generator=g).to(dev)
    dh = torch.zeros_like(hall)
    gs = torch.tensor(1.0, device=dev)
    base = torch.zeros((), device=dev)
    out = torch.empty(3, device=dev)
    b_val = (hall.numel() * 2 + ir.numel()) * 4                 # hall + rgb + ir read
    b_grad = b_val + hall.numel() * 4 * 2                       # + dhall read and written
    res = {}
    for mode, nbytes, kw in (("value", b_val, {}), ("grad", b_grad, dict(gs=gs, dhall=dh))):
        t = graph_time_us(lambda: ops.pixel_loss(hall, rgb, ir, "mse", 1.0, 1.0, base_total=base, out=out, **kw), reps)
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)          # copy_: nbytes / 2 read + nbytes / 2 written
        dst = torch.empty_like(src)
        tc = graph_time_us(lambda: dst.copy_(src), reps)
        res[mode] = {"bytes": nbytes, "kernel_us": round(t, 2), "copy_same_bytes_us": round(tc, 2), "ratio_to_copy": round(t / tc, 3),
                     "kernel_TBps": round(nbytes / t / 1e6, 2), "copy_TBps": round(nbytes / tc / 1e6, 2)}
        del src, dst
    return res


def step_section(blocks, per_block):
    from hallucidet_amd import synthetic
    from hallucidet_amd.config import Config
    w = Config.Losses.hparams_losses_weights
    w["pixel_rgb"], w["pixel_ir"] = 1.0, 1.0
    mods = {"off": synthetic.make_module(seed=123), "on": synthetic.make_module(seed=123, loss_pixel="mse")}
    batches = [synthetic.make_batch(8, seed=200 + i, device="cuda") for i in range(6)]
    k = 0
    for m in mods.values():                       # capture + warm-up
        for _ in range(4):
            m.fit_step(batches[k % len(batches)])
            k += 1
    torch.cuda.synchronize()
    times = {"off": [], "on": []}
    for b in range(blocks):
        for name in (("off", "on") if b % 2 == 0 else ("on", "off")):
            m = mods[name]
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_block):
                loss = m.fit_step(batches[k % len(batches)])
                k += 1
            e.record()
            e.synchronize()
            times[name].append(a.elapsed_time(e) / per_block)
    assert torch.isfinite(loss)
    med = {n: statistics.median(v) for n, v in times.items()}
    return {"ms_per_step_off": round(med["off"], 4), "ms_per_step_on": round(med["on"], 4),
            "delta_ms": round(med["on"] - med["off"], 4),
            "blocks_off": [round(v, 4) for v in times["off"]], "blocks_on": [round(v, 4) for v in times["on"]],
            "steps_per_block": per_block, "captures_on": mods["on"]._detector_graph().captures}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixel_loss: no GPU visible (nothing here runs on the CPU)")
    res = {"kernel_8x3x512x640": kernel_section(a.reps), "fit_step_8x512x640": step_section(a.blocks, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
