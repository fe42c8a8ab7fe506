"""Cost of the structural loss (--structural ssim, hd_ssim_loss).

1. The kernel at 8x3x512x640 (one-plane IR, as the training step holds it), value-only and gradient mode, next to a `copy_` of the
   batch and to the ATen restatement of the same loss on the same GPU: grouped separable `F.conv2d` in fp32, both terms, forward plus
   autograd backward.  Every timing is a captured graph of REPS back-to-back calls, timed with device events, so that host issue cost
   is not measured (if the autograd chain cannot be captured it is timed eagerly, and the result says so).
2. Whole `fit_step` times with the option on (both weights 1.0) and off, two modules in one process, alternating blocks of steps,
   every step on a batch other than the previous one (six distinct batches in rotation: each step stages its inputs).

Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from bench_pixel_loss import graph_time_us


def aten_ssim(x, y, kh, kv):
    """mean SSIM of x [N, 3, H, W] against y [N, 3, H, W]: five grouped separable Gaussian filters and the pointwise index"""
    def G(t):
        return F.conv2d(F.conv2d(t, kh, groups=3), kv, groups=3)
    mx, my = G(x), G(y)
    sx, sy, sxy = G(x * x) - mx * mx, G(y * y) - my * my, G(x * y) - mx * my
    return (((2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4)) * ((2 * sxy + 9e-4) / (sx + sy + 9e-4))).mean()


def eager_time_us(fn, reps, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
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
    out = torch.empty(5, device=dev)
    res = {}
    res["value_us"] = round(graph_time_us(lambda: ops.ssim_loss(hall, rgb, ir, 1.0, 1.0, base_total=base, out=out), reps), 2)
    res["grad_us"] = round(graph_time_us(lambda: ops.ssim_loss(hall, rgb, ir, 1.0, 1.0, base_total=base, out=out, gs=gs, dhall=dh), reps), 2)
    dst = torch.empty_like(hall)
    res["copy_batch_us"] = round(graph_time_us(lambda: dst.copy_(hall), reps), 2)
    win = [math.exp(-((k - 5) ** 2) / 4.5) for k in range(11)]
    w1 = torch.tensor([v / sum(win) for v in win], dtype=torch.float64).float().to(dev)
    kh, kv = w1.view(1, 1, 1, 11).repeat(3, 1, 1, 1), w1.view(1, 1, 11, 1).repeat(3, 1, 1, 1)
    x = hall.clone().requires_grad_(True)
    ir3 = ir.expand(-1, 3, -1, -1)

    def aten():
        loss = (1 - aten_ssim(x, rgb, kh, kv)) + (1 - aten_ssim(x, ir3, kh, kv))
        return torch.autograd.grad(loss, x)[0]
    try:
        res["aten_fwd_bwd_us"], res["aten_timing"] = round(graph_time_us(aten, reps), 2), "graph"
    except Exception as err:          # capture of the autograd chain refused: time it as issued
        torch.cuda.synchronize()
        res["aten_fwd_bwd_us"], res["aten_timing"] = round(eager_time_us(aten, reps), 2), "eager (%s)" % type(err).__name__
    want = aten()
    dh.zero_()
    ops.ssim_loss(hall, rgb, ir, 1.0, 1.0, base_total=base, out=out, gs=gs, dhall=dh)
    torch.cuda.synchronize()
    res["max_abs_diff_to_aten_grad"] = float((dh - want).abs().max())
    res["aten_over_kernel"] = round(res["aten_fwd_bwd_us"] / res["grad_us"], 2)
    res["grad_over_copy"] = round(res["grad_us"] / res["copy_batch_us"], 2)
    res["value_over_copy"] = round(res["value_us"] / res["copy_batch_us"], 2)
    return res


def step_section(blocks, per_block):
    from hallucidet_amd import synthetic
    from hallucidet_amd.config import Config
    w = Config.Losses.hparams_losses_weights
    w["perceptual_rgb"], w["perceptual_ir"] = 1.0, 1.0
    mods = {"off": synthetic.make_module(seed=123), "on": synthetic.make_module(seed=123, loss_structural="ssim")}
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim: no GPU visible (nothing here runs on the CPU)")
    res = {"kernel_8x3x512x640": kernel_section(a.reps), "fit_step_8x512x640": step_section(a.blocks, a.steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
