"""Cost of the IR pre-processing baselines (--ir-preprocess NAME, hd_ir_preprocess).

1. Every preset at 8x1x512x640 (the IR batch as the modules hold it: one plane per image) and 8x3x512x640, next to a `copy_` of the
   same fp32 batch (the least traffic a call can have: the batch read once and written once).  Kernel and copy timings are a captured
   graph of REPS back-to-back calls, timed with device events, so that host issue cost is not measured.
2. The same preset composed from torch device operations (torch.quantile, bincount, F.conv2d), the alternative a user would otherwise
   write.  bincount synchronises and cannot be captured, so these are REPS eager calls between two device events: host issue cost
   is part of that number, as it would be in a step.
3. An evaluation step (EncoderDecoderLit.test_step, 8x512x640) with the option on against off: alternating blocks in one process; the
   spread of the off blocks is printed next to the difference.

Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from bench_augment import graph_time_us

N, H, W = 8, 512, 640


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


# ---- the presets from torch device operations
def t_invert(x):
    return 1.0 - x


def t_stretch(x):
    q = torch.quantile(x.flatten(2), torch.tensor([0.003, 1 - 0.003], device=x.device), dim=2)
    q_min, q_max = q[0][:, :, None, None], q[1][:, :, None, None]
    return torch.minimum(torch.maximum((x - q_min) / (q_max - q_min), q_min), q_max)


def t_equalize(x):
    n, c, h, w = x.shape
    u = (x * 255).to(torch.uint8).to(torch.int64).view(n * c, h * w)
    planes = torch.arange(n * c, device=x.device)[:, None]
    hist = torch.bincount((u + 256 * planes).reshape(-1), minlength=n * c * 256).view(n * c, 256)
    last = 255 - torch.argmax((hist != 0).flip(1).to(torch.int8), dim=1)
    step = (h * w - hist.gather(1, last[:, None])[:, 0]) // 255
    lut = ((hist.cumsum(1) - hist + (step // 2)[:, None]) // step.clamp(min=1)[:, None]).clamp(0, 255)
    lut = torch.where(step[:, None] == 0, torch.arange(256, device=x.device)[None], lut)
    return (lut.gather(1, u).to(torch.float32) / 255.0).view(n, c, h, w)


def t_blur(x, k):
    c = x.shape[1]
    return F.conv2d(F.pad(x, [1, 1, 1, 1], mode="reflect"), k.expand(c, 1, 3, 3), groups=c)


def torch_preset(name, k):
    steps = {"invert": t_invert, "stretching": t_stretch, "equalization": t_equalize, "blur": lambda x: t_blur(x, k)}
    if name == "parallel":
        order = ["equalization", "invert"]
    elif name == "parallel_per_channel":
        return lambda x: torch.cat([t_equalize(x[:, 0:1]), t_invert(x[:, 1:2]), x[:, 2:3]], dim=1)
    else:
        order = [p for p in name.split("_")]
    fns = [steps[p] for p in order]

    def run(x):
        for f in fns:
            x = f(x)
        return x
    return run


def kernel_section(reps):
    from hallucidet_amd import ops
    from hallucidet_amd.models.cnnBasedThermalInfraredDA import IR_PREPROCESS
    dev = "cuda"
    a = torch.linspace(-1.0, 1.0, 3)
    pdf = torch.exp(-0.5 * (a / 0.8).pow(2))
    k1 = pdf / pdf.sum()
    k = torch.mm(k1[:, None], k1[None, :]).to(dev)
    res = {}
    for c in (1, 3):
        x = ((torch.rand(N, c, H, W, generator=torch.Generator().manual_seed(c)) ** 2.5 * 200 + 20).floor() / 255.0).to(dev)
        out = torch.empty_like(x)
        tc = graph_time_us(lambda: out.copy_(x), reps)
        sec = {"batch_bytes": x.numel() * 4, "copy_us": round(tc, 2), "copy_TBps": round(2 * x.numel() * 4 / tc / 1e6, 2)}
        for name, st in IR_PREPROCESS.items():
            if name == "parallel_per_channel" and c == 1:
                continue
            ws = torch.empty(ops.ir_preprocess_ws_bytes(x.shape, len(st)), dtype=torch.uint8, device=dev)
            t = graph_time_us(lambda: ops.ir_preprocess(x, st, out=out, ws=ws), reps)
            tt = eager_time_us(lambda: torch_preset(name, k)(x), reps)
            sec[name] = {"kernel_us": round(t, 2), "ratio_to_copy": round(t / tc, 2), "torch_ops_us": round(tt, 2), "torch_over_kernel": round(tt / t, 1)}
        res["8x%dx512x640" % c] = sec
    return res


def step_section(blocks, per_block, preset):
    from hallucidet_amd import synthetic
    lit = synthetic.make_module(seed=123, device="cuda", precision=16)
    lit.eval()
    batch = synthetic.make_batch(N, H, W, seed=123, device="cuda")
    for name in ("none", preset):
        lit.ir_preprocess = name
        for i in range(3):
            lit.test_step(batch, i)
    torch.cuda.synchronize()
    times = {"none": [], preset: []}
    for b in range(blocks):
        for name in (("none", preset) if b % 2 == 0 else (preset, "none")):
            lit.ir_preprocess = name
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(per_block):
                lit.test_step(batch, i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / per_block)
    lit.on_test_epoch_end()
    med = {n: statistics.median(v) for n, v in times.items()}
    return {"preset": preset, "ms_per_step_off": round(med["none"], 4), "ms_per_step_on": round(med[preset], 4),
            "delta_ms": round(med[preset] - med["none"], 4), "off_blocks_spread_ms": round(max(times["none"]) - min(times["none"]), 4),
            "blocks_off": [round(v, 3) for v in times["none"]], "blocks_on": [round(v, 3) for v in times[preset]],
            "steps_per_block": per_block, "batch": N}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--preset", default="invert_stretching_blur")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ir_preprocess: no GPU visible (nothing here runs on the CPU)")
    res = {"call": kernel_section(a.reps), "test_step_8x512x640": step_section(a.blocks, a.steps, a.preset)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
