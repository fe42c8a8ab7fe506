"""Cost of the log-average miss rate (`miss_rate=True`, hd_mr_accumulate) on top of one COCO mAP evaluation: `compute()` with the option
on against off, as alternating runs in one process over the same state, on the device evaluator and on the host evaluator, at the mAP
case of tools/bench_map.py (3 463 images x 100 detections x 2 classes, LLVIP's test split); and the two accumulation launches side by
side (hd_map_accumulate, hd_mr_accumulate with and without the curve output; device events around repeated calls on the arguments
compute() builds).  Also checks that both evaluators return identical results with the option on.  Prints one JSON line; `--out FILE`
also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_map import scene


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stats(xs, scale=1e3, nd=3):
    return {"median": round(statistics.median(xs) * scale, nd), "min": round(min(xs) * scale, nd), "max": round(max(xs) * scale, nd), "n": len(xs)}


def events(fn, reps):
    """Mean device time of one call in microseconds: events around `reps` back-to-back calls."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=3463)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--device-reps", type=int, default=10, help="alternating on / off compute() pairs on the device evaluator")
    ap.add_argument("--host-reps", type=int, default=2, help="alternating on / off compute() pairs on the host evaluator (0: skip it)")
    ap.add_argument("--launch-reps", type=int, default=50)
    args = ap.parse_args()
    from hallucidet_amd import ops
    from hallucidet_amd.metrics import MeanAveragePrecision
    dev = torch.device("cuda:0")
    preds, targets = scene(args.images, args.dets, args.classes, dev)
    res = {"bench": "miss_rate", "gpu": torch.cuda.get_device_name(0), "images": args.images, "dets_per_image": args.dets, "classes": args.classes}

    ev = {}
    for on in (False, True):
        ev[on] = MeanAveragePrecision(class_metrics=True, miss_rate=on).to(dev)
        for i in range(0, len(preds), 8):
            ev[on].update(preds[i:i + 8], targets[i:i + 8])
        ev[on].compute()                                             # warm-up
    t = {False: [], True: []}
    for _ in range(args.device_reps):
        for on in (False, True):
            d_out, dt = timed(ev[on].compute)
            t[on].append(dt)
    res["device_compute_ms"] = {"off": stats(t[False]), "on": stats(t[True]),
                                "added_median": round((statistics.median(t[True]) - statistics.median(t[False])) * 1e3, 3)}
    _, dt = timed(ev[True].miss_rate_curves)
    res["device_curves_ms"] = round(dt * 1e3, 3)

    # the two accumulation launches on the arguments compute() builds
    seen, real = {}, ops.map_accumulate
    ops.map_accumulate = lambda *a: (seen.setdefault("a", a), real(*a))[1]
    ev[True].compute()
    ops.map_accumulate = real
    order, class_off, flags, npig, n_eval, rec = seen["a"]
    ref = torch.tensor(MeanAveragePrecision.REF_FPPI, device=dev)
    res["launch_us"] = {"map_accumulate": round(events(lambda: ops.map_accumulate(order, class_off, flags, npig, n_eval, rec), args.launch_reps), 2),
                        "mr_accumulate": round(events(lambda: ops.mr_accumulate(order, class_off, flags, npig, n_eval, args.images, ref), args.launch_reps), 2),
                        "mr_accumulate_curve": round(events(lambda: ops.mr_accumulate(order, class_off, flags, npig, n_eval, args.images, ref, curve_t=0),
                                                            args.launch_reps), 2),
                        "class_segment_lengths": (class_off[1:] - class_off[:-1]).tolist()}

    if args.host_reps > 0:
        hv = {}
        for on in (False, True):
            hv[on] = MeanAveragePrecision(class_metrics=True, miss_rate=on)
            hv[on].update(preds, targets)
        t = {False: [], True: []}
        for _ in range(args.host_reps):
            for on in (False, True):
                h_out, dt = timed(hv[on].compute)
                t[on].append(dt)
        res["host_compute_s"] = {"off": stats(t[False], 1.0), "on": stats(t[True], 1.0),
                                 "added_median": round(statistics.median(t[True]) - statistics.median(t[False]), 3)}
        res["identical"] = set(h_out) == set(d_out) and all(torch.equal(h_out[k], d_out[k]) for k in h_out)
        hc, dc = hv[True].miss_rate_curves(), ev[True].miss_rate_curves()
        res["curves_identical"] = list(hc) == list(dc) and all((hc[c][k] == dc[c][k]).all() for c in hc for k in ("score", "fppi", "miss_rate"))
        res["lamr"] = float(h_out["lamr"])
        res["map_50"] = float(h_out["map_50"])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
