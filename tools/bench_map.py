"""Cost of one COCO mAP evaluation: `update` over the split in batches of 8 images + `compute`, for the host evaluator
(metrics/metrics.py) and the device evaluator (metrics/device.py, --map-device cuda), on seeded synthetic scenes of the validation /
test sizes: 2 405 images x 30 detections, 2 405 x 100, 3 463 x 100 with 2 classes (LLVIP's 20 % validation split and its test
split).  Detections and targets start on the GPU, as the evaluation hooks hold them; the host evaluator pays its per-image copies.
Also checks that both evaluators return identical results.  Prints one JSON line; `--out FILE` also writes it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SIZES = ((2405, 30, 1), (2405, 100, 1), (3463, 100, 2))


def scene(n_img, n_det, n_cls, dev, seed=0):
    """Seeded one-GPU scene: ~3 ground truths per image, detections scattered around them (a share of pure false positives)."""
    g = torch.Generator().manual_seed(seed)
    preds, targets = [], []
    for _ in range(n_img):
        ng = int(torch.randint(1, 6, (1,), generator=g))
        xy = torch.rand(ng, 2, generator=g) * 500
        gb = torch.cat([xy, xy + 8 + torch.rand(ng, 2, generator=g) * 120], 1)
        gl = torch.randint(1, n_cls + 1, (ng,), generator=g)
        j = torch.randint(0, ng, (n_det,), generator=g)
        db = gb[j] + torch.randn(n_det, 4, generator=g) * 10
        db[:, 2:] = torch.maximum(db[:, 2:], db[:, :2] + 1)
        dl = torch.where(torch.rand(n_det, generator=g) < 0.85, gl[j], torch.randint(1, n_cls + 1, (n_det,), generator=g))
        ds = torch.rand(n_det, generator=g)
        preds.append({"boxes": db.to(dev), "scores": ds.to(dev), "labels": dl.to(dev)})
        targets.append({"boxes": gb.to(dev), "labels": gl.to(dev)})
    return preds, targets


def run(m, preds, targets, batch=8):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(0, len(preds), batch):
        m.update(preds[i:i + batch], targets[i:i + batch])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out = m.compute()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return out, t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-reps", type=int, default=3, help="device runs per size (the best is reported; the first includes warm-up)")
    ap.add_argument("--no-host", action="store_true", help="skip the host evaluator (and the identity check)")
    args = ap.parse_args()
    from hallucidet_amd.metrics import MeanAveragePrecision
    dev = torch.device("cuda:0")
    rows = []
    for n_img, n_det, n_cls in SIZES:
        preds, targets = scene(n_img, n_det, n_cls, dev)
        row = {"images": n_img, "dets_per_image": n_det, "classes": n_cls}
        best = None
        for _ in range(max(1, args.device_reps)):
            d_out, du, dc = run(MeanAveragePrecision(class_metrics=n_cls > 1).to(dev), preds, targets)
            if best is None or du + dc < best[0] + best[1]:
                best = (du, dc)
        row.update(device_update_s=round(best[0], 4), device_compute_s=round(best[1], 4), device_total_s=round(best[0] + best[1], 4))
        if not args.no_host:
            h_out, hu, hc = run(MeanAveragePrecision(class_metrics=n_cls > 1), preds, targets)
            row.update(host_update_s=round(hu, 3), host_compute_s=round(hc, 3), host_total_s=round(hu + hc, 3),
                       speedup=round((hu + hc) / (best[0] + best[1]), 1),
                       identical=all(torch.equal(h_out[k], d_out[k]) for k in h_out) and set(h_out) == set(d_out),
                       map=float(h_out["map"]))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = {"bench": "coco_map", "gpu": torch.cuda.get_device_name(0), "sizes": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
