"""An independent restatement of the log-average miss rate (Dollar, Wojek, Schiele, Perona: "Pedestrian Detection: An Evaluation of the
State of the Art", PAMI 2012; the procedure of the Caltech toolbox's compRoc): greedy matching per image in descending score order at
one IoU threshold with no ignore regions, a pointwise ROC over ALL detections sorted by score, and for each of the nine reference
false-positives-per-image rates the recall at the last ROC point whose FPPI does not exceed it.  Plain Python loops over plain floats;
it shares no code with hallucidet_amd.metrics.  Also the seeded scenes the miss-rate tests run on."""
import math

import numpy as np
import torch

MAX_DETS = 100


def ref_rates():
    return np.logspace(-2.0, 0.0, 9)


def _iou(a, b):
    aa = (a[2] - a[0]) * (a[3] - a[1])
    ab = (b[2] - b[0]) * (b[3] - b[1])
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    inter = max(w, 0.0) * max(h, 0.0)
    return inter / (aa + ab - inter)


def match_image(det_boxes, det_scores, gt_boxes, thr=0.5):
    """-> (scores, is_tp) of the image's detections in descending score order (ties: input order), at most MAX_DETS of them.  Each
    detection takes the still-free ground truth of largest IoU >= thr (COCO's rule: of equal IoUs the later ground truth)."""
    ranked = sorted(range(len(det_scores)), key=lambda j: -det_scores[j])[:MAX_DETS]          # sorted() is stable
    free = [True] * len(gt_boxes)
    scores, is_tp = [], []
    for j in ranked:
        best, pick = thr, -1
        for g, gb in enumerate(gt_boxes):
            if not free[g]:
                continue
            v = _iou(det_boxes[j], gb)
            if v >= best:
                best, pick = v, g
        if pick >= 0:
            free[pick] = False
        scores.append(det_scores[j])
        is_tp.append(pick >= 0)
    return scores, is_tp


def roc_hits(scores, is_tp, n_img, n_gt):
    """Pointwise ROC over detections already concatenated in image order -> (hit [9] int, miss [9], lamr, xs, ys) with xs / ys the
    curve (FPPI, miss rate) per detection in the global order."""
    order = sorted(range(len(scores)), key=lambda j: -scores[j])
    tp = fp = 0
    xs1, tp1 = [-math.inf], [0]
    for j in order:
        if is_tp[j]:
            tp += 1
        else:
            fp += 1
        xs1.append(fp / n_img)
        tp1.append(tp)
    hit = []
    for ref in ref_rates():
        last = max(i for i, x in enumerate(xs1) if x <= ref)
        hit.append(tp1[last])
    miss = [1.0 - h / n_gt for h in hit]
    lamr = math.exp(sum(math.log(max(1e-10, m)) for m in miss) / len(miss))
    return hit, miss, lamr, xs1[1:], [1.0 - t / n_gt for t in tp1[1:]], [scores[j] for j in order]


def evaluate(preds, targets, thr=0.5):
    """{class: dict(hit, miss, lamr, fppi, miss_rate, score, n_gt, tp, fp) or None when the class has no ground truth}, and the mean
    lamr over the classes that have one (-1 when none has)."""
    P = [{k: np.asarray(v.tolist(), dtype=np.float64) for k, v in p.items()} for p in preds]
    G = [{k: np.asarray(v.tolist(), dtype=np.float64) for k, v in t.items()} for t in targets]
    labels = sorted({int(x) for d in P for x in d["labels"]} | {int(x) for g in G for x in g["labels"]})
    n_img = len(targets)
    out = {}
    for c in labels:
        scores, is_tp, n_gt = [], [], 0
        for p, g in zip(P, G):
            dsel, gsel = p["labels"] == c, g["labels"] == c
            s, t = match_image(p["boxes"].reshape(-1, 4)[dsel].tolist(), p["scores"][dsel].tolist(), g["boxes"].reshape(-1, 4)[gsel].tolist(), thr)
            scores += s
            is_tp += t
            n_gt += int(gsel.sum())
        if n_gt == 0:
            out[c] = None
            continue
        hit, miss, lamr, xs, ys, sc = roc_hits(scores, is_tp, n_img, n_gt)
        out[c] = dict(hit=hit, miss=miss, lamr=lamr, fppi=xs, miss_rate=ys, score=sc, n_gt=n_gt, tp=sum(is_tp), fp=len(is_tp) - sum(is_tp))
    vals = [v["lamr"] for v in out.values() if v is not None]
    return out, (sum(vals) / len(vals) if vals else -1.0)


# ---------------------------------------------------------------------------------------------------------------- scenes
def box(x, y, w, h):
    return [x, y, x + w, y + h]


def tensors(db, ds, dl, gb, gl):
    return ({"boxes": torch.tensor(db, dtype=torch.float32).reshape(-1, 4), "scores": torch.tensor(ds, dtype=torch.float32),
             "labels": torch.tensor(dl, dtype=torch.int64)},
            {"boxes": torch.tensor(gb, dtype=torch.float32).reshape(-1, 4), "labels": torch.tensor(gl, dtype=torch.int64)})


def scene(seed, n_img=24, classes=(1,), big=False):
    """Seeded scenes with the awkward cases: quantised scores (ties within and across images), detections at IoU exactly 0.5 / 0.75
    with a ground truth, ground truths of area exactly 32^2 / 96^2, empty and ground-truth-only images, a class present only in
    detections, images with more than 10 (big: more than 100) detections."""
    rng = np.random.default_rng(seed)
    preds, targets = [], []
    det_only = max(classes) + 1
    for i in range(n_img):
        kind = i % 6
        gb, gl, db, ds, dl = [], [], [], [], []
        if kind == 1:
            for _ in range(rng.integers(1, 4)):
                gb.append(box(*rng.uniform(0, 200, 2), *rng.uniform(5, 120, 2)))
                gl.append(int(rng.choice(classes)))
        elif kind != 0:
            ng = int(rng.integers(1, 9))
            for g in range(ng):
                side = [32.0, 96.0, None][g % 3]
                w, h = (side, side) if side else tuple(rng.uniform(4, 150, 2))
                x, y = rng.uniform(0, 300, 2)
                c = int(rng.choice(classes))
                gb.append(box(x, y, w, h))
                gl.append(c)
                for frac in (0.5, 0.75):
                    if rng.random() < 0.6:
                        db.append(box(x, y, w, h * frac))
                        ds.append(float(rng.integers(1, 9)) / 8.0)
                        dl.append(c)
            nd = int(rng.integers(0, 30)) if not big else int(rng.integers(90, 160))
            if kind == 5:
                nd += 12
            for _ in range(nd):
                j = int(rng.integers(0, ng))
                bx = np.asarray(gb[j]) + rng.normal(0, 6, 4)
                bx[2:] = np.maximum(bx[2:], bx[:2] + 1.0)
                db.append(bx.tolist())
                ds.append(float(rng.integers(1, 17)) / 16.0 if rng.random() < 0.5 else float(rng.random()))
                dl.append(gl[j] if rng.random() < 0.8 else int(rng.choice(classes)))
            if rng.random() < 0.3:
                db.append(box(*rng.uniform(0, 200, 2), 20.0, 20.0))
                ds.append(0.5)
                dl.append(det_only)
        p, t = tensors(db, ds, dl, gb, gl)
        preds.append(p)
        targets.append(t)
    return preds, targets


def grid_scene(n_img, n_gt, flags_per_image, label=1, scores=None):
    """Images of `n_gt` disjoint 20 x 20 ground truths on a grid; detection j of image i is a true positive (an exact copy of a free
    ground truth) where flags_per_image[i][j], else a far-away box.  scores[i][j] (default: descending within the image)."""
    preds, targets = [], []
    for i in range(n_img):
        gb = [box(40.0 * g, 0.0, 20.0, 20.0) for g in range(n_gt[i])]
        fl = flags_per_image[i]
        db, used = [], 0
        for j, f in enumerate(fl):
            if f:
                db.append(gb[used])
                used += 1
            else:
                db.append(box(40.0 * j, 500.0, 20.0, 20.0))
        assert used <= n_gt[i]
        ds = list(scores[i]) if scores is not None else [1.0 - (j + 1) / (len(fl) + 1.0) for j in range(len(fl))]
        p, t = tensors(db, ds, [label] * len(fl), gb, [label] * n_gt[i])
        preds.append(p)
        targets.append(t)
    return preds, targets


def worked_case():
    """The issue's worked case: 4 images, 5 ground truths, nine detections in score order TP FP TP TP FP FP TP FP FP."""
    order = [True, False, True, True, False, False, True, False, False]
    scores = [0.9 - 0.05 * j for j in range(9)]
    # image 0: detections 0-2, image 1: 3-5, image 2: 6-8, image 3: empty
    fl = [order[0:3], order[3:6], order[6:9], []]
    sc = [scores[0:3], scores[3:6], scores[6:9], []]
    return grid_scene(4, [2, 2, 1, 0], fl, scores=sc)
