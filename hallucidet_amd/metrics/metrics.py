"""COCO-style mean average precision for the evaluation hooks (reference src/metrics/metrics.py:7-32 wraps
torchmetrics 0.6.0 `MAP` [EXT, not installable offline]; used at train_hallucidet.py:121-131,213-215,330-332,399-416 and
train_detector.py: `.update(detections, targets)`, `.compute()`, `.reset()`, result keys map / map_50 / map_75 /
map_small / map_medium / map_large / mar_1 / mar_10 / mar_100 / mar_small / mar_medium / mar_large / map_per_class /
mar_100_per_class).

This is host-side bookkeeping off the GPU hot path ("CPU-side"): numpy on the host, restating the
published COCO evaluation (pycocotools `evaluateImg` / `accumulate` / `summarize`, which torchmetrics' MAP re-implements):
IoU thresholds .50:.05:.95, 101 recall points, detections per image 1 / 10 / 100, area ranges all / small (<32^2) /
medium / large (>96^2), greedy matching in descending score order, precision envelope, AP = mean over the sampled
precision values.  PARITY UNPINNED against torchmetrics itself (absent); pinned by hand-worked cases in
tests/test_metrics.py.

Log-average miss rate (`miss_rate=True`; "LAMR", MR^-2 of Dollar et al., PAMI 2012), the ranking figure of the pedestrian benchmarks
(KAIST's only official metric, next to AP in the LLVIP paper), from the SAME per-image matches as the mAP.  For a class k, an area
range a of AREA_RNG and an IoU threshold t of IOU_THRS:
  inputs      the per-image results of `_evaluate_img` at max-dets 100 (scores, dtm[t], dig[t], npos); an image for which it returns
              None contributes nothing
  order       concatenated in image order, then descending score with the stable sort of `_accumulate`
  counts      tp_j = cumsum(dtm & ~dig), fp_j = cumsum(~dtm & ~dig); an ignored detection counts as neither
  images      n_img = the number of images passed to update(), images without any box included (not the per-class evaluated count);
              n_gt = sum of npos
  undefined   no image evaluated for the class, or n_gt == 0: -1, the rule of the mAP arrays
  rates       REF_FPPI = np.logspace(-2.0, 0.0, 9) in float64 (this very array; the device receives these nine doubles)
  hit         fppi_j = float64(fp_j) / float64(n_img); hit_i = max{tp_j : fppi_j <= REF_FPPI[i]}, 0 when no point qualifies or there is
              no detection (Dollar's "recall at the last point with fppi <= ref"; tp is non-decreasing, so the last is the max)
  miss rate   mr_i = 1.0 - hit_i / n_gt; lamr = exp(mean(log(maximum(mr, 1e-10))))
The integer part (hit, the final tp / fp) is what the device evaluator computes in HIP (hd_mr_accumulate); the float part
(`mr_summary`, `mr_curve`) is this module's numpy code on both paths, so the two agree by construction.
"""
from typing import Dict, List

import numpy as np
import torch


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def box_iou_np(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """[A,4] x [B,4] xyxy -> [A,B]"""
    if a.size == 0 or b.size == 0:
        return np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    a, b = a.astype(np.float64), b.astype(np.float64)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b[None, :] - inter)


class MeanAveragePrecision:
    IOU_THRS = np.linspace(0.5, 0.95, 10)
    REC_THRS = np.linspace(0.0, 1.0, 101)
    MAX_DETS = (1, 10, 100)
    AREA_RNG = {"all": (0.0, 1e10), "small": (0.0, 32.0 ** 2), "medium": (32.0 ** 2, 96.0 ** 2), "large": (96.0 ** 2, 1e10)}
    REF_FPPI = np.logspace(-2.0, 0.0, 9)                 # the nine reference false-positives-per-image rates of the log-average miss rate
    MR_FLOOR = 1e-10
    MR_KEYS = ("lamr", "lamr_75", "lamr_small", "lamr_medium", "lamr_large", "mr_fppi01", "lamr_per_class")

    def __init__(self, box_format: str = "xyxy", class_metrics: bool = False, miss_rate: bool = False):
        if box_format != "xyxy":
            raise NotImplementedError("the reference only ever uses xyxy boxes (metrics.py:17)")
        self.class_metrics = class_metrics
        self.miss_rate = bool(miss_rate)
        self.reset()

    def to(self, device):
        """A CPU device keeps this host evaluator; a GPU device returns the device evaluator (metrics/device.py) with the same options
        and the images seen so far."""
        if torch.device(device).type == "cpu":
            return self
        from .device import DeviceMeanAveragePrecision
        d = DeviceMeanAveragePrecision(class_metrics=self.class_metrics, device=device, miss_rate=self.miss_rate)
        if self._gts:
            d.update([{k: torch.from_numpy(v) for k, v in p.items()} for p in self._dets],
                     [{k: torch.from_numpy(v) for k, v in t.items()} for t in self._gts])
        return d

    def reset(self):
        self._dets: List[Dict[str, np.ndarray]] = []
        self._gts: List[Dict[str, np.ndarray]] = []
        self._mr = None                 # (hit, total, npig, n_img) and the curve counts of the last compute(); update() drops them
        self._mr_curves = None

    # ------------------------------------------------------------------ update
    def update(self, preds, target):
        preds, target = list(preds), list(target)
        if len(preds) != len(target):
            raise ValueError("Expected argument `preds` and `target` to have the same length")
        for p in preds:
            for k in ("boxes", "scores", "labels"):
                if k not in p:
                    raise ValueError(f"Expected all dicts in `preds` to contain the `{k}` key")
        for t in target:
            for k in ("boxes", "labels"):
                if k not in t:
                    raise ValueError(f"Expected all dicts in `target` to contain the `{k}` key")
        self._mr = self._mr_curves = None
        for p, t in zip(preds, target):
            self._dets.append({"boxes": _np(p["boxes"]).reshape(-1, 4).astype(np.float64), "scores": _np(p["scores"]).reshape(-1).astype(np.float64),
                               "labels": _np(p["labels"]).reshape(-1).astype(np.int64)})
            self._gts.append({"boxes": _np(t["boxes"]).reshape(-1, 4).astype(np.float64), "labels": _np(t["labels"]).reshape(-1).astype(np.int64)})

    # ------------------------------------------------------------------ per image / class / area evaluation
    def _evaluate_img(self, i, c, rng, max_det):
        g, d = self._gts[i], self._dets[i]
        gsel, dsel = g["labels"] == c, d["labels"] == c
        gb, db, ds = g["boxes"][gsel], d["boxes"][dsel], d["scores"][dsel]
        if gb.shape[0] == 0 and db.shape[0] == 0:
            return None
        garea = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
        gig = (garea < rng[0]) | (garea > rng[1])
        gorder = np.argsort(gig, kind="mergesort")                 # non-ignored ground truth first
        gb, gig = gb[gorder], gig[gorder]
        dorder = np.argsort(-ds, kind="mergesort")[:max_det]
        db, ds = db[dorder], ds[dorder]
        ious = box_iou_np(db, gb)
        T, D, G = len(self.IOU_THRS), db.shape[0], gb.shape[0]
        gtm = np.zeros((T, G), dtype=bool)
        dtm = np.zeros((T, D), dtype=bool)
        dig = np.zeros((T, D), dtype=bool)
        for ti, t in enumerate(self.IOU_THRS):
            for di in range(D):
                best, m = min(t, 1 - 1e-10), -1
                for gi in range(G):
                    if gtm[ti, gi]:
                        continue
                    if m > -1 and not gig[m] and gig[gi]:
                        break                                     # matched a regular gt; only ignored ones follow
                    if ious[di, gi] < best:
                        continue
                    best, m = ious[di, gi], gi
                if m == -1:
                    continue
                dig[ti, di] = gig[m]
                dtm[ti, di] = True
                gtm[ti, m] = True
        darea = (db[:, 2] - db[:, 0]) * (db[:, 3] - db[:, 1])
        out = (darea < rng[0]) | (darea > rng[1])
        dig = dig | (~dtm & out[None, :])
        return {"scores": ds, "dtm": dtm, "dig": dig, "npos": int((~gig).sum())}

    @staticmethod
    def _cut(e, md):
        """The per-image result at max-dets `md` from the one at the largest max-dets: matching runs in score order, one detection
        after the other, so the first md columns are what `_evaluate_img(..., md)` returns."""
        return {"scores": e["scores"][:md], "dtm": e["dtm"][:, :md], "dig": e["dig"][:, :md], "npos": e["npos"]}

    def _accumulate(self, classes):
        T, R, K, A, M = len(self.IOU_THRS), len(self.REC_THRS), len(classes), len(self.AREA_RNG), len(self.MAX_DETS)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        n_img = len(self._gts)
        md_top = max(self.MAX_DETS)
        if self.miss_rate:
            hit = -np.ones((T, K, A, len(self.REF_FPPI)), dtype=np.int32)
            total = -np.ones((T, K, A, 2), dtype=np.int32)
            npigs = np.zeros((K, A), dtype=np.int32)
            curves = {}
        for ki, c in enumerate(classes):
            for ai, rng in enumerate(self.AREA_RNG.values()):
                # one matching per (image, class, area), at the largest max-dets; the smaller ones are its prefixes
                top = [e for e in (self._evaluate_img(i, c, rng, md_top) for i in range(n_img)) if e is not None]
                if not top:
                    continue
                npig = sum(e["npos"] for e in top)
                if self.miss_rate:
                    npigs[ki, ai] = npig
                if npig == 0:
                    continue
                for mi, md in enumerate(self.MAX_DETS):
                    ev = top if md == md_top else [self._cut(e, md) for e in top]
                    scores = np.concatenate([e["scores"] for e in ev])
                    order = np.argsort(-scores, kind="mergesort")
                    dtm = np.concatenate([e["dtm"] for e in ev], axis=1)[:, order]
                    dig = np.concatenate([e["dig"] for e in ev], axis=1)[:, order]
                    tpi = np.cumsum(dtm & ~dig, axis=1)
                    fpi = np.cumsum(~dtm & ~dig, axis=1)
                    tps, fps = tpi.astype(np.float64), fpi.astype(np.float64)
                    if self.miss_rate and md == md_top:
                        for ti in range(T):
                            hit[ti, ki, ai], total[ti, ki, ai] = self.mr_hits(tpi[ti], fpi[ti], ~dig[ti], n_img)
                        if ai == list(self.AREA_RNG).index("all"):
                            curves[c] = (scores[order], tpi[0], fpi[0], npig)
                    for ti in range(T):
                        tp, fp = tps[ti], fps[ti]
                        nd = tp.shape[0]
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[ti, ki, ai, mi] = rc[-1] if nd else 0.0
                        pr = pr.tolist()
                        for j in range(nd - 1, 0, -1):
                            if pr[j] > pr[j - 1]:
                                pr[j - 1] = pr[j]
                        inds = np.searchsorted(rc, self.REC_THRS, side="left")
                        q = np.zeros(R)
                        for ri, pi in enumerate(inds):
                            if pi < nd:
                                q[ri] = pr[pi]
                        precision[ti, :, ki, ai, mi] = q
        if self.miss_rate:
            self._mr, self._mr_curves = (hit, total, npigs, n_img), (n_img, curves)
        return precision, recall

    # ------------------------------------------------------------------ log-average miss rate (definition: module docstring)
    @classmethod
    def mr_hits(cls, tp, fp, counted, n_img):
        """Cumulative integer tp / fp over one segment's detections in the global order, `counted` = not ignored.
        -> (hit [9] = max tp among the counted points with fp / n_img <= REF_FPPI[i], 0 when none; (final tp, final fp))."""
        tpc, fpc = tp[counted], fp[counted]
        fppi = fpc.astype(np.float64) / np.float64(n_img)
        last = np.searchsorted(fppi, cls.REF_FPPI, side="right")          # fppi is non-decreasing: the points with fppi <= ref are a prefix
        hit = np.where(last > 0, tpc[np.maximum(last, 1) - 1] if tpc.size else 0, 0)
        tot = (int(tp[-1]), int(fp[-1])) if tp.size else (0, 0)
        return hit.astype(np.int32), np.asarray(tot, dtype=np.int32)

    @classmethod
    def mr_summary(cls, hit, npig):
        """hit [T,K,A,9] int (-1: undefined), npig [K,A] -> (lamr [T,K,A], mr [T,K,A,9]) float64, -1 where undefined."""
        hit, npig = np.asarray(hit), np.asarray(npig)
        ok = hit[..., 0] >= 0
        n_gt = np.where(npig > 0, npig, 1).astype(np.float64)[None, :, :, None]
        mr = 1.0 - hit.astype(np.float64) / n_gt
        with np.errstate(divide="ignore", invalid="ignore"):
            lamr = np.exp(np.mean(np.log(np.maximum(mr, cls.MR_FLOOR)), axis=-1))
        return np.where(ok, lamr, -1.0), np.where(ok[..., None], mr, -1.0)

    @staticmethod
    def mr_curve(score, tp, fp, n_img, n_gt):
        """One class's MR-FPPI curve from the cumulative integer counts at every position of its global order: one point per
        non-ignored detection (a position where tp + fp grew)."""
        tp, fp = np.asarray(tp, dtype=np.int64), np.asarray(fp, dtype=np.int64)
        seen = tp + fp
        counted = np.diff(seen, prepend=0) > 0
        return {"score": np.asarray(score, dtype=np.float64)[counted], "fppi": fp[counted].astype(np.float64) / np.float64(n_img),
                "miss_rate": 1.0 - tp[counted].astype(np.float64) / np.float64(n_gt), "n_images": int(n_img), "n_gt": int(n_gt)}

    def _mr_results(self, classes):
        """The miss-rate keys of compute() from the integer arrays `_accumulate` left in self._mr."""
        hit, _, npig, _ = self._mr
        lamr, mr = self.mr_summary(hit, npig)
        areas = list(self.AREA_RNG)
        a_all, t50, t75 = areas.index("all"), 0, 5
        res = {"lamr": self._mean(lamr[t50, :, a_all]), "lamr_75": self._mean(lamr[t75, :, a_all]),
               "lamr_small": self._mean(lamr[t50, :, areas.index("small")]), "lamr_medium": self._mean(lamr[t50, :, areas.index("medium")]),
               "lamr_large": self._mean(lamr[t50, :, areas.index("large")]), "mr_fppi01": self._mean(mr[t50, :, a_all, 4])}
        out = {k: torch.tensor(v, dtype=torch.float32) for k, v in res.items()}
        if self.class_metrics and classes:
            out["lamr_per_class"] = torch.tensor([float(lamr[t50, k, a_all]) for k in range(len(classes))], dtype=torch.float32)
        else:
            out["lamr_per_class"] = torch.tensor(-1.0)
        return out

    def miss_rate_counts(self):
        """The integers behind the miss-rate keys: {"classes" [K], "hit" [T,K,A,9], "total" [T,K,A,2] (final tp, fp), "n_gt" [K,A],
        "n_images"}; -1 in hit / total where the segment is undefined.  Call it before reset()."""
        if not self.miss_rate:
            raise ValueError("miss_rate_counts() needs an evaluator built with miss_rate=True")
        if self._mr is None:
            self.compute()
        hit, total, npig, n_img = self._mr
        return {"classes": self._mr_classes, "hit": hit, "total": total, "n_gt": npig, "n_images": int(n_img)}

    def miss_rate_curves(self):
        """{class label: {"score", "fppi", "miss_rate" (float64 arrays, one point per non-ignored detection in the global order, IoU 0.5,
        area all, max-dets 100), "n_images", "n_gt"}} for every class with a defined miss rate.  Call it before reset()."""
        if not self.miss_rate:
            raise ValueError("miss_rate_curves() needs an evaluator built with miss_rate=True")
        if self._mr_curves is None:
            self.compute()
        n_img, curves = self._mr_curves
        return {int(c): self.mr_curve(s, tp, fp, n_img, n_gt) for c, (s, tp, fp, n_gt) in curves.items()}

    @staticmethod
    def _mean(x):
        x = x[x > -1]
        return float(x.mean()) if x.size else -1.0

    def compute(self) -> Dict[str, torch.Tensor]:
        classes = sorted(set(np.concatenate([g["labels"] for g in self._gts] + [d["labels"] for d in self._dets]).tolist())) if self._gts else []
        precision, recall = self._accumulate(classes)
        self._mr_classes = list(classes)
        areas = list(self.AREA_RNG)
        a_all, m100 = areas.index("all"), self.MAX_DETS.index(100)
        t50, t75 = 0, 5
        res = {
            "map": self._mean(precision[:, :, :, a_all, m100]),
            "map_50": self._mean(precision[t50, :, :, a_all, m100]),
            "map_75": self._mean(precision[t75, :, :, a_all, m100]),
            "map_small": self._mean(precision[:, :, :, areas.index("small"), m100]),
            "map_medium": self._mean(precision[:, :, :, areas.index("medium"), m100]),
            "map_large": self._mean(precision[:, :, :, areas.index("large"), m100]),
            "mar_1": self._mean(recall[:, :, a_all, self.MAX_DETS.index(1)]),
            "mar_10": self._mean(recall[:, :, a_all, self.MAX_DETS.index(10)]),
            "mar_100": self._mean(recall[:, :, a_all, m100]),
            "mar_small": self._mean(recall[:, :, areas.index("small"), m100]),
            "mar_medium": self._mean(recall[:, :, areas.index("medium"), m100]),
            "mar_large": self._mean(recall[:, :, areas.index("large"), m100]),
        }
        out = {k: torch.tensor(v, dtype=torch.float32) for k, v in res.items()}
        if self.class_metrics and classes:
            out["map_per_class"] = torch.tensor([self._mean(precision[:, :, k, a_all, m100]) for k in range(len(classes))], dtype=torch.float32)
            out["mar_100_per_class"] = torch.tensor([self._mean(recall[:, k, a_all, m100]) for k in range(len(classes))], dtype=torch.float32)
        else:
            out["map_per_class"] = torch.tensor(-1.0)
            out["mar_100_per_class"] = torch.tensor(-1.0)
        if self.miss_rate:
            out.update(self._mr_results(classes))
        return out


MAP = MeanAveragePrecision


class Detection():
    """metrics.py:14-32"""

    def __init__(self, box_format='xyxy', device='cpu', class_metrics=False, miss_rate=False):
        self.device = device
        self.map = self.metric_map(box_format=box_format, class_metrics=class_metrics, miss_rate=miss_rate)

    def iou_bboxes(self, bbox1, bbox2):
        # the reference slices `[:, 3:]` of its 7-column rows (class, score, ?, x1, y1, x2, y2) and truncates to int
        a = torch.Tensor(bbox1)[:, 3:].int().numpy().astype(np.float64)
        b = torch.Tensor(bbox2)[:, 3:].int().numpy().astype(np.float64)
        return box_iou_np(a, b).astype(np.float32)

    def metric_map(self, box_format='xyxy', class_metrics=False, miss_rate=False):
        return MeanAveragePrecision(box_format=box_format, class_metrics=class_metrics, miss_rate=miss_rate).to(self.device)


def write_miss_rate_curves(metric, dirpath, split, stream):
    """--miss-rate-curves DIR: one `DIR/{split}_{stream}_class{label}.csv` (columns score, fppi, miss_rate; one row per non-ignored
    detection in descending score order, floats written with repr so that they read back exactly) per class of metric.miss_rate_curves().
    Call it before the evaluator is reset.  -> the paths written."""
    import os
    os.makedirs(dirpath, exist_ok=True)
    paths = []
    for label, cv in sorted(metric.miss_rate_curves().items()):
        path = os.path.join(dirpath, "%s_%s_class%d.csv" % (split, stream, label))
        with open(path, "w") as f:
            f.write("score,fppi,miss_rate\n")
            for s, x, y in zip(cv["score"].tolist(), cv["fppi"].tolist(), cv["miss_rate"].tolist()):
                f.write("%r,%r,%r\n" % (s, x, y))
        paths.append(path)
    return paths
