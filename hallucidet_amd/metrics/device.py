"""COCO mAP with its state on the GPU: the same surface and the same numbers as `metrics.MeanAveragePrecision`, with the matching and
the accumulation in HIP (csrc/coco_map.hip: hd_map_match / hd_map_accumulate).  Opt-in: `MeanAveragePrecision(...).to("cuda")`,
`Detection(device="cuda").map`, `--map-device cuda`.

update() keeps device tensors only and never waits for the GPU: detections arrive padded per batch (a `LazyDetections` hands over
its padded tensors through `padded()`; a list of dicts is padded here with shapes the host already knows), converted to the host
evaluator's types (fp64 boxes and scores, int64 labels).  compute() evaluates everything in two launches plus one stable sort, copies
the precision / recall arrays to the host and runs the host evaluator's own summary code on them, so every key comes out identical.
With `miss_rate=True` a third launch (hd_mr_accumulate) counts the log-average miss rate's integers from the same flags and order; the
float summary and the curves of miss_rate_curves() are again the host evaluator's code.

Ranks: when torch.distributed runs with more than one process, compute() gathers every rank's state (sizes first, then one padded
byte payload) and evaluates the union in rank order, so every rank returns the same global numbers; the result is then a
`GlobalResult` (is_global = True) and Trainer._nanmean_over_ranks passes its keys through instead of averaging them.
pack_state / unpack_state / merge_states are device-agnostic (the gloo tests run them on CPU tensors).
"""
import numpy as np
import torch

from .metrics import MeanAveragePrecision

# one evaluation state: padded detections and ground truths of N images (image i holds the first dc[i] / gc[i] rows)
FIELDS = (("db", torch.float64, "P", (4,)), ("ds", torch.float64, "P", ()), ("dl", torch.int64, "P", ()),
          ("gb", torch.float64, "Q", (4,)), ("gl", torch.int64, "Q", ()), ("dc", torch.int32, None, ()), ("gc", torch.int32, None, ()))


class GlobalResult(dict):
    """compute() output that already covers every rank."""
    is_global = True


def carry_global(src, dst):
    """`dst` (a filtered copy of the result `src`) as a GlobalResult when `src` is one."""
    return GlobalResult(dst) if getattr(src, "is_global", False) else dst


def _shape(f, N, P, Q):
    _, _, w, tail = f
    return (N,) + ((P if w == "P" else Q,) if w else ()) + tail


def empty_state(device, N=0, P=0, Q=0):
    return {f[0]: torch.zeros(_shape(f, N, P, Q), dtype=f[1], device=device) for f in FIELDS}


def state_sizes(st):
    return int(st["dc"].shape[0]), int(st["ds"].shape[1]), int(st["gl"].shape[1])


def _pad_width(t, width):
    """Pad dim 1 of t with zeros to `width`."""
    if t.shape[1] == width:
        return t
    out = torch.zeros((t.shape[0], width) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def merge_states(states):
    """Concatenate states in the order given (image order = list order), padding to the widest P / Q."""
    states = [s for s in states if s["dc"].shape[0] > 0] or states[:1]
    if len(states) == 1:
        return states[0]
    P = max(state_sizes(s)[1] for s in states)
    Q = max(state_sizes(s)[2] for s in states)
    out = {}
    for name, _, w, _ in FIELDS:
        parts = [s[name] if w is None else _pad_width(s[name], P if w == "P" else Q) for s in states]
        out[name] = torch.cat(parts)
    return out


def pack_state(st):
    """-> (sizes int64 [3] = (N, P, Q), payload uint8): every field's bytes, in FIELDS order (8-byte fields first)."""
    N, P, Q = state_sizes(st)
    sizes = torch.tensor([N, P, Q], dtype=torch.int64, device=st["dc"].device)
    payload = torch.cat([st[f[0]].contiguous().reshape(-1).view(torch.uint8) for f in FIELDS])
    return sizes, payload


def payload_bytes(N, P, Q):
    return sum(int(np.prod(_shape(f, N, P, Q))) * torch.empty((), dtype=f[1]).element_size() for f in FIELDS)


def unpack_state(sizes, payload):
    N, P, Q = (int(v) for v in sizes)
    out, o = {}, 0
    for f in FIELDS:
        shp = _shape(f, N, P, Q)
        nb = int(np.prod(shp)) * torch.empty((), dtype=f[1]).element_size()
        out[f[0]] = payload[o:o + nb].clone().view(f[1]).reshape(shp)
        o += nb
    return out


def gather_states(st, group=None):
    """All ranks' states in rank order: one all_gather of the sizes, one of the payloads padded to the largest.  The collectives run
    on the GPU under nccl and on the CPU under any other backend."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    comm = st["dc"].device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    sizes, payload = pack_state(st)
    sizes, payload = sizes.to(comm), payload.to(comm)
    all_sizes = [torch.zeros_like(sizes) for _ in range(world)]
    dist.all_gather(all_sizes, sizes, group=group)
    lens = [payload_bytes(*(int(v) for v in s.tolist())) for s in all_sizes]
    width = max(lens)
    buf = torch.zeros((width,), dtype=torch.uint8, device=comm)
    buf[:payload.numel()] = payload
    bufs = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(bufs, buf, group=group)
    return [{k: v.to(st["dc"].device) for k, v in unpack_state(s.tolist(), b[:n]).items()} for s, b, n in zip(all_sizes, bufs, lens)]


def _pinned(values, dtype, device):
    t = torch.tensor(values, dtype=dtype)
    return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t


def _pad_list(ts, tail, dtype, device):
    """Ragged per-image tensors -> ([n, W] + tail, counts [n] i32) on `device`, W = the largest count.  The counts come from the
    shapes (host metadata) and reach the GPU from pinned memory: no host sync."""
    rows = [t.reshape((-1,) + tail) for t in ts]
    counts = [r.shape[0] for r in rows]
    n, W = len(rows), max(counts, default=0)
    out = torch.zeros((n, W) + tail, dtype=dtype, device=device)
    total = sum(counts)
    if total:
        flat = torch.cat([r.to(device, dtype) for r in rows])
        starts = np.repeat(np.arange(n, dtype=np.int64) * W - np.concatenate([[0], np.cumsum(counts)[:-1]]), counts)
        idx = _pinned(starts + np.arange(total, dtype=np.int64), torch.int64, device)
        out.view((n * W,) + tail).index_copy_(0, idx, flat)
    return out, _pinned(counts, torch.int32, device)


def state_from_lists(preds, target, device):
    """A state from lists of per-image dicts (preds: boxes / scores / labels; target: boxes / labels); preds None -> targets only."""
    device = torch.device(device)
    st = {}
    if preds is not None:
        st["db"], st["dc"] = _pad_list([p["boxes"] for p in preds], (4,), torch.float64, device)
        st["ds"], _ = _pad_list([p["scores"] for p in preds], (), torch.float64, device)
        st["dl"], _ = _pad_list([p["labels"] for p in preds], (), torch.int64, device)
    st["gb"], st["gc"] = _pad_list([t["boxes"] for t in target], (4,), torch.float64, device)
    st["gl"], _ = _pad_list([t["labels"] for t in target], (), torch.int64, device)
    return st


class _Summary(MeanAveragePrecision):
    """The host evaluator's compute() over precomputed precision / recall arrays (and, with `mr`, the integer miss-rate arrays
    (hit, total, npig, n_img) of hd_mr_accumulate): the same class list, means, keys and dtypes."""

    def __init__(self, classes, precision, recall, class_metrics, mr=None):
        super().__init__(class_metrics=class_metrics, miss_rate=mr is not None)
        self._gts = [{"labels": np.asarray(classes, dtype=np.int64)}]      # compute() takes its class list from the labels seen
        self._pr, self._mr_in = (precision, recall), mr

    def _accumulate(self, classes):
        self._mr = self._mr_in
        return self._pr


class DeviceMeanAveragePrecision(MeanAveragePrecision):
    """`MeanAveragePrecision` whose state and evaluation live on `device` (a GPU)."""

    def __init__(self, box_format: str = "xyxy", class_metrics: bool = False, device="cuda", miss_rate: bool = False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DeviceMeanAveragePrecision runs on a GPU (got %s); the host evaluator is MeanAveragePrecision" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.is_global = False
        super().__init__(box_format=box_format, class_metrics=class_metrics, miss_rate=miss_rate)

    def to(self, device):
        d = torch.device(device)
        if d.type == "cuda" and (d.index is None or d == self.device):
            return self
        raise ValueError("DeviceMeanAveragePrecision cannot move to %s" % d)

    def reset(self):
        self._chunks = []
        self._mr = self._mr_curves = None

    # ------------------------------------------------------------------ update
    def update(self, preds, target):
        target = list(target)
        pad = preds.padded() if hasattr(preds, "padded") else None
        if pad is None:
            preds = list(preds)
        if len(preds) != len(target):
            raise ValueError("Expected argument `preds` and `target` to have the same length")
        if pad is None:
            for p in preds:
                for k in ("boxes", "scores", "labels"):
                    if k not in p:
                        raise ValueError(f"Expected all dicts in `preds` to contain the `{k}` key")
        for t in target:
            for k in ("boxes", "labels"):
                if k not in t:
                    raise ValueError(f"Expected all dicts in `target` to contain the `{k}` key")
        n = len(target)
        if pad is not None:
            b, s, l, c = pad
            P = s.shape[1] if s.dim() == 2 else 0
            # copies: the producer (a captured detector graph) reuses its buffers
            st = {"db": b.reshape(n, P, 4).to(self.device, torch.float64, copy=True),
                  "ds": s.reshape(n, P).to(self.device, torch.float64, copy=True),
                  "dl": l.reshape(n, P).to(self.device, torch.int64, copy=True),
                  "dc": c.reshape(n).to(self.device, torch.int32, copy=True)}
            st.update(state_from_lists(None, target, self.device))
        else:
            st = state_from_lists(preds, target, self.device)
        if n:
            self._chunks.append(st)
            self._mr = self._mr_curves = None

    def state(self):
        """This evaluator's images as one state (padded tensors on the device)."""
        return merge_states(self._chunks) if self._chunks else empty_state(self.device)

    def merge(self, *others):
        """Append the images of other evaluators (or states), in the order given, after this one's."""
        for o in others:
            st = o.state() if isinstance(o, DeviceMeanAveragePrecision) else o
            if st["dc"].shape[0]:
                self._chunks.append({k: v.to(self.device) for k, v in st.items()})
                self._mr = self._mr_curves = None
        return self

    # ------------------------------------------------------------------ evaluation
    def _evaluate(self, st):
        """-> (classes, precision [T,R,K,A,M], recall [T,K,A,M]) as the host's _accumulate returns them; with miss_rate it also leaves
        the host's integer miss-rate arrays in self._mr and the curve counts in self._mr_curves."""
        from .. import ops
        T, R, A, M = len(self.IOU_THRS), len(self.REC_THRS), len(self.AREA_RNG), len(self.MAX_DETS)
        assert (T, R, A, M) == (ops.MAP_NUM_IOU, ops.MAP_NUM_REC, ops.MAP_NUM_AREA, ops.MAP_NUM_MAXDET) and self.MAX_DETS == (1, 10, 100)
        N, P, Q = state_sizes(st)
        dev = self.device
        dmask = torch.arange(P, device=dev)[None, :] < st["dc"][:, None].long()
        gmask = torch.arange(Q, device=dev)[None, :] < st["gc"][:, None].long()
        if bool(torch.isnan(st["ds"][dmask]).any()):
            raise ValueError("DeviceMeanAveragePrecision: NaN detection scores")
        classes = torch.unique(torch.cat([st["dl"][dmask], st["gl"][gmask]]), sorted=True)
        K = int(classes.numel())
        if K == 0:
            if self.miss_rate:
                self._mr = (-np.ones((T, 0, A, len(self.REF_FPPI)), dtype=np.int32), -np.ones((T, 0, A, 2), dtype=np.int32),
                            np.zeros((0, A), dtype=np.int32), N)
                self._mr_curves = (N, {})
            return [], -np.ones((T, R, 0, A, M)), -np.ones((T, 0, A, M))
        f64 = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), device=dev)
        iou_start = f64([min(t, 1 - 1e-10) for t in self.IOU_THRS])
        area_rng = f64(list(self.AREA_RNG.values()))
        flags, score, ndet, npos, evald, status = ops.map_match(st["db"].contiguous(), st["ds"].contiguous(), st["dl"].contiguous(),
                                                                st["dc"].contiguous(), st["gb"].contiguous(), st["gl"].contiguous(),
                                                                st["gc"].contiguous(), classes, iou_start, area_rng)
        over_d, over_g, bad = status.tolist()
        if over_d:
            raise ValueError("DeviceMeanAveragePrecision: an image has %d detections of one class; the per-image cap is %d (HD_MAP_DET_CAP)"
                             % (over_d, ops.MAP_DET_CAP))
        if over_g:
            raise ValueError("DeviceMeanAveragePrecision: an image has %d ground truths of one class; the per-image cap is %d (HD_MAP_GT_CAP)"
                             % (over_g, ops.MAP_GT_CAP))
        if bad:
            raise ValueError("DeviceMeanAveragePrecision: a detection / ground-truth count lies outside its padded width")
        MD = ops.MAP_MAX_DET
        # the host's global order: per class, descending score, ties in image order then rank (its stable sort of the per-image lists)
        idx = (torch.arange(MD, device=dev)[None, :] < ndet[:, None]).reshape(-1).nonzero().squeeze(1)
        key = score[idx].neg() + 0.0                      # + 0.0: -0.0 and 0.0 tie, as they do in numpy
        idx = idx[torch.sort(key, stable=True).indices]
        cls_of = (idx // MD) % K
        idx = idx[torch.sort(cls_of, stable=True).indices]
        class_off = torch.zeros((K + 1,), dtype=torch.int64, device=dev)
        class_off[1:] = torch.cumsum(torch.bincount(cls_of, minlength=K), 0)
        npig = npos.view(N, K, A).sum(0, dtype=torch.int64).to(torch.int32)
        n_eval = evald.view(N, K).sum(0, dtype=torch.int64).to(torch.int32)
        order, class_off = idx.to(torch.int32), class_off.to(torch.int32)
        precision, recall = ops.map_accumulate(order, class_off, flags, npig, n_eval, f64(self.REC_THRS))
        if self.miss_rate:
            # the same flags and the same order at max-dets 100; the integers go through the host's own summary code
            hit, total, (ctp, cfp) = ops.mr_accumulate(order, class_off, flags, npig, n_eval, N, f64(self.REF_FPPI), curve_t=0)
            npig_h, labels = npig.cpu().numpy(), classes.tolist()
            self._mr = (hit.cpu().numpy(), total.cpu().numpy(), npig_h, N)
            sc = score[idx]

            def curves():                                   # the per-detection arrays leave the GPU only when the curves are asked for
                s, tp, fp, off, n_ev = sc.cpu().numpy(), ctp.cpu().numpy(), cfp.cpu().numpy(), class_off.tolist(), n_eval.tolist()
                return N, {c: (s[off[k]:off[k + 1]], tp[off[k]:off[k + 1]], fp[off[k]:off[k + 1]], int(npig_h[k, 0]))
                           for k, c in enumerate(labels) if n_ev[k] and npig_h[k, 0] > 0}
            self._mr_curves = curves
        return classes.tolist(), precision.cpu().numpy(), recall.cpu().numpy()

    def miss_rate_curves(self):
        """As the host evaluator's, from hd_mr_accumulate's cumulative counts and the scores in the global order.  Under
        torch.distributed the curves cover the whole split; call compute() first (on every rank: it gathers), then this on any rank."""
        if not self.miss_rate:
            raise ValueError("miss_rate_curves() needs an evaluator built with miss_rate=True")
        if self._mr_curves is None:
            self.compute()
        if callable(self._mr_curves):
            self._mr_curves = self._mr_curves()
        return super().miss_rate_curves()

    def compute(self):
        from ..distributed import is_dist
        st = self.state()
        glob = is_dist()
        with torch.cuda.device(self.device):
            if glob:
                st = merge_states(gather_states(st))
            classes, precision, recall = self._evaluate(st)
        self._mr_classes = list(classes)
        out = _Summary(classes, precision, recall, self.class_metrics, mr=self._mr if self.miss_rate else None).compute()
        self.is_global = glob
        return GlobalResult(out) if glob else out
