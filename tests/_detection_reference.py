"""CPU definitions of the selection kernels of csrc/detection.hip (per-level top-k, box decoding and filtering, greedy NMS in three forms,
target matching, the positive/negative sampler, the RoI sampling tail, RoI post-processing, the FPN level mapper), the input builders that
put every shape on a loop edge of its kernel, and the checks both test files apply.  numpy and torch on the CPU only; nothing from
hallucidet_amd is imported here.  Shared by test_detection_reference_cpu.py (the definitions against a second statement of each
operation; mutants of the definitions must be rejected by the case tables) and test_detection_kernels_gpu.py (the HIP kernels against
the definitions).

Three kinds of reference.
  1. Exact definitions of every index, flag, count and label: stable descending sort, torchvision's Matcher with its low-quality rule, the
     k smallest keys (lowest index at the cut), greedy NMS, ascending-index compaction.  Compared with torch.equal.
  2. fp32 emulation in the kernel's operation order.  detection.hip is compiled with `fp contract(off)`, so a chain of + - * / is the
     same chain of correctly rounded IEEE operations that numpy.float32 performs: IoU values, the dx/dy regression targets
     wx*(gcx - ecx)/ew, the decode centres dx*w + cx, the clamped dw/dh and the clamp of the corners are reproduced bit for bit.
  3. float64 of the identical fp32 argument, with a derived tolerance, only where expf / logf enters (softmax scores, the sigmoid, decoded
     corners through exp(dw)*w, the log targets).

The per-call bound of the device expf / logf.  The ROCm installation ships no accuracy table for the device library's expf / logf (no
document under its share/ directory states one), so the bound is MEASURED: test_detection_kernels_gpu.py::test_device_expf_logf reads
both functions through kernels of this file where they are the only inexact step -- hd_roi_decode_clip on the box [-0.5, -0.5, 0.5,
0.5] with unit weights returns z = 0 + 0.5*(expf(c)*1), and hd_roi_samples_finish on the proposal [0, 0, 1, 1] with unit weights
returns 1*logf(gw/1) -- over 2^20 arguments each (expf: uniform in [-20, 12], the range of logit differences, -objectness and clamped
dw; logf: log-uniform in [2^-20, 2^20] plus 2^16 arguments within 2^-8 of 1) and compares with float64 exp / log of the identical fp32
argument, in units of the fp32 spacing at the true value.  Measured on an MI355X (gfx950, ROCm 7.0):
    expf  worst 0.8347 ulp      logf  worst 1.8772 ulp
Twice the worst case, rounded up, and never less than 1 ulp:
    EXPF_ULPS = 1.67,  LOGF_ULPS = 3.76
The test asserts the measured worst case against these bounds on every run and prints it.
log2f enters hd_roi_levels only under a floor: there the expected level is the float64 one and a random box may be left out if its
float64 pre-floor value lies within LEVEL_MARGIN = 1e-4 of an integer (at most 1 % of them, asserted on the CPU); designed boxes are never
left out.

Propagation (u = 2^-24, the relative error of one correctly rounded fp32 operation; ulp(v) = the fp32 spacing at |v|):
  log targets    t = ww*logf(r), r the emulated fp32 ratio:  |ww|*LOGF_ULPS*ulp(log r) + u*|t|
  decoded corner pc -/+ 0.5*(expf(dw)*w), pc and dw emulated:  0.5*(EXPF_ULPS*ulp(e^dw)*|w| + u*|pw|) + u*|corner|  -- scales with pw.
                 A corner whose unclamped reference lies further than that outside [0, L] must be exactly 0 or L (tolerance 0).
  sigmoid        p = 1/(1 + expf(-x)):  p*(EXPF_ULPS*2^-23*e/(1 + e) + 2u)
  softmax        p_k = e_k / sum_c e_c, C terms added serially, the differences l_c - max emulated:  p*(2*EXPF_ULPS*2^-23 + C*u) + 2^-126
                 -- scales with C.
Boolean outputs that depend on a float the kernel also returns (`valid` of hd_rpn_decode_filter and hd_roi_postprocess) are not
re-derived from float64: the flag must equal the kernel's stated test applied in fp32 to the kernel's own returned boxes and scores
(RPN: both sides >= min_size and prob >= score_thresh; RoI post-processing: score > score_thresh and both sides >= min_size), and
separately the boxes and scores must be within tolerance.  The designed rows state their flag by hand as well.

Out of scope: a NaN IoU needs a valid GT box of zero area (0/0).  The loader rejects those upstream (models/detection.py: pad_targets,
the `x2 > x1` note), so no case feeds one and ref_match does not define the result.
"""
import math

import numpy as np
import torch

F = np.float32
U = 2.0 ** -24
EXPF_ULPS = 1.67
LOGF_ULPS = 3.76
XCLIP = math.log(1000.0 / 16)
LEVEL_MARGIN = 1e-4
INT32_MAX = 0x7FFFFFFF


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def ulp(v):
    """fp32 spacing at |v| (float64 array)."""
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def close_ratio(got, ref, tol):
    """max |got - ref| / tol over the finite reference entries (tol 0: must be equal); inf when the NaN / +-inf pattern differs."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    nan, fin = np.isnan(ref), np.isfinite(ref)
    inf = ~nan & ~fin
    if not np.array_equal(np.isnan(got), nan) or not np.array_equal(got[inf], ref[inf]) or not np.isfinite(got[fin]).all():
        return math.inf
    err, t = np.abs(got[fin] - ref[fin]), tol[fin]
    if (err[t == 0] != 0).any():
        return math.inf
    return float((err[t > 0] / t[t > 0]).max()) if (t > 0).any() else 0.0


def bits_equal(got, ref):
    """fp32 arrays equal bit for bit; a NaN matches any NaN (hosts and devices differ in the payload an invalid operation returns)."""
    got, ref = f32(got), f32(ref)
    if got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]))


# ------------------------------------------------------------------------------------------------------------------ top-k
def order_keys(row):
    """The kernel's order_key(): a uint32 whose unsigned order is the order of the floats, -0.0 and +0.0 equal, every NaN the largest."""
    x = f32(row).copy()
    x[x == 0] = 0.0
    u = x.view(np.uint32)
    k = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    k[np.isnan(x)] = 0xFFFFFFFF
    return k


def ref_topk(row, k, mutant=None):
    """Indices of the k largest entries in descending order, equal entries by ascending index (NaN the largest, as torch.sort has it).
    mutants: 'neg_zero_less' (-0.0 < +0.0), 'tie_high' (highest index first among equals), 'nan_bits' (a NaN ordered by its bits)."""
    x = f32(row)
    n = x.shape[0]
    if mutant is None:
        return torch.sort(torch.from_numpy(x), descending=True, stable=True)[1][:min(k, n)]
    key = order_keys(x).astype(np.int64)
    if mutant in ("neg_zero_less", "nan_bits"):
        y = x.copy()
        if mutant == "nan_bits":
            y[y == 0] = 0.0
        u = y.view(np.uint32)
        raw = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.int64)
        key = raw if mutant == "nan_bits" else np.where(np.isnan(x), key, raw)
    idx = np.arange(n)
    order = np.lexsort((-idx if mutant == "tie_high" else idx, -key))
    return torch.from_numpy(order[:min(k, n)].astype(np.int64))


def ref_topk_segments(scores, segs, k, mutant=None):
    """scores [B, sum(segs)] -> [B, sum(min(k, n))] as ops.topk_rows_segments lists them."""
    rows = []
    for b in range(scores.shape[0]):
        off, out = 0, []
        for n in segs:
            out.append(ref_topk(scores[b, off:off + n], k, mutant) + off)
            off += n
        rows.append(torch.cat(out))
    return torch.stack(rows)


TOPK_ROWS = ("equal", "quant4", "low_byte", "high_byte", "zeros", "neg_inf", "pos_inf", "normal")


def topk_row(kind, n, seed):
    r = np.random.RandomState(seed)
    if kind == "equal":
        return np.full(n, 0.5, np.float32)
    if kind == "quant4":                                   # four values: ties at the cut in every radix digit
        return (r.randint(0, 4, n) / 4.0 - 0.25).astype(np.float32)
    if kind == "low_byte":                                 # keys differ in their lowest byte only
        return (np.uint32(0x3F800000) + r.randint(0, 256, n).astype(np.uint32)).view(np.float32)
    if kind == "high_byte":                                # ... in their highest byte only (sign and seven exponent bits; all finite)
        return ((r.randint(0, 256, n).astype(np.uint32) << 24) | np.uint32(0x00123456)).view(np.float32)
    if kind == "zeros":
        return np.array([0.0, -0.0, 1.0, -1.0], np.float32)[r.randint(0, 4, n) if n > 2 else np.arange(n)[::-1] % 2]
    x = r.randn(n).astype(np.float32)
    if kind == "neg_inf":
        x[::3] = -np.inf
    elif kind == "pos_inf":
        x[r.rand(n) < 0.2] = np.inf
        x[r.rand(n) < 0.1] = -np.inf
    elif kind == "nan":                                    # both signs, two payloads, among +-inf, +-0 and ordinary values
        pay = np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC12345, 0x7F800001], np.uint32).view(np.float32)
        m = r.rand(n) < 0.3
        x[m] = pay[r.randint(0, 5, int(m.sum()))]
        x[r.rand(n) < 0.05] = np.inf
        x[r.rand(n) < 0.05] = -0.0
        if n <= 2:
            x[:] = pay[[1, 0][:n]]
    return x


TOPK_N = (1, 2, 1023, 1024, 1025, 2049)


def topk_cases(nan):
    """(name, scores [B, sum(segs)], segs, k).  nan=False: one row per TOPK_ROWS kind; nan=True: three NaN rows."""
    kinds = ("nan", "nan", "nan") if nan else TOPK_ROWS
    def table(segs, seed):
        return np.stack([np.concatenate([topk_row(kd, n, seed + 10 * i + j) for j, n in enumerate(segs)]) for i, kd in enumerate(kinds)])
    out = []
    for n in TOPK_N:
        for k in sorted({1, n - 1, n, n + 5} - {0}):       # n + 5 is clamped to n
            out.append(("n%d-k%d" % (n, k), table([n], n), [n], k))
    out.append(("n2049-k1024", table([2049], 5), [2049], 1024))                   # P == k
    out.append(("n4097-k4096", table([4097], 6), [4097], 4096))                   # the LDS capacity
    out.append(("segs-1-1025-70-k64", table([1, 1025, 70], 7)[:3], [1, 1025, 70], 64))      # three segments, B = 3
    out.append(("segs-1-1025-70-k1030", table([1, 1025, 70], 8)[:3], [1, 1025, 70], 1030))
    return out


# ------------------------------------------------------------------------------------------------------------------ sampler
def ref_sample(labels, keys, batch_size, cap_pos, mutant=None):
    """labels [N, A] int64 (>= 1 positive, 0 negative, < 0 ignored), keys [N, A] int32 >= 0 -> pos_sel, neg_sel [N, A] bool and
    counts [N, 2] int64.  Per class: a stable argsort of the members' keys, the first k taken.  mutant 'tie_high': the highest
    index wins among equal keys; 'cap_off': one positive more than the cap."""
    labels, keys = np.asarray(labels), np.asarray(keys)
    N, A = labels.shape
    pos, neg, counts = np.zeros((N, A), bool), np.zeros((N, A), bool), np.zeros((N, 2), np.int64)
    for n in range(N):
        ip, ine = np.nonzero(labels[n] >= 1)[0], np.nonzero(labels[n] == 0)[0]
        num_pos = min(len(ip), cap_pos + (1 if mutant == "cap_off" else 0))
        num_neg = min(len(ine), batch_size - num_pos)
        for members, k, out in ((ip, num_pos, pos), (ine, num_neg, neg)):
            kk = keys[n, members].astype(np.int64)
            o = np.lexsort((-members, kk)) if mutant == "tie_high" else np.argsort(kk, kind="stable")
            out[n, members[o[:k]]] = True
        counts[n] = (num_pos, num_neg)
    return torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(counts)


SAMPLE_A = (1, 1023, 1024, 1025, 3000, 30721)              # 30721: the first size past the LDS staging (sample_lds_limit)
SAMPLE_KEYS = ("uniform", "eight", "equal", "extremes")
SAMPLE_GROUPS = ("cap", "sparse", "full")


def sample_lds_limit():
    """The largest A whose keys and classes hd_sample_pos_neg stages in LDS: need = 4*A + roundup4(A) <= 150 KiB."""
    a = 0
    while 4 * (a + 1) + ((a + 1 + 3) & ~3) <= 150 * 1024:
        a += 1
    return a


def sample_case(A, group, keykind, seed):
    """-> dict labels [3, A], keys [3, A], batch_size, cap_pos, rows (what each row is).
    'cap':    P == cap_pos, cap_pos + 1, cap_pos - 1 (the rest negatives and ignored)
    'sparse': no positives / nothing to sample / fewer candidates than the batch
    'full':   cap_pos == batch_size with more positives than that (num_neg = 0: the k <= 0 branch) / exactly batch_size - 1 / random"""
    r = np.random.RandomState(seed)
    batch = 64 if A >= 1023 else 4
    cap = batch if group == "full" else batch // 2
    labels = np.full((3, A), -1, np.int64)

    def fill(row, npos, nneg):
        npos, nneg = min(npos, A), min(nneg, A - min(npos, A))
        p = r.permutation(A)
        labels[row, p[:npos]] = r.randint(1, 6, npos)
        labels[row, p[npos:npos + nneg]] = 0

    if group == "cap":
        rows = ("P==cap", "P==cap+1", "P==cap-1")
        for i, P in enumerate((cap, cap + 1, cap - 1)):
            fill(i, P, (A - P) * 2 // 3)
    elif group == "sparse":
        rows = ("no positives", "nothing to sample", "fewer candidates than the batch")
        fill(0, 0, A * 2 // 3)
        fill(2, batch // 4, batch // 4)
    else:
        rows = ("P>batch, num_neg=0", "P==batch-1", "random")
        fill(0, batch + 7, A // 2)
        fill(1, batch - 1, A // 2)
        labels[2] = r.randint(-1, 6, A)
    if keykind == "uniform":
        keys = r.randint(0, 1 << 31, (3, A), dtype=np.int64)
    elif keykind == "eight":                               # ties at the cut: the lowest index wins
        keys = np.array([0, 1, 255, 256, 65536, 1 << 24, (1 << 24) + 1, INT32_MAX], np.int64)[r.randint(0, 8, (3, A))]
    elif keykind == "equal":
        keys = np.full((3, A), 12345, np.int64)
    else:                                                  # one member of each class at key 0 and one at 0x7FFFFFFF
        keys = r.randint(1, INT32_MAX, (3, A), dtype=np.int64)
        for n in range(3):
            for members in (np.nonzero(labels[n] >= 1)[0], np.nonzero(labels[n] == 0)[0]):
                if len(members) >= 2:
                    a, b = r.choice(members, 2, replace=False)
                    keys[n, a], keys[n, b] = 0, INT32_MAX
    return {"labels": torch.from_numpy(labels), "keys": torch.from_numpy(keys.astype(np.int32)), "batch_size": batch, "cap_pos": cap, "rows": rows}


# ------------------------------------------------------------------------------------------------------------------ IoU, encode, matcher
def emu_iou(gt, boxes):
    """gt [G, 4], boxes [A, 4] fp32 -> [G, A] fp32 in box_iou_dev's operation order."""
    a, b = f32(gt)[:, None, :], f32(boxes)[None, :, :]
    with np.errstate(all="ignore"):
        area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        w = np.maximum(F(0), np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]))
        h = np.maximum(F(0), np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]))
        inter = w * h
        return inter / (area_a + area_b - inter)


def emu_encode(ref, prop, weights):
    """BoxCoder.encode_single in the kernels' order.  ref, prop [..., 4] fp32 -> dict: xy [..., 2] fp32 (bit-exact dx, dy),
    wh [..., 2] float64 (ww*log(r) of the emulated fp32 ratio r) and wh_tol."""
    ref, prop = f32(ref), f32(prop)
    wx, wy, ww, wh = (F(v) for v in weights)
    with np.errstate(all="ignore"):
        ew, eh = prop[..., 2] - prop[..., 0], prop[..., 3] - prop[..., 1]
        ecx, ecy = prop[..., 0] + F(0.5) * ew, prop[..., 1] + F(0.5) * eh
        gw, gh = ref[..., 2] - ref[..., 0], ref[..., 3] - ref[..., 1]
        gcx, gcy = ref[..., 0] + F(0.5) * gw, ref[..., 1] + F(0.5) * gh
        xy = np.stack([wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh], -1)
        lg = np.log(np.stack([gw / ew, gh / eh], -1).astype(np.float64))
        wgt = np.array([float(ww), float(wh)])
        t = wgt * lg
        tol = np.abs(wgt) * LOGF_ULPS * ulp(lg) + U * np.abs(t)
    assert xy.dtype == np.float32
    return {"xy": xy, "wh": t, "wh_tol": tol}


def check_encode(got, enc, exact_rows=None):
    """got [..., 4] fp32 against emu_encode's dict -> (dx/dy bit-identical on exact_rows (default: everywhere), dw/dh ratio);
    the NaN / inf pattern must agree everywhere."""
    got = f32(got)
    m = np.ones(got.shape[:-1], bool) if exact_rows is None else np.asarray(exact_rows, bool)
    pattern = np.array_equal(np.isfinite(got[..., :2]), np.isfinite(enc["xy"])) and np.array_equal(np.isnan(got[..., :2]), np.isnan(enc["xy"]))
    return bool(pattern and bits_equal(got[..., :2][m], enc["xy"][m])), close_ratio(got[..., 2:], enc["wh"], enc["wh_tol"])


def ref_match(gt, gvalid, glabels, boxes, high, low, allow_low_quality, weights=None, mutant=None):
    """hd_match_targets: gt [N, G, 4], gvalid [N, G] bool, glabels [N, G] int64 or None, boxes [A, 4] (shared) or [N, A, 4].
    -> dict matched [N, A] int64 (-1 below `low`, -2 between), labels [N, A] int64, enc (emu_encode of the matched GT row, row 0 for
    unmatched boxes: matched.clamp(min=0)), has_gt [N].
    mutants: 'last_max' (last maximal GT), 'lq_gt_index' (a low-quality match takes the index of the GT whose best it is),
    'low_le' / 'high_le' (<= at the threshold), 'by_zeros' (GT rows judged by their coordinates instead of gvalid)."""
    gt, gv = f32(gt), np.asarray(gvalid, bool)
    N, G, _ = gt.shape
    bx = f32(boxes)
    if bx.ndim == 2:
        bx = np.broadcast_to(bx, (N,) + bx.shape)
    A = bx.shape[1]
    if mutant == "by_zeros":
        gv = gt[:, :, 2] > gt[:, :, 0]
    matched, labels = np.zeros((N, A), np.int64), np.zeros((N, A), np.int64)
    lo, hi = F(low), F(high)
    for n in range(N):
        iou = np.where(gv[n][:, None], emu_iou(gt[n], bx[n]), F(-1))
        vals = iou.max(0)
        idx = iou.argmax(0) if mutant != "last_max" else G - 1 - iou[::-1].argmax(0)
        m = idx.astype(np.int64).copy()
        below = vals <= lo if mutant == "low_le" else vals < lo
        between = ~below & (vals <= hi if mutant == "high_le" else vals < hi)
        m[below], m[between] = -1, -2
        if allow_low_quality:
            best = iou.max(1)
            hit = (iou == best[:, None]) & gv[n][:, None]
            if mutant == "lq_gt_index":
                for g in range(G):
                    m[hit[g]] = g
            else:
                m = np.where(hit.any(0), idx, m)
        matched[n] = m
        lab = np.where(m >= 0, (np.asarray(glabels)[n][np.maximum(m, 0)] if glabels is not None else 1), np.where(m == -1, 0, -1))
        labels[n] = lab if gv[n].any() else 0
    out = {"matched": torch.from_numpy(matched), "labels": torch.from_numpy(labels), "has_gt": gv.any(1)}
    if weights is not None:
        ref = np.take_along_axis(gt, np.maximum(matched, 0)[:, :, None], 1)
        out["enc"] = emu_encode(ref, bx, weights)
    return out


MATCH_G = (1, 64, 65, 300)
MATCH_A = (1, 255, 256, 257, 1025)
MATCH_THRESHOLDS = ((0.7, 0.3, True), (0.5, 0.5, False))           # (high, low, allow_low_quality): the RPN's and the RoI heads'
_DESIGNED_BOXES = np.array([
    [0, 0, 2, 1],        # IoU 1/2 with GT A exactly (= low = high of the RoI heads)
    [0, 0, 10, 1],       # IoU 7/10 with GT B = fl(0.7) exactly (= high of the RPN): matched, not "between"
    [0, 0, 10, 1],       # (the same box again)
    [20, 20, 30, 21],    # IoU 3/10 with GT C = fl(0.3) exactly (= low of the RPN): "between", not "below"
    [40, 40, 42, 44],    # the two best boxes of GT D, both IoU 1/2: both get the low-quality match
    [40, 40, 44, 42],
    [5, 5, 5, 9],        # zero-area proposal: IoU 0 with everything
    [0, 0, 1, 1],        # equals GT A: IoU 1
    [0, 0, 7, 1],        # equals GT B, so the 7/10 boxes are not B's best (the low-quality rule would hide a wrong `< high`)
    [20, 20, 23, 21],    # equals GT C, likewise for `< low`
    [30, 30, 40, 42],    # the best box of GT E (IoU 1/19) whose own arg-max is GT F (IoU 5/6): the low-quality match goes to F
], np.float32)
#                          A             B             C                 D                 F                 E
_DESIGNED_GT = np.array([[0, 0, 1, 1], [0, 0, 7, 1], [20, 20, 23, 21], [40, 40, 42, 42], [30, 30, 40, 40], [30, 41, 40, 49]], np.float32)


def match_case(G, A, shared, seed):
    """N = 3.  Image 0: the designed GT boxes (as far as G allows) then random ones; for G >= 64 a duplicated GT (rows 7 and 8, and row 64:
    across the staging loop's 64-row trip) and invalid rows in the middle (6, 60) that hold the stale coordinates of a valid one.
    Image 1: no valid GT, every row stale.  Image 2: random, every row valid.  The designed proposals come first (as far as A allows);
    everything random lies at coordinates >= 50, clear of the designed boxes; the tail of the proposal list repeats GT boxes (IoU 1)."""
    r = np.random.RandomState(seed)
    N = 3
    xy = np.floor(r.rand(N, G, 2) * 180) + 50
    gt = np.concatenate([xy, xy + 4 + np.floor(r.rand(N, G, 2) * 90)], 2).astype(np.float32)
    k = min(G, len(_DESIGNED_GT))
    gt[0, :k] = _DESIGNED_GT[:k]
    gvalid = np.ones((N, G), bool)
    if G >= 64:
        gt[0, 8] = gt[0, 7]                                # duplicate: the first index wins
        gvalid[0, 6] = gvalid[0, 60] = False               # stale rows in the middle of the list
        gt[0, 6] = gt[0, 9]                                # ... holding the coordinates of a valid one
    if G >= 65:
        gt[0, 64] = gt[0, 7]
    gvalid[1] = False
    bxy = r.rand(N, A, 2) * 230 + 50
    boxes = np.concatenate([bxy, bxy + 3 + r.rand(N, A, 2) * 100], 2).astype(np.float32)
    na = min(max(0, A - 1), G * 2) if G > k else 0
    for n in range(N):
        if na:
            boxes[n, A - na:] = gt[n, r.randint(k, G, na)]
    d = min(A, len(_DESIGNED_BOXES))
    boxes[:, :d] = _DESIGNED_BOXES[:d]
    if G >= 64 and A >= d + 2:
        boxes[0, d], boxes[0, d + 1] = gt[0, 9], gt[0, 7]  # the box of the stale row's original, and of the duplicated GT
    glabels = r.randint(1, 6, (N, G)).astype(np.int64)
    return {"gt": torch.from_numpy(gt), "gvalid": torch.from_numpy(gvalid), "glabels": torch.from_numpy(glabels),
            "boxes": torch.from_numpy(boxes[0].copy() if shared else boxes)}


# ------------------------------------------------------------------------------------------------------------------ NMS
def ref_nms_sorted(boxes, thr):
    """Greedy NMS over boxes in descending score order, scalar fp32 IoU in box_iou_dev's order -> keep [n] bool."""
    b = f32(boxes)
    n = b.shape[0]
    areas = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead, keep = np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            if dead[i]:
                continue
            keep[i] = True
            w = np.maximum(F(0), np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]))
            h = np.maximum(F(0), np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]))
            inter = w * h
            dead[i + 1:] |= inter / (areas[i] + areas[i + 1:] - inter) > F(thr)
    return keep


def early_stop(keep, max_keep):
    """hd_nms_sorted_batched_topk's flags: the full scan's up to the end of the 64-box chunk in which the max_keep-th survivor falls,
    nothing kept after it."""
    keep = np.asarray(keep, bool).copy()
    s = np.nonzero(keep)[0]
    if len(s) >= max_keep:
        keep[(s[max_keep - 1] // 64 + 1) * 64:] = False
    return keep


def clustered_boxes(n, seed, span=400.0):
    """n boxes around n/24 centres, in random order: a kept box suppresses members of its cluster many 64-box chunks later."""
    r = np.random.RandomState(seed)
    c = max(1, n // 24)
    cen, size = r.rand(c, 2) * span, 8 + r.rand(c, 2) * 40
    which = r.randint(0, c, n)
    xy = cen[which] + r.randn(n, 2) * 2.0
    wh = size[which] * (1 + 0.1 * r.randn(n, 2))
    return np.concatenate([xy, xy + np.abs(wh) + 1], 1).astype(np.float32)


def nms_big_boxes(n, seed):
    """clustered_boxes plus planted pairs away from every cluster: box 0 (always kept) and a near copy of it as the LAST box, so that its
    only suppressor lies (n-1)/64 chunks before it -- the last word of the first 64-word group at n = 4160, the first word of the second
    group at n = 4161, of the third at n = 8300; for n > 5000 also box 1 and box 5000 (a word in the middle of the second group).
    Boxes 2 and 3 overlap at IoU 1/2 exactly."""
    b = clustered_boxes(n, seed)
    if n >= 2:
        b[0], b[n - 1] = (1000, 1000, 1050, 1050), (1001, 1001, 1050, 1050)
    if n > 5001:
        b[1], b[5000] = (2000, 2000, 2050, 2050), (2000, 2001, 2050, 2050)
    if n >= 4:
        b[2], b[3] = (3000, 3000, 3010, 3001), (3000, 3000, 3005, 3001)       # IoU == 0.5 exactly: kept at threshold 0.5 (strict >)
    return b


def stable_desc_order(key):
    return torch.sort(torch.from_numpy(f32(key)), descending=True, stable=True)[1].numpy()


def ref_nms_pick(boxes, scores, idxs, valid, thr, top_n, mutant=None):
    """One row of torchvision's batched_nms as hd_batched_nms_pick / hd_batched_nms_pick_segments return it: shift the boxes of
    category c by c*(largest valid coordinate + 1) in fp32, stable sort by descending score (invalid last), greedy scan, the first
    top_n survivors as candidate indices -> (pick [min(top_n, n)] int64, padded with order[0]; count).
    mutants: 'shift_per_category' (the largest coordinate of the category instead of the row), 'unstable_merge' (equal scores: the
    higher category first), 'tie_high' (equal scores: the higher index first), 'iou_ge' (>= at the threshold), 'carry_dropped' (the
    segment form's compaction of a segment's valid candidates, 256 per round, restarts its rank every round: the candidates of a later
    round take the places of the segment's first ones, which are lost)."""
    boxes, scores, idxs, valid = f32(boxes), f32(scores), np.asarray(idxs, np.int64), np.asarray(valid, bool)
    n = boxes.shape[0]
    if mutant == "carry_dropped" and not (np.diff(idxs) < 0).any():          # (categories that are segments of the list)
        valid = valid.copy()
        for c in np.unique(idxs):
            lo, hi = np.nonzero(idxs == c)[0][[0, -1]]
            slots = {}
            for c0 in range(lo, hi + 1, 256):
                for r, i in enumerate(np.nonzero(valid[c0:min(c0 + 256, hi + 1)])[0]):
                    slots[r] = c0 + i
            valid[lo:hi + 1] = False
            valid[list(slots.values())] = True
    key = np.where(valid, scores, F(-np.inf))
    order = stable_desc_order(key)
    if mutant in ("unstable_merge", "tie_high"):
        order = np.lexsort((-np.arange(n) if mutant == "tie_high" else np.arange(n), -idxs if mutant == "unstable_merge" else 0 * idxs,
                            -order_keys(key).astype(np.int64)))
    cnt = int(valid.sum())
    bmax = boxes[valid].max() if cnt else F(0)
    scale = np.full(n, bmax + F(1), np.float32)
    if mutant == "shift_per_category":
        for c in np.unique(idxs[valid]):
            scale[idxs == c] = boxes[valid & (idxs == c)].max() + F(1)
    shifted = boxes + (idxs.astype(np.float32) * scale)[:, None]
    srt = shifted[order[:cnt]]
    if mutant == "iou_ge":
        keep = ref_nms_sorted(srt, np.nextafter(F(thr), F(-1)))
    else:
        keep = ref_nms_sorted(srt, thr)
    surv = order[:cnt][keep][:top_n]
    pick = np.full(min(top_n, n), order[0], np.int64)
    pick[:len(surv)] = surv
    return pick, len(surv)


def ref_nms_pick_rows(boxes, scores, idxs, valid, thr, top_n, mutant=None):
    rows = [ref_nms_pick(boxes[b], scores[b], idxs[b], valid[b], thr, top_n, mutant) for b in range(boxes.shape[0])]
    return torch.from_numpy(np.stack([p for p, _ in rows])), torch.tensor([c for _, c in rows], dtype=torch.int64)


def _shift_trap(boxes, scores, idxs, valid):
    """Two candidates that tell a per-category shift from the per-row one: category 0 holds [11, 11, 21, 21] (the row's best score) and
    the row's largest coordinate; category 1's only box is [0, 0, 10, 10] (the second best score) -- shifted by its own maximum + 1 =
    11 it would land on the first and be suppressed."""
    boxes[0], boxes[1] = (11, 11, 21, 21), (0, 0, 10, 10)
    scores[0], scores[1] = 2.0, 1.5
    idxs[0], idxs[1] = 0, 1
    valid[0] = valid[1] = True


_AT_THRESHOLD = np.array([[300, 300, 310, 301], [300, 300, 307, 301],        # IoU 7/10 = fl(0.7): not suppressed at 0.7 (strict >)
                          [300, 310, 310, 311], [300, 310, 303, 311]], np.float32)      # IoU 3/10 = fl(0.3)


def nms_pick_case(n, seed):
    """B = 3 rows of n candidates in 4 categories: quantised scores (ties), ~80 % valid, row 1 with nothing valid, row 2 the shift trap
    (category 1 emptied but for the trap's box), row 0 two pairs of category 0 whose IoU equals the threshold 0.7 / 0.3 exactly."""
    r = np.random.RandomState(seed)
    B = 3
    boxes = np.stack([clustered_boxes(n, seed + b, 200.0) for b in range(B)])
    scores = (np.round(r.rand(B, n) * 16) / 16).astype(np.float32)
    idxs = r.randint(0, 4, (B, n)).astype(np.int64)
    valid = r.rand(B, n) < 0.8
    valid[1] = False
    if n >= 2:
        idxs[2][idxs[2] == 1] = 2
        _shift_trap(boxes[2], scores[2], idxs[2], valid[2])
    if n >= 8:                                             # category 0 is not shifted: the designed IoUs survive
        boxes[0, 2:6], scores[0, 2:6], idxs[0, 2:6], valid[0, 2:6] = _AT_THRESHOLD, (1.25, 1.2, 1.15, 1.1), 0, True
    return {"boxes": boxes, "scores": scores, "idxs": idxs, "valid": valid}


NMS_SEGMENTS = ([70, 1, 130, 64], [257, 600], [300], [1] * 8)


def nms_segments_case(segs, seed):
    """B = 3 rows whose categories are the segments `segs`, each segment in descending score order with scores quantised to 1/16 (equal
    scores inside a segment and across segments).  Row 0: ~80 % valid, the last segment entirely invalid (when there is more than one);
    row 1: nothing valid; row 2: everything valid, and for [70, 1, ...] the shift trap: segment 1's only box is [0, 0, 10, 10] and the
    row's best box is [11, 11, 21, 21] in segment 0."""
    r = np.random.RandomState(seed)
    B, n = 3, sum(segs)
    boxes = np.stack([clustered_boxes(n, seed + b, 120.0) for b in range(B)])
    scores = np.concatenate([-np.sort(-np.round(r.rand(B, s) * 16) / 16, axis=1) for s in segs], 1).astype(np.float32)
    idxs = np.broadcast_to(np.repeat(np.arange(len(segs)), segs), (B, n)).copy()
    valid = r.rand(B, n) < 0.8
    if len(segs) > 1:
        valid[0, n - segs[-1]:] = False
    valid[1] = False
    valid[2] = True
    if len(segs) > 1 and segs[0] >= 2 and segs[1] == 1:
        boxes[2, segs[0]] = (0, 0, 10, 10)
        boxes[2, 0], scores[2, 0] = (11, 11, 21, 21), 2.0
    if segs[0] >= 5:                                       # segment 0 is not shifted: two pairs whose IoU equals the threshold exactly
        boxes[2, 1:5], scores[2, :5] = _AT_THRESHOLD, (2.0, 1.9, 1.8, 1.7, 1.6)
    return {"boxes": boxes, "scores": scores, "idxs": idxs, "valid": valid, "segs": list(segs)}


def top_n_values(total, n):
    return sorted({v for v in (1, 5, total - 1, total, total + 7, n, n + 3) if v >= 1})


# ------------------------------------------------------------------------------------------------------------------ decoding
def emu_decode(codes, boxes, weights, xclip, img_h, img_w):
    """decode_clip_dev: codes, boxes [..., 4] fp32 (broadcastable).  -> dict ref [..., 4] float64 (the clamped corners from the
    emulated fp32 centres and clamped dw/dh and a float64 exp), tol, and emu [..., 4] fp32 (the same in fp32 with a correctly rounded expf: the
    stand-in kernel of the CPU tests)."""
    codes, boxes = f32(codes), f32(boxes)
    iw = [F(1) / F(v) for v in weights]
    xc = F(xclip)
    lim = np.array([img_w, img_h, img_w, img_h], np.float32)
    with np.errstate(all="ignore"):
        wh = np.stack([boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]], -1)
        ctr = boxes[..., :2] + F(0.5) * wh
        dxy = np.stack([codes[..., 0] * iw[0], codes[..., 1] * iw[1]], -1)
        dwh = np.stack([codes[..., 2] * iw[2], codes[..., 3] * iw[3]], -1)
        dwh = np.where(dwh > xc, xc, dwh)                                   # NaN stays
        pc = dxy * wh + ctr
        assert pc.dtype == np.float32 and dwh.dtype == np.float32
        e32 = np.exp(dwh.astype(np.float64)).astype(np.float32)          # a correctly rounded expf
        p32 = e32 * wh
        emu = np.concatenate([pc - F(0.5) * p32, pc + F(0.5) * p32], -1)
        emu = np.where(emu < 0, F(0), np.where(emu > lim, lim, emu))
        e = np.exp(dwh.astype(np.float64))
        pw = e * wh
        raw = np.concatenate([pc - 0.5 * pw, pc + 0.5 * pw], -1)
        t = 0.5 * (EXPF_ULPS * ulp(e) * np.abs(wh) + U * np.abs(pw))
        tol = np.concatenate([t, t], -1) + U * np.abs(raw)
        ref = np.where(raw < 0, 0.0, np.where(raw > lim, lim.astype(np.float64), raw))
        tol = np.where((raw + tol < 0) | (raw - tol > lim), 0.0, tol)
    return {"ref": ref, "tol": tol, "emu": emu.astype(np.float32)}


def sides(b):
    b = f32(b)
    return b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]


def rpn_flags(boxes, prob, min_size, score_thresh, mutant=None):
    """hd_rpn_decode_filter's stated test in fp32 on ITS OWN boxes and probabilities.  mutants: 'score_gt', 'size_gt'."""
    w, h = sides(boxes)
    ms, st, p = F(min_size), F(score_thresh), f32(prob)
    size = (w > ms) & (h > ms) if mutant == "size_gt" else (w >= ms) & (h >= ms)
    return size & (p > st if mutant == "score_gt" else p >= st)


def roi_flags(boxes, scores, min_size, score_thresh, mutant=None):
    """hd_roi_postprocess's: score > score_thresh (strict), both sides >= min_size.  mutants: 'score_ge', 'size_gt'."""
    w, h = sides(boxes)
    ms, st, p = F(min_size), F(score_thresh), f32(scores)
    size = (w > ms) & (h > ms) if mutant == "size_gt" else (w >= ms) & (h >= ms)
    return size & (p >= st if mutant == "score_ge" else p > st)


def ref_sigmoid(x):
    """-> (float64 sigmoid of the fp32 x, tolerance, fp32 emulation 1/(1 + exp(-x)))."""
    x = f32(x)
    with np.errstate(all="ignore"):
        e = np.exp(-x.astype(np.float64))
        p = 1.0 / (1.0 + e)
        tol = p * (EXPF_ULPS * 2.0 ** -23 * e / (1.0 + e) + 2 * U)
        emu = F(1) / (F(1) + e.astype(np.float32))
    return p, tol, emu.astype(np.float32)


def ref_softmax_fg(logits):
    """logits [R, C] fp32 -> (foreground probabilities [R, C-1] float64, tolerance, fp32 emulation in the kernel's order)."""
    lg = f32(logits)
    C = lg.shape[1]
    with np.errstate(all="ignore"):
        d = lg - lg.max(1, keepdims=True)                  # fp32: exact in the emulation
        e = np.exp(d.astype(np.float64))
        p = e[:, 1:] / e.sum(1, keepdims=True)
        tol = p * (2 * EXPF_ULPS * 2.0 ** -23 + C * U) + 2.0 ** -126
        e32 = e.astype(np.float32)
        se = np.zeros(lg.shape[0], np.float32)
        for c in range(C):
            se = se + e32[:, c]
        emu = e32[:, 1:] / se[:, None]
    return p, tol, emu.astype(np.float32)


DECODE_SIZES = ((1, 1), (1, 255), (2, 128), (1, 257), (2, 350))            # (N, K): N*K = 1, 255, 256, 257, 700
_ONE_BELOW = float(np.nextafter(F(1), F(0)))
#                   anchor                      deltas                     objectness     valid at min_size 1, score_thresh 0.5
_RPN_DESIGNED = [
    ((0, 0, 1, 1),                (0, 0, 0, 0),                0.0,           True),      # side == min_size, prob == 0.5 exactly: both >=
    ((0, 0, _ONE_BELOW, 1),       (0, 0, 0, 0),                0.0,           False),     # the next fp32 below min_size
    ((0, 0, 1, 1),                (0, 0, 0, 0),                -2.0 ** -20,   False),     # prob just below 0.5
    ((10, 10, 20, 20),            (0, 0, 9.0, 9.0),            3.0,           True),      # beyond bbox_xform_clip
    ((10, 10, 20, 20),            (0, 0, XCLIP, XCLIP),        3.0,           True),      # exactly at it (fp32 of it)
    ((10, 10, 20, 20),            (0, float("nan"), 0, 0),     3.0,           False),     # NaN stays NaN through the clamp
    ((10, 10, 20, 20),            (0, 0, float("nan"), 0),     3.0,           False),
    ((-500, -500, -400, -400),    (0, 0, 0, 0),                3.0,           False),     # wholly outside: clamps to zero width
    ((900, 900, 950, 950),        (0, 0, 0, 0),                3.0,           False),
]


def rpn_case(N, K, seed, img=(300.0, 320.0)):
    """-> dict deltas [N, A, 4], obj [N, A], anchors [A, 4], top [N, K] (the designed anchors first, as far as K allows), expect
    {(n, t): valid} at min_size 1.0 / score_thresh 0.5, img = (h, w)."""
    r = np.random.RandomState(seed)
    A = K + 37
    axy = r.rand(A, 2) * 280
    anchors = np.concatenate([axy, axy + 0.5 + r.rand(A, 2) * 150], 1).astype(np.float32)
    deltas = (r.randn(N, A, 4) * 0.6).astype(np.float32)
    deltas[:, ::11, 2:] = 6.0                              # beyond the clip
    obj = (r.randn(N, A) * 3).astype(np.float32)
    d = min(K, len(_RPN_DESIGNED))
    for i, (an, de, ob, _) in enumerate(_RPN_DESIGNED[:d]):
        anchors[i], deltas[:, i], obj[:, i] = an, de, ob
    top = np.stack([np.concatenate([np.arange(d), d + r.permutation(A - d)[:K - d]]) for _ in range(N)]).astype(np.int64)
    expect = {(n, i): _RPN_DESIGNED[i][3] for n in range(N) for i in range(d)}
    return {"deltas": deltas, "obj": obj, "anchors": anchors, "top": top, "expect": expect, "img": img}


def ref_rpn(c, xclip=XCLIP):
    """Reference boxes / probabilities of an rpn_case at its `top` candidates."""
    n = np.arange(c["top"].shape[0])[:, None]
    dec = emu_decode(c["deltas"][n, c["top"]], c["anchors"][c["top"]], (1, 1, 1, 1), xclip, *c["img"])
    p, ptol, pemu = ref_sigmoid(c["obj"][n, c["top"]])
    return {"boxes": dec["ref"], "boxes_tol": dec["tol"], "prob": p, "prob_tol": ptol, "emu_boxes": dec["emu"], "emu_prob": pemu}


ROI_DECODE_SIZES = ((1, 1), (255, 1), (256, 1), (257, 1), (700, 1), (1, 4), (64, 4), (175, 4))      # (R, K): K = C - 1
ROI_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def roi_decode_case(R, K, seed, img=(300.0, 320.0)):
    """-> dict codes [R, K*4], rois [R, 5] (image index in column 0), img.  Rows 0..3 (as far as R allows): beyond the clip, exactly
    at it, NaN, wholly outside the image."""
    r = np.random.RandomState(seed)
    xy = r.rand(R, 2) * 280
    rois = np.concatenate([r.randint(0, 3, (R, 1)), xy, xy + 1 + r.rand(R, 2) * 150], 1).astype(np.float32)
    codes = r.randn(R, K, 4).astype(np.float32) * np.array([2, 2, 3, 3], np.float32)
    rows = [(None, (0, 0, 60.0, 60.0)), (None, (0, 0, float(F(XCLIP) * F(5.0)), float(F(XCLIP) * F(5.0)))),
            (None, (float("nan"), 0, 0, float("nan"))), ((-900, -900, -800, -850), (0, 0, 0, 0))]
    for i, (box, code) in enumerate(rows[:R]):
        codes[i, :] = code
        if box is not None:
            rois[i, 1:] = box
    return {"codes": codes.reshape(R, K * 4), "rois": rois, "img": img}


#  (R, S, C, counts per image)
POSTPROCESS_CASES = [(16, 4, 2, (0, 1, 3, 4)), (16, 4, 5, (4, 3, 1, 0)), (1024, 256, 2, (0, 1, 255, 256)), (1024, 256, 5, (256, 255, 0, 1)),
                     (1, 256, 2, (1,)), (255, 256, 2, (255,)), (256, 256, 2, (256,)), (257, 256, 2, (256, 1)), (175, 256, 5, (174,))]
_POST_DESIGNED = [     # logits (C = 2), roi, code of class 1 -> valid at min_size 1, score_thresh 0.5
    ((1.5, 1.5), (0, 0, 1, 1), (0, 0, 0, 0), False),                    # equal logits: score == 0.5, the test is a strict >
    ((1.5, 1.5 + 2.0 ** -12), (0, 0, 1, 1), (0, 0, 0, 0), True),        # just above, side == min_size
    ((1.5, 1.5 + 2.0 ** -12), (0, 0, _ONE_BELOW, 1), (0, 0, 0, 0), False),
]


def postprocess_case(R, S, C, counts, seed, img=(300.0, 320.0)):
    """-> dict logits [R, C], codes [R, C*4], rois [R, 5], counts, real [R] bool, expect {(r, k): valid}.  Padding rows (r % S >=
    counts[r // S]) hold NaN logits and codes."""
    r = np.random.RandomState(seed)
    d = roi_decode_case(R, C, seed, img)
    logits = (r.randn(R, C) * 2).astype(np.float32)
    codes = d["codes"].reshape(R, C, 4).copy()
    rois = d["rois"]
    rows = np.arange(R)
    real = (rows % S) < np.asarray(counts)[rows // S]
    expect = {}
    if C == 2:
        for i, (lg, roi, code, ok) in enumerate(_POST_DESIGNED):
            q = 4 + i
            if q < R and real[q]:
                logits[q], rois[q, 1:], codes[q, 1] = lg, roi, code
                expect[(q, 0)] = ok
    logits[~real] = np.nan
    codes[~real] = np.nan
    rois[:, 0] = rows // S
    return {"logits": logits, "codes": codes.reshape(R, C * 4), "rois": rois, "counts": np.asarray(counts, np.int64), "real": real,
            "expect": expect, "img": img, "S": S}


def ref_postprocess(c, weights=ROI_WEIGHTS, xclip=XCLIP, mutant=None):
    """-> dict boxes [R, K, 4] / scores [R, K] float64 with tolerances, emu_boxes / emu_scores fp32 (the stand-in kernel).
    mutant 'pad_unzeroed': the stand-in computes the padding rows like real ones."""
    R, C = c["logits"].shape
    real = c["real"]
    dec = emu_decode(c["codes"].reshape(R, C, 4)[:, 1:], c["rois"][:, None, 1:], weights, xclip, *c["img"])
    p, ptol, pemu = ref_softmax_fg(c["logits"])
    z = lambda a, fill=0.0: np.where(real.reshape((R,) + (1,) * (a.ndim - 1)), a, fill)
    keep = (lambda a: a) if mutant == "pad_unzeroed" else z
    return {"boxes": z(dec["ref"]), "boxes_tol": z(dec["tol"]), "scores": z(p), "scores_tol": z(ptol),
            "emu_boxes": f32(keep(dec["emu"])), "emu_scores": f32(keep(pemu))}


# ------------------------------------------------------------------------------------------------------------------ RoI sampling tail
def ref_roi_samples(sel_rows, comb, lab, matched, gt, gvalid, weights):
    """Rows of the RoI stage for the flat candidate indices sel_rows (into [N, T]; a negative entry -(image + 1) is a padding row):
    -> rois [R, 5] fp32 (image, box; padding: image, 0, 0, 0, 0), labels [R] int64 (padding -1), enc (emu_encode; padding: zeros with
    tolerance 0), pad [R] bool."""
    comb, gt, gv = f32(comb), f32(gt), np.asarray(gvalid, bool)
    N, T, _ = comb.shape
    s = np.asarray(sel_rows, np.int64)
    pad = s < 0
    sc = np.where(pad, 0, s)
    n = np.where(pad, -s - 1, sc // T)
    box = comb.reshape(-1, 4)[sc]
    m = np.maximum(np.asarray(matched).reshape(-1)[sc], 0)
    ref = np.where(gv.any(1)[n][:, None], gt[n, m], F(0))                 # GT-less image: a zero box
    enc = emu_encode(ref, box, weights)
    enc["xy"][pad], enc["wh"][pad], enc["wh_tol"][pad] = 0, 0, 0
    rois = np.concatenate([n[:, None].astype(np.float32), np.where(pad[:, None], F(0), box)], 1)
    labels = np.where(pad, -1, np.asarray(lab).reshape(-1)[sc])
    return {"rois": torch.from_numpy(f32(rois)), "labels": torch.from_numpy(labels.astype(np.int64)), "enc": enc, "pad": pad}


def ref_roi_samples_padded(pos_sel, neg_sel, comb, lab, matched, gt, gvalid, S, weights, mutant=None):
    """hd_roi_samples_padded: per image the selected candidates (pos | neg) in ascending index order, the first S of them, then padding
    up to S; counts [N] int64.  mutants: 'carry_dropped' (the rank restarts at every 256-candidate round: later rounds overwrite the
    rows of earlier ones), 'double_count' (a candidate in both masks takes two ranks)."""
    pos, neg = np.asarray(pos_sel, bool), np.asarray(neg_sel, bool)
    N, T = pos.shape
    sel, counts = [], []
    for n in range(N):
        on = np.nonzero(pos[n] | neg[n])[0]
        rows = np.full(S, -(n + 1), np.int64)
        if mutant == "carry_dropped":
            rank = np.concatenate([np.arange(int(((on >= t0) & (on < t0 + 256)).sum())) for t0 in range(0, T, 256)])
            cnt = min(S, len(on))
        elif mutant == "double_count":
            w = 1 + (pos[n] & neg[n])[on]
            rank = np.cumsum(w) - w
            cnt = min(S, int(w.sum()))
        else:
            rank, cnt = np.arange(len(on)), min(S, len(on))
        ok = rank < S
        rows[rank[ok]] = n * T + on[ok]
        if mutant:
            rows[cnt:] = -(n + 1)
        sel.append(rows)
        counts.append(cnt)
    out = ref_roi_samples(np.concatenate(sel), comb, lab, matched, gt, gvalid, weights)
    out["counts"] = torch.tensor(counts, dtype=torch.int64)
    return out


SAMPLES_T = (1, 255, 256, 257, 600)
SAMPLES_S = (4, 128)
SAMPLES_G = (1, 7)


def roi_samples_case(T, S, G, part, seed):
    """N = 4 images of T candidates.  Selected count per image: part 0 -> (0, 1, S-1, S), part 1 -> (S+1, T, a third of T, S), each at
    most T.  The selected candidates are spread over the whole list (both sides of every 256 boundary; 255, 256 and the last one are
    always among them when the count allows), some of them in both masks.  Image 2 has no GT (its rows hold stale coordinates)."""
    r = np.random.RandomState(seed)
    N = 4
    want = [(0, 1, S - 1, S), (S + 1, T, max(1, T // 3), S)][part]
    pos, neg = np.zeros((N, T), bool), np.zeros((N, T), bool)
    for n, k in enumerate(want):
        k = min(k, T)
        must = list(dict.fromkeys(t for t in (T - 1, 255, 256, 0) if 0 <= t < T))[:k]
        rest = np.setdiff1d(np.arange(T), must)
        on = np.concatenate([must, r.permutation(rest)[:k - len(must)]]).astype(np.int64)
        cls = r.randint(0, 3, len(on))
        pos[n, on[cls != 1]] = True
        neg[n, on[cls != 0]] = True                        # cls 2: in both masks
    xy = r.rand(N, T, 2) * 250
    comb = np.concatenate([xy, xy + 2 + r.rand(N, T, 2) * 90], 2).astype(np.float32)
    gxy = r.rand(N, G, 2) * 200
    gt = np.concatenate([gxy, gxy + 5 + r.rand(N, G, 2) * 100], 2).astype(np.float32)
    gvalid = r.rand(N, G) < 0.8
    gvalid[:, 0] = True
    gvalid[2] = False
    matched = np.array([-2, -1, 0, G - 1], np.int64)[r.randint(0, 4, (N, T))]
    lab = r.randint(0, 6, (N, T)).astype(np.int64)
    return {"pos": pos, "neg": neg, "comb": comb, "lab": lab, "matched": matched, "gt": gt, "gvalid": gvalid, "S": S, "want": want}


def finish_sel(c, R, seed):
    """R entries for hd_roi_samples_finish: selected candidates of the case in ascending order, every fourth a padding entry."""
    r = np.random.RandomState(seed)
    N, T = c["pos"].shape
    sel = np.sort(r.randint(0, N * T, R)).astype(np.int64)
    sel[3::4] = -(r.randint(0, N, len(sel[3::4])) + 1)
    return sel


# ------------------------------------------------------------------------------------------------------------------ level mapper
LEVEL_ARGS = dict(canonical_scale=224, canonical_level=4, eps=1e-6, k_min=2, k_max=5)
LEVEL_SIDES = (28, 56, 112, 224, 448, 896, 1792)           # sqrt(area)*fl(1/224) is an exact power of two: floor values 1 .. 7


def ref_levels(boxes, mutant=None, canonical_scale=224, canonical_level=4, eps=1e-6, k_min=2, k_max=5):
    """torchvision's LevelMapper in float64 on the fp32 boxes -> (level [R] int32, the pre-floor value's distance to an integer).
    mutant 'no_eps': the floor taken without eps."""
    b = f32(boxes).astype(np.float64)
    with np.errstate(all="ignore"):
        v = canonical_level + np.log2(np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / canonical_scale)
        t = np.floor(v + (0.0 if mutant == "no_eps" else float(F(eps))))
        dist = np.where(np.isfinite(v), np.abs(v - np.round(v)), 1.0)
    lev = np.clip(np.where(np.isnan(t), k_min, t), k_min, k_max) - k_min
    return torch.from_numpy(lev.astype(np.int32)), dist


def emu_levels(boxes, canonical_scale=224, canonical_level=4, eps=1e-6, k_min=2, k_max=5):
    """roi_levels_kernel in numpy fp32 (a correctly rounded log2f in place of the device's): the stand-in kernel of the CPU test."""
    b = f32(boxes)
    with np.errstate(all="ignore"):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        x = np.sqrt(area) * (F(1) / F(canonical_scale))
        t = np.floor((F(canonical_level) + np.log2(x.astype(np.float64)).astype(np.float32)) + F(eps))
    t = np.where(t < k_min, F(k_min), np.where(t > k_max, F(k_max), t))
    return torch.from_numpy((t.astype(np.int64) - k_min).astype(np.int32))


def level_case(seed=0):
    """-> dict boxes [R, 4] fp32, expect [R] int32, designed [R] bool, keep [R] bool (designed, or float64 pre-floor value further than
    LEVEL_MARGIN from an integer).  Designed: the LEVEL_SIDES squares, exact / x2 one fp32 step smaller / larger (eps = 1e-6 outweighs
    the 7e-8 relative step: all on the upper level), a zero-area row (log2(0) = -inf: level 0), a huge box (k_max).  Then 4000 random
    boxes with log-uniform sides in [1, 1200]."""
    r = np.random.RandomState(seed)
    rows, want = [], []
    for j, s in enumerate(LEVEL_SIDES):
        lev = min(max(j + 1, 2), 5) - 2
        x1, y1 = F(3 * j), F(5 * j)
        x2, y2 = x1 + F(s), y1 + F(s)
        for xe in (x2, np.nextafter(x2, F(0)), np.nextafter(x2, F(1e9))):
            rows.append((x1, y1, xe, y2))
            want.append(lev)
    rows += [(7, 7, 7, 7), (0, 0, 0, 50), (0, 0, 1e5, 1e5)]
    want += [0, 0, 3]
    nd = len(rows)
    sides_ = np.exp(r.rand(4000, 2) * math.log(1200.0))
    xy = r.rand(4000, 2) * 100
    boxes = np.concatenate([np.array(rows, np.float32), np.concatenate([xy, xy + sides_], 1).astype(np.float32)])
    lev, dist = ref_levels(boxes)
    designed = np.arange(len(boxes)) < nd
    expect = lev.clone()
    expect[:nd] = torch.tensor(want, dtype=torch.int32)
    return {"boxes": boxes, "expect": expect, "designed": designed, "keep": designed | (dist > LEVEL_MARGIN)}
