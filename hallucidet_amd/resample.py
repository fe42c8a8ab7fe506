"""Tap tables of the detector-input resize (csrc/image_transform.hip; --detector-resize nearest | bilinear | bilinear_aa).

`resample_taps(in_size, out_size, mode)` builds the table of ONE axis on the host, in float64, and stores it as fp32 / int32:

  forward form      start[out], count[out], weight[out, T]     T = the largest tap count of the axis, unused entries zero
                    weight_lo[out, T] = fp32(W - fp32(W))      the part of the float64 weight W that `weight` drops (forward kernel only)
  transposed (CSR)  rstart[in + 1], rout[nnz], rweight[nnz]    the same entries grouped by input index, output index ascending

  nearest      one tap of weight 1 at min(floor(fp32(o) * fp32(in / out)), in - 1): the product is taken in fp32, as `nn_src` of
               csrc/elementwise.hip takes it (ATen's legacy 'nearest')
  bilinear     F.interpolate(mode="bilinear", align_corners=False): source coordinate max((o + 0.5) * in / out - 0.5, 0), two taps
               (one where the second has weight zero or would leave the axis)
  bilinear_aa  the same call with antialias=True: ATen's triangle filter, whose support grows with in / out when shrinking; weights
               normalised to sum to 1

Entries of weight zero at either end of a tap run are dropped, so every listed entry moves data (the coverage of a mode is the share of
input indices whose transposed row is not empty).  Nothing here touches a device; `ops.resample_tables` uploads and caches the tables.
"""
import math

import numpy as np

MODES = ("nearest", "bilinear", "bilinear_aa")
MAX_TAPS = 32


class Taps:
    """One axis' tables.  `weight64` keeps the float64 weights the fp32 ones were rounded from."""

    __slots__ = ("in_size", "out_size", "mode", "T", "start", "count", "weight", "weight_lo", "weight64", "rstart", "rout", "rweight", "nnz")

    def dense(self, dtype=np.float64):
        """[out, in] matrix of the forward form (float64: before the fp32 rounding; float32: what the kernel multiplies by)."""
        w = self.weight64 if dtype == np.float64 else self.weight
        m = np.zeros((self.out_size, self.in_size), dtype=dtype)
        for o in range(self.out_size):
            m[o, self.start[o]:self.start[o] + self.count[o]] = w[o, :self.count[o]]
        return m

    def coverage(self):
        """Share of input indices that at least one output reads with a non-zero weight."""
        return float(np.count_nonzero(np.diff(self.rstart))) / self.in_size


def _axis_nearest(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return [(int(min(s, n_in - 1)), [1.0]) for s in src]


def _axis_bilinear(n_in, n_out):
    scale = n_in / n_out
    taps = []
    for o in range(n_out):
        src = max(scale * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(src), n_in - 1)
        l1 = src - i0
        if i0 < n_in - 1 and l1 != 0.0:
            taps.append((i0, [1.0 - l1, l1]))
        else:
            taps.append((i0, [1.0]))
    return taps


def _axis_bilinear_aa(n_in, n_out):
    """ATen's _compute_indices_min_size_weights_aa with the triangle filter (interp_size 2), align_corners=False."""
    scale = n_in / n_out
    support = scale if scale >= 1.0 else 1.0            # interp_size * 0.5 * scale
    invscale = 1.0 / scale if scale >= 1.0 else 1.0
    max_size = int(math.ceil(support)) * 2 + 1
    taps = []
    for o in range(n_out):
        center = scale * (o + 0.5)
        xmin = max(int(center - support + 0.5), 0)
        xsize = min(int(center + support + 0.5), n_in) - xmin
        xsize = min(max(xsize, 0), max_size)
        w = []
        total = 0.0
        for j in range(xsize):
            a = abs((j + xmin - center + 0.5) * invscale)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        while len(w) > 1 and w[0] == 0.0:
            w.pop(0)
            xmin += 1
        while len(w) > 1 and w[-1] == 0.0:
            w.pop()
        taps.append((xmin, w))
    return taps


_AXIS = {"nearest": _axis_nearest, "bilinear": _axis_bilinear, "bilinear_aa": _axis_bilinear_aa}
_CACHE = {}


def resample_taps(in_size, out_size, mode):
    """-> Taps of one axis (cached per (in, out, mode): treat the arrays as read-only)."""
    if mode not in MODES:
        raise ValueError("resample_taps: mode must be one of %s (got %r)" % (", ".join(MODES), mode))
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resample_taps: in_size and out_size must be >= 1 (got %d -> %d)" % (in_size, out_size))
    key = (in_size, out_size, mode)
    t = _CACHE.get(key)
    if t is not None:
        return t
    if mode == "bilinear_aa" and in_size / out_size > MAX_TAPS:          # 2 * in / out taps and more: refuse before building them
        raise ValueError("resample_taps: %d -> %d with %s needs more than %d taps" % (in_size, out_size, mode, MAX_TAPS))
    taps = _AXIS[mode](in_size, out_size)
    T = max(len(w) for _, w in taps)
    if T > MAX_TAPS:
        raise ValueError("resample_taps: %d -> %d with %s needs %d taps, the kernels take at most %d" % (in_size, out_size, mode, T, MAX_TAPS))
    t = Taps()
    t.in_size, t.out_size, t.mode, t.T = in_size, out_size, mode, T
    t.start = np.array([s for s, _ in taps], dtype=np.int32)
    t.count = np.array([len(w) for _, w in taps], dtype=np.int32)
    t.weight64 = np.zeros((out_size, T), dtype=np.float64)
    for o, (_, w) in enumerate(taps):
        t.weight64[o, :len(w)] = w
    t.weight = t.weight64.astype(np.float32)
    # what fp32 drops of the float64 weight: the forward kernel carries its sum as a pair of floats and reads weight + weight_lo
    t.weight_lo = (t.weight64 - t.weight.astype(np.float64)).astype(np.float32)
    # transposed form: the forward entries, stably sorted by input index (so the output index ascends within a row)
    o_idx = np.repeat(np.arange(out_size, dtype=np.int64), t.count)
    k_idx = np.concatenate([np.arange(c, dtype=np.int64) for c in t.count])
    i_idx = t.start.astype(np.int64)[o_idx] + k_idx
    order = np.argsort(i_idx, kind="stable")
    t.rout = o_idx[order].astype(np.int32)
    t.rweight = t.weight[o_idx[order], k_idx[order]].copy()
    t.rstart = np.zeros(in_size + 1, dtype=np.int32)
    np.cumsum(np.bincount(i_idx, minlength=in_size), out=t.rstart[1:])
    t.nnz = int(t.rout.shape[0])
    for a in (t.start, t.count, t.weight, t.weight_lo, t.weight64, t.rstart, t.rout, t.rweight):
        a.setflags(write=False)
    _CACHE[key] = t
    return t


def check_taps(t):
    """The C boundary's check of a table (hd_resample_taps_check, host pointers): raises _abi.HipCallError on a bad one."""
    import ctypes as C

    from . import _abi

    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    w = np.ascontiguousarray(t.weight)
    _abi.check(_abi.load().hd_resample_taps_check(p(t.start), p(t.count), p(w), t.in_size, t.out_size, t.T, p(t.rstart), p(t.rout), p(t.rweight),
                                                  t.nnz, p(np.ascontiguousarray(t.weight_lo))), "hd_resample_taps_check")


def normalize_stats(image_mean, image_std, channels=3):
    """-> (mean, std) as tuples of `channels` python floats; None = 0 / 1; a sequence of length 1 is broadcast."""
    def one(v, default, name):
        if v is None:
            return (default,) * channels
        v = [float(a) for a in (v if isinstance(v, (list, tuple)) else list(v))]
        if len(v) == 1:
            v = v * channels
        if len(v) != channels:
            raise ValueError("%s must have 1 or %d entries (got %d)" % (name, channels, len(v)))
        if not all(math.isfinite(a) for a in v):
            raise ValueError("%s must be finite (got %s)" % (name, v))
        return tuple(v)
    mean, std = one(image_mean, 0.0, "image_mean"), one(image_std, 1.0, "image_std")
    if any(s <= 0.0 for s in std):
        raise ValueError("image_std must be > 0 in every channel (got %s)" % (list(std),))
    return mean, std


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
