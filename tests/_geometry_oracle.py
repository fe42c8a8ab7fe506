"""Independent restatement of the paired geometric augmentation (hallucidet_amd/dataloader/geometry.py, csrc/geometry.hip), not
collected by pytest.  The tap positions are exact rationals (`fractions.Fraction`); the three interpolations run per pixel in
`numpy.float32`, one rounded operation at a time.  Nothing is shared with `apply_host`.

A record row is [flip, x0, y0, x1, y1, 0, 0, 0]; see the module docstring of dataloader/geometry.py for the definition."""
from fractions import Fraction
from functools import lru_cache
from math import floor

import numpy as np

F = np.float32


@lru_cache(maxsize=None)
def axis_table(extent, c):
    """per output coordinate o of an axis of `extent` samples whose crop has c: (tap a, tap b, fp32 weight of b).  The centre of output
    sample o lies at crop coordinate (o + 1/2) c / extent - 1/2; its floor is the first tap, its fractional part the weight."""
    out = []
    for o in range(extent):
        pos = (Fraction(2 * o + 1, 2) * c) / extent - Fraction(1, 2)
        j = floor(pos)
        frac = pos - j                                   # in [0, 1), denominator divides 2 * extent
        num = frac * (2 * extent)
        assert num.denominator == 1
        w = F(int(num)) / F(2 * extent)
        out.append((min(max(j, 0), c - 1), min(max(j + 1, 0), c - 1), w))
    return tuple(out)


def _plane(plane, H, W, flip, x0, y0, x1, y1):
    xs, ys = axis_table(W, x1 - x0), axis_table(H, y1 - y0)
    src = plane[:, ::-1] if flip else plane              # the flipped image; the crop window is taken from it
    out = np.empty((H, W), dtype=np.uint8)
    half = F(0.5)
    for oy in range(H):
        ya, yb, fy = ys[oy]
        ra, rb = src[y0 + ya], src[y0 + yb]
        for ox in range(W):
            xa, xb, fx = xs[ox]
            v00, v01, v10, v11 = F(ra[x0 + xa]), F(ra[x0 + xb]), F(rb[x0 + xa]), F(rb[x0 + xb])
            d0 = F(v01 - v00)
            m0 = F(fx * d0)
            t0 = F(v00 + m0)
            d1 = F(v11 - v10)
            m1 = F(fx * d1)
            t1 = F(v10 + m1)
            d2 = F(t1 - t0)
            m2 = F(fy * d2)
            v = F(t0 + m2)
            out[oy, ox] = int(np.floor(F(v + half)))
    return out


_cache = {}


def plane(p, row):
    """p: uint8 [H, W] array; row: the record (8 ints) -> the transformed plane.  Memoised on the bytes and the record."""
    p = np.ascontiguousarray(p)
    row = tuple(int(v) for v in row)
    assert len(row) == 8 and row[5:] == (0, 0, 0) and row[0] in (0, 1)
    H, W = p.shape
    assert 0 <= row[1] < row[3] <= W and 0 <= row[2] < row[4] <= H
    key = (p.tobytes(), H, W, row)
    if key not in _cache:
        _cache[key] = _plane(p, H, W, *row[:5])
        _cache[key].setflags(write=False)
    return _cache[key]


def batch(u8, rows):
    """u8: uint8 array [N, C, H, W]; rows: [N, 8] ints -> the transformed batch"""
    u8 = np.asarray(u8)
    out = np.empty_like(u8)
    for n in range(u8.shape[0]):
        for c in range(u8.shape[1]):
            out[n, c] = plane(u8[n, c], rows[n])
    return out
