"""Photometric augmentation of the reference's detector training (train_detector.py:401-410, applied per sample to the decoded PIL
image, dataloader.py:181-183):

    ColorJitter(brightness=0.01, contrast=0.01, saturation=0.01, hue=0.01), RandomInvert(p=0.1),
    RandomAdjustSharpness(sharpness_factor=1.2, p=0.1), RandomEqualize(p=0.1)

Here the random draw is a small host record (`ReferenceAugmentation.draw`: one float32 row per image) and the operations run on the
uint8 batch where it already is: in HBM through `ops.augment_u8` (csrc/augment.hip), or on the host through `apply_host`, the same
definitions in numpy.  Every operation is integer in, integer out, and both paths reproduce Pillow (which torchvision's PIL backend
calls for each of them) bit for bit.

Record row (ROW floats, the layout of hd_augment_u8): [0..3] jitter operations in the order they run (0 brightness, 1 contrast,
2 saturation, 3 hue, -1 none), [4..6] brightness / contrast / saturation factors, [7] hue factor, [8..10] invert / sharpness / equalize
flags, [11] sharpness factor.
"""
import numpy as np
import torch

ROW = 12
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
_M64 = (1 << 64) - 1
f32 = np.float32


def make_row(order=(-1, -1, -1, -1), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, invert=False, sharpness=False, equalize=False,
             sharpness_factor=1.2):
    """One record row from explicit values (tests, tools)."""
    order = tuple(order) + (-1,) * (4 - len(order))
    return torch.tensor([float(o) for o in order] + [brightness, contrast, saturation, hue, float(bool(invert)), float(bool(sharpness)),
                                                     float(bool(equalize)), sharpness_factor], dtype=torch.float32)


def _mix(*vals):
    """splitmix64-style hash of a tuple of integers -> a 63-bit generator seed"""
    h = 0x9E3779B97F4A7C15
    for v in vals:
        h = (h + (int(v) & _M64) + 0x9E3779B97F4A7C15) & _M64
        h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & _M64
        h ^= h >> 31
    return h >> 1


class ReferenceAugmentation:
    """The reference's augmentation parameters; `draw` makes the per-image record, `params_for` makes it a pure function of
    (seed, epoch, rank, batch index)."""

    def __init__(self, brightness=0.01, contrast=0.01, saturation=0.01, hue=0.01, p_invert=0.1, sharpness_factor=1.2, p_sharpness=0.1,
                 p_equalize=0.1, seed=0, rank=0):
        for name, v in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
            if v < 0:
                raise ValueError("%s must be non-negative (got %r)" % (name, v))
        if not 0 <= hue <= 0.5:
            raise ValueError("hue must lie in [0, 0.5] (got %r)" % (hue,))
        for name, v in (("p_invert", p_invert), ("p_sharpness", p_sharpness), ("p_equalize", p_equalize)):
            if not 0 <= v <= 1:
                raise ValueError("%s must be a probability (got %r)" % (name, v))
        self.brightness, self.contrast, self.saturation, self.hue = float(brightness), float(contrast), float(saturation), float(hue)
        self.p_invert, self.p_sharpness, self.p_equalize = float(p_invert), float(p_sharpness), float(p_equalize)
        self.sharpness_factor = float(sharpness_factor)
        self.seed, self.rank, self.epoch = int(seed), int(rank), 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def generator(self, batch_index, epoch=None):
        return torch.Generator().manual_seed(_mix(self.seed, self.epoch if epoch is None else epoch, self.rank, batch_index))

    def params_for(self, n, batch_index, epoch=None):
        return self.draw(n, self.generator(batch_index, epoch))

    @staticmethod
    def _uniform(n, lo, hi, g):
        """n float32 values of U[lo, hi], never outside the interval after the rounding to float32"""
        v = (lo + (hi - lo) * torch.rand(n, dtype=torch.float64, generator=g)).to(torch.float32)
        lo32, hi32 = f32(lo), f32(hi)
        if float(lo32) < lo:
            lo32 = np.nextafter(lo32, f32(np.inf))
        if float(hi32) > hi:
            hi32 = np.nextafter(hi32, f32(-np.inf))
        return v.clamp_(float(lo32), float(hi32))

    def draw(self, n, generator):
        """-> float32 [n, ROW]: per image what torchvision draws: a uniformly random order of the four jitter operations (one whose
        range is zero is left out, as ColorJitter does), b, c, s ~ U[max(0, 1 - x), 1 + x], h ~ U[-hue, hue], three Bernoulli flags."""
        g = generator
        rows = torch.empty(n, ROW, dtype=torch.float32)
        order = torch.rand(n, 4, dtype=torch.float64, generator=g).argsort(dim=1).to(torch.float32)     # a uniform permutation per row
        amount = torch.tensor([self.brightness, self.contrast, self.saturation, self.hue])
        rows[:, 0:4] = torch.where(amount[order.long()] > 0, order, torch.full_like(order, -1.0))
        rows[:, 4] = self._uniform(n, max(0.0, 1.0 - self.brightness), 1.0 + self.brightness, g)
        rows[:, 5] = self._uniform(n, max(0.0, 1.0 - self.contrast), 1.0 + self.contrast, g)
        rows[:, 6] = self._uniform(n, max(0.0, 1.0 - self.saturation), 1.0 + self.saturation, g)
        rows[:, 7] = self._uniform(n, -self.hue, self.hue, g)
        flags = torch.rand(n, 3, dtype=torch.float64, generator=g)
        rows[:, 8] = (flags[:, 0] < self.p_invert).float()
        rows[:, 9] = (flags[:, 1] < self.p_sharpness).float()
        rows[:, 10] = (flags[:, 2] < self.p_equalize).float()
        rows[:, 11] = self.sharpness_factor
        return rows


# ------------------------------------------------------------------------------------------------ the operations, on the host
# x: uint8 array [H, W, 3] or [H, W].  Each function restates Pillow's C code in numpy, operation by operation.
def blend(deg, img, a):
    """ImagingBlend: float32 temp = in1 + alpha * (in2 - in1); alpha in [0, 1]: truncate, else clip then truncate"""
    a = f32(a)
    d = deg.astype(np.int32)
    t = (d.astype(f32) + a * (img.astype(np.int32) - d).astype(f32)).astype(f32)
    if 0.0 <= a <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.clip(t, 0, 255).astype(np.uint8)


def to_l(rgb):
    r, g, b = [rgb[..., i].astype(np.int64) for i in range(3)]
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def brightness(x, f):
    return blend(np.zeros_like(x), x, f)


def contrast(x, f):
    l = to_l(x) if x.ndim == 3 else x
    mean = int(int(l.sum(dtype=np.int64)) / l.size + 0.5)
    return blend(np.full_like(x, mean), x, f)


def saturation(x, f):
    if x.ndim == 2:
        return x
    return blend(np.repeat(to_l(x)[..., None], 3, 2), x, f)


def rgb2hsv(x):
    r, g, b = [x[..., i].astype(np.int32) for i in range(3)]
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    cr = (maxc - minc).astype(f32)
    f64 = np.float64
    with np.errstate(all='ignore'):
        s = cr / maxc.astype(f32)
        rc = (maxc - r).astype(f32) / cr
        gc = (maxc - g).astype(f32) / cr
        bc = (maxc - b).astype(f32) / cr
        h = np.where(r == maxc, (bc - gc).astype(f64),
                     np.where(g == maxc, 2.0 + rc.astype(f64) - bc.astype(f64), 4.0 + gc.astype(f64) - rc.astype(f64))).astype(f32)
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32).astype(f64)
        uh = np.clip((h * 255.0).astype(np.int32), 0, 255)
        us = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    gray = maxc == minc
    return np.stack([np.where(gray, 0, uh), np.where(gray, 0, us), maxc], -1).astype(np.uint8)


def hsv2rgb(x):
    h, s, v = [x[..., i].astype(np.int32) for i in range(3)]
    fs = (s / 255.0).astype(f32)
    hh = (h * 6.0 / 255.0).astype(f32)
    i = np.floor(hh).astype(np.int32)
    f = (hh - i).astype(f32)
    vf = v.astype(f32)
    one = f32(1.0)

    def rnd(t):
        return np.clip(np.floor(t.astype(np.float64) + 0.5), 0, 255).astype(np.int32)
    p = rnd(vf * (one - fs))
    q = rnd(vf * (one - fs * f))
    t = rnd(vf * (one - fs * (one - f)))
    i6 = i % 6
    out = np.stack([np.choose(i6, [v, q, p, p, t, v]), np.choose(i6, [t, v, v, q, p, p]), np.choose(i6, [p, p, t, v, v, q])], -1)
    return np.where((s == 0)[..., None], np.stack([v, v, v], -1), out).astype(np.uint8)


def hue(x, shift):
    """torchvision's PIL recipe: RGB -> HSV, H += shift (uint8 wrap-around), HSV -> RGB; taken also when the shift is 0"""
    if x.ndim == 2:
        return x
    hsv = rgb2hsv(x)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv2rgb(hsv)


def hue_shift_of(h):
    """the uint8 H shift of hue factor h (a float32): trunc(h * 255), the product in double"""
    return int(np.float64(f32(h)) * 255.0)


def smooth(x):
    """ImageFilter.SMOOTH: [1 1 1; 1 5 1; 1 1 1] / 13 in float32, + 0.5, clipped, truncated; the one-pixel border is copied"""
    k = np.array([[1, 1, 1], [1, 5, 1], [1, 1, 1]], dtype=f32)
    out = x.copy()
    xs = x.astype(f32)
    H, W = x.shape[:2]
    acc = np.zeros(x[1:-1, 1:-1].shape, dtype=f32)
    for dy in range(3):
        for dx in range(3):
            acc += xs[dy:H - 2 + dy, dx:W - 2 + dx] * (k[dy, dx] / f32(13))
    out[1:-1, 1:-1] = np.clip(acc + f32(0.5), 0, 255).astype(np.uint8)
    return out


def sharpness(x, f):
    return blend(smooth(x), x, f)


def equalize(x):
    def band(b):
        h = np.bincount(b.ravel(), minlength=256).astype(np.int64)
        nz = h[h > 0]
        if len(nz) <= 1:
            return b
        step = int(nz.sum() - nz[-1]) // 255
        if step == 0:
            return b
        n = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
        return np.clip(n // step, 0, 255).astype(np.uint8)[b]
    if x.ndim == 2:
        return band(x)
    return np.stack([band(x[..., i]) for i in range(3)], -1)


def apply_host_image(x, row):
    """x: uint8 [H, W, 3] or [H, W]; row: ROW floats -> the augmented image"""
    row = np.asarray(row, dtype=f32)
    for op in row[0:4].astype(np.int32):
        if op == BRIGHTNESS:
            x = brightness(x, row[4])
        elif op == CONTRAST:
            x = contrast(x, row[5])
        elif op == SATURATION:
            x = saturation(x, row[6])
        elif op == HUE:
            x = hue(x, hue_shift_of(row[7]))
    if row[8] != 0:
        x = 255 - x
    if row[9] != 0:
        x = sharpness(x, row[11])
    if row[10] != 0:
        x = equalize(x)
    return x


def apply_host(u8, params):
    """u8: uint8 tensor [N, C, H, W] on the CPU, C = 1 or 3; params: float32 [N, ROW] -> the augmented batch (a new tensor)"""
    if u8.dim() != 4 or u8.dtype != torch.uint8 or u8.shape[1] not in (1, 3):
        raise ValueError("apply_host: images must be a uint8 [N, 1 or 3, H, W] tensor (got %s %s)" % (u8.dtype, tuple(u8.shape)))
    if u8.shape[2] < 3 or u8.shape[3] < 3:
        raise ValueError("apply_host: images must be at least 3 x 3 (got %s)" % (tuple(u8.shape),))
    if tuple(params.shape) != (u8.shape[0], ROW):
        raise ValueError("apply_host: params must be [%d, %d] (got %s)" % (u8.shape[0], ROW, tuple(params.shape)))
    a = u8.cpu().numpy()
    rows = params.detach().cpu().to(torch.float32).numpy()
    out = np.empty_like(a)
    for n in range(a.shape[0]):
        if a.shape[1] == 3:
            out[n] = apply_host_image(np.ascontiguousarray(a[n].transpose(1, 2, 0)), rows[n]).transpose(2, 0, 1)
        else:
            out[n, 0] = apply_host_image(a[n, 0], rows[n])
    return torch.from_numpy(out)
