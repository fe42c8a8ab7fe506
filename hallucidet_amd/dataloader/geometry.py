"""Paired geometric training augmentation: horizontal flip and a box-safe random crop resized back to the input's size, the same
transform for every image group of a sample (RGB and IR) and for its boxes.  The reference's HalluciDet training builds the slot for
it (train_hallucidet.py:519-524: an `alb.Compose` with `bbox_params` and `additional_targets`, pushed through
dataloaderPL.py:32-88) and leaves the slot empty; this is what fills it here.  The random draw is a small host record
(`PairedGeometry.params_for`: one int32 row per image) and the pixels move where they already are: in HBM through `ops.geometry_u8`
(csrc/geometry.hip, straight out of the dataset cache's arena when there is one), or on the host through `apply_host`, the same
arithmetic in numpy.

Definition (the one at the top of csrc/geometry.hip).  One record row per image: int32[8] = [flip, x0, y0, x1, y1, 0, 0, 0],
0 <= x0 < x1 <= W, 0 <= y0 < y1 <= H, cw = x1 - x0, ch = y1 - y0.  The output has the input's shape [N, C, H, W] (C = 1 or 3, every
channel alike): the bilinear resize (half-pixel centres, no antialias) of the crop window [x0, x1) x [y0, y1) of the horizontally
flipped image (of the image itself when flip = 0).  The crop is never larger than the image: always a magnification.
  position  integers: px = (2 ox + 1) cw - W, jx = floor(px / 2W) (towards -inf), rx = px - jx 2W; fx = fp32(rx) / fp32(2W), one IEEE
            division of two exactly representable operands; xa = clamp(jx, 0, cw-1), xb = clamp(jx+1, 0, cw-1).  y alike with ch, H.
  edges     taps are clamped to the crop (replicate), never read from outside it
  column    crop column k is source column s = x0 + k, and W - 1 - s when flip
  value     taps as fp32: t0 = v00 + fx (v01 - v00), t1 = v10 + fx (v11 - v10), v = t0 + fy (t1 - t0); every operation rounded once to
            fp32, no fused multiply-add
  byte      b = uint8(floor(v + 0.5f))
  modes     'u8': b;  'f32_ieee': fp32(b) / 255.0f, a true division
The record [0, 0, 0, W, H] returns the input bytes (jx = ox, fx = 0).

Boxes (xyxy) follow on the host in float64 and are cast back to the tensor's dtype; labels and every other key are untouched.
Flip: (W - x2, y1, W - x1, y2).  Crop: x' = (x - x0) * W / cw, y' = (y - y0) * H / ch, evaluated left to right.  Nothing is clipped
and no box is ever dropped: the draw only takes crops that contain every box as far as the box lies in the image.  The reference's
"all boxes gone -> un-augmented targets" fallback (dataloaderPL.py:84-85) therefore cannot trigger and has no counterpart here.

This is the box-safe idea of albumentations' RandomSizedBBoxSafeCrop, written out; bit-equality with that package is not claimed.
"""
import math

import numpy as np
import torch

from .augment import _mix

ROW = 8                              # int32 per image in hd_geometry_u8's record (HD_GEOM_ROW)
MAX_EXTENT = 16384                   # HD_GEOM_MAX_EXTENT: 2 W^2 stays inside int32
TAG = 0x67656F6D                     # 'geom': keeps these draws apart from the photometric ones of the same (seed, epoch, rank, batch)
f32 = np.float32


def make_row(flip=False, x0=0, y0=0, x1=None, y1=None, H=None, W=None):
    """One record row from explicit values (tests, tools); x1 / y1 default to W / H: the whole image."""
    x1 = W if x1 is None else x1
    y1 = H if y1 is None else y1
    if x1 is None or y1 is None:
        raise ValueError("make_row: give x1 and y1, or W and H for the whole image")
    return torch.tensor([int(bool(flip)), int(x0), int(y0), int(x1), int(y1), 0, 0, 0], dtype=torch.int32)


def check_rows(rows, n, H, W, what="geometry"):
    """Host validation of a record: int32 [n, ROW] on the CPU, every row inside the H x W image.  -> the rows, contiguous."""
    if not torch.is_tensor(rows) or rows.is_cuda or rows.dtype != torch.int32 or tuple(rows.shape) != (n, ROW):
        raise ValueError("%s: rows must be an int32 [%d, %d] tensor on the host (got %s %s on %s)"
                         % (what, n, ROW, getattr(rows, "dtype", type(rows)), tuple(getattr(rows, "shape", ())), getattr(rows, "device", "?")))
    if not (2 <= H <= MAX_EXTENT and 2 <= W <= MAX_EXTENT):
        raise ValueError("%s: need 2 <= H, W <= %d (got %d x %d)" % (what, MAX_EXTENT, H, W))
    r = rows.to(torch.int64)
    ok = ((r[:, 0] == 0) | (r[:, 0] == 1)) & (r[:, 1] >= 0) & (r[:, 1] < r[:, 3]) & (r[:, 3] <= W) & (r[:, 2] >= 0) & (r[:, 2] < r[:, 4]) \
        & (r[:, 4] <= H) & (r[:, 5:] == 0).all(dim=1)
    if not bool(ok.all()):
        bad = int((~ok).nonzero()[0])
        raise ValueError("%s: row %d = %s: need [flip in {0, 1}, x0, y0, x1, y1, 0, 0, 0] with 0 <= x0 < x1 <= %d and 0 <= y0 < y1 <= %d"
                         % (what, bad, rows[bad].tolist(), W, H))
    return rows.contiguous()


def _boxes_of(target):
    b = target.get("boxes") if isinstance(target, dict) else None
    if b is None or not torch.is_tensor(b) or b.numel() == 0:
        return np.zeros((0, 4), dtype=np.float64)
    return b.detach().cpu().to(torch.float64).reshape(-1, 4).numpy()


class PairedGeometry:
    """p_flip: probability of the horizontal flip; p_crop: probability of the box-safe crop (0: flip only); min_scale: the crop keeps at
    least ceil(min_scale * side) of each side.  `params_for` makes the record a pure function of (seed, epoch, rank, batch index) and
    of the batch's boxes."""

    def __init__(self, p_flip=0.5, p_crop=0.5, min_scale=0.5, seed=0, rank=0):
        for name, v in (("p_flip", p_flip), ("p_crop", p_crop)):
            if not 0 <= v <= 1:
                raise ValueError("%s must be a probability (got %r)" % (name, v))
        if not 0 < min_scale <= 1:
            raise ValueError("min_scale must lie in (0, 1] (got %r)" % (min_scale,))
        self.p_flip, self.p_crop, self.min_scale = float(p_flip), float(p_crop), float(min_scale)
        self.seed, self.rank, self.epoch = int(seed), int(rank), 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def generator(self, batch_index, epoch=None):
        return torch.Generator().manual_seed(_mix(self.seed, self.epoch if epoch is None else epoch, self.rank, batch_index, TAG))

    def params_for(self, targets_per_group, H, W, batch_index, epoch=None):
        """targets_per_group: one list of N host target dicts per image group (single-modal: one list; paired: RGB, IR) -> int32 [N, ROW].
        Per image six float64 uniforms u0..u5: flip = u0 < p_flip; the crop is taken when u1 < p_crop and the image has a box in any
        group.  The union of its boxes (all groups, after the flip, clipped to the image, rounded outward) is ux0, uy0, ux1, uy1; with
        mw = ceil(min_scale W): x0 uniform on 0 .. min(ux0, W - mw) from u2, x1 uniform on max(ux1, x0 + mw) .. W from u3, each as
        floor(u * count) clipped to count - 1; y alike from u4, u5."""
        groups = [list(g) for g in targets_per_group]
        if not groups or any(len(g) != len(groups[0]) for g in groups):
            raise ValueError("params_for: one target list of the same length per image group")
        n = len(groups[0])
        H, W = int(H), int(W)
        if not (2 <= H <= MAX_EXTENT and 2 <= W <= MAX_EXTENT):
            raise ValueError("params_for: need 2 <= H, W <= %d (got %d x %d)" % (MAX_EXTENT, H, W))
        u = torch.rand(n, 6, dtype=torch.float64, generator=self.generator(batch_index, epoch)).numpy()
        rows = np.zeros((n, ROW), dtype=np.int32)
        mw, mh = math.ceil(self.min_scale * W), math.ceil(self.min_scale * H)

        def pick(uu, lo, hi):
            count = hi - lo + 1
            return lo + min(int(math.floor(uu * count)), count - 1)
        for i in range(n):
            flip = bool(u[i, 0] < self.p_flip)
            x0, y0, x1, y1 = 0, 0, W, H
            boxes = np.concatenate([_boxes_of(g[i]) for g in groups], axis=0)
            if u[i, 1] < self.p_crop and len(boxes):
                bx0, bx1 = boxes[:, 0].min(), boxes[:, 2].max()
                if flip:
                    bx0, bx1 = W - bx1, W - bx0
                ux0 = int(min(max(math.floor(bx0), 0), W))
                ux1 = int(min(max(math.ceil(bx1), 0), W))
                uy0 = int(min(max(math.floor(boxes[:, 1].min()), 0), H))
                uy1 = int(min(max(math.ceil(boxes[:, 3].max()), 0), H))
                x0 = pick(u[i, 2], 0, min(ux0, W - mw))
                x1 = pick(u[i, 3], max(ux1, x0 + mw), W)
                y0 = pick(u[i, 4], 0, min(uy0, H - mh))
                y1 = pick(u[i, 5], max(uy1, y0 + mh), H)
            rows[i, :5] = (int(flip), x0, y0, x1, y1)
        return torch.from_numpy(rows)


def transform_boxes(boxes, row, H, W):
    """boxes: tensor [G, 4] xyxy; row: the image's record -> the boxes after flip and crop, same dtype and device (float64 arithmetic)"""
    flip, x0, y0, x1, y1 = (int(v) for v in row[:5])
    if boxes.numel() == 0 or (not flip and (x0, y0, x1, y1) == (0, 0, W, H)):
        return boxes.clone()
    b = boxes.detach().to(torch.float64).reshape(-1, 4)
    xa, ya, xb, yb = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    if flip:
        xa, xb = W - xb, W - xa
    cw, ch = x1 - x0, y1 - y0
    out = torch.stack([(xa - x0) * W / cw, (ya - y0) * H / ch, (xb - x0) * W / cw, (yb - y0) * H / ch], dim=1)
    return out.to(boxes.dtype).reshape(boxes.shape)


def transform_targets(rows, targets, H, W):
    """rows: int [N, ROW] on the host; targets: N target dicts -> N new dicts whose 'boxes' followed the image; every other key is the
    same object as before."""
    targets = list(targets)
    if len(targets) != int(rows.shape[0]):
        raise ValueError("transform_targets: %d rows for %d targets" % (int(rows.shape[0]), len(targets)))
    r = rows.tolist()
    out = []
    for t, row in zip(targets, r):
        t = dict(t)
        if torch.is_tensor(t.get("boxes")):
            t["boxes"] = transform_boxes(t["boxes"], row, int(H), int(W))
        out.append(t)
    return out


def _positions(n_out, c, extent):
    """per output coordinate: taps a, b in [0, c) and the fp32 weight of b"""
    o = np.arange(n_out, dtype=np.int64)
    p = (2 * o + 1) * c - extent
    d = 2 * extent
    j = np.floor_divide(p, d)
    f = (p - j * d).astype(f32) / f32(d)
    return np.clip(j, 0, c - 1), np.clip(j + 1, 0, c - 1), f


def resample_host_image(x, row):
    """x: uint8 [C, H, W]; row: the record -> the fp32 value v of every output pixel, before the rounding to a byte"""
    _, H, W = x.shape
    flip, x0, y0, x1, y1 = (int(v) for v in row[:5])
    xa, xb, fx = _positions(W, x1 - x0, W)
    ya, yb, fy = _positions(H, y1 - y0, H)
    sa, sb = x0 + xa, x0 + xb
    if flip:
        sa, sb = W - 1 - sa, W - 1 - sb
    ra, rb = x[:, y0 + ya, :].astype(f32), x[:, y0 + yb, :].astype(f32)
    v00, v01, v10, v11 = ra[:, :, sa], ra[:, :, sb], rb[:, :, sa], rb[:, :, sb]
    fx, fy = fx[None, None, :], fy[None, :, None]
    t0 = v00 + fx * (v01 - v00)
    t1 = v10 + fx * (v11 - v10)
    return t0 + fy * (t1 - t0)


def apply_host_image(x, row):
    """x: uint8 [C, H, W]; row: the record -> the transformed image, uint8 [C, H, W]"""
    return np.floor(resample_host_image(x, row) + f32(0.5)).astype(np.uint8)


def apply_host(u8, rows):
    """u8: uint8 tensor [N, C, H, W] on the CPU, C = 1 or 3; rows: int32 [N, ROW] -> the transformed batch (a new tensor)"""
    if u8.dim() != 4 or u8.dtype != torch.uint8 or u8.shape[1] not in (1, 3):
        raise ValueError("apply_host: images must be a uint8 [N, 1 or 3, H, W] tensor (got %s %s)" % (u8.dtype, tuple(u8.shape)))
    N, _, H, W = u8.shape
    rows = check_rows(rows.detach().cpu() if torch.is_tensor(rows) else rows, N, H, W, "apply_host").numpy()
    a = u8.cpu().numpy()
    out = np.empty_like(a)
    for n in range(N):
        out[n] = apply_host_image(a[n], rows[n])
    return torch.from_numpy(out)
