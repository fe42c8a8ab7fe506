"""Oracle of the detection media panels, restated from the reference's control flow: `Utils.normalize_image` + `plot_each_image`
(src/utils/utils.py:237-297: per-channel min / max through torch, the `if range != 0` branch, `(numpy * 255).astype("uint8")`, the
score filter `scores > threshold` in torch, `int()` corners, ground truths before detections), `show_bbox(..., label=None)` with
`cv2.rectangle(thickness=1)` written as its four clipped lines, torchvision's `save_image` quantisation for the raw panels and its
`make_grid(nrow, padding=2, pad_value=0)` placement.  Per-image Python loops on purpose; shares no code with the product
(`ops.media_render_host` is tested against this file, not imported by it)."""
import numpy as np
import torch

YELLOW, RED = (255, 255, 0), (255, 0, 0)


def normalise_u8(image):
    """[3, H, W] fp32 torch (CPU) -> uint8 HWC as plot_each_image:259-266 makes it."""
    image = image.detach().clone()
    mins = [image[idx].min() for idx in range(3)]
    maxs = [image[idx].max() for idx in range(3)]
    for idx in range(3):
        if maxs[idx] - mins[idx] != 0.0:
            image[idx] = (image[idx] - mins[idx]) / (maxs[idx] - mins[idx])
        else:
            image[idx] = 0.0
    return (image.numpy().transpose(1, 2, 0) * 255).astype("uint8").copy()


def quantise_u8(image):
    """[3, H, W] fp32 -> uint8 HWC as torchvision.utils.save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8)."""
    return image.detach().clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy().copy()


def _clipped_range(a, b, n):
    """range(a, b + 1) cut to 0..n-1 (clipped before looping: a corner may lie far outside)."""
    return range(max(a, 0), min(b, n - 1) + 1)


def rectangle(img, c1, c2, colour):
    """cv2.rectangle(img, c1, c2, colour, thickness=1): the four sides as lines, each clipped to the image."""
    H, W = img.shape[:2]
    (x1, y1), (x2, y2) = c1, c2
    for y in (y1, y2):
        if 0 <= y < H:
            for x in _clipped_range(min(x1, x2), max(x1, x2), W):
                img[y, x] = colour
    for x in (x1, x2):
        if 0 <= x < W:
            for y in _clipped_range(min(y1, y2), max(y1, y2), H):
                img[y, x] = colour


def show_bbox(img, bboxes, colour):
    """show_bbox:150-161 with label=None; thickness int(round(0.001 * max(H, W))) bumped from 0 to 1 must be 1."""
    tl = int(round(0.001 * max(img.shape[0:2])))
    tl = tl + 1 if tl == 0 else tl
    assert tl == 1
    for bbox in bboxes:
        c1, c2 = (int(bbox[0]), int(bbox[1])), (int(bbox[2]), int(bbox[3]))
        rectangle(img, c1, c2, colour)
    return img


def plot_each_image(image, output, target, threshold=0.5):
    """-> uint8 HWC (the reference returns this transposed and divided by 255.0)."""
    img = normalise_u8(image.cpu())
    if target is not None:
        img = show_bbox(img, target["boxes"].detach().cpu().numpy(), YELLOW)
    if output is not None:
        boxes_th = output["boxes"].detach().cpu()[output["scores"].detach().cpu() > threshold]
        if len(boxes_th) > 0:
            img = show_bbox(img, boxes_th.numpy(), RED)
    return img


def make_grid(tiles, nrow=8, padding=2):
    """torchvision.utils.make_grid on uint8 HWC tiles, pad_value 0; one tile is returned as it is."""
    n = len(tiles)
    if n == 1:
        return tiles[0]
    H, W = tiles[0].shape[:2]
    xmaps = min(nrow, n)
    ymaps = int(np.ceil(float(n) / xmaps))
    height, width = H + padding, W + padding
    grid = np.zeros((height * ymaps + padding, width * xmaps + padding, 3), dtype=np.uint8)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            grid[y * height + padding:y * height + padding + H, x * width + padding:x * width + padding + W] = tiles[k]
            k += 1
    return grid


def render(batch, mode, outputs=None, targets=None, threshold=0.5, nrow=8):
    """batch [N, 3, H, W] fp32 (any device); outputs / targets: per-image lists of dicts (boxes, scores) / (boxes) or None."""
    batch = batch.detach().cpu()
    tiles = []
    for k in range(batch.shape[0]):
        if mode == "quantise":
            tiles.append(quantise_u8(batch[k]))
        else:
            tiles.append(plot_each_image(batch[k], outputs[k] if outputs is not None else None,
                                         targets[k] if targets is not None else None, threshold))
    return make_grid(tiles, nrow=nrow)
