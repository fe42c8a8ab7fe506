"""Shapes, record rows and seeded images shared by the geometry tests (not collected)."""
import numpy as np
import torch

# H x W.  2 x 16, 5 x 32, 9 x 48: the wide path with one, two, three 16-byte vectors per row; 37 x 53 and 3 x 17: the byte path;
# 64 x 80: eight whole tiles of eight rows
SHAPES = ((2, 16), (5, 32), (9, 48), (37, 53), (3, 17), (64, 80))
KINDS = ("noise", "ramp", "zeros", "full")


def windows(H, W):
    """(name, x0, y0, x1, y1): the crop windows every shape is tested with"""
    ya, yb = (1, H - 1) if H > 2 else (0, H)               # an interior row range where the image has one
    return [("identity", 0, 0, W, H),
            ("corner_tl", 0, 0, 1, 1), ("corner_tr", W - 1, 0, W, 1), ("corner_bl", 0, H - 1, 1, H), ("corner_br", W - 1, H - 1, W, H),
            ("column", W // 3, 0, W // 3 + 1, H), ("row", 0, H // 2, W, H // 2 + 1),
            ("left", 0, ya, max(1, 2 * W // 3), yb), ("right", W // 3, ya, W, yb),
            ("top", 1, 0, W - 1, max(1, 2 * H // 3)), ("bottom", 1, H // 3, W - 1, H),
            ("half", W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2)]


def case_rows(H, W):
    """int32 [24, 8]: every window without and with the flip"""
    rows = [[flip, x0, y0, x1, y1, 0, 0, 0] for flip in (0, 1) for _, x0, y0, x1, y1 in windows(H, W)]
    return torch.tensor(rows, dtype=torch.int32)


def image(kind, n, c, H, W, seed=0):
    """uint8 [n, c, H, W]; no two noise / ramp planes alike"""
    if kind == "noise":
        return torch.randint(0, 256, (n, c, H, W), generator=torch.Generator().manual_seed(1000 * seed + 31 * H + W), dtype=torch.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        planes = [[(3 * x + 7 * y + 50 * ci + 11 * ni) % 256 for ci in range(c)] for ni in range(n)]
        return torch.from_numpy(np.array(planes, dtype=np.uint8))
    return torch.full((n, c, H, W), 0 if kind == "zeros" else 255, dtype=torch.uint8)


def chunks(rows, n):
    """the rows in batches of n, the last one filled up from the front"""
    k = rows.shape[0]
    return [rows[[(s + i) % k for i in range(n)]] for s in range(0, k, n)]
