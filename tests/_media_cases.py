"""Inputs shared by tests/test_media_cpu.py and tests/test_media_gpu.py: the shapes, the value patterns and the box sets that the media
renderer (the HIP kernel and its numpy twin) must reproduce byte for byte against tests/_media_oracle.py."""
import numpy as np
import torch

# (N, H, W, nrow): one pixel; the scalar path with odd sizes, three cells in one row; the wide path with a second grid row of one image
# and seven empty cells; W a multiple of 4 under an odd H; a one-column grid; a row wide enough that a canvas row is split into two units
SHAPES = [(1, 1, 1, 8), (3, 37, 53, 8), (9, 32, 64, 8), (2, 33, 16, 8), (2, 16, 48, 1), (2, 3, 1400, 8)]


def uniform(N, H, W, seed=0, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 3, H, W, generator=g) * (hi - lo) + lo


def levels(N, H, W):
    """Every k/255 and its two fp32 neighbours (the rounding boundaries of x*255 + 0.5 lie next to them), repeated over the batch."""
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    v = np.concatenate([k, np.nextafter(k, np.float32(2.0)), np.nextafter(k, np.float32(-1.0)),
                        (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0)]).astype(np.float32)
    n = N * 3 * H * W
    return torch.from_numpy(np.resize(v, n).reshape(N, 3, H, W).copy())


def special_channels(N, H, W, seed=1):
    """Channel 1 constant (must render 0), channel 2 with exactly two distinct values, channel 0 random with a negative offset."""
    x = uniform(N, H, W, seed, lo=-3.0, hi=5.0)
    x[:, 1] = 0.37
    g = torch.Generator().manual_seed(seed + 1)
    x[:, 2] = torch.where(torch.rand(N, H, W, generator=g) < 0.5, torch.tensor(0.25), torch.tensor(0.75))
    if H * W > 1:
        x[:, 2].reshape(N, -1)[:, 0] = 0.25
        x[:, 2].reshape(N, -1)[:, -1] = 0.75
    return x


def one_plane_view(N, H, W, seed=2):
    """A stride-0 three-channel view of a one-channel batch (what the IR batch is in the evaluation step)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 1, H, W, generator=g).expand(-1, 3, -1, -1)


def _ulp(v, up):
    return float(np.nextafter(np.float32(v), np.float32(2.0 if up else -1.0)))


def boxes(N, H, W, threshold):
    """-> (outputs, targets): per-image lists of dicts.  Image k shifts the set by k pixels."""
    t32 = float(np.float32(threshold))
    outputs, targets = [], []
    for k in range(N):
        ov = [W / 4 + k, H / 4, 3 * W / 4, 3 * H / 4 + k]                  # in both lists: red over yellow
        gt = [[0, 0, W - 1, H - 1],                                        # the image rectangle
              [1 + k, 1, W, H],                                            # x2 == W, y2 == H: far edges clipped away, near ones drawn
              [-0.7, -1.2, W / 2 + 0.3, H / 2 + 0.9 + k],                  # -0.7 -> 0, -1.2 -> -1
              [W + 5, H + 5, W + 20, H + 9],                               # wholly outside
              ov]
        det = [(ov, 0.9),
               ([W / 3 + k, 1, W / 3 + k, H - 2], 0.95),                   # x1 == x2
               ([W - 2, H - 2 - k, 2, 2], 0.8),                            # corners swapped
               ([-30, -30, -10, -10], 0.9),                                # wholly outside
               ([0.999, H / 2, W - 1.5, H / 2], t32),                      # score == fp32(threshold): not drawn (strict)
               ([W / 2, 0, W / 2 + 0.5, H - 1], _ulp(t32, True)),          # one ulp above: drawn
               ([1, 1, W / 2 - 1, H / 2 - 1], _ulp(t32, False)),           # one ulp below: not drawn
               ([2, 2, W - 3, H - 3], 0.1),
               ([-1.9, 3, W + 3.2, H / 3], 0.99)]                          # crosses both vertical borders
        outputs.append({"boxes": torch.tensor([b for b, _ in det], dtype=torch.float32).reshape(-1, 4),
                        "scores": torch.tensor([s for _, s in det], dtype=torch.float32),
                        "labels": torch.ones(len(det), dtype=torch.int64)})
        targets.append({"boxes": torch.tensor(gt[:len(gt) - (k % 2)], dtype=torch.float64).reshape(-1, 4),
                        "labels": torch.ones(len(gt) - (k % 2), dtype=torch.int64)})
    return outputs, targets


def padded(outputs, targets, extra=3, box_dtype=torch.float32):
    """The lists as the renderer takes them: det = (boxes [N, P, 4], scores [N, P], count [N]), gt = (boxes [N, Q, 4] f64, count [N]),
    with `extra` rows past every count filled with large garbage and a passing score: they must not be drawn."""
    N = len(targets)
    P = max(len(o["scores"]) for o in outputs) + extra
    Q = max(len(t["boxes"]) for t in targets) + extra
    db = torch.full((N, P, 4), 3.0e38, dtype=box_dtype)
    db[:, :, :2] = -3.0e38
    db[:, -1] = torch.tensor([0.0, 0.0, 1.0e9, 1.0e9])
    ds = torch.ones((N, P), dtype=torch.float32)
    gb = torch.full((N, Q, 4), 1.0e300, dtype=torch.float64)
    gb[:, :, :2] = -1.0e300
    gb[:, -1] = torch.tensor([0.0, 0.0, 2.0, 2.0], dtype=torch.float64)
    dc, gc = torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    for k in range(N):
        n, m = len(outputs[k]["scores"]), len(targets[k]["boxes"])
        db[k, :n], ds[k, :n], dc[k] = outputs[k]["boxes"].to(box_dtype), outputs[k]["scores"], n
        gb[k, :m], gc[k] = targets[k]["boxes"], m
    return (db, ds, dc), (gb, gc)
