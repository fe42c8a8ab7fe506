"""Float64 definitions of the seven kernels of csrc/fcos.hip (GroupNorm forward / data gradient / parameter gradient, the centre-
sampling matcher, the FCOS losses and their gradients), input builders, fp32 emulations and the tolerances derived from them.  Shared
by test_fcos_reference_cpu.py (definitions against torch's group_norm / autograd and the CPU oracle, mutants, emulations) and
test_fcos_kernels_gpu.py (the HIP kernels against these definitions).

Every ref_* function takes exactly the tensors the kernel takes and evaluates the definition in float64.  GroupNorm activations are
[N, HW, C] (NHWC with the pixels flattened), a group is 8 consecutive channels, stat is [N, C/8, 2] = (mean, rstd) in fp32.

Tolerances.  U16, U32, SCALAR_RTOL, REDUCE_RTOL, worst_ratio and the element formula u16*|ref| + 2^-20*mag + 2^-25 (u32, no floor,
for fp32 storage) are _bn_reference's.  Two are new, both obtained on the CPU by evaluating the kernel's own expressions in numpy
float32 against the float64 definition and taking 4x the worst ratio (the emulation sees neither the device's rsqrtf / expf / logf /
powf nor its division; the library is built with -ffp-contract=off, so there is no fma to see):

  RSTD_RTOL = 2.5e-6    relative error of the returned rstd.  emu_gn_stats_f32(centred=True) adds in the fixed kernel's order (eight
      channels of a pixel, pixels p = lane, lane + PL, ..., then the PL lane partials in order; the mean first, then (x - mean)^2).
      Over GN_TABLE x {fp16, fp32} x N in {1, 3} and the two conditioning cases (derive_rstd_rtol) its worst relative error is 5.4e-7
      (fp32 storage, C = 8, HW = 1025: the 1 024-lane chain of same-sign terms); 4x is 2.2e-6, rounded up to 2.5e-6.  The condition
      RSTD_RTOL <= 2^-13 (a quarter of an fp16 half-ulp) holds with a factor 49 to spare.  The single-pass form tq/n - m*m measures
      1.1e-2 ... 6.4e-2 on the same conditioning cases at |mean|/std = 256 and 0.94 (rstd 18 instead of 316) on the group that is
      constant at 100.125 in the C = 256 case (test_fcos_reference_cpu.py asserts both).
  LOSS_RTOL = 1.1e-6    loss terms and loss-gradient elements, against `mag`: |got - ref| <= LOSS_RTOL*mag + LOSS_FLOOR.
      emu_fcos_losses_f32 evaluates the kernel's expressions; over LOSS_CASES (derive_loss_rtol) its worst (|err| - floor)/mag is
      focal 2.7e-7, d_cls 2.6e-7, d_ctr 1.2e-7, giou 5.8e-8, bce 5.8e-8, d_reg 2.8e-8; 4 x 2.7e-7 = 1.06e-6, rounded up to 1.1e-6.
      `mag` is the first-order error magnitude of the expression: the sum of the absolute values of its terms, where a difference
      that the kernel forms (q = 1 - p, x + ce, the argument of the logarithm near 1, U = Ap + Ag - I, ...) counts with BOTH operands
      (|1| + |p|, not |q|), and a product a*b counts |a|*mag(b) + mag(a)*|b|.  For the focal gradient at target 0 that is
      |w|*(|p| + gamma*((1 + p)*|x + ce| + q*(|x| + mag(ce))))*|gc|.  It judges a saturated logit on its absolute size: at x = 30,
      t = 1 fp32 (the kernel's and ATen's alike) gives q = 0 where float64 gives 9.4e-14.
      LOSS_FLOOR = 2^-118: an intermediate below the smallest normal fp32 (2^-126) may be flushed or keep no bits, and is multiplied
      by at most gamma*(|x| + ce)*|upstream| < 2^8.
  Loss values (sums over B*A locations): (LOSS_RTOL + REDUCE_RTOL) * sum(mag) / nfg + LOSS_FLOOR.
  GroupNorm mean: mean_rtol(HW, C) * mean|x|, with mean_rtol = max(REDUCE_RTOL, 4/3 * sqrt(L) * u32) and L = PL + 8*ceil(HW / PL) the
      longest chain of serial fp32 additions.  On same-sign data (|mean| >> std) the partial sums grow linearly, each addition errs
      uniformly within u32 * partial (rms u32/sqrt(3)), so the sum's relative error has rms u32*sqrt(L)/3: four of those.  Only the
      1 024-lane chains of C = 8 exceed REDUCE_RTOL (L = 1040: 2.6e-6; the emulation measures up to 9.8e-7 over seeds).  A dropped pixel
      in 1 025 of such a group is 1e-3.
  Parameter gradients: REDUCE_RTOL*|scale|*sum|terms| + SCALAR_RTOL*|prior|.
  Data gradient: element formula with mag = r*(|g*gamma| + |m1| + |xh*m2|), plus REDUCE_RTOL * r*(mean|g*gamma| + |xh|*mean|g*gamma*xh|)
  for the two group means inside it.
"""
import math

import numpy as np
import torch

from _bn_reference import U16, U32, SCALAR_RTOL, REDUCE_RTOL, worst_ratio, elem_tol, f32, _d      # noqa: F401  (re-exported)

RSTD_RTOL = 2.5e-6
LOSS_RTOL = 1.1e-6
LOSS_FLOOR = 2.0 ** -118
GN_EPS = 1e-5
GB = 1024                      # GroupNorm block

# (C, HW values): the loop edges of the 1 024-thread block (PL = 1024 / (C/8) pixel lanes)
GN_TABLE = [(8, (1, 1023, 1024, 1025)), (64, (127, 129)), (256, (1, 31, 32, 33, 100)), (1024, (7, 9, 17))]
GN_CONDITIONING = [(3, 100, 256), (10, 1025, 8)]      # (N, HW, C)
RATIOS = (0.0, 8.0, 64.0, 256.0)


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def _grp(t):
    """[N, HW, C] -> float64 [N, HW, C/8, 8]"""
    t = _d(t)
    return t.reshape(t.shape[0], t.shape[1], t.shape[2] // 8, 8)


def _stat(stat):
    s = _d(stat)
    return s[:, None, :, 0:1], s[:, None, :, 1:2]          # mean, rstd broadcast over [N, HW, G, 8]


def ref_gn_stats(x, eps=GN_EPS, *, _w=None):
    """Two-pass float64 statistics of the values as stored -> dict mean, var, rstd [N, C/8] and absmean (mean|x|).
    _w [HW]: pixel multiplicities (the CPU test's mutants; the divisor stays HW*8)."""
    xg = _grp(x)
    n = xg.shape[1] * 8
    w = torch.ones(xg.shape[1], dtype=torch.float64) if _w is None else _d(_w)
    w = w[None, :, None, None]
    mean = (xg * w).sum((1, 3)) / n
    var = (((xg - mean[:, None, :, None]) ** 2) * w).sum((1, 3)) / n
    return {"mean": mean, "var": var, "rstd": 1.0 / torch.sqrt(var + f32(eps)), "absmean": xg.abs().sum((1, 3)) / n}


def mean_rtol(HW, C):
    """Relative tolerance (against mean|x|) of the returned mean: see the module docstring."""
    PL = GB // (C // 8)
    return max(REDUCE_RTOL, 4.0 / 3.0 * math.sqrt(PL + 8 * -(-HW // PL)) * U32)


def stat_tensor(st):
    """ref_gn_stats' result as the fp32 [N, G, 2] tensor the kernels exchange."""
    return torch.stack([st["mean"], st["rstd"]], -1).float()


def ref_gn_apply(x, gamma, beta, stat, relu):
    """y = (x*(gamma*r) + (beta - m*gamma*r)) with the GIVEN stat -> (y, mag) float64 [N, HW, C]."""
    xg, (m, r) = _grp(x), _stat(stat)
    ga = _d(gamma).reshape(1, 1, -1, 8) * r
    be = _d(beta).reshape(1, 1, -1, 8)
    y = xg * ga + (be - m * ga)
    mag = (xg * ga).abs() + be.abs() + (m * ga).abs()
    if relu:
        y = torch.relu(y)
    return y.reshape(x.shape), mag.reshape(x.shape)


def _masked(dy, y, relu, shape):
    g = _grp(dy)
    if relu:
        g = torch.where(_grp(y) > 0, g, torch.zeros((), dtype=torch.float64))
    return g


def ref_gn_bwd(dy, x, y, gamma, stat, relu, *, _w=None):
    """dx = r*(gg - mean_grp(gg) - xh*mean_grp(gg*xh)), gg = dy*[y > 0]*gamma, xh = (x - m)*r -> dict dx, mag, red ([N, HW, C])."""
    xg, (m, r) = _grp(x), _stat(stat)
    gg = _masked(dy, y, relu, x.shape) * _d(gamma).reshape(1, 1, -1, 8)
    xh = (xg - m) * r
    n = xg.shape[1] * 8
    w = torch.ones(xg.shape[1], dtype=torch.float64) if _w is None else _d(_w)
    w = w[None, :, None, None]
    m1 = (gg * w).sum((1, 3), keepdim=True) / n
    m2 = (gg * xh * w).sum((1, 3), keepdim=True) / n
    a1 = gg.abs().sum((1, 3), keepdim=True) / n
    a2 = (gg * xh).abs().sum((1, 3), keepdim=True) / n
    dx = r * (gg - m1 - xh * m2)
    mag = r * (gg.abs() + m1.abs() + (xh * m2).abs())
    red = r * (a1 + xh.abs() * a2)
    return {"dx": dx.reshape(x.shape), "mag": mag.reshape(x.shape), "red": red.reshape(x.shape)}


def gn_bwd_tol(b, dtype):
    return elem_tol(b["dx"], b["mag"], dtype) + REDUCE_RTOL * b["red"]


def ref_gn_param_grad(dy, x, y, stat, scale, accumulate, prior=None, *, _w=None, _img=None):
    """dgamma[c] = scale * sum_{n,p} g*xh (+ prior[0]), dbeta[c] = scale * sum g (+ prior[1]); g = dy*[y > 0] (y None: no ReLU).
    -> dict dgamma, dbeta, tol_dgamma, tol_dbeta.  _w [N*HW] pixel multiplicities, _img [N*HW] the image whose statistics pixel i
    uses (the CPU test's mutants)."""
    N, HW, C = x.shape
    g = _masked(dy, y, y is not None, x.shape).reshape(N * HW, C // 8, 8)
    img = torch.arange(N * HW) // HW if _img is None else _img
    s = _d(stat)[img]                                              # [N*HW, G, 2]
    xh = (_d(x).reshape(N * HW, C // 8, 8) - s[:, :, 0:1]) * s[:, :, 1:2]
    w = (torch.ones(N * HW, dtype=torch.float64) if _w is None else _d(_w))[:, None, None]
    sc = f32(scale)
    out = {"dgamma": sc * (g * xh * w).sum(0).reshape(C), "dbeta": sc * (g * w).sum(0).reshape(C)}
    tg, tb = REDUCE_RTOL * abs(sc) * (g * xh).abs().sum(0).reshape(C), REDUCE_RTOL * abs(sc) * g.abs().sum(0).reshape(C)
    if accumulate:
        out["dgamma"], out["dbeta"] = out["dgamma"] + _d(prior[0]), out["dbeta"] + _d(prior[1])
        tg, tb = tg + SCALAR_RTOL * _d(prior[0]).abs(), tb + SCALAR_RTOL * _d(prior[1]).abs()
    out["tol_dgamma"], out["tol_dbeta"] = tg, tb
    return out


def emu_gn_stats_f32(x, eps=GN_EPS, centred=True):
    """groupnorm8_fwd_kernel's statistics in numpy float32, in the kernel's order of additions -> (mean, rstd) float32 [N, C/8].
    centred=True: the mean first, then the mean of (x - mean)^2.  centred=False: the single pass tq/n - m*m it replaces."""
    N, HW, C = x.shape
    vecs = C // 8
    PL = GB // vecs
    trips = -(-HW // PL)
    xp = np.zeros((N, trips * PL, vecs, 8), np.float32)
    xp[:, :HW] = x.float().numpy().reshape(N, HW, vecs, 8)
    xp = xp.reshape(N, trips, PL, vecs, 8)
    valid = (np.arange(trips * PL) < HW).reshape(1, trips, PL, 1)
    n = np.float32(HW * 8)

    def lanes(term):
        acc = np.zeros((N, PL, vecs), np.float32)
        for t in range(trips):
            for k in range(8):
                acc = acc + np.where(valid[:, t], term(xp[:, t, :, :, k]), np.float32(0))
        tot = np.zeros((N, vecs), np.float32)
        for i in range(PL):
            tot = tot + acc[:, i]
        return tot
    mean = lanes(lambda f: f) / n
    if centred:
        m = mean[:, None, :]
        var = lanes(lambda f: (f - m) * (f - m)) / n
    else:
        var = lanes(lambda f: f * f) / n - mean * mean
    var = np.maximum(var, np.float32(0))
    return mean, np.float32(1) / np.sqrt(var + np.float32(eps))


def gn_inputs(N, HW, C, dtype, seed):
    """Random GroupNorm inputs in storage type `dtype`: x with per-group mean ~ std, gamma of both signs, a beta that leaves about half
    the outputs under the ReLU, dy."""
    g = torch.Generator().manual_seed(seed)
    G = C // 8
    mu = torch.randn(N, 1, G, 1, generator=g, dtype=torch.float64)
    sd = 0.5 + 1.5 * torch.rand(N, 1, G, 1, generator=g, dtype=torch.float64)
    x = (torch.randn(N, HW, G, 8, generator=g, dtype=torch.float64) * sd + mu).reshape(N, HW, C).to(dtype)
    return _gn_rest(x, g, dtype)


def _gn_rest(x, g, dtype):
    C = x.shape[2]
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma = ((0.5 + torch.rand(C, generator=g)) * sign).float()
    beta = (0.3 * torch.randn(C, generator=g)).float()
    dy = torch.randn(x.shape, generator=g, dtype=torch.float64).to(dtype)
    return {"x": x, "gamma": gamma, "beta": beta, "dy": dy}


def gn_conditioning_inputs(N, HW, C, dtype, seed):
    """Groups drawn as mean = ratio*std, ratio cycling through RATIOS, std in [0.1, 1], both signs of the mean; the last two groups
    are constant at 100.125 (exact in fp16; the true variance is 0, rstd = 1/sqrt(f32(eps))) and at 0.  -> (inputs, ratio [N, G])
    with ratio -1 / -2 marking the two constant groups."""
    g = torch.Generator().manual_seed(seed)
    G = C // 8
    idx = torch.arange(N * G).reshape(N, G)
    ratio = torch.tensor(RATIOS, dtype=torch.float64)[idx % 4]
    sign = torch.where((idx // 4) % 2 == 0, 1.0, -1.0).double()
    sd = 0.1 + 0.9 * torch.rand(N, G, generator=g, dtype=torch.float64)
    x = torch.randn(N, HW, G, 8, generator=g, dtype=torch.float64) * sd[:, None, :, None] + (sign * ratio * sd)[:, None, :, None]
    x[N - 1, :, G - 1] = 100.125
    x[N - 1 if G > 1 else N - 2, :, G - 2 if G > 1 else 0] = 0.0
    ratio = ratio.clone()
    ratio[N - 1, G - 1] = -1.0
    ratio[N - 1 if G > 1 else N - 2, G - 2 if G > 1 else 0] = -2.0
    return _gn_rest(x.reshape(N, HW, C).to(dtype), g, dtype), ratio


def gn_integer_inputs(N, HW, C, dtype, seed):
    """Inputs on which every GroupNorm gradient sum is exact in fp32 in any order (N*HW*8 <= 2^15 per group): dy in +-{1..4}, x integers in
    [-8, 8], stat = (integer mean in [-2, 2], rstd 0.5), gamma in {0.5, 1, 2}, y in {0, 1} (a ReLU mask)."""
    assert N * HW * 8 <= 2 ** 15
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    G = C // 8
    stat = torch.stack([ri(-2, 2, N, G).float(), torch.full((N, G), 0.5)], -1)
    return {"x": ri(-8, 8, N, HW, C).to(dtype), "dy": (ri(1, 4, N, HW, C) * (2 * ri(0, 1, N, HW, C) - 1)).to(dtype),
            "y": ri(0, 1, N, HW, C).to(dtype), "gamma": torch.tensor([0.5, 1.0, 2.0])[ri(0, 2, C)], "stat": stat}


def derive_rstd_rtol(centred=True):
    """Worst relative error of the emulated rstd against ref_gn_stats over GN_TABLE x storage x N in {1, 3} and GN_CONDITIONING."""
    worst = 0.0
    for dtype in (torch.float16, torch.float32):
        cases = [(N, HW, C, None) for C, hws in GN_TABLE for HW in hws for N in (1, 3)] + [c + (1,) for c in GN_CONDITIONING]
        for N, HW, C, cond in cases:
            x = (gn_conditioning_inputs(N, HW, C, dtype, 7)[0] if cond else gn_inputs(N, HW, C, dtype, N * 100000 + HW * 10 + C))["x"]
            want = ref_gn_stats(x)["rstd"]
            got = torch.from_numpy(emu_gn_stats_f32(x, centred=centred)[1]).double()
            worst = max(worst, float(((got - want).abs() / want).max()))
    return worst


# ------------------------------------------------------------------------------------------------------------------ matcher
MATCH_MUTANTS = ("ge_radius", "ge_inside", "ge_lower", "ge_upper", "first_level_bounded", "last_index_wins", "gvalid_ignored")


def ref_match(anchors, gt, gvalid, first_n, last_start, radius, *, area_dtype=np.float32, mutant=None):
    """torchvision's FCOS.compute_loss assignment on float32 values: location a matches box j iff the centre distance (max norm) is
    < radius*size, the location lies strictly inside the box, and the largest side distance lies strictly in (lower, upper) with
    lower = 0 for a < first_n, else 4*size, and upper = inf for a >= last_start, else 8*size; among the matches the largest
    1e8 - area (evaluated in `area_dtype`: float32 is the specification) wins, the first index on ties; none -> -1.
    anchors [A, 4], gt [B, G, 4], gvalid [B, G] -> int64 [B, A]."""
    an = np.asarray(anchors, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.float32)
    gv = np.asarray(gvalid).astype(bool)
    A, (B, G) = an.shape[0], gt.shape[:2]
    two = np.float32(2)
    cx, cy, size = (an[:, 0] + an[:, 2]) / two, (an[:, 1] + an[:, 3]) / two, an[:, 2] - an[:, 0]
    ia = np.arange(A)
    lower = size * np.float32(4) if mutant == "first_level_bounded" else np.where(ia < first_n, np.float32(0), size * np.float32(4))
    upper = np.where(ia >= last_start, np.float32(np.inf), size * np.float32(8))
    rs = np.float32(radius) * size
    lt = (lambda a, b: a <= b) if mutant == "ge_radius" else (lambda a, b: a < b)
    inside = (lambda a: a >= 0) if mutant == "ge_inside" else (lambda a: a > 0)
    above = (lambda a, b: a >= b) if mutant == "ge_lower" else (lambda a, b: a > b)
    below = (lambda a, b: a <= b) if mutant == "ge_upper" else (lambda a, b: a < b)
    out = np.empty((B, A), np.int64)
    for b in range(B):
        best = np.zeros(A, area_dtype)
        bi = np.zeros(A, np.int64)
        for j in range(G):
            if not gv[b, j] and mutant != "gvalid_ignored":
                continue
            g = gt[b, j]
            gcx, gcy = (g[0] + g[2]) / two, (g[1] + g[3]) / two
            ok = lt(np.maximum(np.abs(cx - gcx), np.abs(cy - gcy)), rs)
            l, t, r, bt = cx - g[0], cy - g[1], g[2] - cx, g[3] - cy
            ok &= inside(np.minimum(np.minimum(l, t), np.minimum(r, bt)))
            dmax = np.maximum(np.maximum(l, t), np.maximum(r, bt))
            ok &= above(dmax, lower) & below(dmax, upper)
            area = (g[2] - g[0]) * (g[3] - g[1])
            val = np.where(ok, area_dtype(1e8) - area_dtype(area), area_dtype(0))
            take = (val >= best) if mutant == "last_index_wins" else (val > best)
            best = np.where(take, val, best)
            bi = np.where(take, j, bi)
        out[b] = np.where(best < 1e-5, -1, bi)
    return torch.from_numpy(out)


def pyramid(levels=((8, 8), (16, 4), (32, 2))):
    """Synthetic pyramid: per level (stride, n) an n x n grid of stride-sized square anchors centred at (stride*(i + 0.5), ...), x
    fastest.  -> (anchors [A, 4] float32, first_n, last_start)."""
    out = []
    for s, n in levels:
        c = (torch.arange(n, dtype=torch.float32) + 0.5) * s
        cy, cx = torch.meshgrid(c, c, indexing="ij")
        cx, cy = cx.flatten(), cy.flatten()
        out.append(torch.stack([cx - s / 2, cy - s / 2, cx + s / 2, cy + s / 2], 1))
    counts = [o.shape[0] for o in out]
    a = torch.cat(out)
    return a, counts[0], a.shape[0] - counts[-1]


# ------------------------------------------------------------------------------------------------------------------ losses
LOSS_MUTANTS = ("label_image0", "nfg_per_image", "nfg_unclamped", "giou_tie_one_side")


def _gather_targets(matched, gt, glab, mutant=None):
    m = matched.long()
    fg = m >= 0
    mc = m.clamp(min=0)
    gl = glab.long()
    if mutant == "label_image0":
        gl = gl[0:1].expand_as(gl)
    lab = torch.where(fg, gl.gather(1, mc), torch.full_like(mc, -1))
    box = _d(gt).gather(1, mc[..., None].expand(-1, -1, 4))
    return fg, lab, box


def ref_fcos_losses(cls_logits, bbox_regression, bbox_ctrness, matched, gt, glab, anchors, alpha=0.25, gamma=2.0, g3=(1.0, 1.0, 1.0), *,
                    mutant=None):
    """FCOSHead.compute_loss in float64 on the tensors hd_fcos_loss takes (cls [B, A, K], reg [B, A, 4], ctr [B, A], matched [B, A],
    gt [B, G, 4], glab [B, G], anchors [A, 4]) and, through float64 autograd, the gradients of g3 . (classification, bbox_regression,
    bbox_ctrness).  -> dict: losses [3], loss_tol [3], nfg, d_cls / d_reg / d_ctr with their *_mag, and the per-location terms
    focal / giou / bce with their *_mag."""
    x = _d(cls_logits).clone().requires_grad_(True)
    reg = _d(bbox_regression).clone().requires_grad_(True)
    c = _d(bbox_ctrness).reshape(x.shape[0], x.shape[1]).clone().requires_grad_(True)
    B, A, K = x.shape
    fg, lab, g = _gather_targets(matched, gt, glab, mutant)
    zero = torch.zeros((), dtype=torch.float64)
    t = (lab[..., None] == torch.arange(K)).double()
    # sigmoid focal
    p = torch.sigmoid(x)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    pt = p * t + (1 - p) * (1 - t)
    focal = ce if gamma == 0 else ce * (1 - pt) ** gamma
    if alpha >= 0:
        focal = (alpha * t + (1 - alpha) * (1 - t)) * focal
    # generalized IoU on BoxLinearCoder-decoded boxes
    an = _d(anchors)
    cx, cy, w, h = 0.5 * (an[:, 0] + an[:, 2]), 0.5 * (an[:, 1] + an[:, 3]), an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    x1, y1, x2, y2 = cx - reg[..., 0] * w, cy - reg[..., 1] * h, cx + reg[..., 2] * w, cy + reg[..., 3] * h
    even = mutant != "giou_tie_one_side"
    mx = torch.maximum if even else (lambda a, b: torch.where(a >= b, a, b))
    mn = torch.minimum if even else (lambda a, b: torch.where(a <= b, a, b))
    g0, g1, g2, g3_ = g.unbind(-1)
    ix1, iy1, ix2, iy2 = mx(x1, g0), mx(y1, g1), mn(x2, g2), mn(y2, g3_)
    has = (iy2 > iy1) & (ix2 > ix1)
    I = torch.where(has, (ix2 - ix1) * (iy2 - iy1), zero)
    garea = (g2 - g0) * (g3_ - g1)
    U = (x2 - x1) * (y2 - y1) + garea - I
    eps = 1e-7
    iou = I / (U + eps)
    Cc = (mx(x2, g2) - mn(x1, g0)) * (mx(y2, g3_) - mn(y1, g1))
    pen = (Cc - U) / (Cc + eps)
    giou = torch.where(fg, 1 - (iou - pen), zero)
    # centre-ness
    l, tt, r, bb = cx - g0, cy - g1, g2 - cx, g3_ - cy
    one = torch.ones((), dtype=torch.float64)
    safe = lambda v: torch.where(fg, v, one)
    l, tt, r, bb = safe(l), safe(tt), safe(r), safe(bb)
    ct = torch.sqrt((torch.minimum(l, r) / torch.maximum(l, r)) * (torch.minimum(tt, bb) / torch.maximum(tt, bb)))
    bce = torch.where(fg, torch.nn.functional.binary_cross_entropy_with_logits(c, ct, reduction="none"), zero)
    nfg_raw = float(fg.sum())
    if mutant == "nfg_per_image":
        dn = fg.sum(1).clamp(min=1).double()
        losses = torch.stack([(focal.sum((1, 2)) / dn).sum(), (giou.sum(1) / dn).sum(), (bce.sum(1) / dn).sum()])
        nfg = float(dn.max())
    else:
        nfg = nfg_raw if mutant == "nfg_unclamped" else max(1.0, nfg_raw)
        losses = torch.stack([focal.sum(), giou.sum(), bce.sum()]) / nfg
    gw = torch.tensor([f32(v) for v in g3], dtype=torch.float64)
    (losses * gw).sum().backward()
    out = {"losses": losses.detach(), "nfg": nfg, "d_cls": x.grad, "d_reg": reg.grad, "d_ctr": c.grad,
           "focal": focal.detach(), "giou": giou.detach(), "bce": bce.detach(), "fg": fg}
    if mutant is not None:
        return out
    with torch.no_grad():
        gc, gr, gt_ = (abs(float(v)) / nfg for v in gw)
        # focal: softplus terms m + log(e^-m + e^(-x-m)) (+1: the logarithm's argument lies in [1, 2] and carries an absolute u32)
        xd = x.detach()
        m = torch.clamp(-xd, min=0)
        sp = ce - (1 - t) * xd                                # softplus(-x): what the kernel calls ce
        sp_mag = m + (sp - m).abs() + 1
        q = 1 - p
        at = (alpha * t + (1 - alpha) * (1 - t)) if alpha >= 0 else torch.ones_like(t)
        pw = lambda b: torch.ones_like(b) if gamma == 0 else b ** gamma
        # value: ce_t * w;  t = 1: ce = sp, w = q^gamma;  t = 0: ce = x + sp, w = (1 - (1 - p))^gamma
        out["focal_mag"] = at * torch.where(t > 0, pw(q) * sp_mag, pw(p) * (xd.abs() + sp_mag))
        # gradient: t = 1: w*(-gamma*p*sp - q), w = q^gamma;  t = 0: w*(p + gamma*q*(x + sp)), w = p^gamma;  q = 1 - p counts 1 + p
        s0, s0_mag = xd + sp, xd.abs() + sp_mag
        mag1 = pw(q) * (gamma * p * sp_mag + (1 + p))
        mag0 = pw(p) * (p + gamma * ((1 + p) * s0.abs() + q * s0_mag))
        out["d_cls_mag"] = at * torch.where(t > 0, mag1, mag0) * gc
        # GIoU: every coordinate of the test inputs is exact in fp32, so the terms are those of the two quotients
        out["giou_mag"] = torch.where(fg, 1 + iou.abs() + pen.abs(), zero).detach()
        regd = reg.detach()
        X1, Y1, X2, Y2 = cx - regd[..., 0] * w, cy - regd[..., 1] * h, cx + regd[..., 2] * w, cy + regd[..., 3] * h
        pw_, ph_ = (X2 - X1).abs(), (Y2 - Y1).abs()
        iw, ih = torch.where(has, ix2 - ix1, zero).detach().abs(), torch.where(has, iy2 - iy1, zero).detach().abs()
        cw, ch = (torch.maximum(X2, g2) - torch.minimum(X1, g0)).abs(), (torch.maximum(Y2, g3_) - torch.minimum(Y1, g1)).abs()
        Ud, Id, Cd = U.detach().abs() + eps, I.detach().abs(), Cc.detach().abs() + eps
        Uterms = pw_ * ph_ + garea.abs() + Id
        mags = []
        for dAp, dI, dC, sz in ((ph_, ih, ch, w), (pw_, iw, cw, h), (ph_, ih, ch, w), (pw_, iw, cw, h)):
            dU = dAp + dI
            mags.append(sz * ((dI * Ud + Id * dU) / (Ud * Ud) + ((dC + dU) * Cd + (Cd + Uterms) * dC) / (Cd * Cd)) * gr)
        out["d_reg_mag"] = torch.where(fg[..., None], torch.stack(mags, -1), zero)
        cd = c.detach()
        mm = torch.clamp(-cd, min=0)
        spc = torch.nn.functional.softplus(-cd)
        out["bce_mag"] = torch.where(fg, (1 + ct) * cd.abs() + mm + (spc - mm).abs() + 1, zero)
        out["d_ctr_mag"] = torch.where(fg, torch.sigmoid(cd) + ct, zero) * gt_
        sums = torch.stack([out["focal_mag"].sum(), out["giou_mag"].sum(), out["bce_mag"].sum()])
        out["loss_tol"] = (LOSS_RTOL + REDUCE_RTOL) * sums / nfg + LOSS_FLOOR
    return out


def loss_tol(mag):
    return LOSS_RTOL * mag + LOSS_FLOOR


def emu_fcos_losses_f32(cls_logits, bbox_regression, bbox_ctrness, matched, gt, glab, anchors, alpha, gamma, g3, nfg):
    """The expressions of fcos_loss_fwd_kernel / fcos_loss_bwd_kernel (focal_value, focal_grad, giou_terms, ctr_target) in numpy
    float32, per location, before any summation -> dict focal, giou, bce, d_cls, d_reg, d_ctr (float32 arrays)."""
    F = np.float32
    x = cls_logits.float().numpy()
    B, A, K = x.shape
    fg, lab, box = _gather_targets(matched, gt, glab)
    fgn = fg.numpy()
    t = (lab[..., None] == torch.arange(K)).numpy()
    g = box.float().numpy()
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        p = F(1) / (F(1) + np.exp(-x))
        m = np.maximum(-x, F(0))
        ce = m + np.log(np.exp(-m) + np.exp(-x - m))
        pw = (lambda b: b * b) if gamma == 2.0 else (lambda b: np.power(b, F(gamma)))
        al = np.where(t, F(alpha), F(1) - F(alpha)) if alpha >= 0 else F(1)
        cet = np.where(t, ce, x + ce)
        pt = np.where(t, p, F(1) - p)
        focal = cet * pw(F(1) - pt) * al
        q = F(1) - p
        g1 = pw(q) * (-F(gamma) * p * ce - q)
        g0 = pw(p) * (p + F(gamma) * q * (x + ce))
        dn = F(nfg)
        gc, gr, gt_ = F(g3[0]) / dn, F(g3[1]) / dn, F(g3[2]) / dn
        d_cls = np.where(t, g1, g0) * al * gc
        an = anchors.float().numpy()
        cx, cy, w, h = F(0.5) * (an[:, 0] + an[:, 2]), F(0.5) * (an[:, 1] + an[:, 3]), an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
        d = bbox_regression.float().numpy()
        x1, y1, x2, y2 = cx - d[..., 0] * w, cy - d[..., 1] * h, cx + d[..., 2] * w, cy + d[..., 3] * h
        G0, G1, G2, G3 = g[..., 0], g[..., 1], g[..., 2], g[..., 3]
        eps = F(1e-7)
        ix1, iy1, ix2, iy2 = np.maximum(x1, G0), np.maximum(y1, G1), np.minimum(x2, G2), np.minimum(y2, G3)
        has = (iy2 > iy1) & (ix2 > ix1)
        iw, ih = ix2 - ix1, iy2 - iy1
        I = np.where(has, iw * ih, F(0))
        pw_, ph_ = x2 - x1, y2 - y1
        U = pw_ * ph_ + (G2 - G0) * (G3 - G1) - I
        iou = I / (U + eps)
        cw, ch = np.maximum(x2, G2) - np.minimum(x1, G0), np.maximum(y2, G3) - np.minimum(y1, G1)
        Cc = cw * ch
        giou = np.where(fgn, F(1) - (iou - (Cc - U) / (Cc + eps)), F(0))
        share = lambda a, b, a_wins_if_greater: np.where(a == b, F(0.5), np.where((a > b) == a_wins_if_greater, F(1), F(0)))
        dAp = (-ph_, -pw_, ph_, pw_)
        z = np.zeros_like(I)
        dI = (np.where(has, -ih * share(x1, G0, True), z), np.where(has, -iw * share(y1, G1, True), z),
              np.where(has, ih * share(x2, G2, False), z), np.where(has, iw * share(y2, G3, False), z))
        dC = (-ch * share(x1, G0, False), -cw * share(y1, G1, False), ch * share(x2, G2, True), cw * share(y2, G3, True))
        sgn_sz = (-w, -h, w, h)
        d_reg = np.zeros_like(d)
        for k in range(4):
            dU = dAp[k] - dI[k]
            diou = (dI[k] * (U + eps) - I * dU) / ((U + eps) * (U + eps))
            dpen = ((dC[k] - dU) * (Cc + eps) - (Cc - U) * dC[k]) / ((Cc + eps) * (Cc + eps))
            d_reg[..., k] = np.where(fgn, sgn_sz[k] * (-diou + dpen) * gr, F(0))
        l, tt, r, bb = cx - G0, cy - G1, G2 - cx, G3 - cy
        ct = np.sqrt((np.minimum(l, r) / np.maximum(l, r)) * (np.minimum(tt, bb) / np.maximum(tt, bb)))
        c = bbox_ctrness.float().numpy().reshape(B, A)
        mm = np.maximum(-c, F(0))
        bce = np.where(fgn, (F(1) - ct) * c + mm + np.log(np.exp(-mm) + np.exp(-c - mm)), F(0))
        d_ctr = np.where(fgn, (F(1) / (F(1) + np.exp(-c)) - ct) * gt_, F(0))
    return {"focal": focal, "giou": giou, "bce": bce, "d_cls": d_cls, "d_reg": d_reg, "d_ctr": d_ctr}


# (B, A, K, alpha, gamma, g3, foreground): the forward's single and second trip (B*A = 16 384 / 16 386), the same for the backward's
# 256-block cap (65 536 / 65 538), every (alpha, gamma), one loss alone and all three unequally weighted, one batch without foreground
LOSS_CASES = [
    (2, 8192, 1, 0.25, 2.0, (0.7, 1.3, 2.1), True),
    (2, 8193, 3, 0.6, 1.5, (1.0, 0.0, 0.0), True),
    (2, 8193, 1, -1.0, 0.0, (0.0, 1.0, 0.0), True),
    (2, 8193, 3, 0.25, 2.0, (0.0, 0.0, 1.0), True),
    (2, 8193, 3, 0.25, 2.0, (0.7, 1.3, 2.1), False),
    (2, 32768, 2, 0.6, 1.5, (0.7, 1.3, 2.1), True),
    (2, 32769, 2, 0.25, 2.0, (0.7, 1.3, 2.1), True),
    (2, 32769, 2, -1.0, 0.0, (2.1, 0.7, 1.3), True),
]

# target ltrb (pixels) and predicted ltrb (pixels) of the deliberate geometry / centre-ness slots; the rest are random half-integers
_GEOMETRY = [
    ((6.0, 9.0, 14.0, 5.0), (6.0, 9.0, 14.0, 5.0)),         # prediction identical to the target (every max / min a tie)
    ((6.0, 9.0, 14.0, 5.0), (0.0, 0.0, 0.0, 0.0)),          # zero-area prediction
    ((6.0, 9.0, 14.0, 5.0), (-40.0, 3.0, 50.0, 3.0)),       # disjoint (a negative ltrb puts the prediction beside the location)
    ((6.0, 9.0, 14.0, 5.0), (10.5, 12.0, 20.0, 7.5)),       # prediction contains the target
    ((6.0, 9.0, 14.0, 5.0), (2.5, 4.0, 7.0, 1.5)),          # prediction contained in the target
    ((6.0, 9.0, 14.0, 5.0), (6.0, 4.0, 20.0, 2.5)),         # one shared edge (left)
    ((7.0, 7.0, 7.0, 7.0), (3.0, 9.5, 8.0, 2.0)),           # location at the box centre: centre-ness target 1
    ((5.0, 3.5, 5.0, 12.0), (5.0, 1.0, 2.0, 12.0)),         # l == r tie in the centre-ness target; l and b shared with the prediction
    ((0.5, 20.0, 31.5, 9.0), (1.0, 18.0, 30.0, 10.0)),      # location half a unit from a side
]


def loss_inputs(B, A, K, seed, foreground=True):
    """Synthetic FCOS loss inputs with every coordinate a multiple of 0.5 (anchor sizes 8 / 16 / 32, ltrb in pixels / size), so that
    box arithmetic is exact in fp32 and ties are ties on both sides.  Foreground is sparse (about 40 locations per image, each with
    its own box slot), includes the first two and the last two locations of every image, and the two images carry different boxes and
    labels at the same slot.  Logits are 3*randn with +-30, +-100 and a sweep of [-40, 40] written over some, on both target values."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    a = torch.arange(A)
    size = torch.tensor([8.0, 16.0, 32.0])[a % 3]
    cx, cy = size * (0.5 + (a // 3) % 16), size * (0.5 + (a // 48) % 16)
    anchors = torch.stack([cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2], 1)
    G = 40
    matched = torch.full((B, A), -1, dtype=torch.int64)
    gt = torch.zeros(B, G, 4)
    glab = ri(0, K - 1, B, G)
    if K > 1:
        glab[1] = (glab[0] + 1) % K                       # the same slot carries another label in the second image
    reg = ri(0, 160, B, A, 4).float() * 0.5 / size[None, :, None]
    if foreground:
        for b in range(B):
            rest = 2 + torch.randperm(A - 4, generator=g)[:G - 4] if A > 4 else torch.zeros(0, dtype=torch.int64)
            locs = torch.cat([torch.tensor([0, 1, A - 2, A - 1]), rest])[:G]
            for j, loc in enumerate(locs.tolist()):
                k = j - 4 + b                                # the images meet the geometry table one slot apart
                if 0 <= k < len(_GEOMETRY):
                    tg, pr = _GEOMETRY[k]
                    reg[b, loc] = torch.tensor(pr) / size[loc]
                else:
                    tg = (ri(1, 80, 4).float() * 0.5).tolist()
                gt[b, j] = torch.tensor([cx[loc] - tg[0], cy[loc] - tg[1], cx[loc] + tg[2], cy[loc] + tg[3]])
                matched[b, loc] = j
    cls = 3 * torch.randn(B, A, K, generator=g)
    flat = cls.view(-1)
    n = flat.numel()
    sweep = torch.linspace(-40.0, 40.0, 641)
    flat[5:5 + 641] = sweep[:max(0, min(641, n - 5))]
    flat[n - 700:n - 700 + 641] = sweep
    special = torch.tensor([30.0, -30.0, 100.0, -100.0])
    flat[700:704] = special
    if foreground:                                           # the label's own logit (target 1) at foreground locations: saturated and swept
        for b in range(B):
            locs = torch.nonzero(matched[b] >= 0).flatten()
            for i, loc in enumerate(locs.tolist()):
                lab = int(glab[b, matched[b, loc]])
                cls[b, loc, lab] = float(special[i % 4]) if i < 8 else float(-40.0 + 80.0 * torch.rand((), generator=g))
    ctr = 2 * torch.randn(B, A, generator=g)
    ctr.view(-1)[:4] = special
    ctr[B - 1, A - 2:] = torch.tensor([30.0, -30.0])
    return {"anchors": anchors, "gt": gt, "glab": glab, "matched": matched, "cls": cls, "reg": reg, "ctr": ctr}


def derive_loss_rtol():
    """Worst (|emulation - definition| - LOSS_FLOOR) / mag over LOSS_CASES, per output -> dict."""
    worst = {}
    for ci, (B, A, K, alpha, gamma, g3, fgd) in enumerate(LOSS_CASES):
        d = loss_inputs(B, A, K, 100 + ci, fgd)
        ref = ref_fcos_losses(d["cls"], d["reg"], d["ctr"], d["matched"], d["gt"], d["glab"], d["anchors"], alpha, gamma, g3)
        emu = emu_fcos_losses_f32(d["cls"], d["reg"], d["ctr"], d["matched"], d["gt"], d["glab"], d["anchors"], alpha, gamma, g3, ref["nfg"])
        for k in ("focal", "giou", "bce", "d_cls", "d_reg", "d_ctr"):
            err = (torch.from_numpy(emu[k]).double() - ref[k]).abs()
            if not bool(torch.isfinite(err).all()):
                worst[k] = math.inf
                continue
            mag = ref[k + "_mag"]
            r = torch.where(err <= LOSS_FLOOR, torch.zeros_like(err), (err - LOSS_FLOOR) / mag)
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
    return worst


# ------------------------------------------------------------------------------------------------------------------ matcher edge table
RADIUS = 1.5
G_SLOTS = 5


def match_edge_cases():
    """The matcher's strict inequalities and tie rules, each reached on purpose.  Three-level pyramid of pyramid(): level 0 (stride 8)
    a = 8*iy + ix at (8*ix + 4, 8*iy + 4), level 1 (stride 16) a = 64 + 4*iy + ix at (16*ix + 8, 16*iy + 8), level 2 (stride 32)
    a = 80 + 2*iy + ix at (32*ix + 16, 32*iy + 16); first_n = 64, last_start = 80.  Location 27 is (28, 28), size 8, radius*size 12;
    location 69 is (24, 24), size 16, bounds (64, 128), radius*size 24.  `one` is the one-level pyramid (stride 32, 2 x 2, first_n = A,
    last_start = 0: every location is first AND last level); its location 0 is (16, 16).
    -> list of dicts: name, anchors, first_n, last_start, gt [2, 5, 4], gvalid [2, 5], expect {(image, location): index}; the
    expectations are worked out by hand from the rule, not computed."""
    three, one = pyramid(), pyramid(((32, 2),))
    cases = []

    def add(name, img0, img1, expect, pyr=three, invalid=()):
        gt = torch.zeros(2, G_SLOTS, 4)
        gv = torch.zeros(2, G_SLOTS, dtype=torch.uint8)
        for b, boxes in enumerate((img0, img1)):
            for j, box in enumerate(boxes):
                gt[b, j] = torch.tensor(box, dtype=torch.float32)
                gv[b, j] = 0 if (b, j) in invalid else 1
        cases.append({"name": name, "anchors": pyr[0], "first_n": pyr[1], "last_start": pyr[2], "gt": gt, "gvalid": gv, "expect": expect})
    # (28, 28) lies ON the left side (l = 0): not inside.  Its right neighbour (36, 28): l = 8, t = 8, r = 4, b = 8
    add("on_a_side", [(28, 20, 40, 36)], [], {(0, 27): -1, (0, 28): 0})
    # box centre (40, 28): distance exactly 12 = radius*size -> no;  centre (39.5, 28): 11.5 -> yes
    add("radius", [(26, 16, 54, 40)], [(25, 16, 54, 40)], {(0, 27): -1, (1, 27): 0})
    # middle level, l = dmax = 64 = 4*size (centre (2, 24), distance 22 < 24) -> no;  l = 64.5 -> yes
    add("dmax_lower", [(-40, 14, 44, 34)], [(-40.5, 14, 44, 34)], {(0, 69): -1, (1, 69): 0})
    # middle level, l = dmax = 128 = 8*size (centre (5, 24), distance 19) -> no;  l = 127.5 -> yes
    add("dmax_upper", [(-104, 14, 114, 34)], [(-103.5, 14, 114, 34)], {(0, 69): -1, (1, 69): 0})
    # first level: dmax = 3 < 4*size = 32, matched all the same;  last level (16, 16): dmax = 300 > 8*size = 256, matched all the same
    add("open_ends", [(26, 26, 30, 31)], [(-284, 0, 306, 30)], {(0, 27): 0, (1, 80): 0})
    # 63 = first_n - 1 (60, 60) takes a small box, 64 = first_n (8, 8) does not (dmax = 2 <= 64);  79 = last_start - 1 (56, 56) refuses
    # dmax = 300 >= 128, 80 = last_start (16, 16; l = 260, t = 10, r = 336, b = 64; centre (54, 43), distance 38 < 48) takes it
    add("level_boundaries", [(58, 58, 62, 63), (6, 6, 10, 10)], [(-244, 6, 352, 80)], {(0, 63): 0, (0, 64): -1, (1, 79): -1, (1, 80): 0})
    # two boxes contain (28, 28): areas 400 and 81, the smaller wins in either slot order
    add("smaller_area", [(20, 20, 40, 40), (24, 24, 33, 33)], [(24, 24, 33, 33), (20, 20, 40, 40)], {(0, 27): 1, (1, 27): 0})
    add("identical_boxes", [(20, 20, 40, 40), (20, 20, 40, 40)], [], {(0, 27): 0})
    # area 1001 (13 x 77) in slot 0, area 1000 (40 x 25) in slot 1: float32(1e8 - 1001) == 1e8 - 1000 == 99 999 000 (spacing 8): a tie,
    # the first index wins -- exact arithmetic would give slot 1
    add("fp32_area_tie", [(10, -20, 23, 57), (0, 4, 40, 29)], [], {(0, 0): 0}, pyr=one)
    # the tiny box in slot 1 would win, but its slot is invalid
    add("invalid_slot", [(20, 20, 40, 40), (26, 26, 30, 30)], [], {(0, 27): 0}, invalid={(0, 1)})
    # zero width: l = r = 0, never inside;  the other image has no valid slot at all
    add("zero_width_and_no_valid", [(28, 20, 28, 40)], [(20, 20, 40, 40)], {(0, 27): -1, (1, 27): -1}, invalid={(1, 0)})
    return cases


def match_random_inputs(A, G, seed, levels=((8, 16), (16, 8), (32, 4))):
    """The first A locations of a pyramid (A = None: all of it) and B = 2 images of G random half-integer boxes, some slots invalid.
    first_n / last_start are the pyramid's, clipped to A."""
    an, first_n, last_start = pyramid(levels)
    if A is not None:
        an = an[:A]
        first_n, last_start = min(first_n, A), min(last_start, A)
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(-20, 200, (2, G, 2), generator=g).float() * 0.5
    wh = torch.randint(0, 260, (2, G, 2), generator=g).float() * 0.5
    gv = (torch.rand(2, G, generator=g) < 0.8).to(torch.uint8)
    gv[0, 0] = 1
    return {"anchors": an, "first_n": first_n, "last_start": last_start, "gt": torch.cat([xy, xy + wh], -1), "gvalid": gv}
