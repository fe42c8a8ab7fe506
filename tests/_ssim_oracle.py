"""Oracle of the structural loss (hd_ssim_loss), shared by tests/test_ssim_loss_cpu.py and tests/test_ssim_loss_gpu.py; not collected.

SSIM of Wang et al. 2004 in the common pytorch_msssim convention, written out (neither that package nor torchmetrics is a dependency):
window g[k] = exp(-(k-5)^2 / (2 * 1.5^2)) / sum, k = 0..10, computed in float64 and stored as fp32 (the oracle filters with those fp32
values, so every precision evaluates the same definition); separable, 'valid'; data range 1, C1 = 1e-4, C2 = 9e-4."""
import math

import torch
import torch.nn.functional as F

WIN = 11
C1, C2 = 1e-4, 9e-4
EPS = 2.0 ** -24
INPUT_KINDS = ("noise", "smooth", "equal_region", "constant", "near_black")


def window():
    """the 11 taps as the kernel holds them: float64 arithmetic, rounded to fp32 once"""
    g = [math.exp(-((k - 5) ** 2) / (2.0 * 1.5 * 1.5)) for k in range(WIN)]
    s = sum(g)
    return torch.tensor([v / s for v in g], dtype=torch.float64).to(torch.float32)


def gauss(t, dtype=torch.float64, filt="separable", full=False):
    """G * t per plane of t [N, C, H, W]: 'valid' -> [N, C, H-10, W-10]; full=True: the transposed ('full') correlation -> H+10, W+10.
    filt: 'separable' (a 1 x 11 then an 11 x 1 grouped convolution) or 'direct' (one 11 x 11 grouped convolution)."""
    C = t.shape[1]
    g = window().to(torch.float64)
    pad = WIN - 1 if full else 0
    t = t.to(dtype)
    if filt == "separable":
        kh = g.to(dtype).view(1, 1, 1, WIN).expand(C, 1, 1, WIN)
        kv = g.to(dtype).view(1, 1, WIN, 1).expand(C, 1, WIN, 1)
        return F.conv2d(F.conv2d(t, kh, groups=C, padding=(0, pad)), kv, groups=C, padding=(pad, 0))
    if filt == "direct":
        k2 = torch.outer(g, g).to(dtype).view(1, 1, WIN, WIN).expand(C, 1, WIN, WIN)
        return F.conv2d(t, k2, groups=C, padding=pad)
    raise ValueError(filt)


def _index(mx, my, mxx, myy, mxy):
    sx, sy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    A1, B1 = 2 * mx * my + C1, mx * mx + my * my + C1
    A2, B2 = 2 * sxy + C2, sx + sy + C2
    return A1 / B1, A2 / B2, B1, B2


def ssim_maps(x, y, dtype=torch.float64, filt="separable"):
    """S [N, 3, H-10, W-10] of x [N, 3, H, W] against y [N, 1 or 3, H, W] (one plane is compared against every channel)"""
    x = x.to(dtype)
    y = y.to(dtype).expand_as(x)
    l, cs, _, _ = _index(gauss(x, dtype, filt), gauss(y, dtype, filt), gauss(x * x, dtype, filt), gauss(y * y, dtype, filt),
                         gauss(x * y, dtype, filt))
    return l * cs


def grad_closed_form(x, y):
    """d sum(S) / d x in float64 by the closed form: (G (*) Pm) + 2x (G (*) Pxx) + y (G (*) Pxy), (*) the full correlation of the maps
    Pxx = -l cs / B2, Pxy = 2 l / B2, Pm = cs (2/B1)(mu_y - l mu_x) + l (2/B2)(cs mu_x - mu_y)"""
    x = x.double()
    y = y.double().expand_as(x)
    mx, my = gauss(x), gauss(y)
    l, cs, B1, B2 = _index(mx, my, gauss(x * x), gauss(y * y), gauss(x * y))
    pxx = -l * cs / B2
    pxy = 2 * l / B2
    pm = cs * (2 / B1) * (my - l * mx) + l * (2 / B2) * (cs * mx - my)
    return gauss(pm, full=True) + 2 * x * gauss(pxx, full=True) + y * gauss(pxy, full=True)


def moment_bound(x, y):
    """B(p) = sum_k |dS/dm_k|(p) * 24 * 2^-24 * (G*|t_k|)(p) + 16 * 2^-24 over the five moments t = (x, y, x^2, y^2, xy), in float64:
    the first-order effect on S of fp32 rounding in the filtered moments (22 taps plus the products), plus the pointwise formula's own
    rounding.  The partials come from autograd on the moment maps."""
    x = x.double()
    y = y.double().expand_as(x)
    ts = (x, y, x * x, y * y, x * y)
    ms = [gauss(t).detach().requires_grad_(True) for t in ts]
    l, cs, _, _ = _index(*ms)
    parts = torch.autograd.grad((l * cs).sum(), ms)
    b = torch.zeros_like(ms[0])
    for p, t in zip(parts, ts):
        b = b + p.abs() * (24 * EPS) * gauss(t.abs())
    return (b + 16 * EPS).detach()


def loss_and_grad64(hall, rgb, ir, w_rgb, w_ir, gs=1.0):
    """float64 autograd of the oracle: (SSIM_rgb, SSIM_ir, gs * d(w_rgb (1 - SSIM_rgb) + w_ir (1 - SSIM_ir)) / d hall)"""
    return loss_and_grad(hall, rgb, ir, w_rgb, w_ir, gs, torch.float64, "separable")


def loss_and_grad(hall, rgb, ir, w_rgb, w_ir, gs, dtype, filt):
    h = hall.detach().to(dtype).requires_grad_(True)
    sr = ssim_maps(h, rgb, dtype, filt).mean()
    si = ssim_maps(h, ir, dtype, filt).mean()
    (g,) = torch.autograd.grad((w_rgb * (1 - sr) + w_ir * (1 - si)) * gs, h)
    return float(sr), float(si), g


def make_inputs(kind, N, H, W, ir_planes, seed=0):
    """(hall, rgb, ir) fp32 CPU batches of one of INPUT_KINDS.  'equal_region': rgb == hall exactly on rows < ceil(0.6 H), columns
    < ceil(0.6 W) (see equal_interior)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(c):
        return torch.rand(N, c, H, W, generator=g)
    if kind == "noise" or kind == "equal_region":
        hall, rgb, ir = rnd(3), rnd(3), rnd(ir_planes)
        if kind == "equal_region":
            rh, rw = math.ceil(0.6 * H), math.ceil(0.6 * W)
            rgb[:, :, :rh, :rw] = hall[:, :, :rh, :rw]
    elif kind == "smooth":
        yy = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1) / max(H - 1, 1)
        xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W) / max(W - 1, 1)

        def img(c, ph):
            f = torch.arange(1, c + 1, dtype=torch.float32).view(1, c, 1, 1)
            base = 0.5 + 0.25 * torch.sin(6.0 * f * xx + ph) + 0.2 * torch.cos(4.0 * yy * f - ph)
            q = torch.round(base.expand(N, c, H, W).clamp(0, 1) * 255) / 255
            return (q + 0.02 * (rnd(c) - 0.5)).contiguous()
        hall, rgb, ir = img(3, 0.0), img(3, 0.3), img(ir_planes, 1.0)
    elif kind == "constant":
        def const(vals):
            return torch.tensor(vals, dtype=torch.float32).view(1, -1, 1, 1).expand(N, -1, H, W).contiguous()
        hall, rgb = const([0.25, 0.5, 0.8125]), const([0.25, 0.3, 0.1])
        ir = const([0.6, 0.5, 0.0][:ir_planes])
    elif kind == "near_black":
        hall, rgb, ir = rnd(3) * 0.01, rnd(3) * 0.01, rnd(ir_planes) * 0.01
    else:
        raise ValueError(kind)
    return hall.contiguous(), rgb.contiguous(), ir.contiguous()


def equal_interior(H, W):
    """rows, columns of the 'equal_region' pixels all of whose windows lie inside the region (the region starts at the image corner, where
    the valid grid clips the windows itself); empty unless the region is wider than the window"""
    rh, rw = math.ceil(0.6 * H), math.ceil(0.6 * W)
    return max(rh - (WIN - 1), 0), max(rw - (WIN - 1), 0)
