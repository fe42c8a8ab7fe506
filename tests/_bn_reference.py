"""Float64 definitions of the BatchNorm kernel chain (csrc/elementwise.hip), input builders and the tolerances derived from the number
formats.  Shared by test_bn_reference_cpu.py (which checks these definitions against torch's own batch_norm and its autograd) and
test_bn_chain_gpu.py (which checks the HIP kernels against them).

Every ref_* function takes exactly the tensors the kernel takes -- the same fp16 / fp32 activations, the same fp32 per-channel
vectors, the same fp32 partial rows -- and evaluates the definition in float64, so the two sides differ by the kernel's own arithmetic
and nothing else.  Activations are [npix, C] (NHWC with the pixels flattened).

Tolerances (u16 = 2^-11, u32 = 2^-24: half an ulp, relative, of fp16 / fp32):

  element outputs (bn_apply, dy)   |got - ref| <= u16*|ref| + 2^-20*mag + 2^-25
      one fp16 round-to-nearest of the result (u16*|ref|), fewer than 16 fp32 roundings on the terms of the expression whose absolute
      values add up to `mag` (16*u32 = 2^-20), half the spacing of the fp16 subnormals (2^-25).  fp32 storage: u32 for u16, no floor.
  per-channel fp32 scalars          rtol 5e-7 (~8*u32: under four roundings, each <= u32, with room) where the value is a product /
      quotient; atol 5e-7 * (sum of the term magnitudes) where it is a sum (shift, running statistics).
  fp32 reductions on random data    |sum - ref| <= 1e-6 * sum|terms| per channel (~17*u32; three roundings per term for gk*xhat plus
      the pairwise-ish accumulation of the kernel's lanes measure ~2e-8 in an fp32 emulation; one dropped pixel in 2000 is 5e-4).
  colsum / rowsum (double accumulation, fp32 store, at most two stages)   3*u32 * sum|terms|.
  exact-integer data                torch.equal.
"""
import math

import numpy as np
import torch

U16 = 2.0 ** -11
U32 = 2.0 ** -24
SCALAR_RTOL = 5e-7
REDUCE_RTOL = 1e-6
COLSUM_RTOL = 3 * U32
MASK_MARGIN = 1e-3


def f32(v):
    """The value a kernel sees for a Python float passed as a C float."""
    return float(np.float32(v))


def _d(t):
    return None if t is None else t.detach().cpu().double()


# ------------------------------------------------------------------------------------------------------------------ definitions
def ref_finalize(part, count, gamma, beta, rm, rv, momentum, eps):
    """part [rows, 2C] (or [rows, 2, C]): rows of (sum, sum of squares).  Returns a dict of float64 vectors: mean, invstd, scale,
    shift (+ shift_mag), and with running statistics given their updated values running_mean / running_var (+ *_mag)."""
    p = _d(part)
    p = p.reshape(p.shape[0], 2, -1)
    s = p.sum(0)
    C = s.shape[1]
    count = float(count)
    m = s[0] / count
    var = torch.clamp(s[1] / count - m * m, min=0.0)
    invstd = 1.0 / torch.sqrt(var + f32(eps))
    g = _d(gamma) if gamma is not None else torch.ones(C, dtype=torch.float64)
    b = _d(beta) if beta is not None else torch.zeros(C, dtype=torch.float64)
    out = {"mean": m, "var": var, "invstd": invstd, "scale": g * invstd, "shift": b - m * g * invstd,
           "shift_mag": b.abs() + (m * g * invstd).abs()}
    if rm is not None:
        mom = f32(momentum)
        unbiased = var * count / (count - 1.0) if count > 1.0 else var
        out["running_mean"] = (1.0 - mom) * _d(rm) + mom * m
        out["running_mean_mag"] = ((1.0 - mom) * _d(rm)).abs() + (mom * m).abs()
        out["running_var"] = (1.0 - mom) * _d(rv) + mom * unbiased
        out["running_var_mag"] = ((1.0 - mom) * _d(rv)).abs() + (mom * unbiased).abs()
    return out


def ref_eval_scale_shift(gamma, beta, rm, rv, eps):
    rm, rv = _d(rm), _d(rv)
    g = _d(gamma) if gamma is not None else torch.ones_like(rm)
    b = _d(beta) if beta is not None else torch.zeros_like(rm)
    scale = g / torch.sqrt(rv + f32(eps))
    return {"scale": scale, "shift": b - rm * scale, "shift_mag": b.abs() + (rm * scale).abs()}


def ref_apply(y, scale, shift, res=None, relu=True):
    """-> (z, mag) in float64; mag = |y*scale| + |shift| + |res|."""
    y, sc, sh = _d(y), _d(scale), _d(shift)
    z = y * sc + sh
    mag = (y * sc).abs() + sh.abs()
    if res is not None:
        z = z + _d(res)
        mag = mag + _d(res).abs()
    if relu:
        z = torch.relu(z)
    return z, mag


def preactivation(y, mean, invstd, gamma, beta):
    """The forward's y*(gamma*invstd) + (beta - mean*gamma*invstd) in float64 from the fp32 vectors the backward kernels take."""
    y, m, i = _d(y), _d(mean), _d(invstd)
    g = _d(gamma) if gamma is not None else torch.ones_like(m)
    b = _d(beta) if beta is not None else torch.zeros_like(m)
    return y * (g * i) + (b - m * g * i)


def ref_mask(z, y, mean, invstd, gamma, beta, relu):
    if not relu:
        return torch.ones(y.shape, dtype=torch.bool)
    if z is not None:
        return _d(z) > 0
    return preactivation(y, mean, invstd, gamma, beta) > 0


def ref_bwd_sums(dz, z, y, mean, invstd, gamma, beta, relu):
    """Per channel sum gk and sum gk*xhat (xhat = (y - mean)*invstd), the sums of the terms' absolute values, and gk itself."""
    mask = ref_mask(z, y, mean, invstd, gamma, beta, relu)
    gk = torch.where(mask, _d(dz), torch.zeros((), dtype=torch.float64))
    xh = (_d(y) - _d(mean)) * _d(invstd)
    t = gk * xh
    return {"sg": gk.sum(0), "sgx": t.sum(0), "abs_sg": gk.abs().sum(0), "abs_sgx": t.abs().sum(0), "gk": gk, "mask": mask}


def ref_bwd_apply(dz, z, y, mean, invstd, gamma, beta, part, relu, gscale=1.0, dgamma_old=None, dbeta_old=None):
    """part [rows, 2C]: rows of (sum gk, sum gk*xhat).  dy = A*(gk - sum_g/M - xhat*sum_gx/M) with A = gamma*invstd, dres = gk,
    dgamma = gscale*sum_gx (+ old), dbeta = gscale*sum_g (+ old).  dy_mag: see the module docstring."""
    p = _d(part).sum(0)
    C = p.numel() // 2
    sg, sgx = p[:C], p[C:]
    yd, m, i = _d(y), _d(mean), _d(invstd)
    M = float(yd.shape[0])
    g = _d(gamma) if gamma is not None else torch.ones_like(m)
    mask = ref_mask(z, y, mean, invstd, gamma, beta, relu)
    gk = torch.where(mask, _d(dz), torch.zeros((), dtype=torch.float64))
    xh = (yd - m) * i
    A = g * i
    B = -A * i * sgx / M
    dy = A * (gk - sg / M - xh * sgx / M)
    mag = (A * gk).abs() + (A * sg / M).abs() + (A * xh * sgx / M).abs() + (B * m).abs()
    gs = f32(gscale)
    dgamma, dbeta = gs * sgx, gs * sg
    if dgamma_old is not None:
        dgamma = dgamma + _d(dgamma_old)
    if dbeta_old is not None:
        dbeta = dbeta + _d(dbeta_old)
    return {"dy": dy, "dy_mag": mag, "dres": gk, "dgamma": dgamma, "dbeta": dbeta}


# ------------------------------------------------------------------------------------------------------------------ tolerances
def elem_tol(ref, mag, dtype):
    if dtype == torch.float16:
        return U16 * ref.abs() + 2.0 ** -20 * mag + 2.0 ** -25
    assert dtype == torch.float32
    return U32 * ref.abs() + 2.0 ** -20 * mag


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol (tol > 0 elementwise, or 0 where got must equal ref); NaN / inf in got count as inf."""
    got, ref = _d(got), _d(ref)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    tol = tol.expand_as(err) if torch.is_tensor(tol) else torch.full_like(err, float(tol))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)      # 0/0 -> 0, x/0 -> inf
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------ builders
def random_inputs(npix, C, dtype, seed, *, with_z=False, with_res=False, affine=True):
    """Random BatchNorm-backward inputs in storage type `dtype`, conditioned for the recomputed ReLU mask: no float64 pre-activation
    lies within MASK_MARGIN of zero (elements that did were moved by +-0.25 in y), so the kernel's f16(fmaf(y, sc, sh)) > 0 and the
    float64 mask agree.  mean / invstd are the batch's own (rounded to fp32), gamma has mixed signs."""
    g = torch.Generator().manual_seed(seed)
    mu_c = torch.randn(C, generator=g, dtype=torch.float64)
    sd_c = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    y = (torch.randn(npix, C, generator=g, dtype=torch.float64) * sd_c + mu_c).to(dtype)
    yd = y.double()
    mean = yd.mean(0).float()
    invstd = (1.0 / torch.sqrt(yd.var(0, unbiased=False) + 0.05)).float()      # 0.05: a one-pixel batch keeps a finite invstd
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma = ((0.5 + torch.rand(C, generator=g)) * sign).float()
    beta = (0.5 * torch.randn(C, generator=g)).float()
    if not affine:
        gamma = beta = None
    for step in (0.25, -0.5, 0.75, -1.0):
        bad = preactivation(y, mean, invstd, gamma, beta).abs() < MASK_MARGIN
        if not bool(bad.any()):
            break
        y = torch.where(bad, (y.double() + step).to(dtype), y)
    d = {"y": y, "mean": mean, "invstd": invstd, "gamma": gamma, "beta": beta,
         "dz": torch.randn(npix, C, generator=g, dtype=torch.float64).to(dtype)}
    if with_z:       # the saved activation of a residual unit: any tensor with exact zeros will do
        d["z"] = torch.relu(torch.randn(npix, C, generator=g, dtype=torch.float64)).to(dtype)
    if with_res:
        d["res"] = torch.randn(npix, C, generator=g, dtype=torch.float64).to(dtype)
    return d


def mask_margin_violations(d):
    return int((preactivation(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"]).abs() < MASK_MARGIN).sum())


def integer_inputs(npix, C, dtype, seed, *, with_z=False):
    """Inputs whose backward sums are exact in fp32 in ANY summation order (npix <= 20 000): dz in {+-1..+-4}, y integers in [-8, 8],
    mean integers in [-2, 2], invstd and gamma in {0.5, 1, 2}, beta = integer + 0.125, z in {0, 1}.  Every pre-activation is a non-zero
    multiple of 0.125, every gk*xhat a multiple of 0.5 of magnitude <= 80, every partial sum below 2^24 * 0.5."""
    assert npix <= 20000
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    pick = lambda *shape: torch.tensor([0.5, 1.0, 2.0])[ri(0, 2, *shape)]
    dz = (ri(1, 4, npix, C) * (2 * ri(0, 1, npix, C) - 1)).to(dtype)
    d = {"y": ri(-8, 8, npix, C).to(dtype), "dz": dz, "mean": ri(-2, 2, C).float(), "invstd": pick(C), "gamma": pick(C),
         "beta": ri(-3, 3, C).float() + 0.125}
    if with_z:
        d["z"] = ri(0, 1, npix, C).to(dtype)
    return d


def sliced_stat_rows(y, rows):
    """[rows, 2C] fp32: y [npix, C] cut into `rows` contiguous slices (npix >= rows), each slice's sum and sum of squares taken in
    float64 and rounded to fp32 -- what the convolution epilogues hand to bn_finalize."""
    npix, C = y.shape
    assert npix >= rows
    seg = (torch.arange(npix) * rows) // npix
    yd = y.double()
    out = torch.zeros(rows, 2 * C, dtype=torch.float64)
    out[:, :C].index_add_(0, seg, yd)
    out[:, C:].index_add_(0, seg, yd * yd)
    return out.float()
