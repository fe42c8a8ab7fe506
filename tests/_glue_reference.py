"""Float64 / exact-integer definitions of the pooling, resampling and layout kernels of csrc/elementwise.hip (everything in that file
that is not the BatchNorm chain), input builders and the tolerance derived from the number formats.  Shared by
test_glue_reference_cpu.py (which checks these definitions against ATen's max_pool2d / interpolate / cat and their autograd) and
test_glue_kernels_gpu.py (which checks the HIP kernels against them).

Every ref_* function takes exactly the CPU copies of the tensors the kernel takes: activations NHWC [N, H, W, C] in the storage type
(float16 or float32), images NCHW float32.  Functions that return a stored tensor return it in the storage type, rounded ONCE from the
float64 value (twice where the kernel documents two roundings); the *_terms functions return the float64 value and the sum of the
absolute values of its addends, for the tolerance below.

Exactness.  grid_inputs() draws multiples of 2^-6 in [-16, 16]: integers n * 2^-6 with |n| <= 2^10.  A sum of k of them is an integer
multiple of 2^-6 below k * 2^10 units, so for k < 2^14 every partial sum in ANY order fits fp32's 24-bit significand: the kernel's fp32
accumulation is exact and differs from the float64 reference by the one identical rounding to the storage type.  (torch rounds
float64 -> float16 through float32; the value is exact in float32, so that is one rounding too.)  Those cases use torch.equal.  The
largest count here is 169 (the 13 x 13 preimage of a 6 -> 74 resize) plus one accumulated value.

Tolerance for sums of k addends on wild_inputs() (u = U16 for fp16 storage, U32 for fp32 storage):

    |got - ref| <= u * |ref| + (k + 2) * U32 * sum|terms| + 2^-25

one rounding to the storage type, at most k fp32 roundings of partial sums (each below sum|terms|) with room for a scale factor, half
the spacing of the fp16 subnormals.  Where the kernel documents a second storage rounding of an intermediate value m (the max-pool
backward's `add` form), u * |m| is added.
"""
import numpy as np
import torch

from _bn_reference import U16, U32, f32, worst_ratio  # noqa: F401  (re-exported for the tests)

# (input size, output size) pairs at which the fp32 index floorf(dst * (float)in / out) differs from the exact rational index
DIVERGENT_PAIRS = [(26, 22), (39, 33), (14, 46), (21, 69), (6, 74)]
# every (in, out) pair of the resize tests (nchw_to_nhwc_resize, its adjoint): the divergent ones, 1 -> 5, 5 -> 1, identity
RESIZE_PAIRS = DIVERGENT_PAIRS + [(1, 5), (5, 1), (7, 7)]
# (low-resolution size, output size) pairs of the upsample_add tests
UPSAMPLE_PAIRS = [(10, 19), (14, 46), (21, 69), (5, 10), (1, 3), (6, 6)]
# pairs of the cases sized past the 4096-block grid cap
CAP_PAIRS = [(303, 607), (864, 1728), (607, 607), (1728, 1800), (304, 607), (432, 864), (864, 1727)]
ALL_PAIRS = RESIZE_PAIRS + UPSAMPLE_PAIRS + CAP_PAIRS


def _d(t):
    return t.detach().cpu().double()


def _unit(dtype):
    assert dtype in (torch.float16, torch.float32)
    return U16 if dtype == torch.float16 else U32


def sum_tol(ref, abs_terms, k, dtype, extra=None):
    """The module docstring's bound, elementwise; `extra`: float64 magnitude of a value the kernel rounds to storage on the way."""
    tol = _unit(dtype) * ref.abs() + (k + 2) * U32 * abs_terms + 2.0 ** -25
    if extra is not None:
        tol = tol + _unit(dtype) * extra.abs()
    return tol


# ------------------------------------------------------------------------------------------------------------------ max-pool 3x3 / 2 / 1
def pool_out(h):
    return (h - 1) // 2 + 1


def _padded(N, H, W, C, fill):
    """[N, 2*Ho + 1, 2*Wo + 1, C] float64: input pixel (h, w) lives at (h + 1, w + 1); window (ho, wo) position (kh, kw) is the
    strided view [kh::2, kw::2] cut to Ho x Wo."""
    return torch.full((N, 2 * pool_out(H) + 1, 2 * pool_out(W) + 1, C), fill, dtype=torch.float64)


def ref_maxpool(x):
    """-> (y in x's dtype, pos uint8): the window maximum and the position kh*3 + kw of its FIRST occurrence in (kh, kw) scan order.
    Nine shifted views of the -inf padded input, strict-greater scan.  Finite inputs."""
    N, H, W, C = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    pad = _padded(N, H, W, C, -float("inf"))
    pad[:, 1:H + 1, 1:W + 1] = _d(x)
    best = torch.full((N, Ho, Wo, C), -float("inf"), dtype=torch.float64)
    pos = torch.full((N, Ho, Wo, C), 255, dtype=torch.uint8)
    for kh in range(3):
        for kw in range(3):
            v = pad[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
            take = v > best
            best = torch.where(take, v, best)
            pos = torch.where(take, torch.full_like(pos, kh * 3 + kw), pos)
    return best.to(x.dtype), pos


def ref_maxpool_bwd_terms(pos, dy, H, W):
    """-> (routed, abs_terms) float64 [N, H, W, C]: every dy element goes to the input pixel its window's `pos` names."""
    N, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == (pool_out(H), pool_out(W)) and pos.shape == dy.shape
    s, a = _padded(N, H, W, C, 0.0), _padded(N, H, W, C, 0.0)
    g = _d(dy)
    for kh in range(3):
        for kw in range(3):
            m = (pos == kh * 3 + kw).to(torch.float64)
            s[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += g * m          # (a stride-2 view never overlaps itself)
            a[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += g.abs() * m
    return s[:, 1:H + 1, 1:W + 1].contiguous(), a[:, 1:H + 1, 1:W + 1].contiguous()


def ref_maxpool_bwd(pos, dy, H, W, add=None):
    """Routed gradient rounded once to dy's dtype; with `add` the kernel's documented two roundings f16(f16(routed) + add)."""
    routed = ref_maxpool_bwd_terms(pos, dy, H, W)[0].to(dy.dtype)
    if add is None:
        return routed
    return (_d(routed) + _d(add)).to(dy.dtype)


# ------------------------------------------------------------------------------------------------------------------ stride-2 subsample
def ref_subsample2(x):
    return x[:, ::2, ::2].contiguous()


def ref_subsample2_bwd(dy, H, W, prev=None):
    N, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == (pool_out(H), pool_out(W))
    dx = torch.zeros((N, H, W, C), dtype=torch.float64)
    dx[:, ::2, ::2] = _d(dy)
    if prev is not None:
        dx = dx + _d(prev)
    return dx.to(dy.dtype)


# ------------------------------------------------------------------------------------------------------------------ nearest resize
def nn_index(out, inp):
    """int64 [out]: ATen's legacy 'nearest' source index min(floorf(dst * (float)inp / out), inp - 1), evaluated in float32."""
    scale = np.float32(inp) / np.float32(out)
    assert scale.dtype == np.float32
    src = np.floor(np.arange(out, dtype=np.float32) * scale)
    assert src.dtype == np.float32
    return torch.from_numpy(np.minimum(src.astype(np.int64), inp - 1))


def exact_index(out, inp):
    """The exact rational rule (dst * inp) // out, which the fp32 rule is NOT at the DIVERGENT_PAIRS."""
    return torch.clamp((torch.arange(out, dtype=torch.int64) * inp) // out, max=inp - 1)


def max_preimage(out, inp):
    """Largest number of output indices one input index receives."""
    return int(torch.bincount(nn_index(out, inp), minlength=inp).max())


def ref_resize_fwd(x, Ho, Wo, Cp, dtype):
    """x NCHW fp32 [N, Cr, H, W] (any strides) -> NHWC [N, Ho, Wo, Cp] `dtype`: dtype(x[.., hi, wi]), channels >= Cr zero."""
    N, Cr, H, W = x.shape
    hi, wi = nn_index(Ho, H), nn_index(Wo, W)
    y = torch.zeros((N, Ho, Wo, Cp), dtype=dtype)
    y[..., :Cr] = x.detach().cpu()[:, :, hi][:, :, :, wi].permute(0, 2, 3, 1).to(dtype)
    return y


def ref_resize_bwd_terms(dy, N, Cr, H, W, gscale=1.0):
    """dy NHWC [N, Ho, Wo, Cp] -> (dx, abs_terms) float64 NCHW [N, Cr, H, W]: gscale * the sum of dy over each pixel's preimage;
    channels >= Cr of dy are ignored."""
    _, Ho, Wo, _ = dy.shape
    hi, wi = nn_index(Ho, H), nn_index(Wo, W)
    g = _d(dy)[..., :Cr].permute(0, 3, 1, 2) * f32(gscale)

    def route(t):
        rows = torch.zeros((N, Cr, H, Wo), dtype=torch.float64).index_add_(2, hi, t)
        return torch.zeros((N, Cr, H, W), dtype=torch.float64).index_add_(3, wi, rows)
    return route(g), route(g.abs())


def ref_resize_bwd(dy, N, Cr, H, W, gscale=1.0):
    return ref_resize_bwd_terms(dy, N, Cr, H, W, gscale)[0].float()


def ref_nhwc_to_nchw(x, Cr):
    return x[..., :Cr].permute(0, 3, 1, 2).float().contiguous()


def ref_upsample_add(a, b):
    """a [N, H, W, C] + nearest(b [N, Hb, Wb, C]), one rounding."""
    hi, wi = nn_index(a.shape[1], b.shape[1]), nn_index(a.shape[2], b.shape[2])
    return (_d(a) + _d(b)[:, hi][:, :, wi]).to(a.dtype)


def ref_upsample_add_bwd_terms(dy, Hb, Wb, db_prev=None):
    N, H, W, C = dy.shape
    hi, wi = nn_index(H, Hb), nn_index(W, Wb)

    def route(t):
        rows = torch.zeros((N, Hb, W, C), dtype=torch.float64).index_add_(1, hi, t)
        return torch.zeros((N, Hb, Wb, C), dtype=torch.float64).index_add_(2, wi, rows)
    s, a = route(_d(dy)), route(_d(dy).abs())
    if db_prev is not None:
        s, a = s + _d(db_prev), a + _d(db_prev).abs()
    return s, a


def ref_upsample_add_bwd(dy, Hb, Wb, db_prev=None):
    """The adjoint of nearest(b) (+ the previous content of db when accumulating), one rounding."""
    return ref_upsample_add_bwd_terms(dy, Hb, Wb, db_prev)[0].to(dy.dtype)


# ------------------------------------------------------------------------------------------------------------------ decoder gradients
def ref_upsample2_bwd(dy, c_off, C, prev=None):
    """dy [N, 2*Hl, 2*Wl, Ctot] -> [N, Hl, Wl, C]: the 2x2 sum of channels [c_off, c_off + C) (+ prev), one rounding."""
    N, Hu, Wu, _ = dy.shape
    s = _d(dy)[..., c_off:c_off + C].reshape(N, Hu // 2, 2, Wu // 2, 2, C).sum(dim=(2, 4))
    if prev is not None:
        s = s + _d(prev)
    return s.to(dy.dtype)


def ref_slice(x, c_off, C, prev=None):
    s = x[..., c_off:c_off + C]
    if prev is None:
        return s.contiguous()
    return (_d(s) + _d(prev)).to(x.dtype)


def ref_concat_up_bwd(dcat, c_up):
    """Gradient of cat([nearest_2x(a), skip], channel) -> (da, dskip or None)."""
    Ct = dcat.shape[-1]
    return ref_upsample2_bwd(dcat, 0, c_up), (ref_slice(dcat, c_up, Ct - c_up) if Ct > c_up else None)


# ------------------------------------------------------------------------------------------------------------------ element-wise
def ref_add(a, b):
    return (_d(a) + _d(b)).to(a.dtype)


def ref_relu_bwd(dy, z):
    return torch.where(z > 0, dy, torch.zeros_like(dy))


def ref_f32_to_f16(x, scale, dtype):
    """One fp32 multiply, one rounding to the storage type."""
    return (x * torch.tensor(scale, dtype=torch.float32)).to(dtype)


def ref_f32_to_f16_fused(x, scale, dtype):
    """The EXACT product (two fp32 factors: exact in float64) rounded once to the storage type -- what a fused multiply-convert
    instruction computes.  Equal to ref_f32_to_f16 whenever the fp32 product is exact (power-of-two scales short of under- / overflow);
    otherwise the two differ where the fp32 rounding lands on, or crosses, a tie of the storage type.  (numpy converts float64 to
    float16 directly; torch goes through float32.)"""
    prod = x.detach().cpu().double().numpy() * np.float64(f32(scale))
    with np.errstate(over="ignore"):
        return torch.from_numpy(prod.astype(np.float16 if dtype == torch.float16 else np.float32))


def ref_f16_to_f32(x, scale):
    return x.float() * torch.tensor(scale, dtype=torch.float32)


def ref_scale_store_terms(src, scale, prev=None):
    """-> (value, |prev| + |src * scale|) float64."""
    t = _d(src) * f32(scale)
    if prev is None:
        return t, t.abs()
    return t + _d(prev), t.abs() + _d(prev).abs()


def ref_sigmoid_bwd(dy, s, Cp, gscale):
    """dy, s NCHW fp32 [N, Cr, H, W] -> float64 NHWC [N, H, W, Cp]: gscale * dy * s * (1 - s), channels >= Cr zero."""
    N, Cr, H, W = s.shape
    out = torch.zeros((N, H, W, Cp), dtype=torch.float64)
    sd = _d(s)
    out[..., :Cr] = (_d(dy) * sd * (1.0 - sd) * f32(gscale)).permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------------------------------ builders
def grid_inputs(seed, shape, dtype, *, levels=None, negative=False):
    """Multiples of 2^-6 in [-16, 16] (`negative`: in [-16, -2^-6]); `levels`: only that many distinct values occur (windows full of
    ties)."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-1024, -1) if negative else (-1024, 1024)
    if levels is None:
        n = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    else:
        vals = torch.randperm(hi - lo + 1, generator=g)[:levels] + lo
        n = vals[torch.randint(0, levels, tuple(shape), generator=g)]
    return (n.double() / 64.0).to(dtype)


def wild_inputs(seed, shape, dtype, *, max_abs=65504.0):
    """Unconstrained finite values of either storage type: normal deviates spread over twelve binades (clamped to max_abs), and in
    about a quarter of the positions fp16 subnormals, +-0, +-max_abs and its fp16 neighbour below.  fp32 keeps its own low bits."""
    g = torch.Generator().manual_seed(seed)
    shape = tuple(shape)
    v = torch.randn(shape, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-8, 5, shape, generator=g).double())
    v = v.clamp(-max_abs, max_abs)
    special = torch.tensor([2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, -1023 * 2.0 ** -24, 0.0, -0.0,
                            max_abs, -max_abs, max_abs * (1 - 2.0 ** -10), -max_abs * (1 - 2.0 ** -10)], dtype=torch.float64)
    pick = torch.randint(0, 4 * special.numel(), shape, generator=g)
    v = torch.where(pick < special.numel(), special[pick.clamp(max=special.numel() - 1)], v)
    return v.to(dtype)
