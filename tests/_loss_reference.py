"""Float64 definitions of the detector loss kernels of csrc/losses.hip (RPN, Fast R-CNN with and without padding rows, the batched RetinaNet
losses, the element-wise focal loss) and of csrc/optim.hip (fused Adam step, finiteness check), seeded input builders, fp32 emulations
and the tolerances derived from them.  Shared by test_loss_reference_cpu.py (definitions against ATen in float64, torch.optim.Adam and
the CPU oracle; mutants; emulations) and test_loss_kernels_gpu.py (the HIP kernels against these definitions).

Every ref_* function takes exactly the tensors its kernel takes and evaluates the definition in float64; gradients are float64 autograd
of that definition.  Python-float arguments enter as the fp32 value the wrapper hands to the kernel (f32()).  No element is excluded
from any comparison: an element the kernel must leave at zero has tolerance 0.

Loop constants (from the two .hip files): RPN / Fast R-CNN forward 256 blocks x 256 threads = 65 536 elements per trip, their backward
and the element-wise focal kernel 2 048 x 256 = 524 288, RetinaNet forward 32 x 256 = 8 192 anchors per image and trip, its backward
256 x 256 = 65 536, Adam 4 096 x 256 x 4 = 4 194 304, check_finite 2 048 x 256 = 524 288.

Tolerances.  U32, SCALAR_RTOL, REDUCE_RTOL and worst_ratio are _bn_reference's; LOSS_RTOL, LOSS_FLOOR and the focal `mag` expressions are
_fcos_reference's (losses.hip and fcos.hip share ONE focal_terms / focal_value / focal_grad: csrc/hd_det_math.h), and LOSS_RTOL also bounds the RPN's
BCE-with-logits, which is the focal loss's `ce` term: |got - ref| <= RTOL*mag + LOSS_FLOOR.  `mag` is the first-order error magnitude:
the sum of the absolute values of the terms, a difference counting BOTH operands.  Three constants are new.  Each is 4x the worst
(|err| - LOSS_FLOOR) / mag of a numpy float32 evaluation of the defining formulas (ATen's smooth_l1 / log_softmax and torch.optim.Adam's,
in the operand order the kernel headers cite) against the float64 definition over the very cases the GPU test runs, rounded up; the
factor covers the device's expf / logf / sqrtf and division, which the emulation does not see (same factor and reason as LOSS_RTOL):

  SL1_RTOL = 7.5e-7    smooth-L1 value and gradient, BoxCoder.encode inside it for RetinaNet.  d = a - t has mag(d) = |a| + mag(t), with
      mag(t) = |t| for a given target and (|tx|, |ty|, ww*(|log(gw/ew)| + 1), wh*(|log(gh/eh)| + 1)) for an encoded one; value mag is
      |d|*mag(d)/beta below beta and mag(d) + beta/2 above; gradient mag is mag(d)/beta for |d| <= beta and 1 above, times the upstream
      |g| / divisor.  derive_sl1_rtol measures value 1.08e-7 (RetinaNet B = 2, A = 8 193, beta = 1, unit weights) and gradient 1.76e-7
      (Fast R-CNN R = 65 537, K = 2 with padding rows: the quotient d / beta times the rounded g / n_valid, three roundings on one
      term); 4x = 7.04e-7.
  CE_RTOL = 5.5e-7     max-shifted softmax cross-entropy.  Row value -((l_y - mx) - log(se)): mag = |l_y| + |mx| + |log se| + 1 + S with
      S = sum_k p_k*(|l_k| + |mx|) (the error the shifted arguments carry into se).  Gradient (p_k - [k = y])*g/n: mag =
      (p_k*(1 + |l_k| + |mx| + S) + [k = y])*|g|/n.  derive_ce_rtol measures value 7.2e-8 (R = 65 537, K = 2) and gradient 1.33e-7
      (R = 65 537, K = 2 with padding rows); 4x = 5.32e-7.
  ADAM_RTOL = 6.0e-7   Adam's p, m, v.  gr = clip(g*inv_scale) + wd*p has mag(gr) = |c| + |wd*p|; mag(m') = |b1*m| + (1 - b1)*mag(gr);
      mag(v') = b2*v + (1 - b2)*(2*|gr|*mag(gr) + gr^2); mag(denom) = mag(v') / (2*sqrt(v')*sqrt(bc2)) + denom; mag(p') = |p| +
      step*(mag(m')/denom + |m'|*mag(denom)/denom^2).  derive_adam_rtol measures m 1.47e-7 (n = 4 097, weight_decay 0.01, no clip,
      inv_scale 1/8, step 1: the roundings of wd*p, the sum, (1 - b1)*gr, b1*m and the final sum on two terms), v 1.18e-7 and p 8.7e-8
      (both n = 4 194 309, weight_decay 0.01, clip 0.5, inv_scale 1/8, step 1); 4x = 5.87e-7.  The kernel's arithmetic is IEEE add / multiply /
      divide / sqrt in exactly the emulation's order (the library is built with -ffp-contract=off), so the device is expected far inside
      this bound.
  Loss values: (elem_rtol + REDUCE_RTOL) * sum(mag) / divisor + LOSS_FLOOR (RetinaNet: per image, then the mean over images).
  check_finite and every "exactly zero" / "unchanged" / "bit-identical" statement: torch.equal.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from _bn_reference import U32, SCALAR_RTOL, REDUCE_RTOL, worst_ratio, f32, _d      # noqa: F401  (re-exported)
from _fcos_reference import LOSS_RTOL, LOSS_FLOOR                                   # noqa: F401

SL1_RTOL = 7.5e-7
CE_RTOL = 5.5e-7
ADAM_RTOL = 6.0e-7

LB = 256
RPN_TRIP = 256 * LB               # rpn_loss_fwd_kernel / frcnn_loss_fwd_kernel: NPART blocks
ELEM_TRIP = 2048 * LB             # rpn_loss_bwd_kernel, focal_elem_kernel, check_finite_kernel
RETINA_TRIP = 32 * LB             # retina_loss_fwd_kernel: RB blocks per image
RETINA_BWD_TRIP = 256 * LB
ADAM_TRIP = 4096 * 256 * 4
BETA9 = 1.0 / 9                   # what _RPNLossFn / _FastRCNNLossFn pass
FLT_MAX = float(np.finfo(np.float32).max)

MUTANTS = ("second_trip_dropped", "denominator_unclamped", "ignored_counted_as_background", "nfg_shared_across_images",
           "background_rows_regress", "padding_rows_counted", "l1_grad_unscaled", "linear_branch_offset", "decay_before_clip",
           "bc2_not_rooted", "tail_element_dropped", "alpha_swapped")

SATURATED = (20.0, -20.0, 50.0, -50.0, 88.8, -88.8, 104.0, -104.0)      # expf overflows past 88.7; the fp32 sigmoid saturates near 17


def beta_edges(beta):
    """+-beta as the kernel sees it (fp32) and its two fp32 neighbours on either side -> six floats."""
    b = np.float32(beta)
    v = [float(b), float(np.nextafter(b, np.float32(0))), float(np.nextafter(b, np.float32(np.inf)))]
    return v + [-x for x in v]


_ZERO = torch.zeros((), dtype=torch.float64)
_ONE = torch.ones((), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------------ pieces
def _sl1(d, beta, mutant=None):
    """ATen's smooth_l1: 0.5*d^2/beta for |d| < beta, |d| - 0.5*beta otherwise."""
    z = d.abs()
    v = torch.where(z < beta, 0.5 * z * z / beta, z - (beta if mutant == "linear_branch_offset" else 0.5 * beta))
    if mutant == "l1_grad_unscaled":          # the value as defined, the gradient d instead of d / beta inside the quadratic zone
        dd = d.detach()
        gm = torch.where(dd < -beta, -_ONE, torch.where(dd > beta, _ONE, dd))
        v = v.detach() + gm * (d - dd)
    return v


def _sl1_mags(d, dmag, beta):
    """-> (value mag, gradient mag per unit of upstream): see the module docstring."""
    z = d.detach().abs()
    return torch.where(z < beta, z * dmag / beta, dmag + 0.5 * beta), torch.where(z <= beta, dmag / beta, torch.ones_like(dmag))


def _softplus_mag(x):
    """mag of m + log(exp(-m) + exp(-x - m)), m = max(-x, 0) (+1: the logarithm's argument lies in [1, 2] with an absolute u32)."""
    m = torch.clamp(-x, min=0)
    return m + (F.softplus(-x) - m).abs() + 1


def _focal(x, t, alpha, gamma, mutant=None):
    """sigmoid_focal_loss(reduction="none") in float64 on logits x and 0/1 targets t."""
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    pt = p * t + (1 - p) * (1 - t)
    loss = ce if gamma == 0 else ce * (1 - pt) ** gamma
    if alpha >= 0:
        a = f32(alpha)
        loss = ((1 - a) * t + a * (1 - t) if mutant == "alpha_swapped" else a * t + (1 - a) * (1 - t)) * loss
    return loss


def _focal_mags(x, t, alpha, gamma):
    """_fcos_reference's focal_mag / d_cls_mag expressions -> (value mag, gradient mag per unit of upstream)."""
    x = x.detach()
    p = torch.sigmoid(x)
    q = 1 - p
    sp = F.softplus(-x)
    sp_mag = _softplus_mag(x)
    at = (f32(alpha) * t + (1 - f32(alpha)) * (1 - t)) if alpha >= 0 else torch.ones_like(t)
    pw = (lambda b: torch.ones_like(b)) if gamma == 0 else (lambda b: b ** gamma)
    val = at * torch.where(t > 0, pw(q) * sp_mag, pw(p) * (x.abs() + sp_mag))
    s0, s0_mag = x + sp, x.abs() + sp_mag
    mag1 = pw(q) * (gamma * p * sp_mag + (1 + p))
    mag0 = pw(p) * (p + gamma * ((1 + p) * s0.abs() + q * s0_mag))
    return val, at * torch.where(t > 0, mag1, mag0)


def _encode(g, a, weights):
    """BoxCoder.encode_single in float64 -> (targets, mag), both [..., 4]."""
    wx, wy, ww, wh = (f32(w) for w in weights)
    ew, eh = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    ecx, ecy = a[..., 0] + 0.5 * ew, a[..., 1] + 0.5 * eh
    gw, gh = g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
    gcx, gcy = g[..., 0] + 0.5 * gw, g[..., 1] + 0.5 * gh
    lw, lh = torch.log(gw / ew), torch.log(gh / eh)
    t = torch.stack([wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * lw, wh * lh], -1)
    return t, torch.stack([t[..., 0].abs(), t[..., 1].abs(), abs(ww) * (lw.abs() + 1), abs(wh) * (lh.abs() + 1)], -1)


def _tol(mask, rtol, mag):
    """rtol*mag + LOSS_FLOOR where the kernel computes something, 0 where it must write an exact zero."""
    return torch.where(mask, rtol * mag + LOSS_FLOOR, _ZERO)


def _gw(g2):
    return torch.tensor([f32(v) for v in g2], dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------------ RPN
def ref_rpn_loss(obj, deltas, labels, reg_t, pos, samp, n_sampled, beta=BETA9, g2=(1.0, 1.0), *, mutant=None, trip=RPN_TRIP):
    """RegionProposalNetwork.compute_loss on the tensors hd_rpn_loss takes: BCE-with-logits summed over `samp`, smooth-L1 summed over
    `pos`, both / max(n_sampled, 1); gradients of g2 . (objectness, box).  -> dict losses [2], loss_tol [2], d_obj, d_deltas and their
    tol_*, the per-element terms bce / l1 with their *_mag and the gradient mags d_obj_mag / d_deltas_mag."""
    x = _d(obj).reshape(-1).clone().requires_grad_(True)
    dl = _d(deltas).reshape(-1, 4).clone().requires_grad_(True)
    t, rt = _d(labels).reshape(-1), _d(reg_t).reshape(-1, 4)
    s, p = samp.reshape(-1).bool().cpu(), pos.reshape(-1).bool().cpu()
    if mutant == "second_trip_dropped":
        keep = torch.arange(x.numel()) < trip
        s, p = s & keep, p & keep
    b = f32(beta)
    bce = torch.where(s, F.binary_cross_entropy_with_logits(x, t, reduction="none"), _ZERO)
    d = dl - rt
    l1 = torch.where(p[:, None], _sl1(d, b, mutant), _ZERO)
    n = float(n_sampled)
    dn = n if mutant == "denominator_unclamped" else max(n, 1.0)
    losses = torch.stack([bce.sum(), l1.sum()]) / dn
    gw = _gw(g2)
    (losses * gw).sum().backward()
    out = {"losses": losses.detach(), "d_obj": x.grad.reshape(obj.shape), "d_deltas": dl.grad.reshape(deltas.shape), "bce": bce.detach(),
           "l1": l1.detach(), "dn": dn, "samp": s, "pos": p}
    if mutant is not None:
        return out
    with torch.no_grad():
        xd = x.detach()
        go, gb = abs(float(gw[0])) / dn, abs(float(gw[1])) / dn
        out["bce_mag"] = torch.where(s, ((1 - t) * xd).abs() + _softplus_mag(xd), _ZERO)
        out["d_obj_mag"] = torch.where(s, torch.sigmoid(xd) + t, _ZERO) * go
        dmag = dl.detach().abs() + rt.abs()
        vm, gm = _sl1_mags(d, dmag, b)
        out["l1_mag"] = torch.where(p[:, None], vm, _ZERO)
        out["d_deltas_mag"] = torch.where(p[:, None], gm, _ZERO) * gb
        out["tol_d_obj"] = _tol(s, LOSS_RTOL, out["d_obj_mag"]).reshape(obj.shape)
        out["tol_d_deltas"] = _tol(p[:, None].expand(-1, 4), SL1_RTOL, out["d_deltas_mag"]).reshape(deltas.shape)
        out["loss_tol"] = torch.stack([(LOSS_RTOL + REDUCE_RTOL) * out["bce_mag"].sum(), (SL1_RTOL + REDUCE_RTOL) * out["l1_mag"].sum()]) / dn + LOSS_FLOOR
    return out


# ------------------------------------------------------------------------------------------------------------------ Fast R-CNN
def ref_fastrcnn_loss(logits, breg, labels, reg_t, beta=BETA9, n_valid=None, g2=(1.0, 1.0), *, mutant=None, trip=RPN_TRIP):
    """roi_heads.fastrcnn_loss on the tensors hd_fastrcnn_loss(_masked) takes: cross-entropy over the rows with label >= 0, smooth-L1 on
    the labelled class's four columns for label > 0, both / R, or / max(n_valid, 1) when n_valid is given; rows with label < 0 contribute
    nothing and get zero gradient.  -> dict like ref_rpn_loss's with ce / l1, d_logits / d_breg."""
    lg = _d(logits).clone().requires_grad_(True)
    br = _d(breg).clone().requires_grad_(True)
    rt = _d(reg_t)
    R, K = lg.shape
    lab = labels.long().cpu()
    if mutant == "padding_rows_counted":
        lab = lab.clamp(min=0)
    valid = lab >= 0
    fg = valid if mutant == "background_rows_regress" else lab > 0
    if mutant == "second_trip_dropped":
        keep = torch.arange(R) < trip
        valid, fg = valid & keep, fg & keep
    lc = lab.clamp(min=0)
    ce = torch.where(valid, -torch.log_softmax(lg, 1).gather(1, lc[:, None]).squeeze(1), _ZERO)
    d = br.reshape(R, K, 4)[torch.arange(R), lc] - rt
    b = f32(beta)
    l1 = torch.where(fg[:, None], _sl1(d, b, mutant), _ZERO)
    n = float(R if n_valid is None else n_valid)
    dn = n if mutant == "denominator_unclamped" else max(n, 1.0)
    losses = torch.stack([ce.sum(), l1.sum()]) / dn
    gw = _gw(g2)
    (losses * gw).sum().backward()
    out = {"losses": losses.detach(), "d_logits": lg.grad, "d_breg": br.grad, "ce": ce.detach(), "l1": l1.detach(), "dn": dn, "valid": valid,
           "fg": fg, "lc": lc}
    if mutant is not None:
        return out
    with torch.no_grad():
        l = lg.detach()
        gc, gb = abs(float(gw[0])) / dn, abs(float(gw[1])) / dn
        mx = l.max(1, keepdim=True)[0]
        pk = torch.softmax(l, 1)
        lse = torch.logsumexp(l - mx, 1, keepdim=True)
        S = (pk * (l.abs() + mx.abs())).sum(1, keepdim=True)
        onehot = (torch.arange(K)[None] == lc[:, None]).double()
        out["ce_mag"] = torch.where(valid, (l.gather(1, lc[:, None]).abs() + mx.abs() + lse.abs() + 1 + S).squeeze(1), _ZERO)
        out["d_logits_mag"] = torch.where(valid[:, None], pk * (1 + l.abs() + mx.abs() + S) + onehot, _ZERO) * gc
        dmag = br.detach().reshape(R, K, 4)[torch.arange(R), lc].abs() + rt.abs()
        vm, gm = _sl1_mags(d, dmag, b)
        out["l1_mag"] = torch.where(fg[:, None], vm, _ZERO)
        sel = (onehot.bool() & fg[:, None])[:, :, None].expand(R, K, 4)                      # the columns that carry a box gradient
        out["d_breg_mag"] = torch.where(sel, gm[:, None, :].expand(R, K, 4), _ZERO).reshape(R, K * 4) * gb
        out["tol_d_logits"] = _tol(valid[:, None].expand(R, K), CE_RTOL, out["d_logits_mag"])
        out["tol_d_breg"] = _tol(sel.reshape(R, K * 4), SL1_RTOL, out["d_breg_mag"])
        out["loss_tol"] = torch.stack([(CE_RTOL + REDUCE_RTOL) * out["ce_mag"].sum(), (SL1_RTOL + REDUCE_RTOL) * out["l1_mag"].sum()]) / dn + LOSS_FLOOR
    return out


# ------------------------------------------------------------------------------------------------------------------ RetinaNet
def ref_retinanet_loss(cls, breg, matched, gt, glab, anchors, weights=(1.0, 1.0, 1.0, 1.0), alpha=0.25, gamma=2.0, beta=1.0, g2=(1.0, 1.0), *,
                       mutant=None, trip=RETINA_TRIP):
    """compute_retinanet_loss on the tensors hd_retinanet_loss takes (cls [B, A, K], breg [B, A, 4], matched [B, A] with -2 = not counted,
    -1 = background, >= 0 = row of gt [B, G, 4] / glab [B, G], anchors [A, 4]): focal loss over matched != -2, smooth-L1 against
    BoxCoder.encode of the matched box over matched >= 0, each / max(1, nfg_b) per image, then the mean over the B images.
    -> dict like ref_rpn_loss's with focal / l1, d_cls / d_breg, and nfg [B] (clamped)."""
    x = _d(cls).clone().requires_grad_(True)
    br = _d(breg).clone().requires_grad_(True)
    B, A, K = x.shape
    m = matched.long().cpu()
    if mutant == "ignored_counted_as_background":
        m = torch.where(m == -2, torch.full_like(m, -1), m)
    counted, fg = m != -2, m >= 0
    if mutant == "second_trip_dropped":
        keep = (torch.arange(A) < trip)[None]
        counted, fg = counted & keep, fg & keep
    mc = m.clamp(min=0)
    lab = torch.where(fg, glab.long().cpu().gather(1, mc), torch.full_like(mc, -1))
    t = (lab[..., None] == torch.arange(K)).double()
    focal = torch.where(counted[..., None], _focal(x, t, alpha, gamma, mutant), _ZERO)
    an = _d(anchors)[None].expand(B, A, 4)
    box = torch.where(fg[..., None], _d(gt).gather(1, mc[..., None].expand(-1, -1, 4)), an)      # off foreground: any finite target
    tgt, tmag = _encode(box, an, weights)
    d = br - tgt
    b = f32(beta)
    l1 = torch.where(fg[..., None], _sl1(d, b, mutant), _ZERO)
    nfg = fg.sum(1).double()
    if mutant != "denominator_unclamped":
        nfg = nfg.clamp(min=1)
    if mutant == "nfg_shared_across_images":
        nfg = nfg[0:1].expand(B)
    losses = torch.stack([(focal.sum((1, 2)) / nfg).sum(), (l1.sum((1, 2)) / nfg).sum()]) / B
    gw = _gw(g2)
    (losses * gw).sum().backward()
    out = {"losses": losses.detach(), "d_cls": x.grad, "d_breg": br.grad, "focal": focal.detach(), "l1": l1.detach(), "nfg": nfg, "fg": fg,
           "counted": counted, "d": d.detach(), "box": box, "lab": lab}
    if mutant is not None:
        return out
    with torch.no_grad():
        sc = 1.0 / (nfg * B)
        gc, gr = abs(float(gw[0])) * sc[:, None, None], abs(float(gw[1])) * sc[:, None, None]
        fv, fgm = _focal_mags(x, t, alpha, gamma)
        out["focal_mag"] = torch.where(counted[..., None], fv, _ZERO)
        out["d_cls_mag"] = torch.where(counted[..., None], fgm, _ZERO) * gc
        dmag = br.detach().abs() + tmag
        vm, gm = _sl1_mags(d, dmag, b)
        out["l1_mag"] = torch.where(fg[..., None], vm, _ZERO)
        out["d_breg_mag"] = torch.where(fg[..., None], gm, _ZERO) * gr
        out["tol_d_cls"] = _tol(counted[..., None].expand(B, A, K), LOSS_RTOL, out["d_cls_mag"])
        out["tol_d_breg"] = _tol(fg[..., None].expand(B, A, 4), SL1_RTOL, out["d_breg_mag"])
        out["loss_tol"] = torch.stack([(LOSS_RTOL + REDUCE_RTOL) * (out["focal_mag"].sum((1, 2)) / nfg).sum(),
                                       (SL1_RTOL + REDUCE_RTOL) * (out["l1_mag"].sum((1, 2)) / nfg).sum()]) / B + LOSS_FLOOR
    return out


def ref_focal_elem(x, t, alpha, gamma, gout=None, *, mutant=None):
    """hd_sigmoid_focal_loss: the per-element loss (gout None) or its gradient times gout; the target is on iff t > 0.5.
    -> dict out, mag, tol (x's shape)."""
    xd = _d(x).clone().requires_grad_(True)
    td = (_d(t) > 0.5).double()
    loss = _focal(xd, td, alpha, gamma, mutant)
    vm, gm = _focal_mags(xd, td, alpha, gamma)
    if gout is None:
        out, mag = loss.detach(), vm
    else:
        loss.backward(_d(gout))
        out, mag = xd.grad, gm * _d(gout).abs()
    return {"out": out, "mag": mag, "tol": LOSS_RTOL * mag + LOSS_FLOOR}


# ------------------------------------------------------------------------------------------------------------------ Adam
def bias_corrections(beta1, beta2, step):
    """What ops.adam_step hands to hd_adam_step: 1 - beta^step evaluated in Python floats, then rounded to fp32."""
    return f32(1.0 - beta1 ** step), f32(1.0 - beta2 ** step)


def ref_adam(p, g, m, v, lr, b1, b2, eps, wd, clip, inv_scale, step, *, mutant=None):
    """torch.optim.Adam's single-tensor step behind unscale and clip_grad_value_, in the kernel's and torch's order: gr = g*inv_scale,
    clamped to +-clip when clip > 0, + wd*p; m' = b1*m + (1 - b1)*gr; v' = b2*v + (1 - b2)*gr^2; denom = sqrt(v')/sqrt(bc2) + eps;
    p' = p - lr/bc1 * m'/denom.  -> dict p, m, v and tol_p, tol_m, tol_v (float64, p's shape)."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    lr, B1, B2, eps, wd, clip, inv = (f32(a) for a in (lr, b1, b2, eps, wd, clip, inv_scale))
    bc1, bc2 = bias_corrections(b1, b2, step)
    c = g * inv
    if mutant == "decay_before_clip":
        c = c + wd * p
    if clip > 0:
        c = c.clamp(-clip, clip)
    gr = c if mutant == "decay_before_clip" else c + wd * p
    gr_mag = c.abs() + (wd * p).abs()
    m1 = B1 * m + (1 - B1) * gr
    v1 = B2 * v + (1 - B2) * gr * gr
    rbc2 = bc2 if mutant == "bc2_not_rooted" else math.sqrt(bc2)
    denom = torch.sqrt(v1) / rbc2 + eps
    st = lr / bc1
    p1 = p - st * (m1 / denom)
    if mutant == "tail_element_dropped":
        p1, m1, v1 = p1.clone(), m1.clone(), v1.clone()
        p1.reshape(-1)[-1], m1.reshape(-1)[-1], v1.reshape(-1)[-1] = p.reshape(-1)[-1], m.reshape(-1)[-1], v.reshape(-1)[-1]
    out = {"p": p1, "m": m1, "v": v1}
    if mutant is not None:
        return out
    m_mag = (B1 * m).abs() + (1 - B1) * gr_mag
    v_mag = (B2 * v).abs() + (1 - B2) * (2 * gr.abs() * gr_mag + gr * gr)
    sq = torch.sqrt(v1)
    denom_mag = torch.where(sq > 0, 0.5 * v_mag / (sq.clamp(min=1e-300) * rbc2), _ZERO) + denom
    p_mag = p.abs() + st * (m_mag / denom + m1.abs() * denom_mag / (denom * denom))
    out.update(tol_p=ADAM_RTOL * p_mag + LOSS_FLOOR, tol_m=ADAM_RTOL * m_mag + LOSS_FLOOR, tol_v=ADAM_RTOL * v_mag + LOSS_FLOOR,
               p_mag=p_mag, m_mag=m_mag, v_mag=v_mag)
    return out


def ref_check_finite(g):
    """-> True iff the flag must be raised: some element is not finite (torch.isfinite: +-inf and every NaN)."""
    return not bool(torch.isfinite(g.detach().cpu()).all())


# ------------------------------------------------------------------------------------------------------------------ builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _differences(shape, beta, g):
    """Smooth-L1 differences, half of them inside (0.02 .. 0.98)*beta, half in (1.02 .. 4)*beta, random sign (float64)."""
    u = torch.rand(shape, generator=g, dtype=torch.float64)
    inside = torch.rand(shape, generator=g) < 0.5
    mag = torch.where(inside, 0.02 + 0.96 * u, 1.02 + 2.98 * u) * f32(beta)
    return mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()


def side_shares(d, mask, beta):
    """Shares of the masked smooth-L1 differences strictly below and strictly above beta (fp32 value) -> (below, above, count)."""
    z = d[mask].abs()
    n = max(1, z.numel())
    return float((z < f32(beta)).sum()) / n, float((z > f32(beta)).sum()) / n, z.numel()


def edge_hits(d, mask, beta):
    """How many of the six beta_edges values occur among the masked differences."""
    z = d[mask]
    return sum(int(bool((z == e).any())) for e in beta_edges(beta))


def saturated_hits(x):
    return sum(int(bool((x == v).any())) for v in SATURATED)


def rpn_inputs(T, seed):
    """hd_rpn_loss inputs over T anchors.  `samp` is about 5 % of the anchors plus the first 16 and the last one; `pos` = samp & label 1,
    a subset of it.  The first 16 logits are SATURATED on label 0, then on label 1; the last anchor is a sampled positive with logit
    -104 (a loss of 104: a dropped last trip shows).  Rows 8 and 9 (row 0 when T < 10) carry the six beta edges against a zero target.
    promise: what holds for this T (edges, saturated, quarter = a quarter of the differences on each side of beta, five_percent)."""
    g = _gen(seed)
    obj = 3 * torch.randn(T, 1, generator=g)
    labels = (torch.rand(T, generator=g) < 0.5).float()
    samp = torch.rand(T, generator=g) < 0.05
    reg_t = 0.3 * torch.randn(T, 4, generator=g)
    n16 = min(T, 16)
    samp[:n16] = True
    labels[:n16] = (torch.arange(n16) >= 8).float()
    obj[:n16, 0] = torch.tensor(SATURATED * 2)[:n16]
    samp[T - 1], labels[T - 1], obj[T - 1, 0] = True, 1.0, -104.0
    deltas = (reg_t.double() + _differences((T, 4), BETA9, g)).float()
    e = beta_edges(BETA9)
    if T >= 10:
        reg_t[8:10] = 0.0
        deltas[8] = torch.tensor(e[:4])
        deltas[9] = torch.tensor(e[4:] + [0.0, 2 * BETA9])
    else:
        reg_t[0] = 0.0
        deltas[0] = torch.tensor(e[:4])
        labels[0] = 1.0
    pos = samp & (labels > 0)
    n_sampled = int(samp.sum())
    promise = {"edges": 6 if T >= 10 else 4, "saturated": 8 if T >= 17 else 0, "quarter": T >= 255, "five_percent": T >= 65535}
    return {"obj": obj, "deltas": deltas, "labels": labels, "reg_t": reg_t, "pos": pos, "samp": samp, "n_sampled": n_sampled, "promise": promise}


def frcnn_inputs(R, K, seed, padding="none"):
    """hd_fastrcnn_loss inputs: labels in [0, K-1] (row 0 and the last row carry K-1), with padding="some" about 30 % of the rows -1,
    with "all" every row.  Rows 0..7 carry SATURATED logits; the last row has +104 on class 0 and -104 on its own class K-1 (a loss
    of 208).  Rows 1 and 2 (row 0 when R < 3) are foreground with the six beta edges against a zero target (K > 1)."""
    g = _gen(seed)
    logits = 2 * torch.randn(R, K, generator=g)
    labels = torch.randint(0, K, (R,), generator=g)
    reg_t = 0.3 * torch.randn(R, 4, generator=g)
    breg = 0.3 * torch.randn(R, K * 4, generator=g)
    n8 = min(R, 8)
    for i in range(n8):
        logits[i, i % K] = SATURATED[i]
    labels[0] = labels[R - 1] = K - 1
    if K > 1:
        logits[R - 1, 0], logits[R - 1, K - 1] = 104.0, -104.0
    lc = labels.clone()
    e = beta_edges(BETA9)
    edge_rows = (1, 2) if R >= 3 else (0,)
    if K > 1:
        for r in edge_rows:
            lc[r] = labels[r] = K - 1
    diff = _differences((R, 4), BETA9, g)
    cols = (lc[:, None] * 4 + torch.arange(4)[None])
    breg.scatter_(1, cols, (reg_t.double() + diff).float())
    if K > 1:
        for j, r in enumerate(edge_rows):
            reg_t[r] = 0.0
            vals = e[:4] if j == 0 else e[4:] + [0.0, 2 * BETA9]
            breg[r, (K - 1) * 4:(K - 1) * 4 + 4] = torch.tensor(vals)
    if padding == "some":
        pad = torch.rand(R, generator=g) < 0.3
        pad[[0, R - 1] + list(edge_rows)] = False
        labels = torch.where(pad, torch.full_like(labels, -1), labels)
    elif padding == "all":
        labels = torch.full_like(labels, -1)
    promise = {"edges": 0 if (K == 1 or padding == "all") else (6 if R >= 3 else 4), "saturated": 8 if R >= 8 else 0,
               "quarter": K > 1 and R >= 257 and padding != "all"}
    return {"logits": logits, "breg": breg, "labels": labels, "reg_t": reg_t, "n_valid": int((labels >= 0).sum()), "promise": promise}


IMAGE_KINDS = ("mixed", "nofg", "ignored")      # all three codes / no foreground (-1 and -2 only) / every anchor -2


def _grid_boxes(n, g):
    """n boxes on a quarter-pixel grid with sides in [1, 100] pixels: every encode_box input is exact in fp32."""
    xy = torch.randint(0, 1001, (n, 2), generator=g).float() * 0.25
    wh = torch.randint(4, 401, (n, 2), generator=g).float() * 0.25
    return torch.cat([xy, xy + wh], 1)


def retina_inputs(B, A, K, G, seed, kinds=None, beta=1.0, weights=(1.0, 1.0, 1.0, 1.0)):
    """hd_retinanet_loss inputs.  kinds[b] in IMAGE_KINDS (default: cycled).  A "mixed" image has about 10 % foreground and 20 % ignored
    anchors; its anchors 0, 3 (a copy of anchor 0's box) and A-1 are foreground, 1 background, 2 ignored (as far as A reaches).  Slot 0 of
    its ground truth IS anchor 0's box, so the targets of anchors 0 and 3 are exactly 0 and their regressions carry the six beta edges;
    component 0 of anchor 0 is exactly +beta, whose gradient is g / (nfg*B) with no other factor.  Logits are 3*randn with SATURATED
    over the first 16 (anchors 8..15 are background wherever the image counts anything) and -104 on the last anchor's own label (a loss near 104 in the last trip)."""
    g = _gen(seed)
    kinds = tuple(kinds) if kinds is not None else tuple(IMAGE_KINDS[b % 3] for b in range(B))
    anchors = _grid_boxes(A, g)
    if A > 3:
        anchors[3] = anchors[0]
    gt = _grid_boxes(B * G, g).reshape(B, G, 4)
    glab = torch.randint(0, K, (B, G), generator=g)
    matched = torch.full((B, A), -1, dtype=torch.int64)
    for b, kind in enumerate(kinds):
        u = torch.rand(A, generator=g)
        slot = torch.randint(0, G, (A,), generator=g)
        if kind == "mixed":
            matched[b] = torch.where(u < 0.1, slot, torch.where(u < 0.3, torch.full_like(slot, -2), torch.full_like(slot, -1)))
            matched[b, A - 1] = G - 1
            for a, v in ((1, -1), (2, -2), (3, 0)):
                if a < A - 1:
                    matched[b, a] = v
            matched[b, 0] = 0
            gt[b, 0] = anchors[0]
        elif kind == "nofg":
            matched[b] = torch.where(u < 0.3, torch.full_like(slot, -2), torch.full_like(slot, -1))
        else:
            matched[b] = -2
    cls = 3 * torch.randn(B, A, K, generator=g)
    n16 = min(A, 16)
    if A >= 17:
        for b, kind in enumerate(kinds):
            if kind != "ignored":
                matched[b, 8:16] = -1          # the second run of SATURATED sits on counted anchors
    for b in range(B):
        for i in range(n16):
            cls[b, i, i % K] = SATURATED[i % 8]
        if matched[b, A - 1] >= 0:
            cls[b, A - 1, int(glab[b, matched[b, A - 1]])] = -104.0
    fg = matched >= 0
    an = anchors.double()[None].expand(B, A, 4)
    box = torch.where(fg[..., None], gt.double().gather(1, matched.clamp(min=0)[..., None].expand(-1, -1, 4)), an)
    tgt, _ = _encode(box, an, weights)
    breg = (tgt + _differences((B, A, 4), beta, g)).float()
    e = beta_edges(beta)
    n_edges = 0
    for b, kind in enumerate(kinds):
        if kind == "mixed":
            breg[b, 0] = torch.tensor(e[:4])
            n_edges = 4
            if A > 4:
                breg[b, 3] = torch.tensor(e[4:] + [0.0, 2 * f32(beta)])
                n_edges = 6
    promise = {"edges": n_edges, "saturated": 8 if A >= 17 and any(k != "ignored" for k in kinds) else 0,
               "quarter": A >= 300 and "mixed" in kinds, "kinds": kinds}
    return {"cls": cls, "breg": breg, "matched": matched, "gt": gt, "glab": glab, "anchors": anchors, "weights": tuple(weights), "beta": beta,
            "promise": promise}


def focal_inputs(n, seed):
    """Element-wise focal inputs: 3*randn logits, 30 % targets on, SATURATED on both target values over the first 16, -104 on a set
    target at the end, and a random upstream gradient."""
    g = _gen(seed)
    x = 3 * torch.randn(n, generator=g)
    t = (torch.rand(n, generator=g) < 0.3).float()
    n16 = min(n, 16)
    x[:n16] = torch.tensor(SATURATED * 2)[:n16]
    t[:n16] = (torch.arange(n16) >= 8).float()
    x[n - 1], t[n - 1] = -104.0, 1.0
    return {"x": x, "t": t, "gout": torch.randn(n, generator=g), "promise": {"saturated": 8 if n >= 17 else 0}}


def adam_inputs(n, seed):
    """p ~ N(0, 1), g ~ 8*N(0, 1) (clipping at 0.5 bites with and without the 1/8 unscale), m ~ 0.1*N(0, 1), v ~ U(0, 0.5);
    the last element is fixed at p = 0.25, g = 6, m = 0.3, v = 0.01."""
    g = _gen(seed)
    d = {"p": torch.randn(n, generator=g), "g": 8 * torch.randn(n, generator=g), "m": 0.1 * torch.randn(n, generator=g),
         "v": 0.5 * torch.rand(n, generator=g)}
    d["p"][n - 1], d["g"][n - 1], d["m"][n - 1], d["v"][n - 1] = 0.25, 6.0, 0.3, 0.01      # the last element moves far: a dropped tail shows
    return d


# ------------------------------------------------------------------------------------------------------------------ the GPU test's cases
G2 = (0.7, 1.3)                                     # upstream weights of the two losses
RPN_T = (1, 255, 256, 257, 65535, 65536, 65537, 131089)      # one thread, the block edge, one forward trip -1 / exact / +1, two trips + 17
RPN_T_BWD_CAP = 524291                              # three past the backward's 2 048-block trip
FRCNN_CASES = ((1, 2), (5, 1), (257, 2), (300, 91), (65537, 2))
RETINA_CASES = ((1, 1, 1, 1), (2, 8191, 2, 3), (2, 8192, 2, 3), (2, 8193, 2, 3), (3, 65539, 2, 2), (2, 300, 91, 4))
RETINA_PARAMS = ((0.25, 2.0, 1.0, (1.0, 1.0, 1.0, 1.0)), (0.6, 1.5, 0.3, (10.0, 10.0, 5.0, 5.0)), (-1.0, 0.0, 1.0 / 9, (1.0, 1.0, 1.0, 1.0)))
FOCAL_N = (1, 257, 524293)
ADAM_N = (1, 2, 3, 4, 5, 7, 1023, 4097, 4194309)
ADAM_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_GRID = [(wd, clip, inv, step) for wd in (0.0, 1e-2) for clip in (0.0, 0.5) for inv in (1.0, 1.0 / 8) for step in (1, 3, 100000)]
ADAM_GRID_LARGE = [(1e-2, 0.5, 1.0 / 8, 1), (0.0, 0.0, 1.0, 100000)]      # n = 4 194 309: the two opposite corners of the grid
FINITE_N = (1, 63, 64, 65, 300, 524288, 524289)


def adam_grid(n):
    return ADAM_GRID_LARGE if n > 100000 else ADAM_GRID


def retina_kinds(B, variant):
    """The image kinds of a B-image batch: variant 0 is the cycle (mixed, nofg, ignored), variant 1 moves every kind one image on, so that
    each two-image batch meets all three kinds over its two variants and the image that holds the foreground changes."""
    return tuple(IMAGE_KINDS[(b - variant) % 3] for b in range(B)) if B > 1 else ("mixed",)


@functools.lru_cache(maxsize=None)
def rpn_case(T, n_mode="tensor"):
    """Inputs and float64 reference for T anchors: computed once, shared, never modified.  n_mode "zero": n_sampled = 0."""
    d = rpn_inputs(T, 1000 + T % 997)
    n = 0 if n_mode == "zero" else d["n_sampled"]
    return d, ref_rpn_loss(d["obj"], d["deltas"], d["labels"], d["reg_t"], d["pos"], d["samp"], n, BETA9, G2)


@functools.lru_cache(maxsize=None)
def frcnn_case(R, K, padding="none", masked=False):
    d = frcnn_inputs(R, K, 2000 + R % 997 + K, padding)
    return d, ref_fastrcnn_loss(d["logits"], d["breg"], d["labels"], d["reg_t"], BETA9, d["n_valid"] if masked else None, G2)


@functools.lru_cache(maxsize=None)
def retina_case(ci, pi, variant=0):
    B, A, K, G = RETINA_CASES[ci]
    alpha, gamma, beta, weights = RETINA_PARAMS[pi]
    d = retina_inputs(B, A, K, G, 3000 + 10 * ci + pi, retina_kinds(B, variant), beta, weights)
    return d, ref_retinanet_loss(d["cls"], d["breg"], d["matched"], d["gt"], d["glab"], d["anchors"], weights, alpha, gamma, beta, G2)


@functools.lru_cache(maxsize=None)
def focal_case(n):
    return focal_inputs(n, 4000 + n % 997)


@functools.lru_cache(maxsize=None)
def adam_case(n):
    return adam_inputs(n, 5000 + n % 997)


def retina_variants(ci):
    return (0, 1) if RETINA_CASES[ci][0] == 2 else (0,)


# ------------------------------------------------------------------------------------------------------------------ fp32 emulations
_F = np.float32


def emu_sl1_f32(a, t, beta, gscale):
    """The kernel's smooth_l1 / smooth_l1_grad on float32 arrays a (prediction) and t (target); gscale = g / divisor in float32 (scalar or
    broadcastable) -> (value, gradient) float32."""
    b = _F(beta)
    d = a - t
    z = np.abs(d)
    val = np.where(z < b, _F(0.5) * z * z / b, z - _F(0.5) * b)
    grad = np.where(d < -b, _F(-1), np.where(d > b, _F(1), d / b)) * gscale
    return val.astype(_F), grad.astype(_F)


def emu_encode_f32(g, a, weights):
    """encode_box in float32 (BoxCoder.encode_single's operand order)."""
    wx, wy, ww, wh = (_F(w) for w in weights)
    ew, eh = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    ecx, ecy = a[..., 0] + _F(0.5) * ew, a[..., 1] + _F(0.5) * eh
    gw, gh = g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
    gcx, gcy = g[..., 0] + _F(0.5) * gw, g[..., 1] + _F(0.5) * gh
    return np.stack([wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * np.log(gw / ew), wh * np.log(gh / eh)], -1).astype(_F)


def emu_ce_f32(logits, lc, gscale):
    """frcnn_loss_*_kernel's max-shifted log-softmax in float32, the K exponentials added in index order -> (row loss, d_logits)."""
    l = logits.float().numpy()
    R, K = l.shape
    mx = l[:, 0].copy()
    for k in range(1, K):
        mx = np.maximum(mx, l[:, k])
    se = np.zeros(R, _F)
    for k in range(K):
        se = se + np.exp(l[:, k] - mx)
    lab = lc.numpy()
    ce = -((l[np.arange(R), lab] - mx) - np.log(se))
    p = np.exp(l - mx[:, None]) / se[:, None]
    onehot = (np.arange(K)[None] == lab[:, None]).astype(_F)
    return ce.astype(_F), ((p - onehot) * _F(gscale)).astype(_F)


def emu_adam_f32(p, g, m, v, lr, b1, b2, eps, wd, clip, inv_scale, step):
    """adam_kernel's statements in numpy float32 -> (p, m, v)."""
    p, g, m, v = (t.float().numpy() for t in (p, g, m, v))
    lr, B1, B2, eps, wd, clip, inv = (_F(a) for a in (lr, b1, b2, eps, wd, clip, inv_scale))
    bc1, bc2 = (_F(a) for a in bias_corrections(b1, b2, step))
    bc2s = np.sqrt(bc2)
    st = lr / bc1
    gr = g * inv
    if clip > 0:
        gr = np.minimum(np.maximum(gr, -clip), clip)
    if wd != 0:
        gr = gr + wd * p
    m1 = B1 * m + (_F(1) - B1) * gr
    v1 = B2 * v + (_F(1) - B2) * gr * gr
    denom = np.sqrt(v1) / bc2s + eps
    p1 = p - st * (m1 / denom)
    return p1.astype(_F), m1.astype(_F), v1.astype(_F)


def _worst(err, mag, mask=None):
    """max (|err| - LOSS_FLOOR) / mag over the masked elements -> (ratio, flat index)."""
    r = torch.where(err <= LOSS_FLOOR, torch.zeros_like(err), (err - LOSS_FLOOR) / mag.clamp(min=1e-300))
    if mask is not None:
        r = torch.where(mask, r, torch.zeros_like(r))
    if r.numel() == 0:
        return 0.0, -1
    if not bool(torch.isfinite(r).all()):
        return math.inf, -1
    i = int(r.flatten().argmax())
    return float(r.flatten()[i]), i


def _fdiv(g, dn):
    return _F(_F(g) / _F(dn))


def derive_sl1_rtol():
    """Worst emulated smooth-L1 ratio over every RPN, Fast R-CNN and RetinaNet case of the GPU test -> {"value": (ratio, case), "grad": ...}."""
    worst = {"value": (0.0, None), "grad": (0.0, None)}

    def take(name, val, grad, ref_val, ref_grad, vmag, gmag, mask):
        for key, got, want, mag in (("value", val, ref_val, vmag), ("grad", grad, ref_grad, gmag)):
            r, _ = _worst((torch.from_numpy(got).double() - want).abs(), mag, mask)
            if r > worst[key][0]:
                worst[key] = (r, name)
    for T in RPN_T + (RPN_T_BWD_CAP,):
        d, ref = rpn_case(T)
        val, grad = emu_sl1_f32(d["deltas"].numpy(), d["reg_t"].numpy(), BETA9, _fdiv(G2[1], ref["dn"]))
        take("rpn T=%d" % T, val, grad, ref["l1"], ref["d_deltas"], ref["l1_mag"], ref["d_deltas_mag"], ref["pos"][:, None].expand(-1, 4))
    for R, K in FRCNN_CASES:
        for padding, masked in (("none", False), ("some", True)):
            d, ref = frcnn_case(R, K, padding, masked)
            rows = torch.arange(R)
            picked = d["breg"].reshape(R, K, 4)[rows, ref["lc"]].numpy()
            val, grad = emu_sl1_f32(picked, d["reg_t"].numpy(), BETA9, _fdiv(G2[1], ref["dn"]))
            take("frcnn R=%d K=%d %s" % (R, K, padding), val, grad, ref["l1"], ref["d_breg"].reshape(R, K, 4)[rows, ref["lc"]], ref["l1_mag"],
                 ref["d_breg_mag"].reshape(R, K, 4)[rows, ref["lc"]], ref["fg"][:, None].expand(-1, 4))
    for ci, (B, A, K, G) in enumerate(RETINA_CASES):
        for pi, (alpha, gamma, beta, weights) in enumerate(RETINA_PARAMS):
            for variant in retina_variants(ci):
                d, ref = retina_case(ci, pi, variant)
                tgt = emu_encode_f32(ref["box"].float().numpy(), d["anchors"].numpy()[None], weights)
                gs = (_F(f32(G2[1])) / (ref["nfg"].float().numpy() * _F(B))).astype(_F)[:, None, None]
                val, grad = emu_sl1_f32(d["breg"].numpy(), tgt, beta, gs)
                take("retina %s beta=%g weights=%s" % ((B, A, K, G), beta, weights), val, grad, ref["l1"], ref["d_breg"], ref["l1_mag"],
                     ref["d_breg_mag"], ref["fg"][..., None].expand(-1, -1, 4))
    return worst


def derive_ce_rtol():
    """Worst emulated cross-entropy ratio over the Fast R-CNN cases -> {"value": (ratio, case), "grad": ...}."""
    worst = {"value": (0.0, None), "grad": (0.0, None)}
    for R, K in FRCNN_CASES:
        for padding, masked in (("none", False), ("some", True)):
            d, ref = frcnn_case(R, K, padding, masked)
            ce, dl = emu_ce_f32(d["logits"], ref["lc"], _fdiv(G2[0], ref["dn"]))
            name = "frcnn R=%d K=%d %s" % (R, K, padding)
            for key, got, want, mag, mask in (("value", ce, ref["ce"], ref["ce_mag"], ref["valid"]),
                                              ("grad", dl, ref["d_logits"], ref["d_logits_mag"], ref["valid"][:, None].expand(R, K))):
                r, _ = _worst((torch.from_numpy(got).double() - want).abs(), mag, mask)
                if r > worst[key][0]:
                    worst[key] = (r, name)
    return worst


def derive_adam_rtol():
    """Worst emulated Adam ratio over ADAM_N x the hyper-parameter grid the GPU test runs -> {"p": (ratio, case), "m": ..., "v": ...}."""
    worst = {"p": (0.0, None), "m": (0.0, None), "v": (0.0, None)}
    h = ADAM_HYPER
    for n in ADAM_N:
        d = adam_case(n)
        for wd, clip, inv, step in adam_grid(n):
            args = (d["p"], d["g"], d["m"], d["v"], h["lr"], h["beta1"], h["beta2"], h["eps"], wd, clip, inv, step)
            ref = ref_adam(*args)
            for key, got in zip(("p", "m", "v"), emu_adam_f32(*args)):
                r, _ = _worst((torch.from_numpy(got).double() - ref[key]).abs(), ref[key + "_mag"])
                if r > worst[key][0]:
                    worst[key] = (r, "n=%d wd=%g clip=%g inv=%g step=%d" % (n, wd, clip, inv, step))
    return worst


# ------------------------------------------------------------------------------------------------------------------ builder conditions
def _check_sl1_population(d, mask, beta, promise):
    assert edge_hits(d, mask, beta) >= promise["edges"], (edge_hits(d, mask, beta), promise)
    if promise["quarter"]:
        below, above, n = side_shares(d, mask, beta)
        assert below >= 0.25 and above >= 0.25 and n >= 32, (below, above, n)


def check_rpn_conditions(d):
    """The branch populations rpn_inputs promises; asserted on the inputs by the CPU and the GPU test alike."""
    pr, T = d["promise"], d["obj"].numel()
    samp, pos = d["samp"], d["pos"]
    assert not bool((pos & ~samp).any()) and bool(pos[T - 1]) and int(samp.sum()) == d["n_sampled"]
    assert T <= RPN_TRIP or bool(pos[RPN_TRIP:].any())                          # work in the forward's second trip
    assert T <= ELEM_TRIP or bool(pos[ELEM_TRIP:].any())                        # ... and in the backward's
    _check_sl1_population(d["deltas"].double() - d["reg_t"].double(), pos[:, None].expand(-1, 4), BETA9, pr)
    for lab in (0.0, 1.0):
        assert saturated_hits(d["obj"].flatten()[samp & (d["labels"] == lab)]) >= pr["saturated"]
    if pr["five_percent"]:
        assert 0.04 <= float(samp.float().mean()) <= 0.06
    assert bool(((d["labels"] == 0) | (d["labels"] == 1)).all())


def check_frcnn_conditions(d):
    pr = d["promise"]
    R, K = d["logits"].shape
    lab = d["labels"]
    assert int(lab.min()) >= -1 and int(lab.max()) <= K - 1 and d["n_valid"] == int((lab >= 0).sum())
    assert d["n_valid"] == 0 or bool((lab == K - 1).any())
    lc = lab.clamp(min=0)
    picked = d["breg"].reshape(R, K, 4)[torch.arange(R), lc]
    _check_sl1_population(picked.double() - d["reg_t"].double(), (lab > 0)[:, None].expand(-1, 4), BETA9, pr)
    assert saturated_hits(d["logits"]) >= pr["saturated"]
    assert R <= RPN_TRIP or d["n_valid"] == 0 or int(lab[R - 1]) == K - 1    # a labelled row in the forward's second trip


def check_retina_conditions(d):
    pr = d["promise"]
    m, gt, an = d["matched"], d["gt"], d["anchors"]
    B, A = m.shape
    G = gt.shape[1]
    assert int(m.min()) >= -2 and int(m.max()) < G
    for b, kind in enumerate(pr["kinds"]):
        codes = {c: bool((m[b] == c).any()) for c in (-2, -1)}
        has_fg = bool((m[b] >= 0).any())
        if kind == "mixed":
            assert has_fg and int(m[b, 0]) == 0 and int(m[b, A - 1]) >= 0 and (A < 4 or (codes[-2] and codes[-1]))
        elif kind == "nofg":
            assert not has_fg and codes[-1]
        else:
            assert not has_fg and not codes[-1] and codes[-2]
    for boxes in (gt.reshape(-1, 4), an):
        assert torch.equal(boxes * 4, (boxes * 4).round()) and bool((boxes[:, 2] > boxes[:, 0]).all()) and bool((boxes[:, 3] > boxes[:, 1]).all())
    fg = m >= 0
    ad = an.double()[None].expand(B, A, 4)
    box = torch.where(fg[..., None], gt.double().gather(1, m.clamp(min=0)[..., None].expand(-1, -1, 4)), ad)
    tgt, _ = _encode(box, ad, d["weights"])
    _check_sl1_population(d["breg"].double() - tgt, fg[..., None].expand(-1, -1, 4), d["beta"], pr)
    assert saturated_hits(d["cls"][m != -2]) >= pr["saturated"]
    if "mixed" in pr["kinds"]:
        b = pr["kinds"].index("mixed")
        assert float(d["breg"][b, 0, 0]) == f32(d["beta"]) and float(tgt[b, 0, 0]) == 0.0
        assert A <= RETINA_TRIP or int(m[b, A - 1]) >= 0


def check_focal_conditions(d):
    for tv in (0.0, 1.0):
        assert saturated_hits(d["x"][d["t"] == tv]) >= d["promise"]["saturated"]
