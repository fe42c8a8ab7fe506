"""The reference's reconstruction losses (src/losses/losses.py): `Reconstruction.select_loss_pixel` / `select_loss_perceptual`.

The pixel losses (MSE, L1) run in hd_pixel_loss (csrc/pixel_loss.hip): one streaming pass computes the weighted values, and in
gradient mode adds the gradient into the caller's buffer.  LPIPS needs the `lpips` package and its pretrained weights, neither of
which is part of this project: asking for it raises.  The structural loss (`select_loss_structural('ssim')`, --structural ssim) has
no implementation in the reference; it runs in hd_ssim_loss (csrc/ssim_loss.hip) and fills the reference's two perceptual slots.
"""
import warnings

import torch
import torch.nn as nn

from .. import ops


class _PixelLossFn(torch.autograd.Function):
    """mean v(input - target) with v = d*d (mse) | |d| (l1): value-only kernel forward, gradient-mode kernel backward."""

    @staticmethod
    def forward(ctx, inp, target, kind):
        out = ops.pixel_loss(inp, target, target, kind, 1.0, 0.0)
        ctx.save_for_backward(inp, target)
        ctx.kind = kind
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        inp, target = ctx.saved_tensors
        gs = g.reshape(()).to(torch.float32).contiguous()
        d_inp = d_target = None
        # d/d input = g(input - target); d/d target = g(target - input) = -g(input - target) (v and g are even / odd in d)
        if ctx.needs_input_grad[0]:
            d_inp = torch.zeros_like(inp)
            ops.pixel_loss(inp, target, target, ctx.kind, 1.0, 0.0, gs=gs, dhall=d_inp)
        if ctx.needs_input_grad[1]:
            d_target = torch.zeros_like(target)
            ops.pixel_loss(target, inp, inp, ctx.kind, 1.0, 0.0, gs=gs, dhall=d_target)
        return d_inp, d_target, None


class PixelLoss(nn.Module):
    """Drop-in for `nn.MSELoss()` / `nn.L1Loss()` (reduction 'mean') on fp32 device batches [N, 3, H, W] of equal shape."""

    def __init__(self, kind):
        super().__init__()
        if kind not in ops.PIXEL_KINDS:
            raise ValueError("PixelLoss: kind must be one of %s (got %r)" % (sorted(ops.PIXEL_KINDS), kind))
        self.kind = kind

    def forward(self, input, target):
        if input.shape != target.shape:
            raise ValueError("PixelLoss(%s): input %s and target %s must have the same shape (nothing is broadcast)"
                             % (self.kind, tuple(input.shape), tuple(target.shape)))
        return _PixelLossFn.apply(input.contiguous(), target.contiguous(), self.kind)

    def extra_repr(self):
        return "kind=%r" % self.kind


class PixelTerms(torch.autograd.Function):
    """The two weighted pixel terms of the training step and the total they join (train_hallucidet.py:173-176,209):
    (pixel_rgb, pixel_ir, total) = (w_rgb * L(hall, rgb), w_ir * L(hall, ir), (base_total + pixel_rgb) + pixel_ir), one autograd
    node.  The weights are taken here, so the backward pass receives the seed of `total` itself and adds both terms' gradient in
    ONE gradient-mode launch; d total / d base_total = 1 passes the seed on unchanged."""

    @staticmethod
    def forward(ctx, hall, base_total, rgb, ir, kind, w_rgb, w_ir):
        out = ops.pixel_loss(hall.detach(), rgb, ir, kind, w_rgb, w_ir, base_total=base_total.detach())
        ctx.save_for_backward(hall, rgb, ir)
        ctx.args = (kind, w_rgb, w_ir)
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_rgb, g_ir, g_total):
        hall, rgb, ir = ctx.saved_tensors
        kind, w_rgb, w_ir = ctx.args
        dh = None
        if ctx.needs_input_grad[0] and not (g_rgb is None and g_ir is None and g_total is None):
            dh = torch.zeros_like(hall)
            if g_rgb is None and g_ir is None:
                ops.pixel_loss(hall, rgb, ir, kind, w_rgb, w_ir, gs=_seed(g_total), dhall=dh)
            else:                           # the reported terms are differentiated as well: one launch per term
                for gt, wr, wi in ((g_rgb, w_rgb, 0.0), (g_ir, 0.0, w_ir)):
                    s = gt if g_total is None else (g_total if gt is None else gt + g_total)
                    if s is not None:
                        ops.pixel_loss(hall, rgb, ir, kind, wr, wi, gs=_seed(s), dhall=dh)
        return dh, g_total, None, None, None, None, None


def _seed(g):
    return g.reshape(()).to(torch.float32).contiguous()


STRUCTURAL_KINDS = ("ssim",)


class _StructuralLossFn(torch.autograd.Function):
    """1 - SSIM(input, target): value-only kernel forward, gradient-mode kernel backward.  The index is symmetric in its two
    arguments, so the gradient with respect to the target is the same kernel with the roles swapped."""

    @staticmethod
    def forward(ctx, inp, target):
        out = ops.ssim_loss(inp, target, target, 1.0, 0.0)
        ctx.save_for_backward(inp, target)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        inp, target = ctx.saved_tensors
        gs = _seed(g)
        d_inp = d_target = None
        if ctx.needs_input_grad[0]:
            d_inp = torch.zeros_like(inp)
            ops.ssim_loss(inp, target, target, 1.0, 0.0, gs=gs, dhall=d_inp)
        if ctx.needs_input_grad[1]:
            d_target = torch.zeros_like(target)
            ops.ssim_loss(target, inp, inp, 1.0, 0.0, gs=gs, dhall=d_target)
        return d_inp, d_target


class StructuralLoss(nn.Module):
    """`forward(input, target)` -> the scalar 1 - SSIM on fp32 device batches [N, 3, H, W] of equal shape, H, W >= 11 (11-tap Gaussian
    window, sigma 1.5, 'valid', data range 1, C1 = 1e-4, C2 = 9e-4: hd_ssim_loss), differentiable in both arguments."""

    def __init__(self, kind='ssim'):
        super().__init__()
        if kind not in STRUCTURAL_KINDS:
            raise ValueError("StructuralLoss: kind must be one of %s (got %r)" % (list(STRUCTURAL_KINDS), kind))
        self.kind = kind

    def forward(self, input, target):
        if input.shape != target.shape:
            raise ValueError("StructuralLoss(%s): input %s and target %s must have the same shape (nothing is broadcast)"
                             % (self.kind, tuple(input.shape), tuple(target.shape)))
        return _StructuralLossFn.apply(input.contiguous(), target.contiguous())

    def extra_repr(self):
        return "kind=%r" % self.kind


class StructuralTerms(torch.autograd.Function):
    """The two weighted structural terms of the training step and the total they join, in the reference's perceptual slots
    (train_hallucidet.py:174,176,209): (perceptual_rgb, perceptual_ir, total) = (w_rgb * (1 - SSIM(hall, rgb)),
    w_ir * (1 - SSIM(hall, ir)), (base_total + perceptual_rgb) + perceptual_ir), one autograd node shaped like PixelTerms."""

    @staticmethod
    def forward(ctx, hall, base_total, rgb, ir, w_rgb, w_ir):
        out = ops.ssim_loss(hall.detach(), rgb, ir, w_rgb, w_ir, base_total=base_total.detach())
        ctx.save_for_backward(hall, rgb, ir)
        ctx.args = (w_rgb, w_ir)
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_rgb, g_ir, g_total):
        hall, rgb, ir = ctx.saved_tensors
        w_rgb, w_ir = ctx.args
        dh = None
        if ctx.needs_input_grad[0] and not (g_rgb is None and g_ir is None and g_total is None):
            dh = torch.zeros_like(hall)
            if g_rgb is None and g_ir is None:
                ops.ssim_loss(hall, rgb, ir, w_rgb, w_ir, gs=_seed(g_total), dhall=dh)
            else:                           # the reported terms are differentiated as well: one call per term
                for gt, wr, wi in ((g_rgb, w_rgb, 0.0), (g_ir, 0.0, w_ir)):
                    s = gt if g_total is None else (g_total if gt is None else gt + g_total)
                    if s is not None:
                        ops.ssim_loss(hall, rgb, ir, wr, wi, gs=_seed(s), dhall=dh)
        return dh, g_total, None, None, None, None


class Reconstruction():

    @staticmethod
    def select_loss_perceptual(loss_perceptual='lpips_alexnet'):
        """src/losses/losses.py:5-14: 'lpips_alexnet' / 'lpips_vgg' / 'lpips_squeeze' -> LPIPS; anything else -> None (the
        reference's 'psnr', 'ssim', 'msssim' choices included: they select nothing there either)."""
        if loss_perceptual is not None and str(loss_perceptual).startswith('lpips'):
            raise NotImplementedError("perceptual loss %r: LPIPS needs the `lpips` package and its pretrained network weights, "
                                      "neither of which is available to this project" % (loss_perceptual,))
        if loss_perceptual is not None and loss_perceptual not in _WARNED:
            _WARNED.add(loss_perceptual)
            warnings.warn("perceptual loss %r selects no loss (as in the reference): its two terms stay 0.0" % (loss_perceptual,))
        return None

    @staticmethod
    def select_loss_pixel(loss_pixel='mse'):
        """src/losses/losses.py:27-34: 'mse' / 'l1' -> the HIP loss module, anything else -> None."""
        if loss_pixel == 'mse':
            return Reconstruction.Pixel.mse()
        elif loss_pixel == 'l1':
            return Reconstruction.Pixel.l1()
        return None

    @staticmethod
    def select_loss_structural(loss_structural=None):
        """'ssim' -> the HIP structural loss module, None -> None; no reference counterpart (its 'ssim' choice under --perceptual
        selects nothing, which select_loss_perceptual keeps), so an unknown name is an error rather than silence."""
        if loss_structural is None:
            return None
        if loss_structural in STRUCTURAL_KINDS:
            return StructuralLoss(loss_structural)
        raise ValueError("structural loss %r: one of %s" % (loss_structural, list(STRUCTURAL_KINDS)))

    class Pixel():

        @staticmethod
        def mse():
            return PixelLoss('mse')

        @staticmethod
        def l1():
            return PixelLoss('l1')


_WARNED = set()
