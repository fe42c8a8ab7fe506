"""The pixel reconstruction losses (--pixel mse|l1) without a GPU: the CLI flags reach Config, the selectors of
src/losses/losses.py return the HIP module or None (LPIPS raises), and hd_pixel_loss validates its arguments at the C boundary."""
import ctypes
import warnings

import pytest


def test_pixel_flags_reach_config(monkeypatch):
    from hallucidet_amd.config import Config
    monkeypatch.setattr(Config.Losses, "pixel", None)
    monkeypatch.setattr(Config.Losses, "hparams_losses_weights", dict(Config.Losses.hparams_losses_weights))
    args = Config.argument_parser(["--pixel", "l1", "--weight-pixel-rgb", "0.5", "--weight-pixel-ir", "0.25"])
    Config.set_loss_weights(args)
    assert Config.Losses.pixel == "l1"
    w = Config.Losses.hparams_losses_weights
    assert w["pixel_rgb"] == 0.5 and w["pixel_ir"] == 0.25
    assert w["perceptual_rgb"] == 0.0 and w["det_regression"] == 0.1


def test_selectors():
    from hallucidet_amd.losses.losses import PixelLoss, Reconstruction
    mse, l1 = Reconstruction.select_loss_pixel("mse"), Reconstruction.select_loss_pixel("l1")
    assert isinstance(mse, PixelLoss) and mse.kind == "mse"
    assert isinstance(l1, PixelLoss) and l1.kind == "l1"
    assert Reconstruction.select_loss_pixel(None) is None
    assert Reconstruction.select_loss_pixel("huber") is None
    for name in ("lpips_alexnet", "lpips_vgg", "lpips_squeeze"):
        with pytest.raises(NotImplementedError, match="lpips"):
            Reconstruction.select_loss_perceptual(name)
    assert Reconstruction.select_loss_perceptual(None) is None
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        for name in ("psnr", "ssim", "msssim"):
            assert Reconstruction.select_loss_perceptual(name) is None


def test_perceptual_warning_is_given_once():
    from hallucidet_amd.losses import losses
    losses._WARNED.discard("ssim")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        losses.Reconstruction.select_loss_perceptual("ssim")
        losses.Reconstruction.select_loss_perceptual("ssim")
    assert len([r for r in rec if "ssim" in str(r.message)]) == 1


def test_module_takes_the_pixel_option():
    """The constructor accepts the reference's loss options (it raised NotImplementedError for any of them before); LPIPS is refused
    before anything is built."""
    from hallucidet_amd.train_hallucidet import EncoderDecoderLit
    with pytest.raises(NotImplementedError, match="lpips"):
        EncoderDecoderLit(loss_perceptual="lpips_vgg", device="cpu")
    lit = EncoderDecoderLit(batch_size=2, loss_pixel="l1", loss_perceptual="ssim", device="cpu")
    assert lit.loss_pixel.kind == "l1" and lit.loss_perceptual is None
    lit.loss_pixel = None
    assert lit.pixel_setup() is None


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hallucidet_amd import _abi
    return _abi.load()


def test_hd_pixel_loss_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.hd_pixel_loss(None, None, None, 1, 3, 4, 4, 1, 1.0, 1.0, 0, None, None, None, None, None, None) == -1
    assert b"hd_pixel_loss" in lib.hd_last_error() and b"null" in lib.hd_last_error()
    assert lib.hd_pixel_loss(p, p, p, 1, 1, 4, 4, 1, 1.0, 1.0, 0, None, None, None, p, p, None) == -1
    assert b"C must be 3" in lib.hd_last_error()
    assert lib.hd_pixel_loss(p, p, p, 1, 3, 4, 4, 1, 1.0, 1.0, 2, None, None, None, p, p, None) == -1
    assert b"kind" in lib.hd_last_error()
    assert lib.hd_pixel_loss(p, p, p, 1, 3, 4, 4, 2, 1.0, 1.0, 0, None, None, None, p, p, None) == -1
    assert b"ir_channels" in lib.hd_last_error()
    assert lib.hd_pixel_loss(p, p, p, 1, 3, 4, 4, 1, 1.0, 1.0, 0, None, None, p, p, p, None) == -1      # dhall without gs
    assert b"gs" in lib.hd_last_error()


def test_ops_wrapper_refuses_mismatches(monkeypatch):
    """Shapes, dtypes and layouts are checked before the library is called (here on meta tensors posing as device tensors)."""
    import torch
    from hallucidet_amd import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    h = torch.empty(2, 3, 8, 12, device="meta")
    with pytest.raises(ValueError, match="kind"):
        ops.pixel_loss(h, h, h, "huber", 1.0, 1.0)
    with pytest.raises(ValueError, match="rgb must have"):
        ops.pixel_loss(h, torch.empty(2, 3, 8, 10, device="meta"), h, "mse", 1.0, 1.0)
    with pytest.raises(ValueError, match="ir must be"):
        ops.pixel_loss(h, h, torch.empty(2, 2, 8, 12, device="meta"), "mse", 1.0, 1.0)
    with pytest.raises(TypeError, match="float32"):
        ops.pixel_loss(h, h.half(), h, "l1", 1.0, 1.0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.pixel_loss(h, h, torch.empty(2, 1, 8, 12, device="meta").expand(-1, 3, -1, -1), "l1", 1.0, 1.0)
    with pytest.raises(ValueError, match="gs"):
        ops.pixel_loss(h, h, h, "l1", 1.0, 1.0, dhall=torch.empty_like(h))
