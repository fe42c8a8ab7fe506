"""The structural loss (--structural ssim, hd_ssim_loss) on the GPU: the kernel against the float64 oracle of tests/_ssim_oracle.py
(index maps inside the first-order rounding bound, values, the gradient against the error of the fp32 ATen restatements, one-plane IR,
determinism eager and captured), the module, the training step with the option on (detector graph == eager bit for bit, the loss dict,
the U-Net gradient against the CPU oracle), the step with the option off (the kernel is never reached), and the root training script."""
import math
import os
import sys

import pytest
import torch

import _ssim_oracle as so

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shapes():
    from hallucidet_amd import ops
    th, tw = ops.SSIM_TILE
    # a single window; W % 4 != 0 on a tiny map; two 16-byte-path shapes; an odd one; maps one more and one less than two tiles in both
    # axes; the step's test shape
    return [(1, 11, 11), (1, 12, 27), (2, 40, 52), (1, 127, 161), (1, 2 * th + 1 + 10, 2 * tw + 1 + 10), (1, 2 * th - 1 + 10, 2 * tw - 1 + 10),
            (2, 128, 160)]


SHAPES = _shapes()


def _tolerance(hall, rgb, ir, w_rgb, w_ir, gs):
    """-> (g64, tol, yardstick): the float64 autograd gradient of the oracle times gs, and what the kernel may differ from it by: four
    times the larger max-abs error of the two fp32 ATen restatements (separable, direct) through autograd on the same inputs -- the
    kernel's summation order is a third fp32 order -- or 1e-6 of the largest element (the pixel-loss test's floor) if that is larger."""
    _, _, g64 = so.loss_and_grad64(hall, rgb, ir, w_rgb, w_ir, gs)
    yard = 0.0
    for filt in ("separable", "direct"):
        _, _, g32 = so.loss_and_grad(hall, rgb, ir, w_rgb, w_ir, gs, torch.float32, filt)
        yard = max(yard, float((g32.double() - g64).abs().max()))
    return g64, max(4.0 * yard, 1e-6 * float(g64.abs().max())), yard


@pytest.mark.parametrize("kind", so.INPUT_KINDS)
@pytest.mark.parametrize("ir_planes", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_fp64(dev, shape, ir_planes, kind):
    """Maps, values and gradient of one call against the float64 oracle; every figure is printed before it is asserted.  Measured on an
    MI355X over all 70 cases: the worst map position uses 0.20 of its bound (near-black images); the gradient's worst ratio to the
    ATen yardstick is 1.43 (constant images at 75 x 75, allowance 4), typically 0.3-0.5."""
    from hallucidet_amd import ops
    N, H, W = shape
    hall_c, rgb_c, ir_c = so.make_inputs(kind, N, H, W, ir_planes, seed=N + H + W)
    hall, rgb, ir = hall_c.to(dev), rgb_c.to(dev), ir_c.to(dev)
    w_rgb, w_ir, s = 0.75, 0.5, 1024.0
    gs = torch.tensor(s, device=dev)
    base = torch.tensor(0.3125, device=dev)
    maps = torch.full((2, N, 3, H - 10, W - 10), float("nan"), device=dev)
    v = ops.ssim_loss(hall, rgb, ir, w_rgb, w_ir, base_total=base, maps=maps)
    dh = torch.zeros_like(hall)
    vg = ops.ssim_loss(hall, rgb, ir, w_rgb, w_ir, base_total=base, gs=gs, dhall=dh)
    torch.cuda.synchronize()
    assert v.shape == (5,)
    # maps: inside the first-order rounding bound at every position, both terms
    for t, y in enumerate((rgb_c, ir_c)):
        S64, B = so.ssim_maps(hall_c, y), so.moment_bound(hall_c, y)
        got = maps[t].cpu().double()
        share = float(((got - S64).abs() / B).max())
        print("%s ir%d %s term %d: worst map error / bound %.3f" % (shape, ir_planes, kind, t, share))
        assert bool(((got - S64).abs() <= B).all()), share
        m64 = float(S64.mean())
        assert abs(float(v[3 + t]) - m64) <= float(B.mean()), (float(v[3 + t]), m64)
        own = float(got.mean())
        assert abs(float(v[3 + t]) - own) <= 1e-5 * abs(own), (float(v[3 + t]), own)     # the two-stage fp32 sum
    one = torch.tensor(1.0, device=dev)
    assert torch.equal(v[0], torch.tensor(w_rgb, device=dev) * (one - v[3])) and torch.equal(v[1], torch.tensor(w_ir, device=dev) * (one - v[4]))
    assert torch.equal(v[2], (base + v[0]) + v[1])
    assert torch.equal(v, vg), "value-only and gradient mode must give the same bits"
    # gradient
    g64, tol, yard = _tolerance(hall_c, rgb_c, ir_c, w_rgb, w_ir, s)
    err = float((dh.cpu().double() - g64).abs().max())
    print("%s ir%d %s: gradient error %.3e, yardstick %.3e (ratio %.2f), 1e-6 max|g| %.3e"
          % (shape, ir_planes, kind, err, yard, err / yard if yard > 0 else float("inf"), 1e-6 * float(g64.abs().max())))
    assert err <= tol, (err, tol, yard)
    # gradient mode ADDS to the buffer: one rounding of (old + the same contribution)
    d0 = torch.randn(hall.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    acc = d0.clone()
    ops.ssim_loss(hall, rgb, ir, w_rgb, w_ir, gs=gs, dhall=acc)
    assert torch.equal(acc, d0 + dh)
    if ir_planes == 1:
        # one plane gives exactly what its contiguous three-channel copy gives
        dh3 = torch.zeros_like(hall)
        m3 = torch.empty_like(maps)
        v3 = ops.ssim_loss(hall, rgb, ir.expand(-1, 3, -1, -1).contiguous(), w_rgb, w_ir, base_total=base, gs=gs, dhall=dh3, maps=m3)
        assert torch.equal(v3, v) and torch.equal(dh3, dh) and torch.equal(m3, maps)
    if kind == "equal_region":
        ih, iw = so.equal_interior(H, W)
        if ih > 0 and iw > 0:
            # rgb == hall there and every window that sees these pixels lies inside: the rgb term's gradient is 0
            d1 = torch.zeros_like(hall)
            ops.ssim_loss(hall, rgb, ir, w_rgb, 0.0, gs=gs, dhall=d1)
            g1, tol1, _ = _tolerance(hall_c, rgb_c, ir_c, w_rgb, 0.0, s)
            assert float(g1[:, :, :ih, :iw].abs().max()) <= tol1
            assert float(d1[:, :, :ih, :iw].abs().max()) <= tol1, (float(d1[:, :, :ih, :iw].abs().max()), tol1)
            assert float((d1.cpu().double() - g1).abs().max()) <= tol1


def test_small_images_are_refused(dev):
    from hallucidet_amd import ops
    x = torch.rand(1, 3, 10, 32, device=dev)
    with pytest.raises(ValueError, match="window"):
        ops.ssim_loss(x, x, x, 1.0, 1.0)


def test_kernel_is_deterministic_eager_and_captured(dev):
    from hallucidet_amd import ops
    hall, rgb, ir = [t.to(dev) for t in so.make_inputs("noise", 2, 128, 160, 1, seed=7)]
    gs = torch.tensor(65536.0, device=dev)
    base = torch.tensor(0.5, device=dev)
    outs = []
    for _ in range(2):
        dh = torch.zeros_like(hall)
        v = ops.ssim_loss(hall, rgb, ir, 1.0, 0.5, base_total=base, gs=gs, dhall=dh)
        outs.append((v.clone(), dh))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the call is capturable: no host synchronisation
    sdh = torch.zeros_like(hall)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ssim_loss(hall, rgb, ir, 1.0, 0.5, base_total=base, gs=gs, dhall=sdh)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sv = ops.ssim_loss(hall, rgb, ir, 1.0, 0.5, base_total=base, gs=gs, dhall=sdh)
    for _ in range(2):
        sdh.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(sv, outs[0][0]) and torch.equal(sdh, outs[0][1])


def test_module_matches_the_oracle(dev):
    from hallucidet_amd.losses.losses import Reconstruction
    hall_c, rgb_c, _ = so.make_inputs("smooth", 2, 64, 96, 1, seed=5)
    mod = Reconstruction.select_loss_structural("ssim")
    a = rgb_c.to(dev).requires_grad_(True)
    b = hall_c.to(dev).requires_grad_(True)
    loss = mod(a, b)                               # the reference's argument order: loss(imgs_rgb, imgs_hallucinated)
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    S64, B = so.ssim_maps(rgb_c, hall_c), so.moment_bound(rgb_c, hall_c)
    assert abs(float(loss) - (1.0 - float(S64.mean()))) <= float(B.mean()) + 2.0 ** -24      # + the fp32 rounding of 1 - SSIM itself
    for got, x, y in ((a.grad, rgb_c, hall_c), (b.grad, hall_c, rgb_c)):
        g64, tol, _ = _tolerance(x, y, y, 1.0, 0.0, 3.0)
        assert float((got.cpu().double() - g64).abs().max()) <= tol


# ------------------------------------------------------------------------------------------------------------------------- the step
H, W = 128, 160


@pytest.fixture
def weights(monkeypatch):
    from hallucidet_amd.config import Config
    w = dict(Config.Losses.hparams_losses_weights)
    monkeypatch.setattr(Config.Losses, "hparams_losses_weights", w)
    w.update(perceptual_rgb=1.0, perceptual_ir=0.5, pixel_rgb=1.0, pixel_ir=0.5)
    return w


def _graph_step(lit, batch):
    lit.use_detector_graph = True
    lit.encoder_decoder.train()
    torch.manual_seed(77)
    out = lit.forward_step(*batch, 0, step='train')
    r = lit.encoder_decoder.runner
    r.flat_grads.zero_()
    lit.scaler.scale(out['loss']['total']).backward()
    got = {k: (v.detach().clone() if torch.is_tensor(v) else torch.tensor(float(v))) for k, v in out['loss'].items()}
    got["grads"] = r.flat_grads.clone()
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("detector_name,pixel", [("fasterrcnn", None), ("retinanet", None), ("fasterrcnn", "l1")])
def test_graph_equals_eager_bit_for_bit(dev, weights, detector_name, pixel):
    from hallucidet_amd import synthetic
    lit = synthetic.make_module(seed=5, device="cuda", precision=16, detector_name=detector_name, loss_structural="ssim", loss_pixel=pixel)
    batch = synthetic.make_batch(2, H, W, seed=9, device="cuda")
    _graph_step(lit, batch)                    # capture
    g = lit._detector_graph()
    assert g is not None and g.usable and g.captures == 1
    b = _graph_step(lit, batch)                # a pure replay from the seeded generator state
    assert g.captures == 1 and g.replays == 2
    assert float(b["perceptual_rgb"]) > 0 and float(b["perceptual_ir"]) > 0
    assert (float(b["pixel_rgb"]) > 0) == (pixel is not None)
    e = next(iter(g.entries.values()))
    lit.use_detector_graph = False
    lit.encoder_decoder.train()
    torch.manual_seed(77)
    imgs_rgb, targets_rgb, imgs_ir, targets_ir = batch
    ir3 = imgs_ir.expand(-1, 3, -1, -1)
    hall = lit.encoder_decoder(ir3)
    N = hall.shape[0]
    t = [{"boxes": e.tb[i], "labels": e.tl[i], "_rows": e.live[i]} for i in range(3 * N)]
    losses, det_total, _ = lit._detector_section(hall, imgs_rgb, ir3, t[N:2 * N], t[:N], 'train', False, targets_ir_pass=t[2 * N:])
    total = det_total
    if pixel is not None:
        p_rgb, p_ir, total = lit._pixel_terms(hall, total, imgs_rgb, ir3)
        assert torch.equal(p_rgb, b["pixel_rgb"]) and torch.equal(p_ir, b["pixel_ir"])
    s_rgb, s_ir, total = lit._structural_terms(hall, total, imgs_rgb, ir3)
    r = lit.encoder_decoder.runner
    r.flat_grads.zero_()
    lit.scaler.scale(total).backward()
    torch.cuda.synchronize()
    assert torch.equal(total, b["total"]), (float(total), float(b["total"]))
    assert torch.equal(det_total, b["det_total"]) and torch.equal(s_rgb, b["perceptual_rgb"]) and torch.equal(s_ir, b["perceptual_ir"])
    for k, kk in (("bbox_regression", "det_regression"), ("classification", "det_classification")):
        assert torch.equal(losses[k], b[kk])
    assert torch.isfinite(r.flat_grads).all() and float(r.flat_grads.abs().max()) > 0
    assert torch.equal(r.flat_grads, b["grads"])


def test_loss_dict_in_training_and_validation(dev, weights):
    from hallucidet_amd import synthetic
    lit = synthetic.make_module(seed=5, device="cuda", precision=16, loss_structural="ssim", loss_pixel="mse")
    batch = synthetic.make_batch(2, H, W, seed=9, device="cuda")

    def check(L):
        for k in ("perceptual_rgb", "perceptual_ir", "pixel_rgb", "pixel_ir"):
            assert torch.is_tensor(L[k]) and float(L[k]) > 0, k
        assert torch.equal(L['total'], (((L['det_total'] + L['pixel_rgb']) + L['pixel_ir']) + L['perceptual_rgb']) + L['perceptual_ir'])
    for graph in (True, False):
        lit.use_detector_graph = graph
        for _ in range(2):
            out = lit.forward_step(*batch, 0, step='train')
            torch.cuda.synchronize()
            check(out['loss'])
            lit.scaler.backward(out['loss']['total'])
        if graph:
            g = lit._detector_graph()
            assert g is not None and g.usable and g.captures == 1 and g.replays == 2
    lit.eval()
    with torch.no_grad():
        torch.manual_seed(3)
        out = lit.forward_step(*batch, 0, step='val')
    check(out['loss'])
    torch.manual_seed(3)
    tv, _ = lit.validation_step(batch, 0)
    assert torch.equal(tv, out['loss']['total'])


def test_off_means_off(dev, monkeypatch):
    from hallucidet_amd import ops, synthetic

    def boom(*a, **k):
        raise AssertionError("hd_ssim_loss reached with the structural loss off")
    monkeypatch.setattr(ops, "ssim_loss", boom)
    lit = synthetic.make_module(seed=5, device="cuda", precision=16)
    assert lit.loss_structural is None and lit.structural_setup() is None
    batch = synthetic.make_batch(2, H, W, seed=9, device="cuda")
    for _ in range(2):
        loss = lit.fit_step(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    g = lit._detector_graph()
    assert g is not None and g.usable and g.captures == 1 and g.replays == 2
    out = lit.forward_step(*batch, 0, step='train')
    for k in ("perceptual_rgb", "perceptual_ir"):
        assert out['loss'][k] == 0.0 and not torch.is_tensor(out['loss'][k])


@pytest.mark.parametrize("precision,bound", [(32, 1e-3), (16, 0.15)])
def test_unet_gradient_matches_oracle(dev, weights, precision, bound):
    """Every detector and pixel weight 0.0: the step's loss is 1.0 * (1 - SSIM(hall, rgb)) + 0.5 * (1 - SSIM(hall, ir)) alone.
    (1) The image gradient the U-Net's backward receives equals the float64 autograd gradient of the oracle at the product's own
    hallucinated image within the kernel test's tolerance (four times the fp32 ATen restatements' own error, or 1e-6 of the largest
    element), in both storage modes.  (2) The U-Net's parameter gradients after fit_step against oracle.unet in fp32 autograd with the
    fp32 oracle loss on the same weights, batch and ReLU decisions (tests/test_unet_gpu.py: a ulp-level difference next to zero flips a
    ReLU and decorrelates the gradients of this randomly initialised network).  Bounds on the worst tensor's rel-L2: 1e-3 in fp32 (the
    project's fp32 bound with shared decisions); 0.15 with fp16 storage, the loosest bound the project accepts for a reconstruction
    loss (tests/test_pixel_loss_gpu.py, l1).  Measured on an MI355X: 2.96e-5 in fp32 (decoder.blocks.0.conv2.1.weight) and 1.71e-2 with
    fp16 storage (encoder.layer4.2.bn2.weight, a BatchNorm weight whose gradient sum cancels); image gradient error 1.4e-10 / 1.1e-10
    against a yardstick of 3.3e-10 / 4.0e-10."""
    from hallucidet_amd import synthetic
    from oracle import unet as ou
    from _pins import assert_borrowed_decisions_are_noise, grad_agreement, unet_decisions
    for k in list(weights):
        if k.startswith("det_") or k.startswith("pixel_"):
            weights[k] = 0.0
    lit = synthetic.make_module(seed=3, device="cuda", precision=precision, loss_structural="ssim")
    ref = ou.Unet(classes=3)
    ref.load_state_dict({k: v.cpu() for k, v in lit.encoder_decoder.state_dict().items()})
    if precision == 16:
        with torch.no_grad():                  # the product's convolutions read fp16 weights
            for m in ref.modules():
                if isinstance(m, torch.nn.Conv2d):
                    m.weight.copy_(m.weight.half().float())
    batch = synthetic.make_batch(2, H, W, seed=4, device="cuda")
    imgs_rgb, _, imgs_ir, _ = batch
    lit.encoder_decoder.train()
    out = lit.forward_step(*batch, 0, step="train")
    hall_p = out["output"]["imgs_hallucinated"].float().clone()
    umasks, uvalues = unet_decisions(lit.encoder_decoder.runner)
    grabbed = []

    def grab(module, inputs, output):
        if output.requires_grad:
            output.register_hook(lambda g: grabbed.append(g.detach().double().clone()))
    handle = lit.encoder_decoder.register_forward_hook(grab)
    try:
        loss = lit.fit_step(batch)
    finally:
        handle.remove()
    scale = float(lit.scaler.scale_value)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and float(lit.optimizer.found_inf) == 0.0 and len(grabbed) == 1
    rgb, ir1 = imgs_rgb.cpu(), imgs_ir.cpu()
    # (1) the loss gradient itself
    g64, tol, yard = _tolerance(hall_p.cpu(), rgb, ir1, 1.0, 0.5, 1.0)
    err = float((grabbed[0].cpu() / scale - g64).abs().max())
    print("precision %d: image gradient error %.3e, yardstick %.3e, tolerance %.3e" % (precision, err, yard, tol))
    assert err <= tol, (err, tol)
    got = {n: p.grad.detach().cpu().clone() for n, p in lit.encoder_decoder.named_parameters()}
    # (2) end to end through the U-Net
    ir3 = ir1.expand(-1, 3, -1, -1)
    ref.train()
    uctx = ou.Ctx(ou.fp16_round if precision == 16 else (lambda x: x), umasks, uvalues)
    hall = ref(ir3, q=uctx)
    assert_borrowed_decisions_are_noise(uctx, "U-Net")
    total = (1 - so.ssim_maps(hall, rgb, torch.float32).mean()) * 1.0 + (1 - so.ssim_maps(hall, ir1, torch.float32).mean()) * 0.5
    total.backward()
    assert abs(float(loss) - float(total)) <= 2e-3 * float(total), (float(loss), float(total))
    worst = (0.0, "")
    for n, p in ref.named_parameters():
        cos, rel = grad_agreement(got[n], p.grad)
        worst = max(worst, (rel, n))
    print("precision %d ssim: worst U-Net parameter gradient rel-L2 %.2e (%s)" % (precision, worst[0], worst[1]))
    assert worst[0] <= bound, worst


def test_train_script_with_structural_loss(dev, tmp_path, capsys, monkeypatch):
    from _synth_llvip import make_tree
    from hallucidet_amd.config import Config
    monkeypatch.setattr(Config.Losses, "pixel", None)
    monkeypatch.setattr(Config.Losses, "structural", None)
    monkeypatch.setattr(Config.Losses, "hparams_losses_weights", dict(Config.Losses.hparams_losses_weights))
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    root = make_tree(tmp_path, n_train=6, n_test=2, hw=(64, 96), extra_objects=False)
    import train_hallucidet
    train_hallucidet.main(["--dataset", "llvip", "--train", root, "--test", root, "--ext", ".jpg", "--batch", "2", "--num-workers", "0",
                           "--seed", "3", "--detector", "fasterrcnn", "--epochs", "1", "--precision", "16", "--wandb-name", "ss",
                           "--structural", "ssim", "--weight-perceptual-rgb", "1.0", "--pixel", "l1", "--weight-pixel-rgb", "1.0"])
    out = capsys.readouterr().out
    assert Config.Losses.structural == "ssim" and Config.Losses.hparams_losses_weights["perceptual_rgb"] == 1.0
    losses = [float(l.split(" loss ")[1].split()[0]) for l in out.splitlines() if l.startswith("epoch 0 step")]
    assert losses and all(math.isfinite(v) for v in losses), out
    assert "val_loss=" in out and "HalluciDet   on IR  AP@50:" in out
