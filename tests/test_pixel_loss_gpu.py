"""The pixel reconstruction losses (--pixel mse|l1, hd_pixel_loss) on the GPU: the kernel against fp64 torch (values, gradient, the
one-plane IR divisor, L1 ties, determinism), the training step with the option on (detector graph == eager bit for bit, the U-Net
gradient against the CPU oracle, the loss dict in training and validation), the step with the option off (the kernel is never
reached), and the root training script."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(8, 512, 640), (2, 128, 160), (1, 127, 161)]


def _inputs(N, H, W, ir_planes, seed=0, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    hall = torch.rand(N, 3, H, W, generator=g)
    rgb = torch.rand(N, 3, H, W, generator=g)
    ir = torch.rand(N, ir_planes, H, W, generator=g)
    return hall.to(dev), rgb.to(dev), ir.to(dev)


def _ref64(hall, rgb, ir, kind, w_rgb, w_ir, gs):
    h, r, i = hall.double(), rgb.double(), ir.double().expand_as(hall)
    n = h.numel()
    dr, di = h - r, h - i
    if kind == "mse":
        lr, li = (dr * dr).sum() / n, (di * di).sum() / n
        g = (w_rgb * 2 * dr + w_ir * 2 * di) / n
    else:
        lr, li = dr.abs().sum() / n, di.abs().sum() / n
        g = (w_rgb * torch.sign(dr) + w_ir * torch.sign(di)) / n
    return float(w_rgb * lr), float(w_ir * li), g * gs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ir_planes", [1, 3])
@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_kernel_matches_fp64(dev, kind, ir_planes, shape):
    from hallucidet_amd import ops
    N, H, W = shape
    hall, rgb, ir = _inputs(N, H, W, ir_planes, seed=N + H)
    w_rgb, w_ir, s = 0.75, 0.5, 1024.0
    gs = torch.tensor(s, device=dev)
    base = torch.tensor(0.3125, device=dev)
    v = ops.pixel_loss(hall, rgb, ir, kind, w_rgb, w_ir, base_total=base)
    dh = torch.zeros_like(hall)
    vg = ops.pixel_loss(hall, rgb, ir, kind, w_rgb, w_ir, base_total=base, gs=gs, dhall=dh)
    torch.cuda.synchronize()
    lr, li, g = _ref64(hall, rgb, ir, kind, w_rgb, w_ir, s)
    assert abs(float(v[0]) - lr) <= 1e-5 * abs(lr), (float(v[0]), lr)
    assert abs(float(v[1]) - li) <= 1e-5 * abs(li), (float(v[1]), li)
    assert torch.equal(v, vg), "value-only and gradient mode must give the same bits"
    assert torch.equal(v[2], (base + v[0]) + v[1])
    err = float((dh.double() - g).abs().max())
    assert err <= 1e-6 * float(g.abs().max()), (err, float(g.abs().max()))
    # gradient mode ADDS to the buffer: one rounding of (old + the same contribution)
    d0 = torch.randn(hall.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    acc = d0.clone()
    ops.pixel_loss(hall, rgb, ir, kind, w_rgb, w_ir, gs=gs, dhall=acc)
    assert torch.equal(acc, d0 + dh)
    if ir_planes == 1:
        # the IR divisor is N*3*H*W: one plane gives exactly what its three-channel copy gives
        dh3 = torch.zeros_like(hall)
        v3 = ops.pixel_loss(hall, rgb, ir.expand(-1, 3, -1, -1).contiguous(), kind, w_rgb, w_ir, base_total=base, gs=gs, dhall=dh3)
        assert torch.equal(v3, v) and torch.equal(dh3, dh)
        ref_ir = (((hall - ir) ** 2) if kind == "mse" else (hall - ir).abs()).double().sum() / (N * 3 * H * W) * w_ir
        assert abs(float(v[1]) - float(ref_ir)) <= 1e-5 * float(ref_ir)


@pytest.mark.parametrize("ir_planes", [1, 3])
def test_l1_ties_give_the_ir_term_alone(dev, ir_planes):
    from hallucidet_amd import ops
    hall, rgb, ir = _inputs(2, 128, 160, ir_planes, seed=3)
    tie = torch.zeros_like(hall, dtype=torch.bool)
    tie[..., ::2] = True                       # half the pixels: rgb == hall there, sign(0) = 0
    rgb = torch.where(tie, hall, rgb)
    gs = torch.tensor(256.0, device=dev)
    dh = torch.zeros_like(hall)
    ops.pixel_loss(hall, rgb, ir, "l1", 0.75, 0.5, gs=gs, dhall=dh)
    only_ir = torch.zeros_like(hall)
    ops.pixel_loss(hall, rgb, ir, "l1", 0.0, 0.5, gs=gs, dhall=only_ir)
    torch.cuda.synchronize()
    assert torch.equal(dh[tie], only_ir[tie])
    n = hall.numel()
    want = gs * (1.0 / torch.tensor(float(n), device=dev)) * (0.5 * torch.sign(hall - ir.expand_as(hall)))
    assert torch.equal(dh[tie], want[tie])
    assert not torch.equal(dh[~tie], only_ir[~tie])


@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_kernel_is_deterministic(dev, kind):
    from hallucidet_amd import ops
    hall, rgb, ir = _inputs(8, 512, 640, 1, seed=7)
    gs = torch.tensor(65536.0, device=dev)
    outs = []
    for _ in range(2):
        dh = torch.zeros_like(hall)
        v = ops.pixel_loss(hall, rgb, ir, kind, 1.0, 0.5, gs=gs, dhall=dh)
        outs.append((v.clone(), dh))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_module_is_a_drop_in_for_torch_losses(dev):
    from hallucidet_amd.losses.losses import Reconstruction
    hall, rgb, _ = _inputs(2, 64, 96, 1, seed=5)
    for name, ref in (("mse", F.mse_loss), ("l1", F.l1_loss)):
        mod = Reconstruction.select_loss_pixel(name)
        a = rgb.clone().requires_grad_(True)
        b = hall.clone().requires_grad_(True)
        loss = mod(a, b)                       # the reference's argument order: loss_pixel(imgs_rgb, imgs_hallucinated)
        (loss * 3.0).backward()
        a64 = rgb.double().requires_grad_(True)
        b64 = hall.double().requires_grad_(True)
        l64 = ref(a64, b64)
        (l64 * 3.0).backward()
        assert abs(float(loss) - float(l64)) <= 1e-5 * float(l64)
        for got, want in ((a.grad, a64.grad), (b.grad, b64.grad)):
            assert float((got.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------------------- the step
H, W = 128, 160


@pytest.fixture
def pixel_weights(monkeypatch):
    from hallucidet_amd.config import Config
    w = dict(Config.Losses.hparams_losses_weights)
    monkeypatch.setattr(Config.Losses, "hparams_losses_weights", w)
    w.update(pixel_rgb=1.0, pixel_ir=0.5)
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


@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("detector_name", ["fasterrcnn", "retinanet"])
def test_graph_equals_eager_bit_for_bit(dev, pixel_weights, detector_name, kind):
    from hallucidet_amd import synthetic
    lit = synthetic.make_module(seed=5, device="cuda", precision=16, detector_name=detector_name, loss_pixel=kind)
    batch = synthetic.make_batch(2, H, W, seed=9, device="cuda")
    _graph_step(lit, batch)                    # capture
    g = lit._detector_graph()
    assert g is not None and g.usable and g.captures == 1
    b = _graph_step(lit, batch)                # a pure replay from the seeded generator state
    assert g.captures == 1 and g.replays == 2
    assert float(b["pixel_rgb"]) > 0 and float(b["pixel_ir"]) > 0
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
    p_rgb, p_ir, total = lit._pixel_terms(hall, det_total, imgs_rgb, ir3)
    r = lit.encoder_decoder.runner
    r.flat_grads.zero_()
    lit.scaler.scale(total).backward()
    torch.cuda.synchronize()
    assert torch.equal(total, b["total"]), (float(total), float(b["total"]))
    assert torch.equal(det_total, b["det_total"]) and torch.equal(p_rgb, b["pixel_rgb"]) and torch.equal(p_ir, b["pixel_ir"])
    for k, kk in (("bbox_regression", "det_regression"), ("classification", "det_classification")):
        assert torch.equal(losses[k], b[kk])
    assert torch.isfinite(r.flat_grads).all() and float(r.flat_grads.abs().max()) > 0
    assert torch.equal(r.flat_grads, b["grads"])


@pytest.mark.parametrize("kind,precision,bound", [("mse", 32, 1e-3), ("l1", 32, 1e-3), ("mse", 16, 0.05), ("l1", 16, 0.15)])
def test_unet_gradient_matches_oracle(dev, pixel_weights, monkeypatch, precision, bound, kind):
    """Every detector weight 0.0: the step's loss is the pixel loss alone.  (1) The image gradient the U-Net's backward receives
    equals the fp64 loss gradient at the product's own hallucinated image to 1e-6 of its largest element.  (2) The U-Net's parameter
    gradients after fit_step against oracle.unet in fp32 autograd with F.mse_loss / F.l1_loss on the same weights, batch and
    discrete decisions: the ReLU decisions (tests/test_unet_gpu.py: a ulp-level difference next to zero flips a ReLU and decorrelates
    the gradients of this randomly initialised network far beyond the arithmetic's own error) and, for L1, the sign of each pixel
    difference (a difference within rounding noise of 0 flips sign(d), moving that pixel's gradient by 2/n).  Bounds: rel-L2 1e-3 in
    fp32 (tests/test_fp32_mode_gpu.py's bound with shared decisions; measured 7e-5 mse, 1.9e-4 l1).  With fp16 storage the worst
    tensor is an encoder BatchNorm weight, whose gradient sum(dy * xhat) cancels: 0.05 for mse (tests/test_step_gpu.py's end-to-end
    U-Net bound; measured 0.035) and 0.15 for l1 (measured 0.096: its image gradient is +-1/n everywhere, so that sum cancels harder).
    (1) holds the loss gradient itself to 1e-6 in both storage modes."""
    from hallucidet_amd import synthetic
    from oracle import unet as ou
    from _pins import assert_borrowed_decisions_are_noise, grad_agreement, unet_decisions
    for k in list(pixel_weights):
        if k.startswith("det_"):
            pixel_weights[k] = 0.0
    lit = synthetic.make_module(seed=3, device="cuda", precision=precision, loss_pixel=kind)
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
    # (1) the loss gradient itself
    _, _, g64 = _ref64(hall_p, imgs_rgb, imgs_ir, kind, 1.0, 0.5, 1.0)
    err = float((grabbed[0] / scale - g64).abs().max())
    assert err <= 1e-6 * float(g64.abs().max()), err
    got = {n: p.grad.detach().cpu().clone() for n, p in lit.encoder_decoder.named_parameters()}
    # (2) end to end through the U-Net
    rgb, ir3 = imgs_rgb.cpu(), imgs_ir.cpu().expand(-1, 3, -1, -1)
    ref.train()
    uctx = ou.Ctx(ou.fp16_round if precision == 16 else (lambda x: x), umasks, uvalues)
    hall = ref(ir3, q=uctx)
    assert_borrowed_decisions_are_noise(uctx, "U-Net")
    hp = hall_p.cpu()
    if kind == "mse":
        total = F.mse_loss(rgb, hall) * 1.0 + F.mse_loss(ir3, hall) * 0.5
    else:
        terms = []
        for t in (rgb, ir3):
            s_p, s_o = torch.sign(hp - t), torch.sign(hall.detach() - t)
            flips = s_p != s_o                 # borrowed sign decisions: few, and only where the difference is rounding noise
            assert int(flips.sum()) <= 5e-3 * flips.numel() and float((hall.detach() - t)[flips].abs().max() if flips.any() else 0) <= 2e-2
            terms.append((s_p * (hall - t)).mean())
        total = terms[0] * 1.0 + terms[1] * 0.5
    total.backward()
    assert abs(float(loss) - float(total)) <= 2e-3 * float(total), (float(loss), float(total))
    worst = (0.0, "")
    for n, p in ref.named_parameters():
        cos, rel = grad_agreement(got[n], p.grad)
        worst = max(worst, (rel, n))
    print("precision %d %s: worst U-Net parameter gradient rel-L2 %.2e (%s)" % (precision, kind, worst[0], worst[1]))
    assert worst[0] <= bound, worst


def test_loss_dict_in_training_and_validation(dev, pixel_weights):
    from hallucidet_amd import synthetic
    lit = synthetic.make_module(seed=5, device="cuda", precision=16, loss_pixel="mse")
    batch = synthetic.make_batch(2, H, W, seed=9, device="cuda")
    for graph in (True, False):
        lit.use_detector_graph = graph
        for _ in range(2):
            out = lit.forward_step(*batch, 0, step='train')
            L = out['loss']
            torch.cuda.synchronize()
            assert torch.is_tensor(L['pixel_rgb']) and torch.is_tensor(L['pixel_ir']) and float(L['pixel_rgb']) > 0
            assert L['perceptual_rgb'] == 0.0 and L['perceptual_ir'] == 0.0
            assert torch.equal(L['total'], (L['det_total'] + L['pixel_rgb']) + L['pixel_ir'])
            lit.scaler.backward(L['total'])
        if graph:
            g = lit._detector_graph()
            assert g is not None and g.usable and g.captures == 1 and g.replays == 2
    lit.eval()
    with torch.no_grad():
        torch.manual_seed(3)
        out = lit.forward_step(*batch, 0, step='val')
    L = out['loss']
    assert torch.equal(L['total'], (L['det_total'] + L['pixel_rgb']) + L['pixel_ir']) and float(L['pixel_ir']) > 0
    torch.manual_seed(3)
    tv, _ = lit.validation_step(batch, 0)
    assert torch.equal(tv, L['total'])


def test_off_means_off(dev, monkeypatch):
    from hallucidet_amd import ops, synthetic

    def boom(*a, **k):
        raise AssertionError("hd_pixel_loss reached with the pixel loss off")
    monkeypatch.setattr(ops, "pixel_loss", boom)
    lit = synthetic.make_module(seed=5, device="cuda", precision=16)
    assert lit.loss_pixel is None and lit.pixel_setup() is None
    batch = synthetic.make_batch(2, H, W, seed=9, device="cuda")
    for _ in range(2):
        loss = lit.fit_step(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    g = lit._detector_graph()
    assert g is not None and g.usable and g.captures == 1 and g.replays == 2
    out = lit.forward_step(*batch, 0, step='train')
    assert out['loss']['pixel_rgb'] == 0.0 and out['loss']['pixel_ir'] == 0.0 and not torch.is_tensor(out['loss']['pixel_rgb'])


def test_train_script_with_pixel_loss(dev, tmp_path, capsys, monkeypatch):
    from _synth_llvip import make_tree
    from hallucidet_amd.config import Config
    monkeypatch.setattr(Config.Losses, "pixel", None)
    monkeypatch.setattr(Config.Losses, "hparams_losses_weights", dict(Config.Losses.hparams_losses_weights))
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    root = make_tree(tmp_path, n_train=6, n_test=2, hw=(64, 96), extra_objects=False)
    import train_hallucidet
    train_hallucidet.main(["--dataset", "llvip", "--train", root, "--test", root, "--ext", ".jpg", "--batch", "2", "--num-workers", "0",
                           "--seed", "3", "--detector", "fasterrcnn", "--epochs", "1", "--precision", "16", "--wandb-name", "px",
                           "--pixel", "l1", "--weight-pixel-rgb", "1.0"])
    out = capsys.readouterr().out
    assert Config.Losses.pixel == "l1" and Config.Losses.hparams_losses_weights["pixel_rgb"] == 1.0
    losses = [float(l.split(" loss ")[1].split()[0]) for l in out.splitlines() if l.startswith("epoch 0 step")]
    assert losses and all(math.isfinite(v) for v in losses), out
    assert "val_loss=" in out and "HalluciDet   on IR  AP@50:" in out
