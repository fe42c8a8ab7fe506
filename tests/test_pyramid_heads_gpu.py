"""The three pyramid heads (RPNHead, RetinaNetHead, FCOSHead) alone, without a backbone: the ways out of their autograd Functions.

Every head's backward ends in the same three decisions -- pad a level's gradient to the whole batch or hand it to the `_hd_active`
view, walk the levels one by one (parameter gradients) or as batched grids (frozen head), skip an output that got no gradient --
and each of them must not change a single bit of the feature gradients: both sides of every comparison below launch the same
convolutions on the same operands (the tiles are pinned, so a batched grid runs the tiles of the separate launches)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3
LEVELS = ((5, 7), (3, 4), (2, 2), (1, 1), (1, 1))
KINDS = ("rpn", "retinanet", "fcos")


def _build(kind):
    from hallucidet_amd.models import detection as D
    from hallucidet_amd.models.fcos import FCOSHead
    from hallucidet_amd.models.retinanet import RetinaNetHead
    torch.manual_seed({"rpn": 31, "retinanet": 32, "fcos": 33}[kind])
    head = {"rpn": lambda: D.RPNHead(), "retinanet": lambda: RetinaNetHead(256, 9, 2), "fcos": lambda: FCOSHead(256, 1, 2)}[kind]()
    outs = {"rpn": ("cls_logits", "bbox_pred"), "retinanet": ("cls_logits", "bbox_reg"), "fcos": ("cls_logits", "bbox_reg", "bbox_ctrness")}[kind]
    with torch.no_grad():
        for name, m in head.named_modules():
            if isinstance(m, torch.nn.Conv2d):
                # the output convs wide enough that the gradients reaching the towers are not all tiny
                m.weight.normal_(0, 0.05 if name.split(".")[-1] in outs else 0.03)
                m.bias.normal_(0, 0.1)
                m.weight.copy_(m.weight.half().float())
                m.bias.copy_(m.bias.half().float())
            if isinstance(m, torch.nn.GroupNorm):              # non-trivial affine
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    return head


@pytest.fixture(scope="module")
def heads(dev):
    return {k: _build(k).to(dev) for k in KINDS}


@pytest.fixture(scope="module")
def feats(dev):
    """Five NHWC fp16 levels of N images; the first image non-negative, as after a ReLU."""
    g = torch.Generator().manual_seed(7)
    out = []
    for H, W in LEVELS:
        x = torch.randn(N, H, W, 256, generator=g)
        x[0] = x[0].abs()
        out.append(x.half().to(dev))
    return out


def _outputs(kind, head, fs, n_active=None):
    """The flattened [N, sum(HWA), C] outputs, as the training step's losses read them."""
    from hallucidet_amd.models import detection as D
    if kind == "rpn":
        logits, boxes = head(fs, n_active=n_active)
        return list(D.concat_box_prediction_layers(logits, boxes))
    return list(head(fs, n_active=n_active).values())


def _loss(outs, only=None, zeros=False):
    """sum_i (out_i * fixed_random_i).sum(); `only`: the other outputs stay out of the graph (`zeros`: enter it with zero gradients)."""
    total = None
    for i, o in enumerate(outs):
        if only is not None and i != only and not zeros:
            continue
        w = torch.randn(o.shape, generator=torch.Generator().manual_seed(100 + i)).to(o.device)
        if only is not None and i != only:
            w = torch.zeros_like(w)
        term = (o * w).sum()
        total = term if total is None else total + term
    return total


def _leaves(fs):
    return [f.clone().requires_grad_(True) for f in fs]


def _report(tag, a, b):
    d = (a.float() - b.float()).abs().max().item() if a.numel() else 0.0
    print("%s: max |diff| %.3e at gradient magnitude %.3e" % (tag, d, a.float().abs().max().item()))


@pytest.mark.parametrize("kind", KINDS)
def test_exit_paths_agree(dev, pinned_tiles, heads, feats, kind):
    """n_active = 1.  Route A: plain leaves -> the Function pads every gradient to N rows, rows 1: exactly zero.  Route B: the features
    carry `_hd_active` [1, ...] leaves (what the backbone hands out) -> [1, ...] gradients arrive there.  Same kernels, same operands."""
    head = heads[kind]
    head.train_params, head.grad_scale = False, 1.0
    a = _leaves(feats)
    _loss(_outputs(kind, head, a, n_active=1)).backward()
    full = [f.detach().clone() for f in feats]
    acts = []
    for f in full:
        f._hd_active = torch.zeros((1,) + tuple(f.shape[1:]), dtype=f.dtype, device=dev, requires_grad=True)     # values are never read
        acts.append(f._hd_active)
    _loss(_outputs(kind, head, full, n_active=1)).backward()
    for li, (la, lb) in enumerate(zip(a, acts)):
        assert la.grad is not None and lb.grad is not None, (kind, li)
        assert la.grad.shape[0] == N and lb.grad.shape[0] == 1, (kind, li)
        assert float(la.grad[1:].abs().max()) == 0.0, (kind, li)
        assert float(lb.grad.abs().max()) > 0.0, (kind, li)
        _report("%s exit level %d" % (kind, li), la.grad[:1], lb.grad)
        assert torch.equal(la.grad[:1], lb.grad), (kind, li)


@pytest.mark.parametrize("kind", ("rpn", "retinanet"))
def test_both_backward_bodies_agree(dev, pinned_tiles, heads, feats, kind):
    """n_active = N.  Frozen head: the batched grids.  `train_params`: the per-level walk (which also accumulates parameter gradients).
    Both issue the same convolutions with the same residual and mask operands; conv2d_multi is bit-identical to separate launches."""
    head = heads[kind]
    head.train_params, head.grad_scale = False, 1.0
    a = _leaves(feats)
    _loss(_outputs(kind, head, a)).backward()
    try:
        head.train_params = True
        for p in head.parameters():
            p.grad = torch.zeros_like(p)              # _wgrad_into accumulates into it
        b = _leaves(feats)
        _loss(_outputs(kind, head, b)).backward()
        assert all(float(p.grad.abs().max()) > 0.0 for p in head.parameters())
    finally:
        head.train_params = False
        for p in head.parameters():
            p.grad = None
    for li, (la, lb) in enumerate(zip(a, b)):
        _report("%s bodies level %d" % (kind, li), la.grad, lb.grad)
        assert torch.equal(la.grad, lb.grad), (kind, li)


@pytest.mark.parametrize("kind", KINDS)
def test_none_gradients(dev, pinned_tiles, heads, feats, kind):
    """Back-propagation through the classification output only: every feature gradient is still returned, the regression branch's
    parameter gradients stay untouched under `train_params`, and the result is that of explicit zero gradients for the other outputs."""
    head = heads[kind]
    reg = {"rpn": lambda: [head.bbox_pred], "retinanet": lambda: [head.regression_head], "fcos": lambda: [head.regression_head]}[kind]()
    reg_params = [p for m in reg for p in m.parameters()]
    try:
        head.train_params, head.grad_scale = True, 1.0
        for p in head.parameters():
            p.grad = torch.full_like(p, 7.0)
        a = _leaves(feats)
        _loss(_outputs(kind, head, a), only=0).backward()
        assert all(x.grad is not None and float(x.grad.abs().max()) > 0.0 for x in a), kind
        assert all(torch.equal(p.grad, torch.full_like(p, 7.0)) for p in reg_params), kind
        assert not any(torch.equal(p.grad, torch.full_like(p, 7.0)) for p in head.parameters() if all(p is not q for q in reg_params)), kind
        b = _leaves(feats)
        _loss(_outputs(kind, head, b), only=0, zeros=True).backward()
    finally:
        head.train_params = False
        for p in head.parameters():
            p.grad = None
    for li, (la, lb) in enumerate(zip(a, b)):
        _report("%s none level %d" % (kind, li), la.grad, lb.grad)
        assert torch.equal(la.grad, lb.grad), (kind, li)
