"""Loss AND detections in one pass of a one-stage detector (hallucidet_amd.models.one_stage.OneStageDetector: RetinaNet, FCOS) -- the
body the reference writes twice (src/utils/eval_forward_retinanet.py:83-160, src/utils/eval_forward_fcos.py:11-83): transform ->
backbone -> head -> anchor_generator -> losses -> postprocess_detections -> transform.postprocess.  eval_forward_retinanet.py and
eval_forward_fcos.py keep the reference's names and signatures and call in here.

With `model.batched_heads` the per-image loops of the loss and the per-image / per-level loops of the post-processing run in padded,
batched form (same arithmetic -- the GPU tests assert equality with the list route, which stays for that and for API compatibility)."""
import torch

from .eval_forward_fasterrcnn import _check_degenerate, _check_targets, _hw_of, _scale_tensor, _set_mode, check_degenerate_deferred
from ..models import detection as D


def _anchors_per_level(features, head_outputs):
    """Anchors per level (the feature maps are NHWC here: H, W = size(1), size(2)) = cells x anchors per location (1 for FCOS)."""
    cells = [f.size(1) * f.size(2) for f in features]
    per_cell = head_outputs["cls_logits"].size(1) // sum(cells)
    return [c * per_cell for c in cells]


def eval_forward_one_stage(model, images, targets, train_det, list_losses):
    """`list_losses(targets, head_outputs, anchors, napl)`: the detector's reference-shaped loss call, taken by the list route."""
    _set_mode(model, train_det)
    _check_targets(targets)
    original_image_sizes = [_hw_of(img) for img in images]

    images, targets = model.transform(images, targets)
    if targets is not None:
        _check_degenerate(targets)

    features = model.backbone(images.tensors)
    features = [features] if isinstance(features, torch.Tensor) else list(features.values())
    head_outputs = model.head(features)
    anchors = model.anchor_generator(images, features)
    napl = _anchors_per_level(features, head_outputs)

    if getattr(model, "batched_heads", False):
        gt, glab, gvalid = D.pad_targets(targets, images.tensors.device)
        losses = model.loss_padded(anchors[0], gt, glab, gvalid, head_outputs, napl)
        return losses, _detections_padded(model, head_outputs, anchors[0], napl, images.image_sizes, original_image_sizes)

    # list-based route (API compatibility with the reference's model methods; the GPU tests compare it with the batched one)
    losses = list_losses(targets, head_outputs, anchors, napl)
    per_level_outputs = {k: list(v.split(napl, dim=1)) for k, v in head_outputs.items()}
    per_level_anchors = [list(a.split(napl)) for a in anchors]
    raw = model.postprocess_detections(per_level_outputs, per_level_anchors, images.image_sizes)
    return losses, model.transform.postprocess(raw, images.image_sizes, original_image_sizes)


def _detections_padded(model, head_outputs, anchors0, napl, image_sizes, original_image_sizes):
    """Deferred (LazyDetections.deferred): launched by the first access or by the training step's flush() after the backward pass."""
    ho = {k: v.detach() for k, v in head_outputs.items()}
    training = model.transform.training

    def postprocess():
        from ..models.custom_generalized_transform import _ratios
        sb, ss, sl, counts = model.postprocess_detections_padded(ho, anchors0, napl, image_sizes[0])
        scale = None
        if not training:
            rh, rw = _ratios(image_sizes[0], original_image_sizes[0])
            scale = _scale_tensor(rw, rh, sb)
        return sb, ss, sl, counts, ((lambda b: b * scale) if scale is not None else None)
    return D.LazyDetections.deferred(postprocess, ho["cls_logits"].shape[0])


def eval_forward_one_stage_multi(model, image_batches, target_lists):
    """The hallucinated / RGB / IR detector passes of one training step (train_hallucidet.py:180,183,186) as ONE transform + trunk +
    head evaluation over the concatenated batch (frozen eval-mode detector: images are independent; FCOS's GroupNorm normalises per
    image).  Only the first batch carries a gradient and a loss (the reference discards the other two).  A one-stage detector has no
    sampler, so -- unlike the Faster R-CNN fusion -- the result is exactly that of three separate passes."""
    model.eval()
    for t in target_lists:
        _check_targets(t)
    sizes = [[(img.shape[-2], img.shape[-1]) for img in b] for b in image_batches]
    nb = [len(s) for s in sizes]
    flat_targets = [t for tl in target_lists for t in tl]
    il, flat_targets = model.transform.forward_batches(image_batches, flat_targets)       # every batch resized into its slice: no fp32 concat
    check_degenerate_deferred(model, flat_targets)          # no host synchronisation inside the step
    n0 = nb[0]
    if image_batches[0].requires_grad:
        features = list(model.backbone(il.tensors, n_active=n0).values())
        head_outputs = model.head(features, n_active=n0)
    else:
        with torch.no_grad():
            features = list(model.backbone(il.tensors).values())
            head_outputs = model.head(features)
    anchors = model.anchor_generator(il, features)
    napl = _anchors_per_level(features, head_outputs)
    gt, glab, gvalid = D.pad_targets(flat_targets[:n0], il.tensors.device)
    losses = model.loss_padded(anchors[0], gt, glab, gvalid, {k: v[:n0] for k, v in head_outputs.items()}, napl)
    dets = _detections_padded(model, head_outputs, anchors[0], napl, il.image_sizes, sizes[0]).split(nb)
    return [(losses if k == 0 else {}, d) for k, d in enumerate(dets)]
