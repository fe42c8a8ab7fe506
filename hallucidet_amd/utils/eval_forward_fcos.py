"""Loss AND detections in one FCOS pass (reference src/utils/eval_forward_fcos.py:11-83): same function name, argument order,
assertion messages, returned keys ({'classification', 'bbox_regression', 'bbox_ctrness'}) and the same call sequence on the
model (transform -> backbone -> head -> anchor_generator -> compute_loss -> postprocess_detections -> transform.postprocess).
The pass itself is eval_forward_one_stage.py's (shared with RetinaNet); the list route calls `model.compute_loss` as the reference does."""
from .eval_forward_one_stage import eval_forward_one_stage, eval_forward_one_stage_multi


def eval_forward_fcos(model, images, targets, train_det=False, model_name='fcos'):
    return eval_forward_one_stage(model, images, targets, train_det, model.compute_loss)


def eval_forward_fcos_multi(model, image_batches, target_lists, model_name='fcos'):
    """The three detector passes of one training step as one evaluation (eval_forward_one_stage_multi)."""
    return eval_forward_one_stage_multi(model, image_batches, target_lists)
