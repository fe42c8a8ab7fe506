"""What RetinaNet and FCOS share: one one-stage detector (RetinaNet's trunk -- layer2-4 + FPN + P6/P7 --, a dense head over five
pyramid levels, per-level top-k + class-aware NMS) around a different head, score and box code.

A detector supplies three hooks:
  `_scores(outputs)`                      the candidates' scores from head outputs of any leading shape ([B, A, K] padded, [A_l, K] per
                                          level and image): elementwise, no gradient;
  `_decode_clip(breg, anchors, shape)`    [B, C, 4] codes and anchors of the selected candidates -> boxes clipped to the image;
  `loss_padded(anchors0, gt, glab, gvalid, head_outputs, napl)`    the losses of B images that share one anchor set, from the padded
                                          targets of `detection.pad_targets`.
"""
import torch

from .. import ops
from . import detection as D


class OneStageDetector(D._DetectorBase):
    def __init__(self, anchor_generator, head_cls, num_classes, score_thresh, nms_thresh, detections_per_img, topk_candidates):
        """Registers backbone, anchor_generator, head, transform -- torchvision's order, which is the state_dict's key order."""
        super().__init__()
        self.backbone = D.BackboneWithFPN(returned_layers=(2, 3, 4), extra_blocks=D.LastLevelP6P7(256, 256))
        self.anchor_generator = anchor_generator
        self.head = head_cls(256, anchor_generator.num_anchors_per_location()[0], num_classes)
        # torchvision's GeneralizedRCNNTransform is always replaced by the reference (detector.py:43-48); build that one.
        self.transform = D.CustomGeneralizedRCNNTransform(min_size=300, max_size=300, image_mean=[0.0], image_std=[1.0],
                                                          size_divisible=1, fixed_size=(300, 300))
        self.score_thresh, self.nms_thresh = score_thresh, nms_thresh
        self.detections_per_img, self.topk_candidates = detections_per_img, topk_candidates
        self.batched_heads = True

    def _packed(self):
        return (self.backbone, self.head)

    def _trainable(self):
        return (self.backbone.fpn, self.head)

    # ------------------------------------------------------------------ reference-shaped (list based) post-processing
    def postprocess_detections(self, head_outputs, anchors, image_shapes):
        """torchvision's {RetinaNet, FCOS}.postprocess_detections [EXT]: per image, per level: `_scores` > score_thresh, top-k (1000)
        candidates, decode + clip; then class-aware NMS and the first detections_per_img."""
        detections = []
        for index in range(len(image_shapes)):
            ib, is_, il = [], [], []
            for level, anc in enumerate(anchors[index]):
                out = {k: v[level][index] for k, v in head_outputs.items()}
                num_classes = out["cls_logits"].shape[-1]
                scores = self._scores(out).flatten()
                keep = scores > self.score_thresh
                scores, topk_idxs = scores[keep], torch.where(keep)[0]
                num_topk = min(self.topk_candidates, topk_idxs.size(0))
                order = torch.sort(scores, descending=True, stable=True)[1][:num_topk]
                scores, topk_idxs = scores[order], topk_idxs[order]
                anchor_idxs = torch.div(topk_idxs, num_classes, rounding_mode="floor")
                boxes = self.box_coder.decode_single(out["bbox_regression"].detach()[anchor_idxs], anc[anchor_idxs])
                ib.append(D.clip_boxes_to_image(boxes, image_shapes[index]))
                is_.append(scores)
                il.append(topk_idxs % num_classes)
            ib, is_, il = torch.cat(ib, 0), torch.cat(is_, 0), torch.cat(il, 0)
            order, sel, _ = D._batched_nms_padded(ib[None], is_[None], il[None], torch.ones_like(is_[None], dtype=torch.bool),
                                                  self.nms_thresh, self.detections_per_img)
            keep = order[0][sel[0]]
            detections.append({"boxes": ib[keep], "scores": is_[keep], "labels": il[keep]})
        return detections

    # ------------------------------------------------------------------ batched form (no per-image / per-level host syncs)
    def postprocess_detections_padded(self, head_outputs, anchors0, napl, image_shape):
        """Same selection on padded tensors.  head_outputs: cls_logits [B, A, K], bbox_regression [B, A, 4], ...; anchors0 [A, 4], napl =
        anchors per level.  Returns boxes [B, D, 4], scores [B, D], labels [B, D], counts [B] (D = detections_per_img)."""
        B, A, K = head_outputs["cls_logits"].shape
        # every level's score > thresh / top-k (1000) in ONE launch: hd_topk_select_rows over the level segments of the [B, A*K] score
        # rows returns, per segment, the row indices of its largest entries in descending order, ties by ascending index -- what the
        # per-level `sort(descending, stable)[:k]` of the list form gives; candidates at or below the threshold carry -inf.
        scores = self._scores(head_outputs).reshape(B, A * K)
        key = torch.where(scores > self.score_thresh, scores, float("-inf"))
        idx = ops.topk_rows_segments(key, [n * K for n in napl], self.topk_candidates)          # [B, sum(min(k, n*K))]
        sc = torch.gather(key, 1, idx)
        valid = sc > float("-inf")
        aidx = torch.div(idx, K, rounding_mode="floor")                                           # anchor index within the image
        breg = torch.gather(head_outputs["bbox_regression"].detach(), 1, aidx[:, :, None].expand(-1, -1, 4))
        cb = self._decode_clip(breg, anchors0[aidx], image_shape)
        cs = torch.where(valid, sc, 0.0)
        cl = idx % K
        pick, counts = D._batched_nms_pick(cb, cs, cl, valid, self.nms_thresh, self.detections_per_img)
        return (torch.gather(cb, 1, pick[:, :, None].expand(-1, -1, 4)), torch.gather(cs, 1, pick), torch.gather(cl, 1, pick), counts)
