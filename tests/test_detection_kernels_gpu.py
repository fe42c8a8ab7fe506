"""The selection kernels of csrc/detection.hip against the CPU definitions of tests/_detection_reference.py, at the loop edges of each
kernel.  Every index, flag, label and count is compared with torch.equal; dx/dy targets bit for bit with the fp32 emulation; what
passes through expf / logf against float64 within the tolerances derived in _detection_reference's docstring, and those tests print
`detection-kernels ratio <kernel> <largest error / tolerance>` (pytest -s shows it).

Which case covers which path:
  topk_select_kernel        n = 1023 / 1024 / 1025 / 2049: one short of, exactly, one past one 1024-thread trip and two trips + 1; k = n and
                            k = n + 5 (clamped): the everything-selected branch; k = 1024 at n = 2049: P == k; n = 4097, k = 4096: the LDS
                            capacity; segments [1, 1025, 70] with B = 3: grid (B, nseg); rows `low_byte` / `high_byte` / `quant4`: the cut
                            falls in each radix digit; `nan` rows: order_key's NaN mapping.
  sample_pos_neg_kernel     A = 1023 / 1024 / 1025 / 3000: the 1024-thread trips on the LDS path; A = 30721 = sample_lds_limit() + 1: the
                            global-memory path (lds_keys == nullptr); group `full`: num_neg = 0, the k <= 0 branch; `sparse`: k >= population.
  match_best / match_assign G = 65 / 300: second trip of the 256-thread G*4 staging loop (G > 64); A = 255 / 256 / 257 / 1025: one block, its
                            edge, two blocks, five; match_best's 1024-thread trip at A = 1025.
  nms_mask / nms_reduce     n = 4160 / 4161 / 8300: 65 / 66 / 130 chunks, i.e. one full 64-word group, a second one of one word, a third one;
                            max_keep 1 / 64 / 65 at n = 4161: the early stop at and after a chunk edge.
  nms_prepare + reduce pick n = 1 / 64 / 65 / 300 with top_n below, at and above the survivor count; a row with nothing valid.
  nms_seg_prepare / merge   segments [257, 600]: two and three rounds of the 256-wide compaction (the carry `base` crosses 256 and 512);
                            [70, 1, 130, 64], one segment, eight segments of 1; equal scores across and inside segments.
  decode / filter / post    N*K and R*K = 1, 255, 256, 257, 700 (block edges); C = 2 and 5; roi_stride 4 and 5; S = 4 and 256 with counts
                            0, 1, S-1, S.
  roi_samples_padded        T = 255 / 256 / 257 / 600: the 256-candidate rounds and their carry (candidates 255, 256 and T-1 are selected);
                            selected count 0, 1, S-1, S, S+1, T.   roi_samples_finish: R = 1, 256, 257.
  roi_levels                R = 1, 256, 257 and the whole table; strides 4 and 5.
"""
import functools

import numpy as np
import pytest
import torch

import _detection_reference as R
from oracle import kernels as ok

pytestmark = pytest.mark.gpu


def note(kernel, ratio):
    print("detection-kernels ratio %s %.4g" % (kernel, ratio))
    return ratio


def T(a, dev):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)


# ------------------------------------------------------------------------------------------------------------------ expf / logf
def test_device_expf_logf(dev):
    """The device expf and logf alone, read through kernels in which every other step is exact (_detection_reference's docstring):
    worst error in fp32 spacings of the true value, against the bound the tolerances are built on."""
    from hallucidet_amd import ops
    r = np.random.RandomState(1)
    x = (r.rand(1 << 20) * 32 - 20).astype(np.float32)
    rois = torch.tensor([[-0.5, -0.5, 0.5, 0.5]]).repeat(x.size // 2, 1)
    codes = np.zeros((x.size // 2, 4), np.float32)
    codes[:, 2:] = x.reshape(-1, 2)
    got = ops.roi_decode_clip(T(codes, dev), rois.to(dev), (1.0, 1.0, 1.0, 1.0), 80.0, (1e30, 1e30)).cpu().numpy()[:, 0, 2:]
    want = np.exp(x.reshape(-1, 2).astype(np.float64))
    e_ulps = float((np.abs(2.0 * got.astype(np.float64) - want) / R.ulp(want)).max())
    y = np.concatenate([np.exp2(r.rand((1 << 20) - (1 << 16)) * 40 - 20), 1 + (r.rand(1 << 16) * 2 - 1) * 2.0 ** -8]).astype(np.float32)
    n = y.size // 2                                        # n images of one candidate [0, 0, 1, 1] and one GT box [0, 0, gw, gh]
    gt = np.zeros((n, 1, 4), np.float32)
    gt[:, 0, 2:] = y.reshape(-1, 2)
    comb = torch.tensor([0.0, 0.0, 1.0, 1.0]).repeat(n, 1, 1)
    zeros = torch.zeros(n, 1, dtype=torch.int64, device=dev)
    _, _, reg = ops.roi_samples_finish(torch.arange(n, dtype=torch.int64, device=dev), comb.to(dev), zeros, zeros, T(gt, dev),
                                       torch.ones(n, 1, dtype=torch.bool, device=dev), (1.0, 1.0, 1.0, 1.0))
    got = reg.cpu().numpy()[:, 2:]
    want = np.log(y.reshape(-1, 2).astype(np.float64))
    l_ulps = float((np.abs(got.astype(np.float64) - want) / R.ulp(want)).max())
    print("detection-kernels measured expf %.4f ulp logf %.4f ulp" % (e_ulps, l_ulps))
    note("expf", e_ulps / R.EXPF_ULPS)
    note("logf", l_ulps / R.LOGF_ULPS)
    assert e_ulps <= R.EXPF_ULPS and l_ulps <= R.LOGF_ULPS


# ------------------------------------------------------------------------------------------------------------------ top-k
@pytest.mark.parametrize("nan", [False, True], ids=["ordinary", "nan"])
def test_topk_select_rows(dev, nan):
    """Every index list equals torch.sort(descending=True, stable=True) on the CPU.  The `nan` rows hold NaNs of both signs and several
    payloads: torch.sort lists every NaN first, in index order."""
    from hallucidet_amd import ops
    for name, scores, segs, k in R.topk_cases(nan):
        got = ops.topk_rows_segments(T(scores, dev), segs, k).cpu()
        assert torch.equal(got, R.ref_topk_segments(scores, segs, k)), name


# ------------------------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("A", R.SAMPLE_A)
def test_sample_pos_neg(dev, A):
    from hallucidet_amd import ops
    assert R.sample_lds_limit() == 30720 and (A > 30720) == (A == 30721)          # the switch point, from the `need` formula
    for gi, group in enumerate(R.SAMPLE_GROUPS):
        for ki, keykind in enumerate(R.SAMPLE_KEYS):
            c = R.sample_case(A, group, keykind, A + 10 * gi + ki)
            pos, neg, counts = ops.sample_pos_neg(c["labels"].to(dev), c["keys"].to(dev), c["batch_size"], c["cap_pos"])
            rp, rn, rc = R.ref_sample(c["labels"], c["keys"], c["batch_size"], c["cap_pos"])
            assert torch.equal(counts.cpu(), rc), (group, keykind)
            assert torch.equal(pos.cpu(), rp) and torch.equal(neg.cpu(), rn), (group, keykind)


# ------------------------------------------------------------------------------------------------------------------ matcher
@pytest.mark.parametrize("G", R.MATCH_G)
@pytest.mark.parametrize("A", R.MATCH_A)
def test_match_targets(dev, A, G):
    from hallucidet_amd import ops
    worst = 0.0
    for shared in (True, False):
        c = R.match_case(G, A, shared, 1000 * G + A)
        for high, low, lq in R.MATCH_THRESHOLDS:
            for glabels, weights in ((c["glabels"], R.ROI_WEIGHTS), (None, (1.0, 1.0, 1.0, 1.0)), (c["glabels"], None)):
                m, lab, reg = ops.match_targets(c["gt"].to(dev), c["gvalid"].to(dev), None if glabels is None else glabels.to(dev),
                                                c["boxes"].to(dev), high, low, lq, coder_weights=weights)
                ref = R.ref_match(c["gt"], c["gvalid"], glabels, c["boxes"], high, low, lq, weights)
                what = (shared, high, glabels is None, weights)
                assert torch.equal(m.cpu(), ref["matched"]), what
                assert torch.equal(lab.cpu(), ref["labels"]), what
                if weights is None:
                    assert reg is None
                    continue
                rows = (ref["matched"].numpy() >= 0) & ref["has_gt"][:, None]
                exact, ratio = R.check_encode(reg.cpu().numpy(), ref["enc"], rows)
                assert exact and ratio <= 1.0, (what, exact, ratio)
                worst = max(worst, ratio)
    note("match_targets[G=%d,A=%d].dw_dh" % (G, A), worst)


# ------------------------------------------------------------------------------------------------------------------ NMS
@functools.lru_cache(maxsize=None)
def nms_big(n):
    """B = 2 rows of n clustered boxes (row 1: n - 64 of them) and the oracle's keep flags at 0.5: computed once, shared, never modified."""
    boxes = np.zeros((2, n, 4), np.float32)
    counts = (n, n - 64)
    keep = []
    for b in range(2):
        boxes[b, :counts[b]] = R.nms_big_boxes(counts[b], 7 * n + b)
        keep.append(ok.nms_sorted(torch.from_numpy(boxes[b, :counts[b]]), 0.5).numpy())
    return boxes, counts, keep


@pytest.mark.parametrize("n", [4160, 4161, 8300])
def test_nms_sorted_batched_word_groups(dev, n):
    """65, 66 and 130 chunks: nms_reduce_kernel's second and third group of 64 mask words.  Clustered boxes: a kept box of an early chunk
    suppresses boxes more than 64 chunks later."""
    from hallucidet_amd import ops
    boxes, counts, want = nms_big(n)
    keep = ops.nms_sorted_batched(T(boxes, dev), torch.tensor(counts, dtype=torch.int32, device=dev), 0.5).cpu()
    for b in range(2):
        c = counts[b]
        assert torch.equal(keep[b, :c], torch.from_numpy(want[b])), (n, b)
        assert not keep[b, c:].any()


@pytest.mark.parametrize("max_keep", [1, 64, 65])
def test_nms_sorted_batched_early_stop(dev, max_keep):
    from hallucidet_amd import ops
    boxes, counts, want = nms_big(4161)
    keep = ops.nms_sorted_batched(T(boxes, dev), torch.tensor(counts, dtype=torch.int32, device=dev), 0.5, max_keep=max_keep).cpu()
    for b in range(2):
        c = counts[b]
        assert torch.equal(keep[b, :c], torch.from_numpy(R.early_stop(want[b], max_keep))), (max_keep, b)
        assert not keep[b, c:].any()


def _order(scores, valid):
    key = np.where(valid, scores, np.float32(-np.inf))
    return np.stack([R.stable_desc_order(k) for k in key])


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_batched_nms_pick(dev, n):
    from hallucidet_amd import ops
    c = R.nms_pick_case(n, 40 + n)
    order = _order(c["scores"], c["valid"])
    for thr in (0.7, 0.3):
        total = int(R.ref_nms_pick_rows(c["boxes"], c["scores"], c["idxs"], c["valid"], thr, n)[1][0])
        for top_n in R.top_n_values(total, n):
            pick, picked = ops.batched_nms_pick(T(c["boxes"], dev), T(c["idxs"], dev), T(c["valid"], dev), T(order, dev), thr, top_n)
            rp, rc = R.ref_nms_pick_rows(c["boxes"], c["scores"], c["idxs"], c["valid"], thr, top_n)
            assert torch.equal(picked.cpu(), rc) and torch.equal(pick.cpu(), rp), (thr, top_n)
            assert int(rc[1]) == 0 and bool((rp[1] == int(order[1, 0])).all())


@pytest.mark.parametrize("segs", R.NMS_SEGMENTS, ids=lambda s: "-".join(map(str, s)))
def test_batched_nms_pick_segments(dev, segs):
    from hallucidet_amd import ops
    c = R.nms_segments_case(segs, 60 + len(segs))
    n = sum(segs)
    for thr in (0.7, 0.3):
        total = int(R.ref_nms_pick_rows(c["boxes"], c["scores"], c["idxs"], c["valid"], thr, n)[1][2])
        for top_n in R.top_n_values(total, n):
            pick, picked = ops.batched_nms_pick_segments(T(c["boxes"], dev), T(c["scores"], dev), T(c["valid"], dev), segs, thr, top_n)
            rp, rc = R.ref_nms_pick_rows(c["boxes"], c["scores"], c["idxs"], c["valid"], thr, top_n)
            assert torch.equal(picked.cpu(), rc) and torch.equal(pick.cpu(), rp), (thr, top_n)
            assert int(rc[1]) == 0 and bool((rp[1] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ decoding
@pytest.mark.parametrize("N,K", R.DECODE_SIZES)
def test_rpn_decode_filter(dev, N, K):
    from hallucidet_amd import ops
    c = R.rpn_case(N, K, 100 + K)
    ref = R.ref_rpn(c)
    wb = wp = 0.0
    for min_size, thresh in ((1.0, 0.5), (1e-3, 0.0)):
        boxes, prob, valid = (t.cpu().numpy() for t in ops.rpn_decode_filter(T(c["deltas"], dev), T(c["obj"], dev), T(c["anchors"], dev),
                                                                             T(c["top"], dev), R.XCLIP, c["img"], min_size, thresh))
        assert torch.equal(torch.from_numpy(valid), torch.from_numpy(R.rpn_flags(boxes, prob, min_size, thresh))), (min_size, thresh)
        if min_size == 1.0:
            for (n, t), want in c["expect"].items():
                assert bool(valid[n, t]) == want, (n, t)
        wb, wp = max(wb, R.close_ratio(boxes, ref["boxes"], ref["boxes_tol"])), max(wp, R.close_ratio(prob, ref["prob"], ref["prob_tol"]))
    note("rpn_decode_filter[%dx%d].boxes" % (N, K), wb)
    note("rpn_decode_filter[%dx%d].prob" % (N, K), wp)
    assert wb <= 1.0 and wp <= 1.0


@pytest.mark.parametrize("Rn,K", R.ROI_DECODE_SIZES)
def test_roi_decode_clip(dev, Rn, K):
    from hallucidet_amd import ops
    c = R.roi_decode_case(Rn, K, 200 + Rn)
    dec = R.emu_decode(c["codes"].reshape(Rn, K, 4), c["rois"][:, None, 1:], R.ROI_WEIGHTS, R.XCLIP, *c["img"])
    worst = 0.0
    for rois in (c["rois"], c["rois"][:, 1:]):                                  # roi_stride 5 (image index in column 0) and 4
        got = ops.roi_decode_clip(T(c["codes"], dev), T(rois, dev), R.ROI_WEIGHTS, R.XCLIP, c["img"]).cpu().numpy()
        worst = max(worst, R.close_ratio(got, dec["ref"], dec["tol"]))
    note("roi_decode_clip[%dx%d]" % (Rn, K), worst)
    assert worst <= 1.0


@pytest.mark.parametrize("ci", range(len(R.POSTPROCESS_CASES)), ids=lambda i: "R%d-S%d-C%d" % R.POSTPROCESS_CASES[i][:3])
def test_roi_postprocess(dev, ci):
    from hallucidet_amd import ops
    Rn, S, C, counts = R.POSTPROCESS_CASES[ci]
    c = R.postprocess_case(Rn, S, C, counts, 300 + ci)
    ref = R.ref_postprocess(c)
    wb = ws = 0.0
    for rois in (c["rois"], c["rois"][:, 1:]):
        for min_size, thresh in ((1.0, 0.5), (1e-2, 0.05)):
            boxes, scores, valid = (t.cpu().numpy() for t in ops.roi_postprocess(T(c["logits"], dev), T(c["codes"], dev), T(rois, dev), T(c["counts"], dev),
                                                                                 S, R.ROI_WEIGHTS, R.XCLIP, c["img"], thresh, min_size))
            assert torch.equal(torch.from_numpy(valid), torch.from_numpy(R.roi_flags(boxes, scores, min_size, thresh))), (min_size, thresh)
            pad = ~c["real"]
            assert not boxes[pad].any() and not scores[pad].any() and not valid[pad].any()          # exact zeros, NaN inputs notwithstanding
            if min_size == 1.0:
                for (r, k), want in c["expect"].items():
                    assert bool(valid[r, k]) == want, (r, k)
            wb = max(wb, R.close_ratio(boxes, ref["boxes"], ref["boxes_tol"]))
            ws = max(ws, R.close_ratio(scores, ref["scores"], ref["scores_tol"]))
    note("roi_postprocess[R=%d,S=%d,C=%d].boxes" % (Rn, S, C), wb)
    note("roi_postprocess[R=%d,S=%d,C=%d].scores" % (Rn, S, C), ws)
    assert wb <= 1.0 and ws <= 1.0


# ------------------------------------------------------------------------------------------------------------------ RoI sampling tail
def _check_samples(got, ref, what):
    rois, labels, reg = got[:3]
    assert torch.equal(rois.cpu(), ref["rois"]), what
    assert torch.equal(labels.cpu(), ref["labels"]), what
    exact, ratio = R.check_encode(reg.cpu().numpy(), ref["enc"])
    assert exact and ratio <= 1.0, (what, exact, ratio)
    return ratio


@pytest.mark.parametrize("T_", R.SAMPLES_T)
@pytest.mark.parametrize("S", R.SAMPLES_S)
def test_roi_samples_padded(dev, S, T_):
    from hallucidet_amd import ops
    worst = 0.0
    for G in R.SAMPLES_G:
        for part in (0, 1):
            c = R.roi_samples_case(T_, S, G, part, 17 * T_ + S + G + part)
            got = ops.roi_samples_padded(*(T(c[k], dev) for k in ("pos", "neg", "comb", "lab", "matched", "gt", "gvalid")), S, R.ROI_WEIGHTS)
            ref = R.ref_roi_samples_padded(c["pos"], c["neg"], c["comb"], c["lab"], c["matched"], c["gt"], c["gvalid"], S, R.ROI_WEIGHTS)
            assert torch.equal(got[3].cpu(), ref["counts"]), (G, part)
            assert ref["counts"].tolist() == [min(k, T_, S) for k in c["want"]]
            worst = max(worst, _check_samples(got, ref, (G, part)))
    note("roi_samples_padded[T=%d,S=%d].dw_dh" % (T_, S), worst)


@pytest.mark.parametrize("Rn", [1, 256, 257])
def test_roi_samples_finish(dev, Rn):
    from hallucidet_amd import ops
    worst = 0.0
    for G in R.SAMPLES_G:
        c = R.roi_samples_case(600, 128, G, 1, 5 + G)
        sel = R.finish_sel(c, Rn, Rn)
        got = ops.roi_samples_finish(T(sel, dev), *(T(c[k], dev) for k in ("comb", "lab", "matched", "gt", "gvalid")), R.ROI_WEIGHTS)
        ref = R.ref_roi_samples(sel, c["comb"], c["lab"], c["matched"], c["gt"], c["gvalid"], R.ROI_WEIGHTS)
        worst = max(worst, _check_samples(got, ref, G))
    note("roi_samples_finish[R=%d].dw_dh" % Rn, worst)


# ------------------------------------------------------------------------------------------------------------------ level mapper
@pytest.mark.parametrize("Rn", [1, 256, 257, None], ids=lambda v: "all" if v is None else str(v))
def test_roi_levels(dev, Rn):
    from hallucidet_amd import ops
    c = R.level_case()
    boxes, expect, keep = c["boxes"][:Rn], c["expect"][:Rn], torch.from_numpy(c["keep"][:Rn])
    with5 = np.concatenate([np.zeros((len(boxes), 1), np.float32), boxes], 1)
    for rois in (boxes, with5):
        got = ops.roi_levels(T(rois, dev), **R.LEVEL_ARGS).cpu()
        assert torch.equal(got[keep], expect[keep])
