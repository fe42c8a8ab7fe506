"""The CPU definitions of tests/_detection_reference.py checked without a GPU.  First each definition against an independent second
statement of the same operation (the project's own per-op code on CPU tensors -- _match_batched, BoxCoder.encode_single / decode_single,
clip_boxes_to_image --, torch.sort, torch.softmax / sigmoid in float64, oracle.kernels); these serve as a cross-check here only, the
kernels are compared with the definitions.  Then the case tables of test_detection_kernels_gpu.py against mutants: a subtly wrong copy
of each definition (or of the fp32 stand-in kernel) must be rejected by the very cases and checks the GPU tests apply."""
import numpy as np
import pytest
import torch

import _detection_reference as R
from oracle import kernels as ok


def T(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------------------------ top-k
def test_topk_key_order_is_torch_sort_nan_included():
    """order_keys (what order_key() in the kernel has to produce) sorted descending with ascending indices among equals is torch.sort's
    stable descending order on every row kind -- with NaNs of both signs and several payloads all first, in index order."""
    for nan in (False, True):
        for name, scores, segs, k in R.topk_cases(nan):
            assert torch.equal(R.ref_topk_segments(scores, segs, k, "keys"), R.ref_topk_segments(scores, segs, k)), name
    x = np.array([1.0, np.nan, -np.inf, np.inf, -0.0, 0.0], np.float32)
    x[1:2] = np.array([0xFFC00001], np.uint32).view(np.float32)
    assert R.ref_topk(x, 6).tolist() == [1, 3, 0, 4, 5, 2]


@pytest.mark.parametrize("mutant,nan", [("neg_zero_less", False), ("tie_high", False), ("nan_bits", True)])
def test_topk_cases_catch(mutant, nan):
    caught = [name for name, scores, segs, k in R.topk_cases(nan)
              if not torch.equal(R.ref_topk_segments(scores, segs, k, mutant), R.ref_topk_segments(scores, segs, k))]
    assert len(caught) >= 10, caught
    if nan:                                                # the ordinary rows hold no NaN: they do not depend on its mapping
        assert all(torch.equal(R.ref_topk_segments(s, g, k, mutant), R.ref_topk_segments(s, g, k)) for _, s, g, k in R.topk_cases(False))


# ------------------------------------------------------------------------------------------------------------------ sampler
def _sample_cases():
    for A in R.SAMPLE_A:
        for gi, group in enumerate(R.SAMPLE_GROUPS):
            for ki, keykind in enumerate(R.SAMPLE_KEYS):
                yield (A, group, keykind), R.sample_case(A, group, keykind, A + 10 * gi + ki)


def test_sampler_definition_and_rows():
    assert R.sample_lds_limit() == 30720 and 4 * 30721 + ((30721 + 3) & ~3) > 150 * 1024 and max(R.SAMPLE_A) == 30721
    seen = set()
    for what, c in _sample_cases():
        lab, keys, B, cap = c["labels"], c["keys"].to(torch.int64), c["batch_size"], c["cap_pos"]
        pos, neg, counts = R.ref_sample(lab, c["keys"], B, cap)
        # second statement: keyed top-k by one stable sort per class, non-members pushed behind every member
        P, Nn = (lab >= 1).sum(1), (lab == 0).sum(1)
        num_pos = P.clamp(max=cap)
        num_neg = torch.minimum(Nn, B - num_pos)
        assert torch.equal(counts, torch.stack([num_pos, num_neg], 1)), what
        for member, num, got in ((lab >= 1, num_pos, pos), (lab == 0, num_neg, neg)):
            order = torch.sort(torch.where(member, keys, torch.full_like(keys, 1 << 40)), dim=1, stable=True)[1]
            want = torch.zeros_like(member).scatter_(1, order, torch.arange(lab.shape[1])[None, :] < num[:, None])
            assert torch.equal(got, want), what
        assert int(lab.min()) >= -1 and int(lab.max()) <= 5
        if what[0] >= 1023:
            for n, row in enumerate(c["rows"]):
                seen.add(row)
                p, q = int(P[n]), int(Nn[n])
                if row == "P==cap":
                    assert p == cap
                elif row == "P==cap+1":
                    assert p == cap + 1 and int(counts[n, 0]) == cap
                elif row == "P==cap-1":
                    assert p == cap - 1
                elif row == "P>batch, num_neg=0":
                    assert cap == B and p > B and q > 0 and int(counts[n, 1]) == 0
                elif row == "no positives":
                    assert p == 0 and q > B
                elif row == "nothing to sample":
                    assert p == 0 and q == 0
                elif row == "fewer candidates than the batch":
                    assert 0 < p + q < B and int(counts[n].sum()) == p + q
    assert len(seen) == 9


@pytest.mark.parametrize("mutant", ["tie_high", "cap_off"])
def test_sampler_cases_catch(mutant):
    caught = [what for what, c in _sample_cases()
              if any(not torch.equal(a, b) for a, b in zip(R.ref_sample(c["labels"], c["keys"], c["batch_size"], c["cap_pos"], mutant),
                                                           R.ref_sample(c["labels"], c["keys"], c["batch_size"], c["cap_pos"])))]
    assert len(caught) >= 6, caught
    if mutant == "tie_high":                               # only tied keys can tell: never the uniform ones
        assert all(w[2] in ("eight", "equal") for w in caught) and {w[0] for w in caught} >= {1023, 1024, 1025, 3000, 30721}


# ------------------------------------------------------------------------------------------------------------------ matcher
def _match_cases():
    for G in R.MATCH_G:
        for A in R.MATCH_A:
            for shared in (True, False):
                yield (G, A, shared), R.match_case(G, A, shared, 1000 * G + A)


def test_matcher_definition_equals_per_op_code():
    import hallucidet_amd.models.detection as D
    for what, c in _match_cases():
        gt, gv, gl, bx = c["gt"], c["gvalid"], c["glabels"], c["boxes"]
        N, G, A = gt.shape[0], gt.shape[1], bx.shape[-2]
        bxn = bx[None].expand(N, -1, -1) if bx.dim() == 2 else bx
        iou = torch.stack([ok.box_iou(gt[n], bxn[n]) for n in range(N)])
        assert all(R.bits_equal(R.emu_iou(gt[n], bxn[n]), iou[n].numpy()) for n in range(N)), what
        for high, low, lq in R.MATCH_THRESHOLDS:
            ref = R.ref_match(gt, gv, gl, bx, high, low, lq, R.ROI_WEIGHTS)
            m = D._match_batched(iou, gv, high, low, lq)
            assert torch.equal(ref["matched"], m), (what, high)
            lab = torch.gather(gl, 1, m.clamp(min=0))
            lab = torch.where(m == -1, torch.zeros_like(lab), lab)
            lab = torch.where(m == -2, torch.full_like(lab, -1), lab)
            lab = torch.where(gv.any(1)[:, None], lab, torch.zeros_like(lab))
            assert torch.equal(ref["labels"], lab), (what, high)
            picked = torch.gather(gt, 1, m.clamp(min=0)[:, :, None].expand(-1, -1, 4)).reshape(-1, 4)
            with np.errstate(all="ignore"):
                enc = D.BoxCoder(R.ROI_WEIGHTS).encode_single(picked, bxn.reshape(-1, 4)).reshape(N, A, 4).numpy()
            exact, ratio = R.check_encode(enc, ref["enc"])
            assert exact and ratio <= 2.0, (what, high, exact, ratio)          # torch's CPU logf: a cross-check, twice the device bound
    one = R.ref_match(c["gt"], c["gvalid"], None, c["boxes"], 0.5, 0.5, False)
    assert set(one["labels"].unique().tolist()) <= {0, 1} and "enc" not in one


def test_matcher_designed_rows():
    """The designed boxes of image 0 do what their comments say (G = 64, A = 255)."""
    c = R.match_case(64, 255, False, 1)
    rpn = R.ref_match(c["gt"], c["gvalid"], None, c["boxes"], 0.7, 0.3, True)["matched"][0].tolist()
    roi = R.ref_match(c["gt"], c["gvalid"], None, c["boxes"], 0.5, 0.5, False)["matched"][0].tolist()
    iou = R.emu_iou(c["gt"][0], c["boxes"][0])
    assert iou[0, 0] == np.float32(0.5) and iou[1, 1] == np.float32(0.7) and iou[2, 3] == np.float32(0.3) and iou[3, 4] == iou[3, 5] == np.float32(0.5)
    assert roi[0] == 0 and rpn[0] == -2                    # IoU == low == high of the RoI heads: matched; between for the RPN
    assert rpn[1] == 1 and rpn[2] == 1                     # IoU == high: matched
    assert rpn[3] == -2 and roi[3] == -1                   # IoU == low of the RPN: between, not below
    assert rpn[4] == 3 and rpn[5] == 3 and roi[4] == 3     # both best boxes of GT D take the low-quality match
    assert rpn[6] == -1 and not iou[:, 6].any()            # zero-area proposal
    assert rpn[10] == 4 and iou[5, 10] == iou[5].max() < np.float32(0.3)          # best box of E, matched to its own arg-max F
    assert rpn[11] == 9 and rpn[12] == 7 and not bool(c["gvalid"][0, 6]) and torch.equal(c["gt"][0, 6], c["gt"][0, 9]) and torch.equal(c["gt"][0, 8], c["gt"][0, 7])
    assert not R.ref_match(c["gt"], c["gvalid"], c["glabels"], c["boxes"], 0.7, 0.3, True)["labels"][1].any()          # the image without GT


@pytest.mark.parametrize("mutant", ["last_max", "lq_gt_index", "low_le", "high_le", "by_zeros"])
def test_matcher_cases_catch(mutant):
    caught = set()
    for what, c in _match_cases():
        for high, low, lq in R.MATCH_THRESHOLDS:
            a = R.ref_match(c["gt"], c["gvalid"], c["glabels"], c["boxes"], high, low, lq, None, mutant)
            b = R.ref_match(c["gt"], c["gvalid"], c["glabels"], c["boxes"], high, low, lq)
            if not torch.equal(a["matched"], b["matched"]):
                caught.add((what[0], lq))
    if mutant in ("low_le", "high_le"):
        assert {(1, False), (64, True), (64, False), (300, True)} <= caught, caught          # at both threshold pairs
    elif mutant == "lq_gt_index":
        assert {(64, True), (65, True), (300, True)} <= caught, caught
    else:
        assert {(g, lq) for g in (64, 65, 300) for lq in (True, False)} <= caught, caught


def test_encode_tolerance_rejects_a_wrong_target():
    c = R.match_case(64, 257, False, 5)
    ref = R.ref_match(c["gt"], c["gvalid"], c["glabels"], c["boxes"], 0.5, 0.5, False, R.ROI_WEIGHTS)
    enc = ref["enc"]
    with np.errstate(all="ignore"):
        good = np.concatenate([enc["xy"], enc["wh"].astype(np.float32)], -1)
    assert R.check_encode(good, enc) == (True, R.check_encode(good, enc)[1]) and R.check_encode(good, enc)[1] <= 1.0
    rows = (ref["matched"].numpy() >= 0) & ref["has_gt"][:, None]
    n, a = np.argwhere(rows & np.isfinite(good).all(-1) & (np.abs(good[..., 2:]) > 0.1).all(-1))[0]
    for k in range(4):
        bad = good.copy()
        if k < 2:
            bad[n, a, k] = np.nextafter(bad[n, a, k], np.float32(1e9))          # dx, dy: one fp32 step
        else:
            bad[n, a, k] *= np.float32(1 + 2.0 ** -20)       # dw, dh: 8 .. 16 fp32 steps (the bound: 3.76 ulp of the logarithm + 1/2 ulp)
        exact, ratio = R.check_encode(bad, enc, rows)
        assert (not exact) if k < 2 else ratio > 1.0, k
    bad = good.copy()
    bad[np.isinf(good)] = np.nan                            # the zero-area proposal's pattern
    assert np.isinf(good).any() and R.check_encode(bad, enc, rows) != R.check_encode(good, enc, rows)


# ------------------------------------------------------------------------------------------------------------------ NMS
def test_nms_definitions_equal_the_oracle():
    for n, seed in ((1, 0), (65, 1), (700, 2), (4161, 3)):
        b = R.clustered_boxes(n, seed)
        for thr in (0.5, 0.7):
            assert np.array_equal(R.ref_nms_sorted(b, thr), ok.nms_sorted(torch.from_numpy(b), thr).numpy()), (n, thr)
    keep = np.zeros(200, bool)
    keep[[0, 5, 63, 64, 130]] = True
    assert R.early_stop(keep, 3).nonzero()[0].tolist() == [0, 5, 63] and R.early_stop(keep, 4).nonzero()[0].tolist() == [0, 5, 63, 64]
    assert np.array_equal(R.early_stop(keep, 5), keep) and np.array_equal(R.early_stop(keep, 6), keep)


def test_nms_word_group_cases_reach_across_groups():
    """In the n = 4161 and 8300 cases some box of a chunk >= 65 is suppressed ONLY by kept boxes more than 64 chunks before its own: a
    reduction that ORs only the first 64 words after the current chunk keeps it."""
    for n in (4161, 8300):
        b = R.nms_big_boxes(n, 7 * n)
        keep = R.ref_nms_sorted(b, 0.5)
        assert R.emu_iou(b[2:3], b[3:4])[0, 0] == np.float32(0.5) and keep[2] and keep[3] and not R.ref_nms_sorted(b[:4], np.nextafter(np.float32(0.5), np.float32(0)))[3]
        kept = np.nonzero(keep)[0]
        iou = R.emu_iou(b[kept], b)                          # [kept, n]
        sup = (iou > np.float32(0.5)) & (kept[:, None] < np.arange(n)[None, :])
        near = sup & (np.arange(n)[None, :] // 64 - kept[:, None] // 64 <= 64)
        assert int((sup.any(0) & ~near.any(0) & ~keep).sum()) > 0, n


def _pick_second_statement(c, thr, top_n):
    """torchvision's batched_nms coordinate trick in torch fp32 ops (as models/detection.py: _batched_nms_padded states it), the greedy
    scan by the oracle."""
    boxes, scores, idxs, valid = T(c["boxes"]), T(c["scores"]), T(c["idxs"]), T(c["valid"])
    B, n = scores.shape
    key = torch.where(valid, scores, torch.full_like(scores, float("-inf")))
    order = torch.sort(key, dim=1, descending=True, stable=True)[1]
    counts = valid.sum(1)
    bmax = torch.where(valid[..., None], boxes, torch.full_like(boxes, float("-inf"))).amax(dim=(1, 2))
    bmax = torch.where(counts > 0, bmax, torch.zeros_like(bmax))
    shifted = boxes + (idxs.to(boxes) * (bmax[:, None] + 1))[:, :, None]
    picks, cnts = [], []
    for b in range(B):
        cnt = int(counts[b])
        keep = ok.nms_sorted(shifted[b][order[b, :cnt]], thr) if cnt else torch.zeros(0, dtype=torch.bool)
        surv = order[b, :cnt][keep][:top_n]
        picks.append(torch.cat([surv, order[b, :1].expand(min(top_n, n) - len(surv))]))
        cnts.append(len(surv))
    return torch.stack(picks), torch.tensor(cnts)


def _pick_cases():
    for n in (1, 64, 65, 300):
        yield ("pick", n), R.nms_pick_case(n, 40 + n), n
    for segs in R.NMS_SEGMENTS:
        yield ("segments", tuple(segs)), R.nms_segments_case(segs, 60 + len(segs)), sum(segs)


def test_nms_pick_definition_equals_torch_statement():
    for what, c, n in _pick_cases():
        if "segs" in c:                                    # what the segment kernel relies on: every segment in descending score order
            off = 0
            for s in c["segs"]:
                assert bool((np.diff(c["scores"][:, off:off + s], axis=1) <= 0).all())
                off += s
            assert np.array_equal(c["idxs"][0], np.repeat(np.arange(len(c["segs"])), c["segs"]))
        for thr in (0.7, 0.3):
            total = int(R.ref_nms_pick_rows(c["boxes"], c["scores"], c["idxs"], c["valid"], thr, n)[1].max())
            for top_n in R.top_n_values(total, n):
                a = R.ref_nms_pick_rows(c["boxes"], c["scores"], c["idxs"], c["valid"], thr, top_n)
                b = _pick_second_statement(c, thr, top_n)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (what, thr, top_n)
                assert int(a[1][1]) == 0


@pytest.mark.parametrize("mutant", ["shift_per_category", "unstable_merge", "tie_high", "iou_ge", "carry_dropped"])
def test_nms_pick_cases_catch(mutant):
    caught = set()
    for what, c, n in _pick_cases():
        for thr in (0.7, 0.3):
            a = R.ref_nms_pick_rows(c["boxes"], c["scores"], c["idxs"], c["valid"], thr, n, mutant)
            b = R.ref_nms_pick_rows(c["boxes"], c["scores"], c["idxs"], c["valid"], thr, n)
            if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
                caught.add(what)
    if mutant == "iou_ge":                                 # the planted pairs at IoU == 0.7 and == 0.3
        assert {("pick", 64), ("pick", 65), ("pick", 300), ("segments", (70, 1, 130, 64)), ("segments", (257, 600)), ("segments", (300,))} <= caught, caught
        return
    if mutant == "carry_dropped":                          # every segment longer than one 256-candidate round
        assert caught == {("segments", (257, 600)), ("segments", (300,))}, caught
        return
    assert {k for k, _ in caught} == {"pick", "segments"}, caught
    if mutant == "shift_per_category":
        assert ("segments", (70, 1, 130, 64)) in caught and ("pick", 65) in caught
    if mutant == "unstable_merge":
        assert {("segments", (70, 1, 130, 64)), ("segments", (257, 600)), ("segments", (1,) * 8)} <= caught


# ------------------------------------------------------------------------------------------------------------------ decoding
def test_decode_definition_equals_per_op_code():
    import hallucidet_amd.models.detection as D
    for Rn, K in R.ROI_DECODE_SIZES:
        c = R.roi_decode_case(Rn, K, 200 + Rn)
        dec = R.emu_decode(c["codes"].reshape(Rn, K, 4), c["rois"][:, None, 1:], R.ROI_WEIGHTS, R.XCLIP, *c["img"])
        coder = D.BoxCoder(R.ROI_WEIGHTS)
        want = D.clip_boxes_to_image(coder.decode_single(T(c["codes"]), T(c["rois"][:, 1:])).reshape(Rn, K, 4), c["img"]).numpy()
        # (a cross-check: on the CPU torch divides by the weight where the kernel multiplies by its fp32 reciprocal, and has its own expf)
        assert R.close_ratio(want, dec["ref"], dec["tol"]) <= 4.0 and R.close_ratio(dec["emu"], dec["ref"], dec["tol"]) <= 1.0, (Rn, K)
        if Rn >= 4:
            assert np.isnan(dec["ref"][2]).any() and (dec["ref"][3, :, 2] - dec["ref"][3, :, 0] == 0).all() and (dec["tol"][3] == 0).all()
            assert (dec["ref"][0, :, 2] == 320.0).all() and (dec["ref"][0, :, 0] == 0.0).all()          # beyond the clip: exp(XCLIP)*w


def test_rpn_cases_and_mutants():
    for N, K in R.DECODE_SIZES:
        c = R.rpn_case(N, K, 100 + K)
        ref = R.ref_rpn(c)
        assert R.close_ratio(ref["emu_boxes"], ref["boxes"], ref["boxes_tol"]) <= 1.0 and R.close_ratio(ref["emu_prob"], ref["prob"], ref["prob_tol"]) <= 1.0
        want = torch.sigmoid(T(c["obj"]).double()).numpy()[np.arange(N)[:, None], c["top"]]
        assert np.allclose(ref["prob"], want, rtol=1e-14, atol=0)
        flags = R.rpn_flags(ref["emu_boxes"], ref["emu_prob"], 1.0, 0.5)
        for (n, t), ok_ in c["expect"].items():
            assert bool(flags[n, t]) == ok_, (N, K, n, t)
        if K >= 9:
            assert flags.any() and not flags.all()
            for mutant in ("score_gt", "size_gt"):             # the designed row 0 sits on both thresholds
                m = R.rpn_flags(ref["emu_boxes"], ref["emu_prob"], 1.0, 0.5, mutant)
                assert not m[0, 0] and not np.array_equal(m, flags)
            worse = ref["emu_boxes"].copy()
            worse[0, 3] += np.spacing(worse[0, 3]) * 2         # two fp32 steps on a corner
            assert R.close_ratio(worse, ref["boxes"], ref["boxes_tol"]) > 1.0
            p = ref["emu_prob"].copy()
            p[0, 5] *= np.float32(1 + 2.0 ** -20)                 # 8 .. 16 fp32 steps
            assert R.close_ratio(p, ref["prob"], ref["prob_tol"]) > 1.0


def test_postprocess_cases_and_mutants():
    seen_expect = 0
    for ci, (Rn, S, C, counts) in enumerate(R.POSTPROCESS_CASES):
        c = R.postprocess_case(Rn, S, C, counts, 300 + ci)
        ref = R.ref_postprocess(c)
        assert R.close_ratio(ref["emu_boxes"], ref["boxes"], ref["boxes_tol"]) <= 1.0 and R.close_ratio(ref["emu_scores"], ref["scores"], ref["scores_tol"]) <= 1.0
        real = c["real"]
        sm = torch.softmax(T(c["logits"][real]).double(), 1)[:, 1:].numpy()
        assert np.allclose(ref["scores"][real], sm, rtol=2e-6, atol=0)          # (the definition takes exp of the fp32 difference l - max)
        assert [int(real[i * S:(i + 1) * S].sum()) for i in range(len(counts))] == [min(k, Rn - i * S) for i, k in enumerate(counts)]
        assert np.isnan(c["logits"][~real]).all() and np.isnan(c["codes"][~real]).all()
        flags = R.roi_flags(ref["emu_boxes"], ref["emu_scores"], 1.0, 0.5)
        for (r, k), ok_ in c["expect"].items():
            assert bool(flags[r, k]) == ok_, (ci, r, k)
        seen_expect += len(c["expect"])
        if (~real).any():                                  # padding rows left unzeroed: NaN where exact zeros are due
            bad = R.ref_postprocess(c, mutant="pad_unzeroed")
            assert R.close_ratio(bad["emu_boxes"], ref["boxes"], ref["boxes_tol"]) == np.inf
            assert R.close_ratio(bad["emu_scores"], ref["scores"], ref["scores_tol"]) == np.inf
        if len(c["expect"]) == 3:
            for mutant in ("score_ge", "size_gt"):
                assert not np.array_equal(R.roi_flags(ref["emu_boxes"], ref["emu_scores"], 1.0, 0.5, mutant), flags), mutant
            s = ref["emu_scores"].copy()
            s[5, 0] *= np.float32(1 + 2.0 ** -20)
            assert R.close_ratio(s, ref["scores"], ref["scores_tol"]) > 1.0
    assert seen_expect >= 10


# ------------------------------------------------------------------------------------------------------------------ RoI sampling tail
def _samples_cases():
    for T_ in R.SAMPLES_T:
        for S in R.SAMPLES_S:
            for G in R.SAMPLES_G:
                for part in (0, 1):
                    yield (T_, S, G, part), R.roi_samples_case(T_, S, G, part, 17 * T_ + S + G + part)


def _padded(c, mutant=None):
    return R.ref_roi_samples_padded(c["pos"], c["neg"], c["comb"], c["lab"], c["matched"], c["gt"], c["gvalid"], c["S"], R.ROI_WEIGHTS, mutant)


def test_roi_samples_definition_equals_per_op_code():
    import hallucidet_amd.models.detection as D
    coder = D.BoxCoder(R.ROI_WEIGHTS)
    both = 0
    for what, c in _samples_cases():
        T_, S, G, part = what
        ref = _padded(c)
        assert ref["counts"].tolist() == [min(k, T_, S) for k in c["want"]], what
        both += int((c["pos"] & c["neg"]).sum())
        assert set(np.unique(c["matched"]).tolist()) <= {-2, -1, 0, G - 1} and not c["gvalid"][2].any()
        for n in range(4):
            on = torch.where(T(c["pos"][n]) | T(c["neg"][n]))[0][:S]
            k = len(on)
            rows = slice(n * S, n * S + k)
            assert torch.equal(ref["rois"][rows], torch.cat([torch.full((k, 1), float(n)), T(c["comb"][n])[on]], 1)), what
            assert torch.equal(ref["labels"][rows], T(c["lab"][n])[on]), what
            pad = slice(n * S + k, (n + 1) * S)
            assert torch.equal(ref["rois"][pad], torch.tensor([float(n), 0, 0, 0, 0]).expand(S - k, 5)) and bool((ref["labels"][pad] == -1).all())
            assert not ref["enc"]["xy"][pad].any() and not ref["enc"]["wh"][pad].any()
            if k:
                g = T(c["gt"][n])[T(c["matched"][n])[on].clamp(min=0)] if c["gvalid"][n].any() else torch.zeros(k, 4)
                with np.errstate(all="ignore"):
                    enc = coder.encode_single(g, T(c["comb"][n])[on]).numpy()
                sub = {key: v[rows] for key, v in ref["enc"].items()}
                exact, ratio = R.check_encode(enc, sub)
                assert exact and ratio <= 2.0, (what, n, exact, ratio)
                if n == 2:
                    assert np.isneginf(sub["wh"]).all()          # the zero GT box of the image without GT: log(0 / ew)
        sel = R.finish_sel(c, 257, T_)
        fin = R.ref_roi_samples(sel, c["comb"], c["lab"], c["matched"], c["gt"], c["gvalid"], R.ROI_WEIGHTS)
        assert bool((fin["labels"][3::4] == -1).all()) and torch.equal(fin["rois"][3::4, 0], T((-sel[3::4] - 1).astype(np.float32)))
        assert not fin["rois"][3::4, 1:].any() and not fin["enc"]["xy"][3::4].any() and fin["pad"][3::4].all() and not fin["pad"][0::4].any()
    assert both > 100


@pytest.mark.parametrize("mutant", ["carry_dropped", "double_count"])
def test_roi_samples_cases_catch(mutant):
    caught = set()
    for what, c in _samples_cases():
        a, b = _padded(c, mutant), _padded(c)
        if not (torch.equal(a["rois"], b["rois"]) and torch.equal(a["labels"], b["labels"]) and torch.equal(a["counts"], b["counts"])):
            caught.add(what[:2])
    if mutant == "carry_dropped":                          # every T with a second round, at both S; never a single-round T
        assert caught == {(t, s) for t in (257, 600) for s in R.SAMPLES_S}, caught
    else:
        assert {(t, s) for t in (255, 256, 257, 600) for s in R.SAMPLES_S} <= caught, caught


# ------------------------------------------------------------------------------------------------------------------ level mapper
def test_level_cases():
    c = R.level_case()
    keep, designed = c["keep"], c["designed"]
    lev, dist = R.ref_levels(c["boxes"])
    nd = int(designed.sum())
    assert nd == 24 and keep[:nd].all()                    # no designed box is left out
    assert float((~keep[nd:]).mean()) <= 0.01 and len(keep) - nd == 4000
    assert torch.equal(lev[:nd], c["expect"][:nd])         # the hand-stated levels are the float64 definition's
    assert (dist[:21] < 2e-7).all()                        # ... although every designed square sits on a level boundary
    assert c["expect"][:21:3].tolist() == [0, 0, 1, 2, 3, 3, 3] and c["expect"][21:24].tolist() == [0, 0, 3]
    b = c["boxes"]
    x = np.sqrt((b[:21:3, 2] - b[:21:3, 0]) * (b[:21:3, 3] - b[:21:3, 1])) * (np.float32(1) / np.float32(224))
    assert x.dtype == np.float32 and x.tolist() == [2.0 ** j for j in range(-3, 4)]
    t = T(b).double()
    second = torch.floor(4 + torch.log2(torch.sqrt((t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])) / 224) + float(np.float32(1e-6))).clamp(2, 5) - 2
    assert torch.equal(lev, second.to(torch.int32))        # torchvision's LevelMapper, written with torch ops in float64
    emu = R.emu_levels(b)
    k = T(keep)
    assert torch.equal(emu[k], c["expect"][k])             # the fp32 stand-in passes the GPU test's check
    hist = torch.bincount(c["expect"][k].long(), minlength=4)
    assert int(hist.min()) > 100                           # every level is populated
    no_eps = R.ref_levels(b, "no_eps")[0]
    assert not torch.equal(no_eps[k], c["expect"][k]) and int((no_eps[:21] != c["expect"][:21]).sum()) == 3          # the shrunk 112, 224, 448 squares (the others clamp)
