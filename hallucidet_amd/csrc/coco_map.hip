// COCO mAP on the device: the per-image matching and the per-segment accumulation of hallucidet_amd/metrics/metrics.py
// (`MeanAveragePrecision._evaluate_img` / `_accumulate`), restated rule for rule so that the precision / recall arrays come out
// bit-identical to the host evaluator's.  The final means stay on the host (metrics/device.py).
//
// hd_map_match: one wave per (image n, class k).  The image's class-k detections are ranked by descending score, ties by ascending
// detection index (np.argsort(-s, kind="mergesort")); the first HD_MAP_MAX_DET are kept.  Ground truths of class k are ordered
// non-ignored first, stably, per area range.  Lane (area a, threshold t) runs the greedy matching of _evaluate_img over the kept
// detections with IoUs in fp64 in box_iou_np's operation order (-ffp-contract=off keeps the products unfused).  Matching in score
// order is prefix-stable: the results for max-dets 1 / 10 / 100 are rank filters of this one.
//
// hd_map_accumulate: one block per (threshold, class, area, max-dets) segment.  It walks the class's detections in the global order
// (descending score, then image, then rank: the host's stable sort of the per-image lists, computed by the caller) and keeps those
// whose rank is below the max-dets cap.  A block scan gives the exact cumulative TP / FP counts; rc and pr are the host's fp64
// expressions.  The precision envelope sampled at recall r (a reverse running max read at searchsorted(rc, r, "left")) equals the
// largest pr among the points with rc >= r: every point contributes to the bins of the recall thresholds it reaches through an LDS
// integer max on the bits of the (non-negative) double, then a suffix max over the bins.  Max is exact and order-free, so the result
// does not depend on scheduling.  No float atomics.
//
// hd_mr_accumulate: the integer half of the log-average miss rate ("LAMR", MR^-2 of Dollar et al., PAMI 2012) over the same flags and
// the same global order; the float half (1 - hit / n_gt, the log-mean) is the host evaluator's numpy code on both paths, so device and
// host agree by construction.  Definition (metrics/metrics.py states the same), per class k, area range a, IoU threshold t:
//   inputs      hd_map_match's per-image results at max-dets 100 (every entry of `order`); unevaluated images contribute nothing
//   order       the caller's global order: descending score, ties in image order then rank (the host's stable sorts)
//   counts      tp_j = cumsum(matched & !ignored), fp_j = cumsum(!matched & !ignored); an ignored detection counts as neither
//   images      n_img = the images passed to update(), images without a box included; n_gt = npig[k][a]
//   undefined   n_eval[k] == 0 or n_gt == 0: -1 in every entry of the segment
//   rates       ref [9] = the host's np.logspace(-2, 0, 9) doubles, passed in (not recomputed here)
//   hit         fppi_j = double(fp_j) / double(n_img), an IEEE fp64 division; hit_i = max{tp_j : fppi_j <= ref[i]}, 0 when no point
//               qualifies or the class has no detection
//   miss rate   (host) mr_i = 1.0 - hit_i / n_gt; lamr = exp(mean(log(max(mr, 1e-10))))
// One block per (t, k, a) with the chunked block scan of hd_map_accumulate; a counted point raises LDS bin i0 = #{i : ref[i] < fppi}
// to its tp with an integer max (it qualifies for exactly the rates i >= i0), one thread takes the prefix max over the bins.
#include "hd_block.h"

namespace {

constexpr int T = HD_MAP_NUM_IOU;       // 10 IoU thresholds
constexpr int A = HD_MAP_NUM_AREA;      // 4 area ranges: all, small, medium, large
constexpr int M = HD_MAP_NUM_MAXDET;    // 3 max-dets: 1, 10, 100
constexpr int R = HD_MAP_NUM_REC;       // 101 recall thresholds
constexpr int MAXD = HD_MAP_MAX_DET;    // 100 detections kept per (image, class)
constexpr int DCAP = HD_MAP_DET_CAP;    // detections of one class in one image
constexpr int GCAP = HD_MAP_GT_CAP;     // ground truths of one class in one image
constexpr int GW = GCAP / 32;           // words of a matched-gt bitset

__device__ __forceinline__ double box_area(const double* b) { return (b[2] - b[0]) * (b[3] - b[1]); }

// box_iou_np for one pair: area_a, area_b, lt = max, rb = min, wh = clip(rb - lt, 0), inter = wh0 * wh1, inter / (area_a + area_b - inter)
__device__ __forceinline__ double pair_iou(const double* a, const double* b) {
  const double area_a = box_area(a), area_b = box_area(b);
  const double l0 = a[0] > b[0] ? a[0] : b[0], l1 = a[1] > b[1] ? a[1] : b[1];
  const double r0 = a[2] < b[2] ? a[2] : b[2], r1 = a[3] < b[3] ? a[3] : b[3];
  double w = r0 - l0, h = r1 - l1;
  w = w < 0.0 ? 0.0 : w;
  h = h < 0.0 ? 0.0 : h;
  const double inter = w * h;
  return inter / ((area_a + area_b) - inter);
}

__global__ __launch_bounds__(64) void map_match_kernel(const double* __restrict__ dbox, const double* __restrict__ dscore,
                                                       const int64_t* __restrict__ dlabel, const int32_t* __restrict__ dcount, int P,
                                                       const double* __restrict__ gbox, const int64_t* __restrict__ glabel,
                                                       const int32_t* __restrict__ gcount, int Q, const int64_t* __restrict__ classes, int K,
                                                       const double* __restrict__ iou_start, const double* __restrict__ area_rng,
                                                       int32_t* __restrict__ flags, double* __restrict__ score, int32_t* __restrict__ ndet,
                                                       int32_t* __restrict__ npos, int32_t* __restrict__ evald, int32_t* __restrict__ status) {
  __shared__ double s_sc[DCAP];           // class-k detection scores, in detection order
  __shared__ int s_di[DCAP];              // ... their detection indices
  __shared__ int s_top[MAXD];             // detection index at each rank
  __shared__ double s_db[MAXD][4];        // kept detection boxes, by rank
  __shared__ double s_gb[GCAP][4];        // class-k ground-truth boxes, in ground-truth order
  __shared__ short s_go[A][GCAP];         // per area: positions into s_gb, non-ignored first (stable)
  __shared__ int s_np[A];                 // per area: number of non-ignored ground truths
  __shared__ uint32_t s_gtm[T * A][GW];   // per (area, threshold) lane: matched ground truths (sorted positions)
  __shared__ int s_fl[A][MAXD];           // bits 0-9 matched at threshold t, bits 10-19 ignored at threshold t
  __shared__ int s_cnt[2];

  const int lane = threadIdx.x;
  const int item = blockIdx.x;            // n * K + k
  const int n = item / K, k = item - n * K;
  const int64_t cls = classes[k];
  const int64_t NK = (int64_t)gridDim.x;

  // ---- detections of class k, compacted in detection order
  int dc = dcount[n];
  if (dc < 0 || dc > P) {
    atomicMax(&status[2], 1);
    dc = dc < 0 ? 0 : P;
  }
  int cnt = 0;
  for (int base = 0; base < dc; base += 64) {
    const int j = base + lane;
    const bool hit = j < dc && dlabel[(int64_t)n * P + j] == cls;
    const uint64_t bal = __ballot(hit);
    const int pos = cnt + hd_ballot_rank(bal, lane);
    if (hit && pos < DCAP) {
      s_sc[pos] = dscore[(int64_t)n * P + j];
      s_di[pos] = j;
    }
    cnt += __popcll(bal);
  }
  int gc = gcount[n];
  if (gc < 0 || gc > Q) {
    atomicMax(&status[2], 1);
    gc = gc < 0 ? 0 : Q;
  }
  int G = 0;
  for (int base = 0; base < gc; base += 64) {
    const int j = base + lane;
    const bool hit = j < gc && glabel[(int64_t)n * Q + j] == cls;
    const uint64_t bal = __ballot(hit);
    const int pos = G + hd_ballot_rank(bal, lane);
    if (hit && pos < GCAP) {
      const double* b = gbox + ((int64_t)n * Q + j) * 4;
      s_gb[pos][0] = b[0]; s_gb[pos][1] = b[1]; s_gb[pos][2] = b[2]; s_gb[pos][3] = b[3];
    }
    G += __popcll(bal);
  }
  __syncthreads();
  const bool over = cnt > DCAP || G > GCAP;
  if (lane == 0) {
    if (cnt > DCAP) atomicMax(&status[0], cnt);
    if (G > GCAP) atomicMax(&status[1], G);
  }
  const bool ev = (cnt > 0 || G > 0) && !over;
  if (!ev) {
    if (lane == 0) {
      ndet[item] = 0;
      evald[item] = 0;
    }
    if (lane < A) npos[(int64_t)item * A + lane] = 0;
    return;
  }
  const int D = cnt < MAXD ? cnt : MAXD;
  for (int r = lane; r < MAXD; r += 64) s_top[r] = s_di[0];
  __syncthreads();

  // ---- rank = #{i : s_i > s_j or (s_i == s_j and i < j)}: a strict total order, so the ranks below MAXD are distinct
  for (int j = lane; j < cnt; j += 64) {
    const double sj = s_sc[j];
    int rank = 0;
    for (int i = 0; i < cnt && rank < MAXD; ++i) {
      const double si = s_sc[i];
      rank += (si > sj || (si == sj && i < j)) ? 1 : 0;
    }
    if (rank < MAXD) s_top[rank] = s_di[j];
  }
  __syncthreads();
  for (int r = lane; r < D; r += 64) {
    const int j = s_top[r];
    const double* b = dbox + ((int64_t)n * P + j) * 4;
    s_db[r][0] = b[0]; s_db[r][1] = b[1]; s_db[r][2] = b[2]; s_db[r][3] = b[3];
    score[(int64_t)item * MAXD + r] = dscore[(int64_t)n * P + j];
  }
  for (int i = lane; i < A * MAXD; i += 64) (&s_fl[0][0])[i] = 0;
  for (int i = lane; i < T * A * GW; i += 64) (&s_gtm[0][0])[i] = 0u;

  // ---- per area: ground-truth order (np.argsort(gig, kind="mergesort")) and npos
  if (lane < A) {
    const double lo = area_rng[lane * 2], hi = area_rng[lane * 2 + 1];
    int w = 0;
    for (int g = 0; g < G; ++g) {
      const double ga = box_area(s_gb[g]);
      if (!(ga < lo || ga > hi)) s_go[lane][w++] = (short)g;
    }
    s_np[lane] = w;
    for (int g = 0; g < G; ++g) {
      const double ga = box_area(s_gb[g]);
      if (ga < lo || ga > hi) s_go[lane][w++] = (short)g;
    }
    npos[(int64_t)item * A + lane] = s_np[lane];
  }
  __syncthreads();

  // ---- greedy matching, lane = (area a, threshold t)
  if (lane < T * A) {
    const int a = lane / T, t = lane - a * T;
    const int np_ = s_np[a];
    uint32_t* gtm = s_gtm[lane];
    const double start = iou_start[t];
    for (int d = 0; d < D; ++d) {
      double best = start;
      int m = -1;
      for (int gi = 0; gi < G; ++gi) {
        if (gtm[gi >> 5] & (1u << (gi & 31))) continue;
        if (m > -1 && m < np_ && gi >= np_) break;          // matched a regular gt; only ignored ones follow
        const double iou = pair_iou(s_db[d], s_gb[s_go[a][gi]]);
        if (iou < best) continue;
        best = iou;
        m = gi;
      }
      if (m == -1) continue;
      gtm[m >> 5] |= 1u << (m & 31);
      atomicOr(&s_fl[a][d], (1 << t) | (m >= np_ ? (1 << (T + t)) : 0));
    }
  }
  __syncthreads();

  // ---- an unmatched detection outside the area range is ignored
  for (int i = lane; i < A * D; i += 64) {
    const int a = i / D, d = i - a * D;
    const double lo = area_rng[a * 2], hi = area_rng[a * 2 + 1];
    const double da = box_area(s_db[d]);
    int f = s_fl[a][d];
    if (da < lo || da > hi) f |= (~f & ((1 << T) - 1)) << T;
    flags[(int64_t)a * NK * MAXD + (int64_t)item * MAXD + d] = f;
  }
  if (lane == 0) {
    ndet[item] = D;
    evald[item] = 1;
  }
}

constexpr int AB = 256;                 // threads of an accumulate block
constexpr int AW = AB / 64;

__global__ __launch_bounds__(AB) void map_accumulate_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ class_off,
                                                            const int32_t* __restrict__ flags, int64_t nk100,
                                                            const int32_t* __restrict__ npig, const int32_t* __restrict__ n_eval, int K,
                                                            const double* __restrict__ rec_thrs, double* __restrict__ precision,
                                                            double* __restrict__ recall) {
  __shared__ double s_rt[R];
  __shared__ unsigned long long s_best[R + 1];     // bin c: the largest pr (as bits) of the points reaching exactly c thresholds
  __shared__ int s_scan[AW];

  // segment (t, k, a, m), m fastest
  int s = blockIdx.x;
  const int m = s % M; s /= M;
  const int a = s % A; s /= A;
  const int k = s % K; s /= K;
  const int t = s;
  const int64_t rec_at = (((int64_t)t * K + k) * A + a) * M + m;
  const int64_t pstride = (int64_t)K * A * M;        // precision[t][ri][k][a][m]
  const int64_t p0 = ((int64_t)t * R * K + k) * A * M + (int64_t)a * M + m;

  const int np_ = npig[k * A + a];
  if (n_eval[k] == 0 || np_ == 0) {                  // no evaluated image, or no regular ground truth: -1 stays
    for (int ri = threadIdx.x; ri < R; ri += AB) precision[p0 + ri * pstride] = -1.0;
    if (threadIdx.x == 0) recall[rec_at] = -1.0;
    return;
  }
  for (int i = threadIdx.x; i < R; i += AB) s_rt[i] = rec_thrs[i];
  for (int i = threadIdx.x; i <= R; i += AB) s_best[i] = 0ull;       // bits of +0.0
  __syncthreads();

  const int md = m == 0 ? 1 : (m == 1 ? 10 : 100);
  const int lo = class_off[k], hi = class_off[k + 1];
  const int* fl = flags + (int64_t)a * nk100;
  const double npd = (double)np_;
  int run_tp = 0, run_fp = 0, run_nd = 0;
  for (int base = lo; base < hi; base += AB) {
    const int j = base + threadIdx.x;
    int packed = 0;
    if (j < hi) {
      const int e = order[j];
      if (e % MAXD < md) {
        const int f = fl[e];
        const bool tpb = (f >> t) & 1, igb = (f >> (T + t)) & 1;
        packed = (igb ? 0 : (tpb ? 1 : (1 << 10))) | (1 << 20);        // tp | fp << 10 | counted << 20
      }
    }
    int tot;
    const int inc = hd_block_scan<AW>(packed, s_scan, &tot);
    if (packed) {
      const int tp = run_tp + (inc & 1023), fp = run_fp + ((inc >> 10) & 1023);
      const double tpd = (double)tp, fpd = (double)fp;
      const double rc = tpd / npd;
      const double pr = tpd / ((fpd + tpd) + 2.220446049250313e-16);
      // c = #{ri : rec_thrs[ri] <= rc} (rec_thrs ascending)
      int c0 = 0, c1 = R;
      while (c0 < c1) {
        const int mid = (c0 + c1) >> 1;
        if (s_rt[mid] <= rc) c0 = mid + 1;
        else c1 = mid;
      }
      atomicMax(&s_best[c0], (unsigned long long)__double_as_longlong(pr));
    }
    run_tp += tot & 1023;
    run_fp += (tot >> 10) & 1023;
    run_nd += tot >> 20;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // q[ri] = max over bins c > ri (0 when no point reaches threshold ri)
    unsigned long long q = 0ull;
    for (int ri = R - 1; ri >= 0; --ri) {
      q = s_best[ri + 1] > q ? s_best[ri + 1] : q;
      precision[p0 + ri * pstride] = __longlong_as_double((long long)q);
    }
    recall[rec_at] = run_nd ? (double)run_tp / npd : 0.0;
  }
}

constexpr int NREF = HD_MR_NUM_REF;     // 9 reference FPPI rates

__global__ __launch_bounds__(AB) void mr_accumulate_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ class_off,
                                                           const int32_t* __restrict__ flags, int64_t nk100,
                                                           const int32_t* __restrict__ npig, const int32_t* __restrict__ n_eval, int K,
                                                           int n_images, const double* __restrict__ ref_fppi, int32_t* __restrict__ hit,
                                                           int32_t* __restrict__ total, int curve_t, int32_t* __restrict__ curve_tp,
                                                           int32_t* __restrict__ curve_fp) {
  __shared__ double s_ref[NREF];
  __shared__ int s_bin[NREF + 1];                  // bin c: the largest tp of the points with exactly c rates below their fppi
  __shared__ int s_scan[AW];

  // segment (t, k, a), a fastest
  int s = blockIdx.x;
  const int a = s % A; s /= A;
  const int k = s % K; s /= K;
  const int t = s;
  const int64_t seg = ((int64_t)t * K + k) * A + a;
  const int lo = class_off[k], hi = class_off[k + 1];
  const bool curve = curve_tp != nullptr && t == curve_t && a == 0;

  const int np_ = npig[k * A + a];
  if (n_eval[k] == 0 || np_ == 0) {                  // no evaluated image, or no regular ground truth: undefined
    if (threadIdx.x < NREF) hit[seg * NREF + threadIdx.x] = -1;
    if (threadIdx.x < 2) total[seg * 2 + threadIdx.x] = -1;
    if (curve)
      for (int j = lo + threadIdx.x; j < hi; j += AB) {
        curve_tp[j] = -1;
        curve_fp[j] = -1;
      }
    return;
  }
  if (threadIdx.x < NREF) s_ref[threadIdx.x] = ref_fppi[threadIdx.x];
  if (threadIdx.x <= NREF) s_bin[threadIdx.x] = 0;
  __syncthreads();

  const int* fl = flags + (int64_t)a * nk100;
  const double nimg = (double)n_images;
  int run_tp = 0, run_fp = 0;
  for (int base = lo; base < hi; base += AB) {
    const int j = base + threadIdx.x;
    int packed = 0;
    if (j < hi) {
      const int f = fl[order[j]];
      const bool tpb = (f >> t) & 1, igb = (f >> (T + t)) & 1;
      packed = igb ? 0 : (tpb ? 1 : (1 << 10));        // tp | fp << 10: at most AB of either per chunk
    }
    int tot;
    const int inc = hd_block_scan<AW>(packed, s_scan, &tot);
    const int tp = run_tp + (inc & 1023), fp = run_fp + ((inc >> 10) & 1023);
    if (curve && j < hi) {                             // an ignored detection repeats the pair before it
      curve_tp[j] = tp;
      curve_fp[j] = fp;
    }
    if (packed) {
      const double fppi = (double)fp / nimg;
      int i0 = 0;
#pragma unroll
      for (int i = 0; i < NREF; ++i) i0 += s_ref[i] < fppi ? 1 : 0;
      atomicMax(&s_bin[i0], tp);
    }
    run_tp += tot & 1023;
    run_fp += (tot >> 10) & 1023;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int h = 0;
    for (int i = 0; i < NREF; ++i) {
      h = s_bin[i] > h ? s_bin[i] : h;
      hit[seg * NREF + i] = h;
    }
    total[seg * 2] = run_tp;
    total[seg * 2 + 1] = run_fp;
  }
}

}  // namespace

extern "C" int hd_map_match(const double* det_boxes, const double* det_scores, const int64_t* det_labels, const int32_t* det_count, int N,
                            int P, const double* gt_boxes, const int64_t* gt_labels, const int32_t* gt_count, int Q, const int64_t* classes,
                            int K, const double* iou_start, const double* area_rng, int32_t* flags, double* score, int32_t* ndet,
                            int32_t* npos, int32_t* evald, int32_t* status, void* stream) {
  HD_CHECK_ARG(det_count && gt_count && classes && iou_start && area_rng && flags && score && ndet && npos && evald && status,
               "hd_map_match: null pointer");
  HD_CHECK_ARG(N >= 0 && P >= 0 && Q >= 0 && K >= 0, "hd_map_match: bad sizes N=%d P=%d Q=%d K=%d", N, P, Q, K);
  HD_CHECK_ARG(P == 0 || (det_boxes && det_scores && det_labels), "hd_map_match: null detection arrays");
  HD_CHECK_ARG(Q == 0 || (gt_boxes && gt_labels), "hd_map_match: null ground-truth arrays");
  HD_CHECK_ARG((int64_t)N * K * MAXD <= INT32_MAX, "hd_map_match: N*K*%d exceeds int32 (N=%d K=%d)", MAXD, N, K);
  if ((int64_t)N * K == 0) return HD_OK;
  hipLaunchKernelGGL(map_match_kernel, dim3((unsigned)(N * K)), dim3(64), 0, (hipStream_t)stream, det_boxes, det_scores, det_labels,
                     det_count, P, gt_boxes, gt_labels, gt_count, Q, classes, K, iou_start, area_rng, flags, score, ndet, npos, evald,
                     status);
  HD_CHECK_LAUNCH();
  return HD_OK;
}

extern "C" int hd_map_accumulate(const int32_t* order, const int32_t* class_off, const int32_t* flags, int64_t nk100, const int32_t* npig,
                                 const int32_t* n_eval, int K, const double* rec_thrs, double* precision, double* recall, void* stream) {
  HD_CHECK_ARG(class_off && flags && npig && n_eval && rec_thrs && precision && recall, "hd_map_accumulate: null pointer");
  HD_CHECK_ARG(K >= 0 && nk100 >= 0, "hd_map_accumulate: bad sizes K=%d", K);
  if (K == 0) return HD_OK;
  hipLaunchKernelGGL(map_accumulate_kernel, dim3((unsigned)(T * K * A * M)), dim3(AB), 0, (hipStream_t)stream, order, class_off, flags, nk100,
                     npig, n_eval, K, rec_thrs, precision, recall);
  HD_CHECK_LAUNCH();
  return HD_OK;
}

extern "C" int hd_mr_accumulate(const int32_t* order, const int32_t* class_off, const int32_t* flags, int64_t nk100, const int32_t* npig,
                                const int32_t* n_eval, int K, int n_images, const double* ref_fppi, int32_t* hit, int32_t* total,
                                int curve_t, int32_t* curve_tp, int32_t* curve_fp, void* stream) {
  HD_CHECK_ARG(class_off && flags && npig && n_eval && ref_fppi && hit && total, "hd_mr_accumulate: null pointer");
  HD_CHECK_ARG(K >= 0 && nk100 >= 0 && n_images >= 0, "hd_mr_accumulate: bad sizes K=%d n_images=%d", K, n_images);
  HD_CHECK_ARG(curve_t < T, "hd_mr_accumulate: curve threshold index %d outside [0, %d)", curve_t, T);
  HD_CHECK_ARG(curve_t < 0 || ((curve_tp != nullptr) == (curve_fp != nullptr)), "hd_mr_accumulate: one curve buffer without the other");
  if (K == 0) return HD_OK;
  HD_CHECK_ARG(n_images >= 1, "hd_mr_accumulate: %d classes but no image", K);
  HD_CHECK_ARG((int64_t)T * K * A <= INT32_MAX, "hd_mr_accumulate: too many segments (K=%d)", K);
  const bool curve = curve_t >= 0 && curve_tp && curve_fp;
  hipLaunchKernelGGL(mr_accumulate_kernel, dim3((unsigned)(T * K * A)), dim3(AB), 0, (hipStream_t)stream, order, class_off, flags, nk100, npig,
                     n_eval, K, n_images, ref_fppi, hit, total, curve ? curve_t : -1, curve ? curve_tp : nullptr,
                     curve ? curve_fp : nullptr);
  HD_CHECK_LAUNCH();
  return HD_OK;
}
