// coco_eval.hip — COCO AP / AR evaluation for gfx950: keypoints (object keypoint similarity) and boxes (iouType 'bbox').
//
// Replaces the pycocotools leg of Tester.coco_eval (evaluate/tester.py:179-186: COCOeval(coco, res, 'keypoints') evaluate /
// accumulate) and scores the detection head.  The published COCOeval algorithm is restated, not linked: computeOks,
// maskApi.c:bbIou / computeIoU, evaluateImg and accumulate.  All arithmetic is float64; the file is compiled with
// -ffp-contract=off, and the box path is only + - * / min max: every box result equals the numpy restatement bit for bit.  The
// constant tables (sigma variances, thresholds, recall thresholds, area ranges, maxDets) come from the caller exactly as numpy
// builds them.
//
// The two metrics differ in stage 1 alone.  A row is what COCOeval evaluates as one unit: an image for keypoints, a (category,
// image) pair with at least one detection or ground truth for boxes (category-major, then ascending image id).  Rows are described
// by a table tab[n_row + 1][4] = (first detection, first ground truth, first kept detection, first similarity element), int64, the
// last row holding the totals.  cat_tab[n_cat + 1][2] = (first kept detection, first ground truth) of every category: a category's
// kept detections and ground truths are contiguous.  Keypoints have no category table: one segment, everything.
//   1. oks_matrix_kernel / box_iou_kernel: one workgroup per row.  Stable rank sort of the row's detections by descending score
//      (ties: lower input index first, as nms.hip), truncation to max_dets, detection areas (the extent of the 17 (x, y); w * h of
//      the detection's own box), for boxes the position inside the row, and the kept x G block of OKS / IoU values.
//   2. oks_match_kernel: one wave per (row, area range, threshold), on any similarity blocks.  The detection loop is sequential; the
//      scan over the ordered ground truths is a lane-parallel arg-max.  The ordered list is "non-ignored first, stable", so inside
//      each of the two classes the order is the input order and COCOeval's scan (">=" moves the match to the later ground truth;
//      stop at the first ignored one once a non-ignored match exists) is: arg-max with ties to the LARGEST index over the available
//      non-ignored ground truths, and only if none reaches the threshold, the same over the ignored ones.  Lane l owns ground truths
//      l, l + 64, ..., and is the only reader and writer of their match state, which lives in the gt_match result itself.
//   3. coco_rank_kernel + coco_accum_kernel: stable descending sort of every category's kept detections by (score, concatenation
//      position) as a segmented rank sort (compares through LDS broadcasts inside the segment, unique ranks, no scratch), then one workgroup
//      per (category, area range, maxDets entry, threshold): gather of the flags in sorted order, chunked inclusive scan of tp / fp,
//      the two divisions, a right-to-left running maximum and the lower-bound searches over the recall thresholds.  COCOeval slices
//      every image's list to maxDets[m] and merge-sorts the concatenation; a stable subsequence of the full stable order is the same
//      order, so the one sort serves every m and a detection whose in-row position is >= maxDets[m] is carried as an entry that adds
//      to neither tp nor fp: it repeats its predecessor's (tp, fp), hence its precision, and changes no maximum and no lower bound.
//      The keypoint accumulate is this with one category and one maxDets entry that slices nothing off (stage 1 truncated already).
#include "common.h"

namespace {

constexpr int kJ = 17;
constexpr int kMaxDets = 128;
constexpr int kMaxM = 4;
constexpr double kEps = 2.220446049250313e-16;       // np.spacing(1) = 2^-52

__device__ __forceinline__ double oks_pair(const double* __restrict__ dk, const double* __restrict__ gk, double g_area,
                                           const double* __restrict__ bb, const double* __restrict__ var) {
    int k1 = 0;
    for (int k = 0; k < kJ; ++k) k1 += gk[3 * k + 2] > 0.0;
    const double den = g_area + kEps;
    double sum = 0.0;
    if (k1 > 0) {
        for (int k = 0; k < kJ; ++k) {
            if (!(gk[3 * k + 2] > 0.0)) continue;
            const double dx = dk[3 * k] - gk[3 * k], dy = dk[3 * k + 1] - gk[3 * k + 1];
            const double e = (dx * dx + dy * dy) / var[k] / den / 2.0;
            sum += exp(-e);
        }
        return sum / (double)k1;
    }
    const double x0 = bb[0] - bb[2], x1 = bb[0] + bb[2] * 2.0, y0 = bb[1] - bb[3], y1 = bb[1] + bb[3] * 2.0;
    for (int k = 0; k < kJ; ++k) {
        const double xd = dk[3 * k], yd = dk[3 * k + 1];
        const double dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1), dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        const double e = (dx * dx + dy * dy) / var[k] / den / 2.0;
        sum += exp(-e);
    }
    return sum / (double)kJ;
}

// maskApi.c:bbIou for one pair, operation for operation; boxes (x, y, w, h)
__device__ __forceinline__ double bb_iou(const double* __restrict__ D, const double* __restrict__ G, bool crowd) {
    const double ga = G[2] * G[3];
    const double da = D[2] * D[3];
    const double w = fmin(D[2] + D[0], G[2] + G[0]) - fmax(D[0], G[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(D[3] + D[1], G[3] + G[1]) - fmax(D[1], G[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

// order_s[r] = the row's detection of rank r < nk in the stable descending-score sort; a workgroup of 256 threads, all of them call
__device__ __forceinline__ void row_order(const double* __restrict__ det_score, long det0, int nd, int nk, int* order_s) {
    const int tid = threadIdx.x;
    if (tid < kMaxDets) order_s[tid] = 0;                // a NaN score leaves ranks unassigned: never an index outside the row
    __syncthreads();
    for (int d = tid; d < nd; d += 256) {
        const double s = det_score[det0 + d];
        int rank = 0;
        for (int j = 0; j < nd; ++j) {
            const double sj = det_score[det0 + j];
            rank += (sj > s) || (sj == s && j < d);
        }
        if (rank < nk) order_s[rank] = d;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) oks_matrix_kernel(const double* __restrict__ det_kp, const double* __restrict__ det_score,
                                                         const double* __restrict__ gt_kp, const double* __restrict__ gt_area,
                                                         const double* __restrict__ gt_bbox, const int64_t* __restrict__ img_tab,
                                                         const double* __restrict__ var, int32_t* __restrict__ kept_src,
                                                         double* __restrict__ kept_score, double* __restrict__ kept_area,
                                                         double* __restrict__ oks) {
    __shared__ int order_s[kMaxDets];
    __shared__ double var_s[kJ];
    const int64_t* row = img_tab + (long)blockIdx.x * 4;
    const long det0 = row[0], gt0 = row[1], kept0 = row[2], oks0 = row[3];
    const int nd = (int)(row[4] - det0), G = (int)(row[5] - gt0), nk = (int)(row[6] - kept0);
    const int tid = threadIdx.x;
    if (tid < kJ) var_s[tid] = var[tid];
    row_order(det_score, det0, nd, nk, order_s);
    for (int r = tid; r < nk; r += 256) {
        const long d = det0 + order_s[r];
        const double* dk = det_kp + d * (kJ * 3);
        double xa = dk[0], xb = dk[0], ya = dk[1], yb = dk[1];
        for (int k = 1; k < kJ; ++k) {
            xa = fmin(xa, dk[3 * k]); xb = fmax(xb, dk[3 * k]);
            ya = fmin(ya, dk[3 * k + 1]); yb = fmax(yb, dk[3 * k + 1]);
        }
        kept_src[kept0 + r] = (int32_t)d;
        kept_score[kept0 + r] = det_score[d];
        kept_area[kept0 + r] = (xb - xa) * (yb - ya);
    }
    const int np = nk * G;
    for (int p = tid; p < np; p += 256) {
        const int r = p / G, g = p - r * G;
        const long d = det0 + order_s[r];
        oks[oks0 + p] = oks_pair(det_kp + d * (kJ * 3), gt_kp + (gt0 + g) * (kJ * 3), gt_area[gt0 + g], gt_bbox + (gt0 + g) * 4, var_s);
    }
}

// gt_flags: bit 0 = ignored, bit 1 = iscrowd
__global__ void __launch_bounds__(256) box_iou_kernel(const double* __restrict__ det_box, const double* __restrict__ det_score,
                                                      const double* __restrict__ gt_box, const int32_t* __restrict__ gt_flags,
                                                      const int64_t* __restrict__ tab, int32_t* __restrict__ kept_src,
                                                      double* __restrict__ kept_score, double* __restrict__ kept_area,
                                                      int32_t* __restrict__ kept_rank, double* __restrict__ iou) {
    __shared__ int order_s[kMaxDets];
    const int64_t* row = tab + (long)blockIdx.x * 4;
    const long det0 = row[0], gt0 = row[1], kept0 = row[2], iou0 = row[3];
    const int nd = (int)(row[4] - det0), G = (int)(row[5] - gt0), nk = (int)(row[6] - kept0);
    const int tid = threadIdx.x;
    row_order(det_score, det0, nd, nk, order_s);
    for (int r = tid; r < nk; r += 256) {
        const long d = det0 + order_s[r];
        kept_src[kept0 + r] = (int32_t)d;
        kept_score[kept0 + r] = det_score[d];
        kept_area[kept0 + r] = det_box[d * 4 + 2] * det_box[d * 4 + 3];
        kept_rank[kept0 + r] = r;
    }
    const int np = nk * G;
    for (int p = tid; p < np; p += 256) {
        const int r = p / G, g = p - r * G;
        const long d = det0 + order_s[r];
        iou[iou0 + p] = bb_iou(det_box + d * 4, gt_box + (gt0 + g) * 4, (gt_flags[gt0 + g] & 2) != 0);
    }
}

// gt_flags: bit 0 = ignored (iscrowd or num_keypoints == 0), bit 1 = iscrowd
__global__ void __launch_bounds__(256) oks_match_kernel(const double* __restrict__ oks, const double* __restrict__ kept_area,
                                                        const double* __restrict__ gt_area, const int32_t* __restrict__ gt_flags,
                                                        const int64_t* __restrict__ img_tab, int n_img, const double* __restrict__ area_rng,
                                                        int A, const double* __restrict__ thrs, int T, long K, long Gtot,
                                                        int32_t* __restrict__ det_match, int32_t* __restrict__ det_ig,
                                                        int32_t* __restrict__ gt_ig, int32_t* gt_match) {
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= (long)n_img * A * T) return;                // wave-uniform
    const int t = (int)(w % T), a = (int)((w / T) % A);
    const int64_t* row = img_tab + (w / ((long)T * A)) * 4;
    const long gt0 = row[1], kept0 = row[2], oks0 = row[3];
    const int G = (int)(row[5] - gt0), nk = (int)(row[6] - kept0);
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr = fmin(thrs[t], 1.0 - 1e-10);
    const long at = (long)a * T + t;
    int32_t* gm = gt_match + at * Gtot + gt0;            // lane l reads and writes entries l, l + 64, ... only
    for (int g = lane; g < G; g += 64) {
        gm[g] = -1;
        if (t == 0) {
            const double ar = gt_area[gt0 + g];
            gt_ig[(long)a * Gtot + gt0 + g] = ((gt_flags[gt0 + g] & 1) || ar < lo || ar > hi) ? 1 : 0;
        }
    }
    for (int r = 0; r < nk; ++r) {
        const double* orow = oks + oks0 + (long)r * G;
        int m = -1, dig = 0;
        for (int phase = 0; phase < 2 && m < 0; ++phase) {
            double bv = -1.0;
            int bg = -1;
            for (int g = lane; g < G; g += 64) {
                const int f = gt_flags[gt0 + g];
                const double ar = gt_area[gt0 + g];
                const int ig = ((f & 1) || ar < lo || ar > hi) ? 1 : 0;
                if (ig != phase) continue;
                if (gm[g] >= 0 && !(f & 2)) continue;
                const double v = orow[g];
                if (v < thr) continue;
                if (v >= bv) { bv = v; bg = g; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int og = __shfl_xor(bg, o, 64);
                if (ov > bv || (ov == bv && og > bg)) { bv = ov; bg = og; }
            }
            m = bg;
            dig = phase;
        }
        const long kidx = kept0 + r;
        if (m >= 0) {
            if (lane == (m & 63)) gm[m] = (int32_t)kidx;
        } else {
            const double ar = kept_area[kidx];
            dig = (ar < lo || ar > hi) ? 1 : 0;
        }
        if (lane == 0) {
            det_match[at * K + kidx] = m >= 0 ? (int32_t)(gt0 + m) : -1;
            det_ig[at * K + kidx] = dig;
        }
    }
}

// blockIdx.y = category, blockIdx.x = 256-detection chunk of its segment; without a category table the one segment is [0, K).
// Rank of kept detection k inside the segment = #{j in segment : s_j > s_k or (s_j == s_k and j < k)}; order[segment start + rank] = k
__global__ void __launch_bounds__(256) coco_rank_kernel(const double* __restrict__ score, const int64_t* __restrict__ cat_tab, long K,
                                                   int32_t* __restrict__ order) {
    __shared__ double ssc[1024];
    const long s0 = cat_tab ? cat_tab[2 * blockIdx.y] : 0, s1 = cat_tab ? cat_tab[2 * blockIdx.y + 2] : K;
    const long n = s1 - s0;
    if ((long)blockIdx.x * 256 >= n) return;             // block-uniform
    const long k = (long)blockIdx.x * 256 + threadIdx.x; // position inside the segment
    const double sk = (k < n) ? score[s0 + k] : 0.0;
    long rank = 0;
    for (long j0 = 0; j0 < n; j0 += 1024) {
        for (int t = threadIdx.x; t < 1024; t += 256) ssc[t] = (j0 + t < n) ? score[s0 + j0 + t] : 0.0;
        __syncthreads();
        const int lim = (n - j0) < 1024 ? (int)(n - j0) : 1024;
        for (int t = 0; t < lim; ++t) {
            const double sj = ssc[t];
            rank += (sj > sk) || (sj == sk && (j0 + t) < k);
        }
        __syncthreads();
    }
    if (k < n) order[s0 + rank] = (int32_t)(s0 + k);
}

__device__ __forceinline__ int wave_incl_sum(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    return v;
}

// one workgroup of 1024 threads per (category c, area range a, maxDets entry m, threshold t): blockIdx.x = ((c*A + a)*M + m)*T + t.
// Without a category table the one category is all K detections and all Gtot ground truths; without kept_rank nothing is sliced off.
__global__ void __launch_bounds__(1024) coco_accum_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ kept_rank,
                                                     const int32_t* __restrict__ det_match, const int32_t* __restrict__ det_ig,
                                                     const int32_t* __restrict__ gt_ig, const int64_t* __restrict__ cat_tab, long K,
                                                     long Gtot, int A, int M, int T, unsigned md_packed,
                                                     const double* __restrict__ rec_thrs, int R, int32_t* tp_all, double* pr_all,
                                                     double* __restrict__ precision, double* __restrict__ recall) {
    __shared__ int w_tp[16], w_fp[16];
    __shared__ double w_mx[16];
    int b = blockIdx.x;
    const int t = b % T; b /= T;
    const int m = b % M; b /= M;
    const int a = b % A;
    const int c = b / A;
    const int md = (int)((md_packed >> (8 * m)) & 255u) + 1;      // maxDets[m] - 1 in eight bits each
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long s0 = 0, g0 = 0, n = K, ng = Gtot;
    if (cat_tab) {
        s0 = cat_tab[2 * c]; g0 = cat_tab[2 * c + 1];
        n = cat_tab[2 * c + 2] - s0; ng = cat_tab[2 * c + 3] - g0;
    }
    const long at = (long)a * T + t;
    // npig = #(gIg == 0) over the category's ground truths
    int cnt = 0;
    for (long g = tid; g < ng; g += 1024) cnt += gt_ig[(long)a * Gtot + g0 + g] == 0;
    cnt = wave_incl_sum(cnt, lane);
    if (lane == 63) w_tp[wave] = cnt;
    __syncthreads();
    int npig = 0;
    for (int w = 0; w < 16; ++w) npig += w_tp[w];
    __syncthreads();
    const long pstride = (long)(gridDim.x / T);           // C * A * M: precision [T][R][C][A][M], recall [T][C][A][M]
    const long pcol = ((long)c * A + a) * M + m;
    if (npig == 0) {                                     // block-uniform
        for (int r = tid; r < R; r += 1024) precision[((long)t * R + r) * pstride + pcol] = -1.0;
        if (tid == 0) recall[(long)t * pstride + pcol] = -1.0;
        return;
    }
    const long slab = ((long)(a * M + m) * T + t) * K + s0;
    int32_t* tp_ws = tp_all + slab;
    double* pr_ws = pr_all + slab;
    const int32_t* dm = det_match + at * K;
    const int32_t* di = det_ig + at * K;
    int c_tp = 0, c_fp = 0;
    for (long c0 = 0; c0 < n; c0 += 1024) {
        const long i = c0 + tid;
        int tpv = 0, fpv = 0;
        if (i < n) {
            const long k = order[s0 + i];
            // ranks are unique for finite scores; anything else, and an entry past this maxDets, counts as neither tp nor fp
            if (k >= s0 && k < s0 + n && (kept_rank ? kept_rank[k] : 0) < md) {
                const bool mt = dm[k] >= 0, ig = di[k] != 0;
                tpv = (mt && !ig) ? 1 : 0;
                fpv = (!mt && !ig) ? 1 : 0;
            }
        }
        tpv = wave_incl_sum(tpv, lane);
        fpv = wave_incl_sum(fpv, lane);
        if (lane == 63) { w_tp[wave] = tpv; w_fp[wave] = fpv; }
        __syncthreads();
        int tot_tp = 0, tot_fp = 0;
        for (int w = 0; w < 16; ++w) {
            if (w == wave) { tpv += tot_tp; fpv += tot_fp; }
            tot_tp += w_tp[w]; tot_fp += w_fp[w];
        }
        if (i < n) {
            const int tp = c_tp + tpv, fp = c_fp + fpv;
            tp_ws[i] = tp;
            pr_ws[i] = (double)tp / ((double)fp + (double)tp + kEps);
        }
        c_tp += tot_tp; c_fp += tot_fp;
        __syncthreads();
    }
    // pr[i - 1] = max(pr[i - 1], pr[i]) from the right; every thread revisits the elements it wrote itself
    double c_mx = -1.0;
    const long nchunk = (n + 1023) / 1024;
    for (long ch = nchunk - 1; ch >= 0; --ch) {
        const long i = ch * 1024 + tid;
        double v = (i < n) ? pr_ws[i] : -1.0;
        for (int o = 1; o < 64; o <<= 1) {
            const double nb = __shfl_down(v, o, 64);
            if (lane + o < 64) v = fmax(v, nb);
        }
        if (lane == 0) w_mx[wave] = v;
        __syncthreads();
        double all = c_mx;
        for (int w = 15; w >= 0; --w) {
            if (w == wave) v = fmax(v, all);
            all = fmax(all, w_mx[w]);
        }
        if (i < n) pr_ws[i] = v;
        c_mx = all;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    const double dn = (double)npig;
    for (int r = tid; r < R; r += 1024) {
        const double thr = rec_thrs[r];
        long lo = 0, hi = n;                             // first i with tp[i] / npig >= thr (np.searchsorted, side='left')
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if ((double)tp_ws[mid] / dn >= thr) hi = mid; else lo = mid + 1;
        }
        precision[((long)t * R + r) * pstride + pcol] = (lo < n) ? pr_ws[lo] : 0.0;
    }
    if (tid == 0) recall[(long)t * pstride + pcol] = (n > 0) ? (double)tp_ws[n - 1] / dn : 0.0;
}

inline long align256(long v) { return (v + 255) / 256 * 256; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// tp (int32) and precision (double) of every detection, one slab of n_kept per (area range, maxDets entry, threshold)
inline int64_t ws_bytes(int64_t n_kept, long slabs) {
    return n_kept <= 0 || slabs <= 0 ? 256 : align256(slabs * n_kept * 4) + align256(slabs * n_kept * 8);
}

// the table on the host: rows ascend, every row keeps min(detections, max_dets), its similarity block is kept x ground truths
inline bool row_tab_ok(const int64_t* tab, int n_row, int max_dets) {
    if (tab[0] != 0 || tab[1] != 0 || tab[2] != 0 || tab[3] != 0) return false;
    for (int i = 0; i < n_row; ++i) {
        const int64_t* r = tab + (long)i * 4;
        const int64_t nd = r[4] - r[0], ng = r[5] - r[1], nk = r[6] - r[2], no = r[7] - r[3];
        if (nd < 0 || ng < 0 || nd > 0x7fffffffLL / 2 || ng > 0x7fffffffLL / 2) return false;
        if (nk != (nd < max_dets ? nd : max_dets) || no != nk * ng) return false;
    }
    const int64_t* last = tab + (long)n_row * 4;
    return last[0] < 0x7fffffffLL && last[1] < 0x7fffffffLL;
}

// the category table on the host: starts at zero, ascends, ends at the totals
inline bool cat_tab_ok(const int64_t* ct, int n_cat, int64_t n_kept, int64_t n_gt) {
    if (ct[0] != 0 || ct[1] != 0) return false;
    for (int c = 0; c < n_cat; ++c)
        if (ct[2 * c + 2] < ct[2 * c] || ct[2 * c + 3] < ct[2 * c + 1]) return false;
    return ct[2 * n_cat] == n_kept && ct[2 * n_cat + 1] == n_gt;
}

// stage 3 of both metrics, arguments checked by the caller.  cat_tab_host / cat_tab null: one category holding everything.
int accumulate(const double* kept_score, const int32_t* kept_rank, const int32_t* det_match, const int32_t* det_ig,
               const int32_t* gt_ig, const int64_t* cat_tab_host, const int64_t* cat_tab, int n_cat, long n_kept, long n_gt, int n_area,
               int n_max, int n_thr, unsigned md_packed, const double* rec_thrs, int n_rec, int32_t* order, double* precision,
               double* recall, void* workspace, hipStream_t st) {
    const long amt = (long)n_area * n_max * n_thr;
    int32_t* tp_ws = (int32_t*)workspace;
    double* pr_ws = (double*)((char*)workspace + align256(amt * n_kept * 4));
    long seg = cat_tab_host ? 0 : n_kept;                // the longest segment
    for (int c = 0; cat_tab_host && c < n_cat; ++c) {
        const long n = (long)(cat_tab_host[2 * c + 2] - cat_tab_host[2 * c]);
        seg = n > seg ? n : seg;
    }
    if (seg > 0)
        hipLaunchKernelGGL(coco_rank_kernel, dim3((unsigned)((seg + 255) / 256), (unsigned)n_cat), dim3(256), 0, st, kept_score, cat_tab, n_kept,
                           order);
    hipLaunchKernelGGL(coco_accum_kernel, dim3((unsigned)(n_cat * amt)), dim3(1024), 0, st, order, kept_rank, det_match, det_ig, gt_ig, cat_tab,
                       n_kept, n_gt, n_area, n_max, n_thr, md_packed, rec_thrs, n_rec, tp_ws, pr_ws, precision, recall);
    return mpn_launch_status();
}

}  // namespace

extern "C" int64_t mpn_oks_eval_workspace_bytes(int64_t n_kept, int n_area, int n_thr) {
    return n_area <= 0 || n_thr <= 0 ? 256 : ws_bytes(n_kept, (long)n_area * n_thr);
}

extern "C" int64_t mpn_box_eval_workspace_bytes(int64_t n_kept, int n_area, int n_max, int n_thr) {
    return n_area <= 0 || n_max <= 0 || n_thr <= 0 ? 256 : ws_bytes(n_kept, (long)n_area * n_max * n_thr);
}

extern "C" int mpn_oks_matrix(const double* det_kp, const double* det_score, const double* gt_kp, const double* gt_area,
                              const double* gt_bbox, const int64_t* img_tab_host, const int64_t* img_tab, int n_img, int max_dets,
                              const double* var, int32_t* kept_src, double* kept_score, double* kept_area, double* oks, void* stream) {
    MPN_CHECK_ARG(det_kp && det_score && gt_kp && gt_area && gt_bbox && img_tab_host && img_tab && var && kept_src && kept_score &&
                  kept_area && oks);
    MPN_CHECK_ARG(n_img > 0 && max_dets >= 1 && max_dets <= kMaxDets);
    MPN_CHECK_ARG(al8(det_kp) && al8(det_score) && al8(gt_kp) && al8(gt_area) && al8(gt_bbox) && al8(img_tab) && al8(var) &&
                  al8(kept_score) && al8(kept_area) && al8(oks));
    MPN_CHECK_ARG(row_tab_ok(img_tab_host, n_img, max_dets));
    hipLaunchKernelGGL(oks_matrix_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, det_kp, det_score, gt_kp, gt_area, gt_bbox,
                       img_tab, var, kept_src, kept_score, kept_area, oks);
    return mpn_launch_status();
}

extern "C" int mpn_box_iou_matrix(const double* det_box, const double* det_score, const double* gt_box, const int32_t* gt_flags,
                                  const int64_t* tab_host, const int64_t* tab, int n_row, int max_dets, int32_t* kept_src,
                                  double* kept_score, double* kept_area, int32_t* kept_rank, double* iou, void* stream) {
    MPN_CHECK_ARG(det_box && det_score && gt_box && gt_flags && tab_host && tab && kept_src && kept_score && kept_area && kept_rank &&
                  iou);
    MPN_CHECK_ARG(n_row > 0 && max_dets >= 1 && max_dets <= kMaxDets);
    MPN_CHECK_ARG(al8(det_box) && al8(det_score) && al8(gt_box) && al8(tab) && al8(kept_score) && al8(kept_area) && al8(iou));
    MPN_CHECK_ARG(row_tab_ok(tab_host, n_row, max_dets));
    hipLaunchKernelGGL(box_iou_kernel, dim3(n_row), dim3(256), 0, (hipStream_t)stream, det_box, det_score, gt_box, gt_flags, tab,
                       kept_src, kept_score, kept_area, kept_rank, iou);
    return mpn_launch_status();
}

extern "C" int mpn_oks_match(const double* oks, const double* kept_area, const double* gt_area, const int32_t* gt_flags,
                             const int64_t* img_tab_host, const int64_t* img_tab, int n_img, int max_dets, const double* area_rng,
                             int n_area, const double* iou_thrs, int n_thr, int32_t* det_match, int32_t* det_ig, int32_t* gt_ig,
                             int32_t* gt_match, void* stream) {
    MPN_CHECK_ARG(oks && kept_area && gt_area && gt_flags && img_tab_host && img_tab && area_rng && iou_thrs && det_match && det_ig &&
                  gt_ig && gt_match);
    MPN_CHECK_ARG(n_img > 0 && max_dets >= 1 && max_dets <= kMaxDets && n_area >= 1 && n_area <= 8 && n_thr >= 1 && n_thr <= 64);
    MPN_CHECK_ARG(al8(oks) && al8(kept_area) && al8(gt_area) && al8(img_tab) && al8(area_rng) && al8(iou_thrs));
    MPN_CHECK_ARG(row_tab_ok(img_tab_host, n_img, max_dets));
    const int64_t* last = img_tab_host + (long)n_img * 4;
    const long waves = (long)n_img * n_area * n_thr;
    MPN_CHECK_ARG((waves + 3) / 4 <= 0x7fffffffL);
    hipLaunchKernelGGL(oks_match_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, oks, kept_area, gt_area,
                       gt_flags, img_tab, n_img, area_rng, n_area, iou_thrs, n_thr, (long)last[2], (long)last[1], det_match, det_ig, gt_ig,
                       gt_match);
    return mpn_launch_status();
}

extern "C" int mpn_oks_accumulate(const double* kept_score, const int32_t* det_match, const int32_t* det_ig, const int32_t* gt_ig,
                                  int64_t n_kept, int64_t n_gt, int n_area, int n_thr, const double* rec_thrs, int n_rec,
                                  int32_t* order, double* precision, double* recall, void* workspace, void* stream) {
    MPN_CHECK_ARG(kept_score && det_match && det_ig && gt_ig && rec_thrs && order && precision && recall && workspace);
    MPN_CHECK_ARG(n_kept >= 0 && n_kept < 0x7fffffffLL && n_gt >= 0 && n_gt < 0x7fffffffLL);
    MPN_CHECK_ARG(n_area >= 1 && n_area <= 8 && n_thr >= 1 && n_thr <= 64 && n_rec >= 1 && n_rec <= 4096);
    MPN_CHECK_ARG(al8(kept_score) && al8(rec_thrs) && al8(precision) && al8(recall) && al8(workspace));
    return accumulate(kept_score, nullptr, det_match, det_ig, gt_ig, nullptr, nullptr, 1, (long)n_kept, (long)n_gt, n_area, 1, n_thr, 0u,
                      rec_thrs, n_rec, order, precision, recall, workspace, (hipStream_t)stream);
}

extern "C" int mpn_box_accumulate(const double* kept_score, const int32_t* kept_rank, const int32_t* det_match, const int32_t* det_ig,
                                  const int32_t* gt_ig, const int64_t* cat_tab_host, const int64_t* cat_tab, int n_cat, int64_t n_kept,
                                  int64_t n_gt, int n_area, int n_thr, const int32_t* max_dets_host, int n_max, const double* rec_thrs,
                                  int n_rec, int32_t* order, double* precision, double* recall, void* workspace, void* stream) {
    MPN_CHECK_ARG(kept_score && kept_rank && det_match && det_ig && gt_ig && cat_tab_host && cat_tab && max_dets_host && rec_thrs &&
                  order && precision && recall && workspace);
    MPN_CHECK_ARG(n_kept >= 0 && n_kept < 0x7fffffffLL && n_gt >= 0 && n_gt < 0x7fffffffLL && n_cat >= 1 && n_cat <= 65535);
    MPN_CHECK_ARG(n_area >= 1 && n_area <= 8 && n_thr >= 1 && n_thr <= 64 && n_rec >= 1 && n_rec <= 4096 && n_max >= 1 && n_max <= kMaxM);
    MPN_CHECK_ARG(al8(kept_score) && al8(cat_tab) && al8(rec_thrs) && al8(precision) && al8(recall) && al8(workspace));
    MPN_CHECK_ARG(cat_tab_ok(cat_tab_host, n_cat, n_kept, n_gt));
    unsigned md_packed = 0;                              // maxDets[m] - 1 in eight bits each
    for (int m = 0; m < n_max; ++m) {
        MPN_CHECK_ARG(max_dets_host[m] >= 1 && max_dets_host[m] <= kMaxDets);
        md_packed |= (unsigned)(max_dets_host[m] - 1) << (8 * m);
    }
    MPN_CHECK_ARG((long)n_cat * n_area * n_max * n_thr <= 0x7fffffffL);
    return accumulate(kept_score, kept_rank, det_match, det_ig, gt_ig, cat_tab_host, cat_tab, n_cat, (long)n_kept, (long)n_gt, n_area, n_max,
                      n_thr, md_packed, rec_thrs, n_rec, order, precision, recall, workspace, (hipStream_t)stream);
}
