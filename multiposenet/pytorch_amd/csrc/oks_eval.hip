// oks_eval.hip — COCO keypoint AP / AR (object keypoint similarity) evaluation for gfx950.
//
// Replaces the pycocotools leg of Tester.coco_eval (evaluate/tester.py:179-186: COCOeval(coco, res, 'keypoints') evaluate /
// accumulate).  The published COCOeval(iouType='keypoints') algorithm is restated, not linked: computeOks, evaluateImg
// and accumulate.  All arithmetic is float64; the file is compiled with -ffp-contract=off.  The constant tables (sigma variances,
// OKS thresholds, recall thresholds, area ranges) come from the caller exactly as numpy builds them.
//
// Three stages, every image described by one row of a table img_tab[n_img + 1][4] = (first detection, first ground truth, first
// kept detection, first OKS element), int64, the last row holding the totals:
//   1. oks_matrix_kernel: one workgroup per image.  Stable rank sort of the image's detections by descending score (ties: lower
//      input index first, as nms.hip), truncation to max_dets, detection areas from the 17 (x, y), the kept x G OKS block.
//   2. oks_match_kernel: one wave per (image, area range, threshold).  The detection loop is sequential; the scan over the ordered
//      ground truths is a lane-parallel arg-max.  The ordered list is "non-ignored first, stable", so inside each of the two classes
//      the order is the input order and COCOeval's scan (">=" moves the match to the later ground truth; stop at the first ignored
//      one once a non-ignored match exists) is: arg-max with ties to the LARGEST index over the available non-ignored ground
//      truths, and only if none reaches the threshold, the same over the ignored ones.  Lane l owns ground truths l, l + 64, ...,
//      and is the only reader and writer of their match state, which lives in the gt_match result itself.
//   3. oks_rank_kernel + oks_accum_kernel: stable sort of all kept detections by (-score, concatenation position) as a rank sort
//      (K^2 compares through LDS broadcasts, unique ranks, no scratch), then one workgroup per (area range, threshold): gather of
//      the flags in sorted order, chunked inclusive scan of tp / fp, the two divisions, a right-to-left running maximum and the
//      lower-bound searches over the recall thresholds.
#include "common.h"

namespace {

constexpr int kJ = 17;
constexpr int kMaxDets = 128;
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
    if (tid < kMaxDets) order_s[tid] = 0;                // a NaN score leaves ranks unassigned: never an index outside the image
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

// rank of kept detection k in the stable descending sort = #{j : s_j > s_k or (s_j == s_k and j < k)}; order[rank] = k
__global__ void __launch_bounds__(256) oks_rank_kernel(const double* __restrict__ score, long K, int32_t* __restrict__ order) {
    __shared__ double ssc[1024];
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    const double sk = (k < K) ? score[k] : 0.0;
    long rank = 0;
    for (long j0 = 0; j0 < K; j0 += 1024) {
        for (int t = threadIdx.x; t < 1024; t += 256) ssc[t] = (j0 + t < K) ? score[j0 + t] : 0.0;
        __syncthreads();
        const int lim = (K - j0) < 1024 ? (int)(K - j0) : 1024;
        for (int t = 0; t < lim; ++t) {
            const double sj = ssc[t];
            rank += (sj > sk) || (sj == sk && (j0 + t) < k);
        }
        __syncthreads();
    }
    if (k < K) order[rank] = (int32_t)k;
}

__device__ __forceinline__ int wave_incl_sum(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    return v;
}

// one workgroup of 1024 threads per (area range, threshold)
__global__ void __launch_bounds__(1024) oks_accum_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ det_match,
                                                         const int32_t* __restrict__ det_ig, const int32_t* __restrict__ gt_ig, long K,
                                                         long Gtot, int A, int T, const double* __restrict__ rec_thrs, int R,
                                                         int32_t* tp_all, double* pr_all, double* __restrict__ precision,
                                                         double* __restrict__ recall) {
    __shared__ int w_tp[16], w_fp[16];
    __shared__ double w_mx[16];
    const int a = blockIdx.x / T, t = blockIdx.x % T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long at = (long)a * T + t;
    // npig = #(gIg == 0) over all images
    int cnt = 0;
    for (long g = tid; g < Gtot; g += 1024) cnt += gt_ig[(long)a * Gtot + g] == 0;
    cnt = wave_incl_sum(cnt, lane);
    if (lane == 63) w_tp[wave] = cnt;
    __syncthreads();
    int npig = 0;
    for (int w = 0; w < 16; ++w) npig += w_tp[w];
    __syncthreads();
    if (npig == 0) {                                     // block-uniform
        for (int r = tid; r < R; r += 1024) precision[((long)t * R + r) * A + a] = -1.0;
        if (tid == 0) recall[(long)t * A + a] = -1.0;
        return;
    }
    int32_t* tp_ws = tp_all + at * K;
    double* pr_ws = pr_all + at * K;
    const int32_t* dm = det_match + at * K;
    const int32_t* di = det_ig + at * K;
    int c_tp = 0, c_fp = 0;
    for (long c0 = 0; c0 < K; c0 += 1024) {
        const long i = c0 + tid;
        int tpv = 0, fpv = 0;
        if (i < K) {
            const int k = order[i];
            if (k >= 0 && k < K) {                       // ranks are unique for finite scores; anything else counts as ignored
                const bool m = dm[k] >= 0, ig = di[k] != 0;
                tpv = (m && !ig) ? 1 : 0;
                fpv = (!m && !ig) ? 1 : 0;
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
        if (i < K) {
            const int tp = c_tp + tpv, fp = c_fp + fpv;
            tp_ws[i] = tp;
            pr_ws[i] = (double)tp / ((double)fp + (double)tp + kEps);
        }
        c_tp += tot_tp; c_fp += tot_fp;
        __syncthreads();
    }
    // pr[i - 1] = max(pr[i - 1], pr[i]) from the right; every thread revisits the elements it wrote itself
    double c_mx = -1.0;
    const long nchunk = (K + 1023) / 1024;
    for (long c = nchunk - 1; c >= 0; --c) {
        const long i = c * 1024 + tid;
        double v = (i < K) ? pr_ws[i] : -1.0;
        for (int o = 1; o < 64; o <<= 1) {
            const double n = __shfl_down(v, o, 64);
            if (lane + o < 64) v = fmax(v, n);
        }
        if (lane == 0) w_mx[wave] = v;
        __syncthreads();
        double all = c_mx;
        for (int w = 15; w >= 0; --w) {
            if (w == wave) v = fmax(v, all);
            all = fmax(all, w_mx[w]);
        }
        if (i < K) pr_ws[i] = v;
        c_mx = all;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    const double dn = (double)npig;
    for (int r = tid; r < R; r += 1024) {
        const double thr = rec_thrs[r];
        long lo = 0, hi = K;                             // first i with tp[i] / npig >= thr (np.searchsorted, side='left')
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if ((double)tp_ws[mid] / dn >= thr) hi = mid; else lo = mid + 1;
        }
        precision[((long)t * R + r) * A + a] = (lo < K) ? pr_ws[lo] : 0.0;
    }
    if (tid == 0) recall[(long)t * A + a] = (K > 0) ? (double)tp_ws[K - 1] / dn : 0.0;
}

inline long oks_align(long v) { return (v + 255) / 256 * 256; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// the table on the host: rows ascend, every image keeps min(detections, max_dets), its OKS block is kept x ground truths
inline bool oks_tab_ok(const int64_t* tab, int n_img, int max_dets) {
    if (tab[0] != 0 || tab[1] != 0 || tab[2] != 0 || tab[3] != 0) return false;
    for (int i = 0; i < n_img; ++i) {
        const int64_t* r = tab + (long)i * 4;
        const int64_t nd = r[4] - r[0], ng = r[5] - r[1], nk = r[6] - r[2], no = r[7] - r[3];
        if (nd < 0 || ng < 0 || nd > 0x7fffffffLL / 2 || ng > 0x7fffffffLL / 2) return false;
        if (nk != (nd < max_dets ? nd : max_dets) || no != nk * ng) return false;
    }
    const int64_t* last = tab + (long)n_img * 4;
    return last[0] < 0x7fffffffLL && last[1] < 0x7fffffffLL;
}

}  // namespace

extern "C" int64_t mpn_oks_eval_workspace_bytes(int64_t n_kept, int n_area, int n_thr) {
    if (n_kept <= 0 || n_area <= 0 || n_thr <= 0) return 256;
    const long at = (long)n_area * n_thr;
    return oks_align(at * n_kept * 4) + oks_align(at * n_kept * 8);
}

extern "C" int mpn_oks_matrix(const double* det_kp, const double* det_score, const double* gt_kp, const double* gt_area,
                              const double* gt_bbox, const int64_t* img_tab_host, const int64_t* img_tab, int n_img, int max_dets,
                              const double* var, int32_t* kept_src, double* kept_score, double* kept_area, double* oks, void* stream) {
    MPN_CHECK_ARG(det_kp && det_score && gt_kp && gt_area && gt_bbox && img_tab_host && img_tab && var && kept_src && kept_score &&
                  kept_area && oks);
    MPN_CHECK_ARG(n_img > 0 && max_dets >= 1 && max_dets <= kMaxDets);
    MPN_CHECK_ARG(al8(det_kp) && al8(det_score) && al8(gt_kp) && al8(gt_area) && al8(gt_bbox) && al8(img_tab) && al8(var) &&
                  al8(kept_score) && al8(kept_area) && al8(oks));
    MPN_CHECK_ARG(oks_tab_ok(img_tab_host, n_img, max_dets));
    hipLaunchKernelGGL(oks_matrix_kernel, dim3(n_img), dim3(256), 0, (hipStream_t)stream, det_kp, det_score, gt_kp, gt_area, gt_bbox,
                       img_tab, var, kept_src, kept_score, kept_area, oks);
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
    MPN_CHECK_ARG(oks_tab_ok(img_tab_host, n_img, max_dets));
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
    hipStream_t st = (hipStream_t)stream;
    const long at = (long)n_area * n_thr;
    int32_t* tp_ws = (int32_t*)workspace;
    double* pr_ws = (double*)((char*)workspace + oks_align(at * n_kept * 4));
    if (n_kept > 0)
        hipLaunchKernelGGL(oks_rank_kernel, dim3((unsigned)((n_kept + 255) / 256)), dim3(256), 0, st, kept_score, (long)n_kept, order);
    hipLaunchKernelGGL(oks_accum_kernel, dim3((unsigned)at), dim3(1024), 0, st, order, det_match, det_ig, gt_ig, (long)n_kept, (long)n_gt,
                       n_area, n_thr, rec_thrs, n_rec, tp_ws, pr_ws, precision, recall);
    return mpn_launch_status();
}
