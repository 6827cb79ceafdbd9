// box_eval.hip — COCO box AP / AR (iouType 'bbox') evaluation for gfx950: the IoU stage and the per-category, per-maxDets
// accumulation.  The matching between them is mpn_oks_match of oks_eval.hip, unchanged: it works on any similarity blocks.
//
// The published COCOeval(iouType='bbox') is restated, not linked: maskApi.c:bbIou, computeIoU, accumulate.  All
// arithmetic is float64 and only + - * / min max, the file is compiled with -ffp-contract=off: every result equals the numpy
// restatement bit for bit.  The constant tables (recall thresholds, maxDets) come from the caller as numpy builds them.
//
// A row is one (category, image) pair with at least one detection or ground truth; rows are category-major, then ascending image
// id.  tab[n_row + 1][4] = (first detection, first ground truth, first kept detection, first IoU element), int64, totals last —
// the convention of oks_eval.hip, so the table is also mpn_oks_match's.  cat_tab[n_cat + 1][2] = (first kept detection, first
// ground truth) of every category: a category's kept detections and ground truths are contiguous.
//   1. box_iou_kernel: one workgroup per row.  Stable rank sort of the row's detections by descending score (ties: lower input
//      index first), truncation to max_dets, w * h of the detection's own box, its position inside the row, the kept x G IoU block.
//   2. box_rank_kernel: stable descending sort of every category's kept detections by (score, concatenation position) as a
//      segmented rank sort (compares through LDS broadcasts inside the segment, unique ranks, no scratch).
//   3. box_accum_kernel: one workgroup per (category, area range, maxDets entry, threshold).  COCOeval slices every image's list
//      to maxDets[m] and merge-sorts the concatenation; a stable subsequence of the full stable order is the same order, so the
//      one sort serves every m and a detection whose in-row position is >= maxDets[m] is carried as an entry that adds to neither
//      tp nor fp: it repeats its predecessor's (tp, fp), hence its precision, and changes no maximum and no lower bound.
#include "common.h"

namespace {

constexpr int kMaxDets = 128;
constexpr int kMaxM = 4;
constexpr double kEps = 2.220446049250313e-16;       // np.spacing(1) = 2^-52

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

// blockIdx.y = category, blockIdx.x = 256-detection chunk of its segment.  Rank of kept detection k inside the segment =
// #{j in segment : s_j > s_k or (s_j == s_k and j < k)}; order[segment start + rank] = k
__global__ void __launch_bounds__(256) box_rank_kernel(const double* __restrict__ score, const int64_t* __restrict__ cat_tab,
                                                       int32_t* __restrict__ order) {
    __shared__ double ssc[1024];
    const long s0 = cat_tab[2 * blockIdx.y], s1 = cat_tab[2 * blockIdx.y + 2];
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

// one workgroup of 1024 threads per (category c, area range a, maxDets entry m, threshold t): blockIdx.x = ((c*A + a)*M + m)*T + t
__global__ void __launch_bounds__(1024) box_accum_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ kept_rank,
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
    const long s0 = cat_tab[2 * c], g0 = cat_tab[2 * c + 1];
    const long n = cat_tab[2 * c + 2] - s0, ng = cat_tab[2 * c + 3] - g0;
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
            if (k >= s0 && k < s0 + n && kept_rank[k] < md) {
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

inline long box_align(long v) { return (v + 255) / 256 * 256; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// the table on the host: rows ascend, every row keeps min(detections, max_dets), its IoU block is kept x ground truths
inline bool box_tab_ok(const int64_t* tab, int n_row, int max_dets) {
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
inline bool box_cat_tab_ok(const int64_t* ct, int n_cat, int64_t n_kept, int64_t n_gt) {
    if (ct[0] != 0 || ct[1] != 0) return false;
    for (int c = 0; c < n_cat; ++c)
        if (ct[2 * c + 2] < ct[2 * c] || ct[2 * c + 3] < ct[2 * c + 1]) return false;
    return ct[2 * n_cat] == n_kept && ct[2 * n_cat + 1] == n_gt;
}

}  // namespace

extern "C" int64_t mpn_box_eval_workspace_bytes(int64_t n_kept, int n_area, int n_max, int n_thr) {
    if (n_kept <= 0 || n_area <= 0 || n_max <= 0 || n_thr <= 0) return 256;
    const long amt = (long)n_area * n_max * n_thr;
    return box_align(amt * n_kept * 4) + box_align(amt * n_kept * 8);
}

extern "C" int mpn_box_iou_matrix(const double* det_box, const double* det_score, const double* gt_box, const int32_t* gt_flags,
                                  const int64_t* tab_host, const int64_t* tab, int n_row, int max_dets, int32_t* kept_src,
                                  double* kept_score, double* kept_area, int32_t* kept_rank, double* iou, void* stream) {
    MPN_CHECK_ARG(det_box && det_score && gt_box && gt_flags && tab_host && tab && kept_src && kept_score && kept_area && kept_rank &&
                  iou);
    MPN_CHECK_ARG(n_row > 0 && max_dets >= 1 && max_dets <= kMaxDets);
    MPN_CHECK_ARG(al8(det_box) && al8(det_score) && al8(gt_box) && al8(tab) && al8(kept_score) && al8(kept_area) && al8(iou));
    MPN_CHECK_ARG(box_tab_ok(tab_host, n_row, max_dets));
    hipLaunchKernelGGL(box_iou_kernel, dim3(n_row), dim3(256), 0, (hipStream_t)stream, det_box, det_score, gt_box, gt_flags, tab,
                       kept_src, kept_score, kept_area, kept_rank, iou);
    return mpn_launch_status();
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
    MPN_CHECK_ARG(box_cat_tab_ok(cat_tab_host, n_cat, n_kept, n_gt));
    unsigned md_packed = 0;                              // maxDets[m] - 1 in eight bits each
    for (int m = 0; m < n_max; ++m) {
        MPN_CHECK_ARG(max_dets_host[m] >= 1 && max_dets_host[m] <= kMaxDets);
        md_packed |= (unsigned)(max_dets_host[m] - 1) << (8 * m);
    }
    const long blocks = (long)n_cat * n_area * n_max * n_thr;
    MPN_CHECK_ARG(blocks <= 0x7fffffffL);
    hipStream_t st = (hipStream_t)stream;
    const long amt = (long)n_area * n_max * n_thr;
    int32_t* tp_ws = (int32_t*)workspace;
    double* pr_ws = (double*)((char*)workspace + box_align(amt * n_kept * 4));
    long seg = 0;
    for (int c = 0; c < n_cat; ++c) {
        const long n = (long)(cat_tab_host[2 * c + 2] - cat_tab_host[2 * c]);
        seg = n > seg ? n : seg;
    }
    if (seg > 0)
        hipLaunchKernelGGL(box_rank_kernel, dim3((unsigned)((seg + 255) / 256), (unsigned)n_cat), dim3(256), 0, st, kept_score, cat_tab, order);
    hipLaunchKernelGGL(box_accum_kernel, dim3((unsigned)blocks), dim3(1024), 0, st, order, kept_rank, det_match, det_ig, gt_ig, cat_tab,
                       (long)n_kept, (long)n_gt, n_area, n_max, n_thr, md_packed, rec_thrs, n_rec, tp_ws, pr_ws, precision, recall);
    return mpn_launch_status();
}
