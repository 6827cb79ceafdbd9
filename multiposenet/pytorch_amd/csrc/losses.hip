// losses.hip — heat-map MSE, focal + smooth-L1 detection loss, PRN softmax / BCE for gfx950.
//
// Reference: build_keypoint_loss network/posenet.py:367-403 (5 x MSELoss(size_average=True) over
// pred[:, :18]*w vs w*gt, plus max/min of the final heat-map), FocalLoss network/losses.py:27-137
// (alpha .25, gamma 2, IoU<.4 negative / >=.5 positive, smooth-L1 beta 1/9, per-image python loop
// replaced by one thread per (image, anchor)), calc_iou losses.py:5-22, PRN softmax + BCELoss
// posenet.py:345-347,427-445.  All reductions are two-stage and deterministic (no atomics).
#include "common.h"

namespace {

constexpr int MSE_CHUNK = 256 * 16;     // elements (pixel*18 + c) per block

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}

struct PredPtrs { const float* p[5]; long sP[5]; };
struct DPredPtrs { float* p[5]; long sP[5]; int C[5]; };
struct SegC { int C[5]; };              // live channels of the five predictions: a level has the person-segmentation channel iff C >= 19

// partial[block][8] = {sum_j (5), unused, max, min}
__global__ void mse_fwd_kernel(PredPtrs pr, const float* __restrict__ gt, const float* __restrict__ wgt, long nelem,
                               float* __restrict__ partial) {
    __shared__ float sh[4][8];
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float mx = -INFINITY, mn = INFINITY;
    const long base = (long)blockIdx.x * MSE_CHUNK;
    for (int it = 0; it < 16; ++it) {
        const long e = base + it * 256 + threadIdx.x;
        if (e < nelem) {
            const long pix = e / 18; const int c = (int)(e - pix * 18);
            const float w = wgt[e], g = gt[e];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float pv = pr.p[j][pix * pr.sP[j] + c];
                const float d = pv * w - w * g;
                s[j] += d * d;
                if (j == 4) { mx = fmaxf(mx, pv); mn = fminf(mn, pv); }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = wave_sum(s[j]);
    mx = wave_max(mx); mn = wave_min(mn);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) sh[wave][j] = s[j];
        sh[wave][6] = mx; sh[wave][7] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = partial + (long)blockIdx.x * 8;
#pragma unroll
        for (int j = 0; j < 5; ++j) o[j] = sh[0][j] + sh[1][j] + sh[2][j] + sh[3][j];
        o[5] = 0.f;
        o[6] = fmaxf(fmaxf(sh[0][6], sh[1][6]), fmaxf(sh[2][6], sh[3][6]));
        o[7] = fminf(fminf(sh[0][7], sh[1][7]), fminf(sh[2][7], sh[3][7]));
    }
}

__global__ void mse_finalize_kernel(const float* __restrict__ partial, int chunks, double nelem, float* __restrict__ out) {
    __shared__ double sh[256][5];
    __shared__ float shm[256][2];
    double s[5] = {0, 0, 0, 0, 0};
    float mx = -INFINITY, mn = INFINITY;
    for (int i = threadIdx.x; i < chunks; i += 256) {
        const float* o = partial + (long)i * 8;
        for (int j = 0; j < 5; ++j) s[j] += (double)o[j];
        mx = fmaxf(mx, o[6]); mn = fminf(mn, o[7]);
    }
    for (int j = 0; j < 5; ++j) sh[threadIdx.x][j] = s[j];
    shm[threadIdx.x][0] = mx; shm[threadIdx.x][1] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 256; ++i) {
            for (int j = 0; j < 5; ++j) tot[j] += sh[i][j];
            mx = fmaxf(mx, shm[i][0]); mn = fminf(mn, shm[i][1]);
        }
        float total = 0.f;
        for (int j = 0; j < 5; ++j) { const float l = (float)(tot[j] / nelem); out[j] = l; total += l; }
        out[5] = total; out[6] = mx; out[7] = mn;
    }
}

// d(total)/d(pred_j) at one full-resolution element.  Contraction is off so that mse_bwd_kernel (API path: full-resolution f32
// gradients, summed onto the coarser levels by import_grad) and mse_train_kernel (recorded step: the same sums inside one launch)
// round identically; the recorded step's parameters then stay bit-identical to the eager step's.
__device__ __forceinline__ float mse_grad(float k, float w, float g, float pv) {
#pragma clang fp contract(off)
    const float a = pv * w;
    const float b = w * g;
    const float d = a - b;
    const float kw = k * w;
    return kw * d;
}

// d(total)/d(pred_j[.., 18]) of the person-segmentation term mean((P - M)^2) / 100: ks = gs * 2 / (100 * npix).  Contraction off
// for the same reason as above.
__device__ __forceinline__ float seg_grad(float ks, float m, float pv) {
#pragma clang fp contract(off)
    const float d = pv - m;
    return ks * d;
}

// one thread per (pixel, channel < Cmax); dpred_j[pix*sP + c] = gs*2*w*(p*w - w*g)/N, 0 for c >= 18.  SEG (the sibling with a
// mask_all target, mask [npix]): channel 18 of every level that has one carries the seg term's gradient instead of 0.
template <bool SEG>
__global__ void mse_bwd_kernel(PredPtrs pr, DPredPtrs dp, const float* __restrict__ gt, const float* __restrict__ wgt,
                               const float* __restrict__ mask, long npix, int Cmax, const float* __restrict__ gscale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix * Cmax) return;
    const long pix = i / Cmax; const int c = (int)(i - pix * Cmax);
    const float gs = gscale ? gscale[0] : 1.f;
    const float k = gs * 2.0f / (float)((double)npix * 18.0);
    float w = 0.f, g = 0.f;
    if (c < 18) { w = wgt[pix * 18 + c]; g = gt[pix * 18 + c]; }
    float ks = 0.f, m = 0.f;
    if (SEG && c == 18) { ks = gs * 2.0f / (float)((double)npix * 100.0); m = mask[pix]; }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        if (c >= dp.C[j] || dp.p[j] == nullptr) continue;
        float v = 0.f;
        if (c < 18) v = mse_grad(k, w, g, pr.p[j][pix * pr.sP[j] + c]);
        else if (SEG && c == 18) v = seg_grad(ks, m, pr.p[j][pix * pr.sP[j] + 18]);
        dp.p[j][pix * dp.sP[j] + c] = v;
    }
}

// ---- the person-segmentation term of the API forward: seg_j = mean_pix((P_j[pix, 18] - M[pix])^2) / 100 for every level with a
// nineteenth channel (C[j] >= 19), 0 for the others.  One lane per pixel, 16 pixels per lane and block sums as mse_fwd_kernel's;
// partial[block][8] = {sum_j (5), unused, max, min of channel 18 of the final prediction (-inf / +inf without one)}.
constexpr int SEG_CHUNK = 256 * 16;     // pixels per block
__global__ void mse_seg_fwd_kernel(PredPtrs pr, SegC sc, const float* __restrict__ mask, long npix, float* __restrict__ partial) {
    __shared__ float sh[4][8];
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float mx = -INFINITY, mn = INFINITY;
    const long base = (long)blockIdx.x * SEG_CHUNK;
    for (int it = 0; it < 16; ++it) {
        const long pix = base + it * 256 + threadIdx.x;
        if (pix < npix) {
            const float m = mask[pix];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (sc.C[j] < 19) continue;
                const float pv = pr.p[j][pix * pr.sP[j] + 18];
                const float d = pv - m;
                s[j] += d * d;
                if (j == 4) { mx = fmaxf(mx, pv); mn = fminf(mn, pv); }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = wave_sum(s[j]);
    mx = wave_max(mx); mn = wave_min(mn);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) sh[wave][j] = s[j];
        sh[wave][6] = mx; sh[wave][7] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = partial + (long)blockIdx.x * 8;
#pragma unroll
        for (int j = 0; j < 5; ++j) o[j] = sh[0][j] + sh[1][j] + sh[2][j] + sh[3][j];
        o[5] = 0.f;
        o[6] = fmaxf(fmaxf(sh[0][6], sh[1][6]), fmaxf(sh[2][6], sh[3][6]));
        o[7] = fminf(fminf(sh[0][7], sh[1][7]), fminf(sh[2][7], sh[3][7]));
    }
}

// out[MPN_MSE_SEG_OUT]: [0..7] the heat-map vector mse_finalize_kernel has written; [8..12] seg means, [13] their sum, [14] / [15]
// max / min of channel 18 of the final prediction (0 / 0 without one), [16] = out[5] + out[13], the total.  Sums in float64.
__global__ void mse_seg_finalize_kernel(const float* __restrict__ partial, int chunks, double npix, int final_has_seg,
                                        float* __restrict__ out) {
    __shared__ double sh[256][5];
    __shared__ float shm[256][2];
    double s[5] = {0, 0, 0, 0, 0};
    float mx = -INFINITY, mn = INFINITY;
    for (int i = threadIdx.x; i < chunks; i += 256) {
        const float* o = partial + (long)i * 8;
        for (int j = 0; j < 5; ++j) s[j] += (double)o[j];
        mx = fmaxf(mx, o[6]); mn = fminf(mn, o[7]);
    }
    for (int j = 0; j < 5; ++j) sh[threadIdx.x][j] = s[j];
    shm[threadIdx.x][0] = mx; shm[threadIdx.x][1] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 256; ++i) {
            for (int j = 0; j < 5; ++j) tot[j] += sh[i][j];
            mx = fmaxf(mx, shm[i][0]); mn = fminf(mn, shm[i][1]);
        }
        float total = 0.f;
        for (int j = 0; j < 5; ++j) { const float l = (float)(tot[j] / (npix * 100.0)); out[8 + j] = l; total += l; }
        out[13] = total;
        out[14] = final_has_seg ? mx : 0.f;
        out[15] = final_has_seg ? mn : 0.f;
        out[16] = out[5] + total;
        for (int j = 17; j < MPN_MSE_SEG_OUT; ++j) out[j] = 0.f;
    }
}

// ---- recorded training step: loss AND gradients in one pass over the INTERNAL tensors (no exported f32 copies) --------------
// Levels 0..3 are the intermediate maps k2..k5 at 1, 1/2, 1/4, 1/8 of the heat-map resolution (posenet.py:243-257 up-samples them
// with nearest neighbours, so a full-resolution pixel (y, x) reads level s at (y >> s, x >> s) and the gradient of a coarse cell is
// the sum over its 4^s children); level 4 is the final prediction.  One thread owns (8x8 pixel cell, channel): it walks its 64
// pixels in row-major order, which is the order import_grad_kernel sums children in, so the coarse gradients round identically.
// Block = 8 cells x 32 channel lanes; lanes >= 18 write the zero padding of the gradient tensors.
struct TrainPtrs { const float* p[5]; void* d[5]; int Cs[5]; };

// SEG (mpn_mse_heatmap_seg_train): lane 18 is live on every level with a nineteenth channel, with w = 1, g = M (the mask_all plane,
// [B][1][H][W] dense, read with the same two 16-byte loads per row) and its own scale 2 gs / (100 B H W).  With w = 1 the heat
// term's expressions ARE the seg term's (p * 1 - 1 * g = p - M, (k * 1) * d = k d: multiplying by 1 is exact), so the lane takes
// the same cell walk and its coarse sums round as import_grad's; its sums, max and min leave through seg_partial.  On a level
// without the channel lane 18 reads nothing and writes the zero it always wrote.  With SEG false every `on` is `live` and the
// kernel is mpn_mse_heatmap_train's as it was.
template <typename T, bool SEG>
__global__ void __launch_bounds__(256) mse_train_kernel(TrainPtrs tp, const float* __restrict__ gt, const float* __restrict__ wgt,
                                                        long g_sB, long g_sC, long g_sH, int B, int H, int W, long ncell,
                                                        const float* __restrict__ gscale, float* __restrict__ partial,
                                                        const float* __restrict__ mask, SegC sc, float* __restrict__ seg_partial) {
    __shared__ float sh[4][SEG ? 16 : 8];
    const int c = threadIdx.x & 31;
    const long cell = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float mx = -INFINITY, mn = INFINITY;
    const bool live = c < 18;
    const bool segl = SEG && c == 18;
    if (cell < ncell) {
        const int cw = W >> 3, ch = H >> 3;
        const int cx = (int)(cell % cw);
        const int cy = (int)((cell / cw) % ch);
        const int b = (int)(cell / ((long)cw * ch));
        const int y0 = cy * 8, x0 = cx * 8;
        const float gs = gscale ? gscale[0] : 1.f;
        const float k = segl ? gs * 2.0f / (float)((double)B * H * W * 100.0) : gs * 2.0f / (float)((double)B * H * W * 18.0);
        const bool act = live || segl;
        const bool on0 = live || (segl && sc.C[0] >= 19), on1 = live || (segl && sc.C[1] >= 19), on2 = live || (segl && sc.C[2] >= 19),
                   on3 = live || (segl && sc.C[3] >= 19), on4 = live || (segl && sc.C[4] >= 19);
        T* d0 = (T*)tp.d[0]; T* d1 = (T*)tp.d[1]; T* d2 = (T*)tp.d[2]; T* d3 = (T*)tp.d[3]; T* d4 = (T*)tp.d[4];
        float pv1[4] = {0.f, 0.f, 0.f, 0.f}, pv2[2] = {0.f, 0.f}, pv3 = 0.f;
        float a1[4], a2[2], a3 = 0.f;
        if (on3) pv3 = tp.p[3][(((long)b * ch + cy) * cw + cx) * tp.Cs[3] + c];
        for (int r = 0; r < 8; ++r) {
            const int y = y0 + r;
            float g[8], w[8];
            if (act) {
                if (segl) {
                    const float* mp = mask + ((long)b * H + y) * W + x0;
                    const float4 ga = *(const float4*)mp, gb = *(const float4*)(mp + 4);
                    g[0] = ga.x; g[1] = ga.y; g[2] = ga.z; g[3] = ga.w; g[4] = gb.x; g[5] = gb.y; g[6] = gb.z; g[7] = gb.w;
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[i] = 1.f;
                } else {
                    const float* gp = gt + b * g_sB + c * g_sC + y * g_sH + x0;
                    const float* wp = wgt + b * g_sB + c * g_sC + y * g_sH + x0;
                    const float4 ga = *(const float4*)gp, gb = *(const float4*)(gp + 4);
                    const float4 wa = *(const float4*)wp, wb = *(const float4*)(wp + 4);
                    g[0] = ga.x; g[1] = ga.y; g[2] = ga.z; g[3] = ga.w; g[4] = gb.x; g[5] = gb.y; g[6] = gb.z; g[7] = gb.w;
                    w[0] = wa.x; w[1] = wa.y; w[2] = wa.z; w[3] = wa.w; w[4] = wb.x; w[5] = wb.y; w[6] = wb.z; w[7] = wb.w;
                }
                if ((r & 1) == 0) {
                    const float* q = tp.p[1] + (((long)b * (H >> 1) + (y >> 1)) * (W >> 1) + (x0 >> 1)) * tp.Cs[1] + c;
#pragma unroll
                    for (int i = 0; i < 4; ++i) { pv1[i] = on1 ? q[(long)i * tp.Cs[1]] : 0.f; a1[i] = 0.f; }
                }
                if ((r & 3) == 0) {
                    const float* q = tp.p[2] + (((long)b * (H >> 2) + (y >> 2)) * (W >> 2) + (x0 >> 2)) * tp.Cs[2] + c;
#pragma unroll
                    for (int i = 0; i < 2; ++i) { pv2[i] = on2 ? q[(long)i * tp.Cs[2]] : 0.f; a2[i] = 0.f; }
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) { g[i] = 0.f; w[i] = 0.f; }
#pragma unroll
                for (int i = 0; i < 4; ++i) a1[i] = 0.f;
                a2[0] = a2[1] = 0.f;
            }
            const long row = ((long)b * H + y) * W + x0;
#pragma unroll
            for (int px = 0; px < 8; ++px) {
                float v0 = 0.f, v4 = 0.f;
                if (act) {
                    const float wv = w[px], gv = g[px];
                    const float wg = wv * gv;
                    float e;
                    if (on0) {
                        const float p0 = tp.p[0][(row + px) * tp.Cs[0] + c];
                        e = p0 * wv - wg;      s[0] += e * e;
                        v0 = 0.f + mse_grad(k, wv, gv, p0);
                    }
                    if (on1) { e = pv1[px >> 1] * wv - wg; s[1] += e * e; a1[px >> 1] += mse_grad(k, wv, gv, pv1[px >> 1]); }
                    if (on2) { e = pv2[px >> 2] * wv - wg; s[2] += e * e; a2[px >> 2] += mse_grad(k, wv, gv, pv2[px >> 2]); }
                    if (on3) { e = pv3 * wv - wg;     s[3] += e * e; a3 += mse_grad(k, wv, gv, pv3); }
                    if (on4) {
                        const float p4 = tp.p[4][(row + px) * tp.Cs[4] + c];
                        e = p4 * wv - wg;      s[4] += e * e;
                        mx = fmaxf(mx, p4); mn = fminf(mn, p4);
                        v4 = 0.f + mse_grad(k, wv, gv, p4);
                    }
                }
                Elem<T>::st(d0 + (row + px) * tp.Cs[0] + c, v0);
                Elem<T>::st(d4 + (row + px) * tp.Cs[4] + c, v4);
            }
            if (r & 1) {
                T* q = d1 + (((long)b * (H >> 1) + (y >> 1)) * (W >> 1) + (x0 >> 1)) * tp.Cs[1] + c;
#pragma unroll
                for (int i = 0; i < 4; ++i) Elem<T>::st(q + (long)i * tp.Cs[1], a1[i]);
            }
            if ((r & 3) == 3) {
                T* q = d2 + (((long)b * (H >> 2) + (y >> 2)) * (W >> 2) + (x0 >> 2)) * tp.Cs[2] + c;
#pragma unroll
                for (int i = 0; i < 2; ++i) Elem<T>::st(q + (long)i * tp.Cs[2], a2[i]);
            }
        }
        Elem<T>::st(d3 + (((long)b * ch + cy) * cw + cx) * tp.Cs[3] + c, a3);
    }
    // lane 18's sums are the seg term's: they leave the heat sums before the wave folds
    float ss[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float smx = -INFINITY, smn = INFINITY;
    if (segl) {
#pragma unroll
        for (int j = 0; j < 5; ++j) { ss[j] = s[j]; s[j] = 0.f; }
        smx = mx; smn = mn; mx = -INFINITY; mn = INFINITY;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = wave_sum(s[j]);
    mx = wave_max(mx); mn = wave_min(mn);
    if (SEG) {
#pragma unroll
        for (int j = 0; j < 5; ++j) ss[j] = wave_sum(ss[j]);
        smx = wave_max(smx); smn = wave_min(smn);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) sh[wave][j] = s[j];
        sh[wave][6] = mx; sh[wave][7] = mn;
        if (SEG) {
#pragma unroll
            for (int j = 0; j < 5; ++j) sh[wave][(SEG ? 8 : 0) + j] = ss[j];
            sh[wave][SEG ? 14 : 6] = smx; sh[wave][SEG ? 15 : 7] = smn;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = partial + (long)blockIdx.x * 8;
#pragma unroll
        for (int j = 0; j < 5; ++j) o[j] = sh[0][j] + sh[1][j] + sh[2][j] + sh[3][j];
        o[5] = 0.f;
        o[6] = fmaxf(fmaxf(sh[0][6], sh[1][6]), fmaxf(sh[2][6], sh[3][6]));
        o[7] = fminf(fminf(sh[0][7], sh[1][7]), fminf(sh[2][7], sh[3][7]));
        if (SEG) {
            constexpr int S0 = SEG ? 8 : 0;
            float* q = seg_partial + (long)blockIdx.x * 8;
#pragma unroll
            for (int j = 0; j < 5; ++j) q[j] = sh[0][S0 + j] + sh[1][S0 + j] + sh[2][S0 + j] + sh[3][S0 + j];
            q[5] = 0.f;
            q[6] = fmaxf(fmaxf(sh[0][S0 + 6], sh[1][S0 + 6]), fmaxf(sh[2][S0 + 6], sh[3][S0 + 6]));
            q[7] = fminf(fminf(sh[0][S0 + 7], sh[1][S0 + 7]), fminf(sh[2][S0 + 7], sh[3][S0 + 7]));
        }
    }
}

// ------------------------------------------------------------------------------- focal loss
struct Assign { float iou_max; int arg; };

__device__ __forceinline__ Assign assign_anchor(const float4 a, const float* __restrict__ anno, int maxN) {
    // losses.py:5-22 (no +1; union clamped at 1e-8), argmax = first maximum (losses.py:59)
    Assign r; r.iou_max = -1.f; r.arg = -1;
    const float area_a = (a.z - a.x) * (a.w - a.y);
    for (int n = 0; n < maxN; ++n) {
        const float* g = anno + n * 5;
        if (g[4] == -1.f) continue;
        const float area_b = (g[2] - g[0]) * (g[3] - g[1]);
        float iw = fminf(a.z, g[2]) - fmaxf(a.x, g[0]);
        float ih = fminf(a.w, g[3]) - fmaxf(a.y, g[1]);
        iw = fmaxf(iw, 0.f); ih = fmaxf(ih, 0.f);
        float ua = area_a + area_b - iw * ih;
        ua = fmaxf(ua, 1e-8f);
        const float iou = (iw * ih) / ua;
        if (iou > r.iou_max) { r.iou_max = iou; r.arg = n; }
    }
    return r;
}

__device__ __forceinline__ void reg_targets(const float4 a, const float* g, float t[4]) {
    // losses.py:97-121
    const float aw = a.z - a.x, ah = a.w - a.y;
    const float acx = a.x + 0.5f * aw, acy = a.y + 0.5f * ah;
    float gw = g[2] - g[0], gh = g[3] - g[1];
    const float gcx = g[0] + 0.5f * gw, gcy = g[1] + 0.5f * gh;
    gw = fmaxf(gw, 1.f); gh = fmaxf(gh, 1.f);
    t[0] = ((gcx - acx) / aw) / 0.1f;
    t[1] = ((gcy - acy) / ah) / 0.1f;
    t[2] = logf(gw / aw) / 0.2f;
    t[3] = logf(gh / ah) / 0.2f;
}

// grid (blocksA, B); partial[(b*blocksA + blk)*4] = {cls_sum, reg_sum, npos, nvalid_anno}
__global__ void focal_fwd_kernel(const float* __restrict__ cls, const float* __restrict__ reg, const float* __restrict__ anchors,
                                 const float* __restrict__ anno, int A, int maxN, float* __restrict__ partial) {
    __shared__ float sh[4][3];
    const int b = blockIdx.y;
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const float* an = anno + (long)b * maxN * 5;
    float cl = 0.f, rl = 0.f, np = 0.f;
    int nvalid = 0;
    for (int n = 0; n < maxN; ++n) nvalid += (an[n * 5 + 4] != -1.f);
    if (a < A && nvalid > 0) {
        const float4 box = *reinterpret_cast<const float4*>(anchors + (long)a * 4);
        const Assign as = assign_anchor(box, an, maxN);
        float p = cls[(long)b * A + a];
        p = fminf(fmaxf(p, 1e-4f), 1.0f - 1e-4f);
        if (as.iou_max >= 0.5f) {
            const float om = 1.f - p;
            cl = 0.25f * om * om * (-logf(p));
            np = 1.f;
            float t[4]; reg_targets(box, an + as.arg * 5, t);
            const float4 r = *reinterpret_cast<const float4*>(reg + ((long)b * A + a) * 4);
            const float rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = fabsf(t[k] - rr[k]);
                rl += (d <= 1.0f / 9.0f) ? 0.5f * 9.0f * d * d : d - 0.5f / 9.0f;
            }
        } else if (as.iou_max < 0.4f) {
            cl = 0.75f * p * p * (-logf(1.f - p));
        }
    }
    cl = wave_sum(cl); rl = wave_sum(rl); np = wave_sum(np);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[wave][0] = cl; sh[wave][1] = rl; sh[wave][2] = np; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = partial + ((long)b * gridDim.x + blockIdx.x) * 4;
        o[0] = sh[0][0] + sh[1][0] + sh[2][0] + sh[3][0];
        o[1] = sh[0][1] + sh[1][1] + sh[2][1] + sh[3][1];
        o[2] = sh[0][2] + sh[1][2] + sh[2][2] + sh[3][2];
        o[3] = (float)nvalid;
    }
}

// one block; per_img[b] = {cls_sum, reg_sum, npos, nvalid}; out = {cls_loss, reg_loss}
__global__ void focal_finalize_kernel(const float* __restrict__ partial, int B, int blocksA, float* __restrict__ per_img,
                                      float* __restrict__ out) {
    __shared__ double shc[256], shr[256];
    double csum = 0.0, rsum = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        double c = 0.0, r = 0.0, n = 0.0; float nv = 0.f;
        for (int k = 0; k < blocksA; ++k) {
            const float* o = partial + ((long)b * blocksA + k) * 4;
            c += o[0]; r += o[1]; n += o[2]; nv = o[3];
        }
        per_img[b * 4 + 0] = (float)c; per_img[b * 4 + 1] = (float)r; per_img[b * 4 + 2] = (float)n; per_img[b * 4 + 3] = nv;
        if (nv > 0.f) {
            csum += (double)((float)c / fmaxf((float)n, 1.f));
            if (n > 0.0) rsum += (double)((float)r / (4.f * (float)n));
        }
    }
    shc[threadIdx.x] = csum; shr[threadIdx.x] = rsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0, r = 0.0;
        for (int i = 0; i < 256; ++i) { c += shc[i]; r += shr[i]; }
        out[0] = (float)(c / B); out[1] = (float)(r / B);
    }
}

__global__ void focal_bwd_kernel(const float* __restrict__ cls, const float* __restrict__ reg, const float* __restrict__ anchors,
                                 const float* __restrict__ anno, int B, int A, int maxN, const float* __restrict__ per_img,
                                 const float* __restrict__ gscale, float* __restrict__ dcls, float* __restrict__ dreg) {
    const int b = blockIdx.y;
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    const float gs = gscale ? gscale[0] : 1.f;        // upstream grad of the classification loss
    const float gsr = gscale ? gscale[1] : 1.f;       // upstream grad of the regression loss
    const float* an = anno + (long)b * maxN * 5;
    const float npos = per_img[b * 4 + 2], nvalid = per_img[b * 4 + 3];
    float dc = 0.f;
    float dr[4] = {0.f, 0.f, 0.f, 0.f};
    if (nvalid > 0.f) {
        const float4 box = *reinterpret_cast<const float4*>(anchors + (long)a * 4);
        const Assign as = assign_anchor(box, an, maxN);
        const float praw = cls[(long)b * A + a];
        const bool inrange = (praw >= 1e-4f) && (praw <= 1.0f - 1e-4f);     // clamp passes gradient inside [min, max]
        const float p = fminf(fmaxf(praw, 1e-4f), 1.0f - 1e-4f);
        const float kc = gs / ((float)B * fmaxf(npos, 1.f));
        if (as.iou_max >= 0.5f) {
            const float om = 1.f - p;
            if (inrange) dc = kc * 0.25f * (2.f * om * logf(p) - om * om / p);
            float t[4]; reg_targets(box, an + as.arg * 5, t);
            const float4 r = *reinterpret_cast<const float4*>(reg + ((long)b * A + a) * 4);
            const float rr[4] = {r.x, r.y, r.z, r.w};
            const float kr = gsr / ((float)B * 4.f * npos);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float e = rr[k] - t[k];
                const float d = fabsf(e);
                dr[k] = kr * ((d <= 1.0f / 9.0f) ? 9.0f * e : (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)));
            }
        } else if (as.iou_max < 0.4f) {
            if (inrange) dc = kc * 0.75f * (-2.f * p * logf(1.f - p) + p * p / (1.f - p));
        }
    }
    dcls[(long)b * A + a] = dc;
    *reinterpret_cast<float4*>(dreg + ((long)b * A + a) * 4) = make_float4(dr[0], dr[1], dr[2], dr[3]);
}

// ------------------------------------------------------------------------- multi-class focal loss
// losses.py:27-137 with K > 1 classes: one-hot targets (IoU >= .5: 1 at the annotation's class, 0 at the other K - 1; IoU < .4: 0
// everywhere; between: ignored).  A block owns FMC_TILE anchors of one image.  Its lanes first assign one anchor each (the state goes
// to LDS, the smooth-L1 term stays in the lane), then the block streams the anchors' contiguous [FMC_TILE x K] slice of cls with
// 16-byte accesses: no lane walks a K-float row of its own.
constexpr int FMC_TILE = 256;
constexpr int FMC_IGNORE = -1;      // anchor state in LDS: ignored, negative at every class, or (>= 0) positive at that class;
constexpr int FMC_NEG = -2;         // a positive whose class id lies outside [0, K) is stored as K and matches no column

// int(anno[..., 4]) (losses.py:77 .long(), truncation) when it lies in [0, K), else K (NaN included)
__device__ __forceinline__ int focal_class(float c, int K) {
    const float t = truncf(c);
    return (t >= 0.f && t < (float)K) ? (int)t : K;
}

// Lane t of the block visits the elements [0, n) of a slice of rows of K floats: the scalar head up to a 16-byte boundary of src,
// a float4 body, a scalar tail.  f(r, c, x) gets the element's row and column within the slice and its value: one division per
// float4, then the column steps.  STORE: f's result goes to the same element of dst (same address as src modulo 16 bytes).
template <bool STORE, typename F>
__device__ __forceinline__ void stream_rows(const float* __restrict__ src, float* __restrict__ dst, int n, int K, F f) {
    const int t = threadIdx.x;
    const unsigned uK = (unsigned)K;
    int head = (int)(((16u - ((unsigned)(uintptr_t)src & 15u)) & 15u) >> 2);
    head = head < n ? head : n;
    auto one = [&](int e) {
        const unsigned r = (unsigned)e / uK;
        const float y = f((int)r, (int)((unsigned)e - r * uK), src[e]);
        if (STORE) dst[e] = y;
    };
    if (t < head) one(t);
    const int nv = (n - head) >> 2;
    const float4* __restrict__ v = reinterpret_cast<const float4*>(src + head);
    auto quad = [&](int i, const float4 x) {
        const unsigned e = (unsigned)(head + 4 * i);
        int r = (int)(e / uK), c = (int)(e - (unsigned)r * uK);
        const float xs[4] = {x.x, x.y, x.z, x.w};
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y[j] = f(r, c, xs[j]);
            if (++c == K) { c = 0; ++r; }
        }
        if (STORE) reinterpret_cast<float4*>(dst + head)[i] = make_float4(y[0], y[1], y[2], y[3]);
    };
    // two 16-byte loads in flight per lane
    const int stride = blockDim.x;
    int i = t;
    for (; i + stride < nv; i += 2 * stride) {
        const float4 x0 = v[i], x1 = v[i + stride];
        quad(i, x0);
        quad(i + stride, x1);
    }
    if (i < nv) quad(i, v[i]);
    const int e = head + 4 * nv + t;
    if (e < n) one(e);
}

// per image: valid annotations and those among them whose class id lies outside [0, K)
__device__ __forceinline__ void focal_count_anno(const float* __restrict__ an, int maxN, int K, int& nvalid, int& nbad) {
    nvalid = 0; nbad = 0;
    for (int n = 0; n < maxN; ++n) {
        const float c = an[n * 5 + 4];
        if (c == -1.f) continue;
        ++nvalid;
        nbad += focal_class(c, K) == K;
    }
}

// grid (mpn_focal_mc_blocks(A), B); partial as focal_fwd_kernel's; bad[b] = annotations of image b with a class outside [0, K)
__global__ void __launch_bounds__(FMC_TILE) focal_fwd_mc_kernel(const float* __restrict__ cls, const float* __restrict__ reg,
        const float* __restrict__ anchors, const float* __restrict__ anno, int A, int K, int maxN, float* __restrict__ partial,
        float* __restrict__ bad) {
    __shared__ int st[FMC_TILE];
    __shared__ float sh[4][3];
    const int b = blockIdx.y, a0 = blockIdx.x * FMC_TILE, t = threadIdx.x;
    const float* an = anno + (long)b * maxN * 5;
    int nvalid, nbad;
    focal_count_anno(an, maxN, K, nvalid, nbad);
    float cl = 0.f, rl = 0.f, np = 0.f;
    int s = FMC_IGNORE;
    const int a = a0 + t;
    if (a < A && nvalid > 0) {
        const float4 box = *reinterpret_cast<const float4*>(anchors + (long)a * 4);
        const Assign as = assign_anchor(box, an, maxN);
        if (as.iou_max >= 0.5f) {
            s = focal_class(an[as.arg * 5 + 4], K);
            np = 1.f;
            float tg[4]; reg_targets(box, an + as.arg * 5, tg);
            const float4 r = *reinterpret_cast<const float4*>(reg + ((long)b * A + a) * 4);
            const float rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = fabsf(tg[k] - rr[k]);
                rl += (d <= 1.0f / 9.0f) ? 0.5f * 9.0f * d * d : d - 0.5f / 9.0f;
            }
        } else if (as.iou_max < 0.4f) {
            s = FMC_NEG;
        }
    }
    st[t] = s;
    __syncthreads();
    if (nvalid > 0) {
        const int na = min(FMC_TILE, A - a0);
        stream_rows<false>(cls + ((long)b * A + a0) * K, nullptr, na * K, K, [&](int r, int c, float x) -> float {
            const int sa = st[r];
            if (sa == FMC_IGNORE) return 0.f;
            const float p = fminf(fmaxf(x, 1e-4f), 1.0f - 1e-4f);
            if (sa == c) {
                const float om = 1.f - p;
                cl += 0.25f * (om * om) * (-logf(p));
            } else {
                cl += 0.75f * (p * p) * (-logf(1.f - p));
            }
            return 0.f;
        });
    }
    cl = wave_sum(cl); rl = wave_sum(rl); np = wave_sum(np);
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) { sh[wave][0] = cl; sh[wave][1] = rl; sh[wave][2] = np; }
    __syncthreads();
    if (t == 0) {
        float* o = partial + ((long)b * gridDim.x + blockIdx.x) * 4;
        o[0] = sh[0][0] + sh[1][0] + sh[2][0] + sh[3][0];
        o[1] = sh[0][1] + sh[1][1] + sh[2][1] + sh[3][1];
        o[2] = sh[0][2] + sh[1][2] + sh[2][2] + sh[3][2];
        o[3] = (float)nvalid;
        if (blockIdx.x == 0) bad[b] = (float)nbad;
    }
}

// grid (mpn_focal_mc_blocks(A), B): dcls [B,A,K] (every element written), dreg [B,A,4]; ((cls ^ dcls) & 15) == 0
__global__ void __launch_bounds__(FMC_TILE) focal_bwd_mc_kernel(const float* __restrict__ cls, const float* __restrict__ reg,
        const float* __restrict__ anchors, const float* __restrict__ anno, int B, int A, int K, int maxN,
        const float* __restrict__ per_img, const float* __restrict__ gscale, float* __restrict__ dcls, float* __restrict__ dreg) {
    __shared__ int st[FMC_TILE];
    const int b = blockIdx.y, a0 = blockIdx.x * FMC_TILE, t = threadIdx.x;
    const float gs = gscale ? gscale[0] : 1.f;
    const float gsr = gscale ? gscale[1] : 1.f;
    const float* an = anno + (long)b * maxN * 5;
    const float npos = per_img[b * 4 + 2], nvalid = per_img[b * 4 + 3];
    int s = FMC_IGNORE;
    const int a = a0 + t;
    if (a < A) {
        float dr[4] = {0.f, 0.f, 0.f, 0.f};
        if (nvalid > 0.f) {
            const float4 box = *reinterpret_cast<const float4*>(anchors + (long)a * 4);
            const Assign as = assign_anchor(box, an, maxN);
            if (as.iou_max >= 0.5f) {
                s = focal_class(an[as.arg * 5 + 4], K);
                float tg[4]; reg_targets(box, an + as.arg * 5, tg);
                const float4 r = *reinterpret_cast<const float4*>(reg + ((long)b * A + a) * 4);
                const float rr[4] = {r.x, r.y, r.z, r.w};
                const float kr = gsr / ((float)B * 4.f * npos);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float e = rr[k] - tg[k];
                    const float d = fabsf(e);
                    dr[k] = kr * ((d <= 1.0f / 9.0f) ? 9.0f * e : (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)));
                }
            } else if (as.iou_max < 0.4f) {
                s = FMC_NEG;
            }
        }
        *reinterpret_cast<float4*>(dreg + ((long)b * A + a) * 4) = make_float4(dr[0], dr[1], dr[2], dr[3]);
    }
    st[t] = s;
    __syncthreads();
    const int na = min(FMC_TILE, A - a0);
    const long base = ((long)b * A + a0) * K;
    const float kc = gs / ((float)B * fmaxf(npos, 1.f));
    stream_rows<true>(cls + base, dcls + base, na * K, K, [&](int r, int c, float x) -> float {
        const int sa = st[r];
        if (sa == FMC_IGNORE || !((x >= 1e-4f) && (x <= 1.0f - 1e-4f))) return 0.f;     // clamp passes gradient inside [min, max]
        const float p = x;
        if (sa == c) {
            const float om = 1.f - p;
            return kc * 0.25f * (2.f * om * logf(p) - om * om / p);
        }
        return kc * 0.75f * (-2.f * p * logf(1.f - p) + p * p / (1.f - p));
    });
}

// ------------------------------------------------------------------------- class maximum
// posenet.py:267 / :283: max over the K classes of every anchor and the index of the first maximum (torch.max(dim) ties; a NaN
// wins, the first NaN).  A block stages R whole rows through LDS (coalesced 16-byte loads; row stride K + 1 words spreads the
// banks), then 256 / R lanes reduce each row and combine with shuffles.
__device__ __forceinline__ bool cmax_better(float v2, int i2, float v1, int i1) {
    const bool n2 = v2 != v2, n1 = v1 != v1;
    if (n2 != n1) return n2;
    if (n2) return i2 < i1;
    return v2 > v1 || (v2 == v1 && i2 < i1);
}

__global__ void __launch_bounds__(256) class_max_kernel(const float* __restrict__ cls, long rows, int K, int R,
                                                        float* __restrict__ score, int64_t* __restrict__ cls_id) {
    extern __shared__ float rows_lds[];
    const long r0 = (long)blockIdx.x * R;
    const int nr = (int)min((long)R, rows - r0);
    const int ld = K + 1;
    stream_rows<false>(cls + r0 * K, nullptr, nr * K, K, [&](int r, int c, float x) -> float {
        rows_lds[r * ld + c] = x;
        return 0.f;
    });
    __syncthreads();
    const int L = 256 / R;                 // lanes per row: a power of two <= 64, so a row's lanes sit in one wave
    const int row = threadIdx.x / L, j = threadIdx.x % L;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if (row < nr) {
        for (int c = j; c < K; c += L) {
            const float v = rows_lds[row * ld + c];
            if (cmax_better(v, c, best, bi)) { best = v; bi = c; }
        }
    }
    for (int m = L >> 1; m >= 1; m >>= 1) {
        const float v2 = __shfl_xor(best, m, 64);
        const int i2 = __shfl_xor(bi, m, 64);
        if (cmax_better(v2, i2, best, bi)) { best = v2; bi = i2; }
    }
    if (row < nr && j == 0) {
        score[r0 + row] = best;
        cls_id[r0 + row] = (int64_t)bi;
    }
}

__global__ void sigmoid_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ p, float* __restrict__ dl, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const float pv = p[i]; dl[i] = dp[i] * pv * (1.f - pv); }
}

__global__ void sigmoid_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = 1.0f / (1.0f + expf(-x[i]));
}

// ------------------------------------------------------------------------------- PRN pieces
__global__ void add_softmax_rows_kernel(const float* __restrict__ a, long a_stride, const float* __restrict__ res, float* __restrict__ out, int cols, int relu) {
    __shared__ float sh[4];
    __shared__ float bc;
    const long row = blockIdx.x;
    const float* pa = a + row * a_stride; const float* pr = res + row * cols; float* po = out + row * cols;
    float mx = -INFINITY;
    const float lo = relu ? 0.f : -INFINITY;      // F.relu(dens2(.)) is folded in (posenet.py:343)
    for (int i = threadIdx.x; i < cols; i += 256) mx = fmaxf(mx, fmaxf(pa[i], lo) + pr[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) bc = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    __syncthreads();
    mx = bc;
    float s = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256) s += expf(fmaxf(pa[i], lo) + pr[i] - mx);
    s = wave_sum(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bc = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    const float inv = 1.0f / bc;
    for (int i = threadIdx.x; i < cols; i += 256) po[i] = expf(fmaxf(pa[i], lo) + pr[i] - mx) * inv;
}

// dlogit[r][i] = p * (dp - sum_j p_j dp_j)  (softmax backward, one block per row)
__global__ void softmax_rows_bwd_kernel(const float* __restrict__ p, const float* __restrict__ dp, const float* __restrict__ pre, long pre_stride, float* __restrict__ dl, int cols) {
    __shared__ float sh[4];
    __shared__ float bc;
    const long row = blockIdx.x;
    const float* pp = p + row * cols; const float* pd = dp + row * cols; float* po = dl + row * cols;
    float s = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256) s += pp[i] * pd[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bc = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    const float dot = bc;
    for (int i = threadIdx.x; i < cols; i += 256) {
        const float g = pp[i] * (pd[i] - dot);
        po[i] = (pre == nullptr || pre[row * pre_stride + i] > 0.f) ? g : 0.f;      // relu mask of the pre-activation
    }
}

// BCELoss(mean) backward, torch semantics: d/dp = (p - y) / max(p (1 - p), 1e-12) / N
__global__ void bce_bwd_kernel(const float* __restrict__ p, const float* __restrict__ y, float* __restrict__ dp, long n,
                               const float* __restrict__ gscale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gs = (gscale ? gscale[0] : 1.f) / (float)n;
    const float pv = p[i];
    dp[i] = gs * (pv - y[i]) / fmaxf(pv * (1.f - pv), 1e-12f);
}

// counter-based dropout: keep element i iff hash(seed, i) >= p; kept values are scaled by 1/(1-p).
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ y, long n, unsigned long long seed, float p, float scale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long h = mix64(mix64(seed) ^ (unsigned long long)i);
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
    Elem<T>::st(y + i, u >= p ? Elem<T>::ld(x + i) * scale : 0.f);
}

__global__ void bce_partial_kernel(const float* __restrict__ p, const float* __restrict__ y, long n, float* __restrict__ partial) {
    __shared__ float sh[4];
    float s = 0.f;
    const long base = (long)blockIdx.x * 4096;
    for (int it = 0; it < 16; ++it) {
        const long i = base + it * 256 + threadIdx.x;
        if (i < n) {
            const float lp = fmaxf(logf(p[i]), -100.f), lq = fmaxf(logf(1.f - p[i]), -100.f);
            s += -(y[i] * lp + (1.f - y[i]) * lq);
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void mean_finalize_kernel(const float* __restrict__ partial, int chunks, double n, float* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < chunks; i += 256) s += (double)partial[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0.0; for (int i = 0; i < 256; ++i) t += sh[i]; out[0] = (float)(t / n); }
}

// ---- recorded PRN step (replay.py): dropout seeded from device memory, input packing, loss head in one launch ----------------
// dropout_kernel with seed = state[0] + k (wrapping): the recorded launch list holds the pointer and k, the word moves on by
// dropout_advance_kernel once per step, so every replay draws the masks the eager step's host-made seeds would give.
template <typename T>
__global__ void dropout_dev_kernel(const T* __restrict__ x, T* __restrict__ y, long n, const unsigned long long* __restrict__ state,
                                   unsigned long long k, float p, float scale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long seed = state[0] + k;
    const unsigned long long h = mix64(mix64(seed) ^ (unsigned long long)i);
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);
    Elem<T>::st(y + i, u >= p ? Elem<T>::ld(x + i) * scale : 0.f);
}

__global__ void dropout_advance_kernel(unsigned long long* __restrict__ state, unsigned long long inc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    state[0] = state[0] + inc;
}

// y[r][c] = (T) x[r][c] for c < n, 0 for n <= c < npad: the PRN's input row as the first Linear layer reads it
template <typename T>
__global__ void prn_pack_kernel(const float* __restrict__ x, T* __restrict__ y, long total, int n, int npad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long r = i / npad; const int c = (int)(i - r * npad);
    Elem<T>::st(y + i, c < n ? x[r * n + c] : 0.f);
}

// The values add_softmax_rows_kernel stores and bce_bwd_kernel / softmax_rows_bwd_kernel read back are f32 in memory; here they
// stay in registers, so the products that were rounded by that store must not fuse with the operation that consumes them.
__device__ __forceinline__ float prn_prob(float e, float inv) {
#pragma clang fp contract(off)
    const float p = e * inv;
    return p;
}
__device__ __forceinline__ float prn_dprob(float gs, float pv, float y) {
#pragma clang fp contract(off)
    const float d = gs * (pv - y) / fmaxf(pv * (1.f - pv), 1e-12f);
    return d;
}
__device__ __forceinline__ float prn_dlogit(float pv, float dp, float dot) {
#pragma clang fp contract(off)
    const float g = pv * (dp - dot);
    return g;
}

// add_softmax_rows (relu = 1) -> BCE mean forward / backward -> softmax_rows_backward -> cast, one workgroup per row; p and dp
// are recomputed per pass instead of stored (four passes over o / res, two over label).  Each pass keeps the producing kernel's
// lane-strided accumulation, wave reduction and four-wave combine, so dl carries the chain's bits; the loss leaves as one f32
// partial per row (mean_finalize_kernel sums them in double).
template <typename T>
__global__ void __launch_bounds__(256) prn_head_train_kernel(const float* __restrict__ a, long a_stride, const float* __restrict__ res,
                                                             const float* __restrict__ label, const float* __restrict__ gscale,
                                                             T* __restrict__ dl, int cols, int npad, long ntotal,
                                                             float* __restrict__ partial) {
    __shared__ float sh[4];
    __shared__ float sl[4];
    __shared__ float bc;
    const long row = blockIdx.x;
    const float* pa = a + row * a_stride; const float* pr = res + row * cols; const float* py = label + row * cols;
    T* po = dl + row * npad;
    float mx = -INFINITY;
    const float lo = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256) mx = fmaxf(mx, fmaxf(pa[i], lo) + pr[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) bc = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    __syncthreads();
    mx = bc;
    float s = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256) s += expf(fmaxf(pa[i], lo) + pr[i] - mx);
    s = wave_sum(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bc = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    const float inv = 1.0f / bc;
    const float gs = (gscale ? gscale[0] : 1.f) / (float)ntotal;
    s = 0.f;
    float ls = 0.f;
    for (int i = threadIdx.x; i < cols; i += 256) {
        const float pv = prn_prob(expf(fmaxf(pa[i], lo) + pr[i] - mx), inv);
        const float yv = py[i];
        const float dp = prn_dprob(gs, pv, yv);
        s += pv * dp;
        const float lp = fmaxf(logf(pv), -100.f), lq = fmaxf(logf(1.f - pv), -100.f);
        ls += -(yv * lp + (1.f - yv) * lq);
    }
    s = wave_sum(s);
    ls = wave_sum(ls);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = s; sl[threadIdx.x >> 6] = ls; }
    __syncthreads();
    if (threadIdx.x == 0) { bc = sh[0] + sh[1] + sh[2] + sh[3]; partial[row] = sl[0] + sl[1] + sl[2] + sl[3]; }
    __syncthreads();
    const float dot = bc;
    for (int i = threadIdx.x; i < cols; i += 256) {
        const float av = pa[i];
        const float pv = prn_prob(expf(fmaxf(av, lo) + pr[i] - mx), inv);
        const float dp = prn_dprob(gs, pv, py[i]);
        const float g = prn_dlogit(pv, dp, dot);
        Elem<T>::st(po + i, av > 0.f ? g : 0.f);      // relu mask of the pre-activation
    }
    for (int i = cols + threadIdx.x; i < npad; i += 256) Elem<T>::st(po + i, 0.f);
}

}  // namespace

extern "C" int mpn_mse_chunks(int64_t npix) { return (int)((npix * 18 + MSE_CHUNK - 1) / MSE_CHUNK); }

extern "C" int mpn_mse_heatmap_forward(const float* const* preds, const int64_t* pred_sP, const float* gt, const float* wgt,
                                       int64_t npix, float* partial, int chunks, float* out, void* stream) {
    MPN_CHECK_ARG(preds && pred_sP && gt && wgt && partial && out && npix > 0);
    MPN_CHECK_ARG(chunks == mpn_mse_chunks(npix));
    PredPtrs pr;
    for (int j = 0; j < 5; ++j) { pr.p[j] = preds[j]; pr.sP[j] = (long)pred_sP[j]; MPN_CHECK_ARG(preds[j] != nullptr); }
    hipLaunchKernelGGL(mse_fwd_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, pr, gt, wgt, (long)npix * 18, partial);
    hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, chunks, (double)npix * 18.0, out);
    return mpn_launch_status();
}

extern "C" int mpn_mse_heatmap_backward(const float* const* preds, float* const* dpreds, const int64_t* pred_sP,
                                        const int64_t* dpred_sP, const int32_t* pred_C, const float* gt, const float* wgt,
                                        int64_t npix, const float* gscale, void* stream) {
    MPN_CHECK_ARG(preds && dpreds && pred_sP && dpred_sP && pred_C && gt && wgt && npix > 0);
    PredPtrs pr; DPredPtrs dp; int cmax = 0;
    for (int j = 0; j < 5; ++j) {
        pr.p[j] = preds[j]; pr.sP[j] = (long)pred_sP[j];
        dp.p[j] = dpreds[j]; dp.sP[j] = (long)dpred_sP[j]; dp.C[j] = pred_C[j];
        if (pred_C[j] > cmax) cmax = pred_C[j];
    }
    const long n = (long)npix * cmax;
    hipLaunchKernelGGL(mse_bwd_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pr, dp, gt, wgt,
                       (const float*)nullptr, (long)npix, cmax, gscale);
    return mpn_launch_status();
}

extern "C" int mpn_mse_seg_chunks(int64_t npix) { return (int)((npix + SEG_CHUNK - 1) / SEG_CHUNK); }

extern "C" int mpn_mse_heatmap_seg_forward(const float* const* preds, const int64_t* pred_sP, const int32_t* pred_C, const float* gt,
                                           const float* wgt, const float* mask, int64_t npix, float* partial, int chunks,
                                           float* seg_partial, int seg_chunks, float* out, void* stream) {
    MPN_CHECK_ARG(preds && pred_sP && pred_C && gt && wgt && mask && partial && seg_partial && out && npix > 0 && npix <= 0x7fffffffL);
    MPN_CHECK_ARG(chunks == mpn_mse_chunks(npix) && seg_chunks == mpn_mse_seg_chunks(npix));
    MPN_CHECK_ARG(((uintptr_t)gt | (uintptr_t)wgt | (uintptr_t)mask | (uintptr_t)partial | (uintptr_t)seg_partial | (uintptr_t)out) % 4 == 0);
    PredPtrs pr; SegC sc;
    for (int j = 0; j < 5; ++j) {
        MPN_CHECK_ARG(preds[j] != nullptr && (uintptr_t)preds[j] % 4 == 0 && pred_C[j] >= 18 && pred_sP[j] >= pred_C[j]);
        pr.p[j] = preds[j]; pr.sP[j] = (long)pred_sP[j]; sc.C[j] = pred_C[j];
    }
    hipStream_t st = (hipStream_t)stream;
    // the heat term: mpn_mse_heatmap_forward's two launches, so out[0..7] are its bits
    hipLaunchKernelGGL(mse_fwd_kernel, dim3((unsigned)chunks), dim3(256), 0, st, pr, gt, wgt, (long)npix * 18, partial);
    hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, chunks, (double)npix * 18.0, out);
    hipLaunchKernelGGL(mse_seg_fwd_kernel, dim3((unsigned)seg_chunks), dim3(256), 0, st, pr, sc, mask, (long)npix, seg_partial);
    hipLaunchKernelGGL(mse_seg_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)seg_partial, seg_chunks, (double)npix,
                       sc.C[4] >= 19 ? 1 : 0, out);
    return mpn_launch_status();
}

extern "C" int mpn_mse_heatmap_seg_backward(const float* const* preds, float* const* dpreds, const int64_t* pred_sP,
                                            const int64_t* dpred_sP, const int32_t* pred_C, const float* gt, const float* wgt,
                                            const float* mask, int64_t npix, const float* gscale, void* stream) {
    MPN_CHECK_ARG(preds && dpreds && pred_sP && dpred_sP && pred_C && gt && wgt && mask && npix > 0 && npix <= 0x7fffffffL);
    MPN_CHECK_ARG(((uintptr_t)gt | (uintptr_t)wgt | (uintptr_t)mask | (uintptr_t)gscale) % 4 == 0);
    PredPtrs pr; DPredPtrs dp; int cmax = 0;
    for (int j = 0; j < 5; ++j) {
        // a level that gets a gradient is read at channel c < pred_C[j] of both tensors
        MPN_CHECK_ARG(preds[j] != nullptr && (uintptr_t)preds[j] % 4 == 0 && (uintptr_t)dpreds[j] % 4 == 0 && pred_C[j] >= 0 && pred_C[j] <= 32);
        MPN_CHECK_ARG(dpreds[j] == nullptr || (pred_C[j] >= 18 && pred_sP[j] >= pred_C[j] && dpred_sP[j] >= pred_C[j]));
        pr.p[j] = preds[j]; pr.sP[j] = (long)pred_sP[j];
        dp.p[j] = dpreds[j]; dp.sP[j] = (long)dpred_sP[j]; dp.C[j] = pred_C[j];
        if (pred_C[j] > cmax) cmax = pred_C[j];
    }
    MPN_CHECK_ARG(cmax >= 18);
    const long n = (long)npix * cmax;
    hipLaunchKernelGGL(mse_bwd_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pr, dp, gt, wgt, mask,
                       (long)npix, cmax, gscale);
    return mpn_launch_status();
}

extern "C" int mpn_mse_train_blocks(int B, int H, int W) { return (int)(((long)B * (H / 8) * (W / 8) + 7) / 8); }

extern "C" int mpn_mse_heatmap_train(const float* const* levels, void* const* dlevels, const int32_t* level_Cs, int dtype,
                                     const float* gt, const float* wgt, int64_t g_sB, int64_t g_sC, int64_t g_sH,
                                     int B, int H, int W, const float* gscale, float* partial, int blocks, float* out, void* stream) {
    MPN_CHECK_ARG(levels && dlevels && level_Cs && gt && wgt && partial && out && B > 0);
    MPN_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && blocks == mpn_mse_train_blocks(B, H, W));
    MPN_CHECK_ARG(g_sH % 4 == 0 && g_sC % 4 == 0 && g_sB % 4 == 0 && ((uintptr_t)gt & 15) == 0 && ((uintptr_t)wgt & 15) == 0);
    TrainPtrs tp;
    for (int j = 0; j < 5; ++j) {
        MPN_CHECK_ARG(levels[j] && dlevels[j] && level_Cs[j] == 32);
        tp.p[j] = levels[j]; tp.d[j] = dlevels[j]; tp.Cs[j] = level_Cs[j];
    }
    const long ncell = (long)B * (H / 8) * (W / 8);
    MPN_DISPATCH_T(dtype, hipLaunchKernelGGL((mse_train_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tp, gt, wgt,
                                             (long)g_sB, (long)g_sC, (long)g_sH, B, H, W, ncell, gscale, partial, (const float*)nullptr, SegC(),
                                             (float*)nullptr));
    hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, blocks,
                       (double)B * H * W * 18.0, out);
    return mpn_launch_status();
}

extern "C" int mpn_mse_heatmap_seg_train(const float* const* levels, void* const* dlevels, const int32_t* level_Cs, const int32_t* level_C,
                                         int dtype, const float* gt, const float* wgt, const float* mask, int64_t g_sB, int64_t g_sC,
                                         int64_t g_sH, int B, int H, int W, const float* gscale, float* partial, int blocks, float* out,
                                         void* stream) {
    MPN_CHECK_ARG(levels && dlevels && level_Cs && level_C && gt && wgt && mask && partial && out && B > 0);
    MPN_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && blocks == mpn_mse_train_blocks(B, H, W) && (long)B * H * W <= 0x7fffffffL);
    MPN_CHECK_ARG(g_sH % 4 == 0 && g_sC % 4 == 0 && g_sB % 4 == 0 && ((uintptr_t)gt & 15) == 0 && ((uintptr_t)wgt & 15) == 0);
    MPN_CHECK_ARG(((uintptr_t)mask & 15) == 0 && (((uintptr_t)partial | (uintptr_t)out | (uintptr_t)gscale) & 3) == 0);
    MPN_CHECK_ARG(dtype == MPN_F32 || dtype == MPN_BF16 || dtype == MPN_F16);
    TrainPtrs tp; SegC sc;
    for (int j = 0; j < 5; ++j) {
        MPN_CHECK_ARG(levels[j] && dlevels[j] && level_Cs[j] == 32 && level_C[j] >= 18 && level_C[j] <= 32 && ((uintptr_t)levels[j] & 3) == 0);
        tp.p[j] = levels[j]; tp.d[j] = dlevels[j]; tp.Cs[j] = level_Cs[j]; sc.C[j] = level_C[j];
    }
    const long ncell = (long)B * (H / 8) * (W / 8);
    float* seg_partial = partial + (long)blocks * 8;                     // partial: blocks * 16 floats, the heat records first
    MPN_DISPATCH_T(dtype, hipLaunchKernelGGL((mse_train_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tp, gt, wgt,
                                             (long)g_sB, (long)g_sC, (long)g_sH, B, H, W, ncell, gscale, partial, mask, sc, seg_partial));
    hipLaunchKernelGGL(mse_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, blocks,
                       (double)B * H * W * 18.0, out);
    hipLaunchKernelGGL(mse_seg_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)seg_partial, blocks,
                       (double)B * H * W, sc.C[4] >= 19 ? 1 : 0, out);
    return mpn_launch_status();
}

extern "C" int mpn_focal_blocks(int A) { return (A + 255) / 256; }

extern "C" int mpn_focal_forward(const float* cls, const float* reg, const float* anchors, const float* anno, int B, int A,
                                 int maxN, float* partial, float* per_img, float* out, void* stream) {
    MPN_CHECK_ARG(cls && reg && anchors && anno && partial && per_img && out && B > 0 && A > 0 && maxN > 0);
    const int blocksA = (A + 255) / 256;
    hipLaunchKernelGGL(focal_fwd_kernel, dim3(blocksA, B), dim3(256), 0, (hipStream_t)stream, cls, reg, anchors, anno, A, maxN, partial);
    hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, B, blocksA, per_img, out);
    return mpn_launch_status();
}

extern "C" int mpn_focal_backward(const float* cls, const float* reg, const float* anchors, const float* anno, int B, int A,
                                  int maxN, const float* per_img, const float* gscale, float* dcls, float* dreg, void* stream) {
    MPN_CHECK_ARG(cls && reg && anchors && anno && per_img && dcls && dreg && B > 0 && A > 0 && maxN > 0);
    hipLaunchKernelGGL(focal_bwd_kernel, dim3((A + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, cls, reg, anchors, anno, B, A, maxN,
                       per_img, gscale, dcls, dreg);
    return mpn_launch_status();
}

extern "C" int mpn_focal_mc_blocks(int A) { return (A + FMC_TILE - 1) / FMC_TILE; }

extern "C" int mpn_focal_forward_mc(const float* cls, const float* reg, const float* anchors, const float* anno, int B, int A, int K,
                                    int maxN, float* partial, float* per_img, float* bad, float* out, void* stream) {
    MPN_CHECK_ARG(cls && reg && anchors && anno && partial && per_img && bad && out && B > 0 && A > 0 && K > 0 && maxN > 0);
    MPN_CHECK_ARG((int64_t)FMC_TILE * K < (int64_t)1 << 31);
    const int blocksA = mpn_focal_mc_blocks(A);
    hipLaunchKernelGGL(focal_fwd_mc_kernel, dim3(blocksA, B), dim3(FMC_TILE), 0, (hipStream_t)stream, cls, reg, anchors, anno, A, K, maxN,
                       partial, bad);
    hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, B, blocksA, per_img, out);
    return mpn_launch_status();
}

extern "C" int mpn_focal_backward_mc(const float* cls, const float* reg, const float* anchors, const float* anno, int B, int A, int K,
                                     int maxN, const float* per_img, const float* gscale, float* dcls, float* dreg, void* stream) {
    MPN_CHECK_ARG(cls && reg && anchors && anno && per_img && dcls && dreg && B > 0 && A > 0 && K > 0 && maxN > 0);
    MPN_CHECK_ARG((int64_t)FMC_TILE * K < (int64_t)1 << 31);
    MPN_CHECK_ARG((((uintptr_t)cls ^ (uintptr_t)dcls) & 15) == 0 && ((uintptr_t)cls & 3) == 0);
    hipLaunchKernelGGL(focal_bwd_mc_kernel, dim3(mpn_focal_mc_blocks(A), B), dim3(FMC_TILE), 0, (hipStream_t)stream, cls, reg, anchors,
                       anno, B, A, K, maxN, per_img, gscale, dcls, dreg);
    return mpn_launch_status();
}

extern "C" int mpn_class_max(const float* cls, int B, int A, int K, float* score, int64_t* cls_id, void* stream) {
    MPN_CHECK_ARG(cls && score && cls_id && B > 0 && A > 0 && K > 0 && K < 4096 && ((uintptr_t)cls & 3) == 0);
    int R = 256;                                              // rows per block: the staged rows fill at most 32 KB (64 KB for K > 2047)
    while (R > 4 && (long)R * (K + 1) * 4 > 32768) R >>= 1;
    const long rows = (long)B * A;
    const long blocks = (rows + R - 1) / R;
    MPN_CHECK_ARG(blocks < (1L << 31));
    hipLaunchKernelGGL(class_max_kernel, dim3((unsigned)blocks), dim3(256), (size_t)R * (K + 1) * 4, (hipStream_t)stream, cls, rows, K, R,
                       score, cls_id);
    return mpn_launch_status();
}

extern "C" int mpn_sigmoid_backward(const float* dp, const float* p, float* dlogit, int64_t n, void* stream) {
    MPN_CHECK_ARG(dp && p && dlogit && n > 0);
    hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dp, p, dlogit, (long)n);
    return mpn_launch_status();
}

extern "C" int mpn_sigmoid_forward(const float* x, float* y, int64_t n, void* stream) {
    MPN_CHECK_ARG(x && y && n > 0);
    hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n);
    return mpn_launch_status();
}

extern "C" int mpn_add_softmax_rows(const float* a, int64_t a_stride, const float* res, float* out, int rows, int cols, int relu, void* stream) {
    MPN_CHECK_ARG(a && res && out && rows > 0 && cols > 0 && a_stride >= cols);
    hipLaunchKernelGGL(add_softmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, a, (long)a_stride, res, out, cols, relu);
    return mpn_launch_status();
}

extern "C" int mpn_softmax_rows_backward(const float* p, const float* dp, const float* pre_relu, int64_t pre_stride, float* dlogit, int rows, int cols, void* stream) {
    MPN_CHECK_ARG(p && dp && dlogit && rows > 0 && cols > 0 && (!pre_relu || pre_stride >= cols));
    hipLaunchKernelGGL(softmax_rows_bwd_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, p, dp, pre_relu, (long)pre_stride, dlogit, cols);
    return mpn_launch_status();
}

extern "C" int mpn_bce_mean_backward(const float* p, const float* label, float* dp, int64_t n, const float* gscale, void* stream) {
    MPN_CHECK_ARG(p && label && dp && n > 0);
    hipLaunchKernelGGL(bce_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, label, dp, (long)n, gscale);
    return mpn_launch_status();
}

extern "C" int mpn_dropout(const void* x, void* y, int64_t n, uint64_t seed, float p, int dtype, void* stream) {
    MPN_CHECK_ARG(x && y && n > 0 && p >= 0.f && p < 1.f);
    const float scale = 1.0f / (1.0f - p);
    MPN_DISPATCH_T(dtype, hipLaunchKernelGGL((dropout_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, (long)n, (unsigned long long)seed, p, scale));
    return mpn_launch_status();
}

// log vector of the combined step: [0..4] level losses, [5] heat-map total, [6] max_ht, [7] min_ht, [8] detection total
// (cls + reg), [9] cls, [10] reg, [11] loss = heat-map total + detection total — the additions torch would do on the host side
__global__ void step_log_kernel(const float* __restrict__ kp8, const float* __restrict__ det2, float* __restrict__ logv) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float kp_total = 0.f, det_total = 0.f;
    if (kp8) {
        for (int i = 0; i < 8; ++i) logv[i] = kp8[i];
        kp_total = kp8[5];
    }
    if (det2) {
        det_total = det2[0] + det2[1];
        logv[8] = det_total; logv[9] = det2[0]; logv[10] = det2[1];
    }
    logv[11] = (kp8 && det2) ? kp_total + det_total : (kp8 ? kp_total : det_total);
}

extern "C" int mpn_step_log(const float* kp8, const float* det2, float* logv, void* stream) {
    MPN_CHECK_ARG(logv && (kp8 || det2));
    hipLaunchKernelGGL(step_log_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, kp8, det2, logv);
    return mpn_launch_status();
}

// The step log with the person-segmentation term (kp = the MPN_MSE_SEG_OUT vector of mpn_mse_heatmap_seg_forward): [0..12] keep their
// meaning ([11] loss = kp[16] + detection total, [12] is the clip's), [13..17] seg means, [18] seg total, [19] / [20] max / min of
// channel 18 of the final prediction.
__global__ void step_log_seg_kernel(const float* __restrict__ kp, const float* __restrict__ det2, float* __restrict__ logv) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < 8; ++i) { logv[i] = kp[i]; logv[13 + i] = kp[8 + i]; }
    float det_total = 0.f;
    if (det2) {
        det_total = det2[0] + det2[1];
        logv[8] = det_total; logv[9] = det2[0]; logv[10] = det2[1];
    }
    logv[11] = det2 ? kp[16] + det_total : kp[16];
}

extern "C" int mpn_step_log_seg(const float* kp, const float* det2, float* logv, void* stream) {
    MPN_CHECK_ARG(logv && kp && ((uintptr_t)logv | (uintptr_t)kp | (uintptr_t)det2) % 4 == 0);
    hipLaunchKernelGGL(step_log_seg_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, kp, det2, logv);
    return mpn_launch_status();
}

extern "C" int mpn_bce_chunks(int64_t n) { return (int)((n + 4095) / 4096); }

extern "C" int mpn_bce_mean_forward(const float* p, const float* label, int64_t n, float* partial, int chunks, float* out, void* stream) {
    MPN_CHECK_ARG(p && label && partial && out && n > 0 && chunks == mpn_bce_chunks(n));
    hipLaunchKernelGGL(bce_partial_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, p, label, (long)n, partial);
    hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, chunks, (double)n, out);
    return mpn_launch_status();
}

extern "C" int mpn_dropout_dev(const void* x, void* y, int64_t n, const uint64_t* state, uint64_t k, float p, int dtype, void* stream) {
    MPN_CHECK_ARG(x && y && state && n > 0 && p >= 0.f && p < 1.f && mpn_dtype_ok(dtype));
    const uintptr_t esz = dtype == MPN_F32 ? 4 : 2;
    MPN_CHECK_ARG(((uintptr_t)state & 7) == 0 && ((uintptr_t)x & (esz - 1)) == 0 && ((uintptr_t)y & (esz - 1)) == 0);
    const float scale = 1.0f / (1.0f - p);
    MPN_DISPATCH_T(dtype, hipLaunchKernelGGL((dropout_dev_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, (long)n,
                                             (const unsigned long long*)state, (unsigned long long)k, p, scale));
    return mpn_launch_status();
}

extern "C" int mpn_dropout_advance(uint64_t* state, uint64_t inc, void* stream) {
    MPN_CHECK_ARG(state && ((uintptr_t)state & 7) == 0);
    hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)state, (unsigned long long)inc);
    return mpn_launch_status();
}

extern "C" int mpn_prn_pack(const float* x, void* y, int rows, int n, int npad, int dtype, void* stream) {
    MPN_CHECK_ARG(x && y && rows > 0 && n > 0 && npad >= n && mpn_dtype_ok(dtype));
    MPN_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & (dtype == MPN_F32 ? 3 : 1)) == 0);
    const long total = (long)rows * npad;
    MPN_DISPATCH_T(dtype, hipLaunchKernelGGL((prn_pack_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (T*)y, total, n, npad));
    return mpn_launch_status();
}

extern "C" int mpn_prn_head_train(const float* o, int64_t o_stride, const float* res, const float* label, const float* gscale, void* dl,
                                  int rows, int cols, int npad, int dtype, float* partial, float* loss, void* stream) {
    MPN_CHECK_ARG(o && res && label && dl && partial && loss && rows > 0 && cols > 0 && npad >= cols && o_stride >= cols && mpn_dtype_ok(dtype));
    MPN_CHECK_ARG((((uintptr_t)o | (uintptr_t)res | (uintptr_t)label | (uintptr_t)gscale | (uintptr_t)partial | (uintptr_t)loss) & 3) == 0);
    MPN_CHECK_ARG(((uintptr_t)dl & (dtype == MPN_F32 ? 3 : 1)) == 0);
    const long ntotal = (long)rows * cols;
    MPN_DISPATCH_T(dtype, hipLaunchKernelGGL((prn_head_train_kernel<T>), dim3(rows), dim3(256), 0, (hipStream_t)stream, o, (long)o_stride, res, label, gscale,
                                             (T*)dl, cols, npad, ntotal, partial));
    hipLaunchKernelGGL(mean_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, rows, (double)ntotal, loss);
    return mpn_launch_status();
}
