// seg_infer.hip — the inference side of the keypoint subnet's person-segmentation channel (channel 18 of a person_seg model's maps;
// evaluate/tester.py: return_masks, Tester.seg_eval).  include/mpn.h states the definitions.
//
//   mpn_seg_masks      : channel 18 of every image of a single-scale batch -> its image-sized binary mask (and, optionally, the
//                        float32 plane it thresholds): the H x W corner of the dsize-form bicubic resize of the [Hs, Ws] map to the
//                        D x D padded square, one launch for the batch.
//   mpn_tta_merge_mask : the multi-scale + flip merge (mpn_tta_merge's op sequence) of channel 18 alone: two-channel pair maps, no
//                        channel permutation, plane and / or mask, no accumulator plane in memory.
//   mpn_mask_iou       : per image the three integer counts (intersection, prediction, ground truth) of two uint8 planes.
//
// The bicubic sums are resize_kernel's (peaks.hip) in the same left-to-right form, the tap rule is resize_taps.h's; built with
// -ffp-contract=off like them, so both mask kernels equal the composed chain of existing launches bit for bit.  The counting kernel
// uses integer arithmetic only: its counts are the same on every run.
#include "common.h"
#include "resize_taps.h"

namespace {

constexpr int SGI_THREADS = 256;
constexpr int SGI_PX = 4;                                        // consecutive pixels of one row per lane: one 32-bit mask store
constexpr int SGI_TILE_W = 16 * SGI_PX;                          // 16 lanes along x
constexpr int SGI_TILE_H = SGI_THREADS / 16;

// INTER_CUBIC sample of one channel: element (y, x) at u[y * sY + x * sX]; rows first, then the column of the four row sums
__device__ __forceinline__ float cubic_sample(const float* __restrict__ u, long sY, long sX, const int (&yi)[4], const float (&yc)[4],
                                              const int (&xi)[4], const float (&xc)[4]) {
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* __restrict__ row = u + (long)yi[k] * sY;
        float a = row[(long)xi[0] * sX] * xc[0];
        a = a + row[(long)xi[1] * sX] * xc[1];
        a = a + row[(long)xi[2] * sX] * xc[2];
        a = a + row[(long)xi[3] * sX] * xc[3];
        r[k] = a;
    }
    float v = r[0] * yc[0];
    v = v + r[1] * yc[1];
    v = v + r[2] * yc[2];
    v = v + r[3] * yc[3];
    return v;
}

// The SGI_PX pixels (y, x .. x + SGI_PX - 1) of one lane: mask bytes as one word where the row start and the pitch are 4-byte aligned
// and all pixels lie inside the row, byte by byte otherwise (the store loop of segm_mask_miss_kernel); the plane values next to them.
__device__ __forceinline__ void store_pixels(const float (&p)[SGI_PX], float thr, int x, int W, uint8_t* __restrict__ mrow, bool aligned,
                                             float* __restrict__ prow) {
    uint32_t v = 0;
#pragma unroll
    for (int t = 0; t < SGI_PX; ++t) v |= (p[t] > thr ? 0xffu : 0u) << (8 * t);                // strict; a NaN compares false
    if (mrow) {
        if (aligned && x + SGI_PX <= W) {
            *reinterpret_cast<uint32_t*>(mrow + x) = v;
        } else {
#pragma unroll
            for (int t = 0; t < SGI_PX; ++t)
                if (x + t < W) mrow[x + t] = (uint8_t)(v >> (8 * t));
        }
    }
    if (prow) {
#pragma unroll
        for (int t = 0; t < SGI_PX; ++t)
            if (x + t < W) prow[x + t] = p[t];
    }
}

struct SegView {
    int D, H, W;
    long src, off, pitch, plane;
    bool ok;
};

// Image row -> registers.  ok: the [Hs, Ws] map lies in the source, the H x W mask in `out`, the dense plane (if any) in `planes`,
// and the image fits the grid.
__device__ __forceinline__ SegView load_view(const int64_t* __restrict__ row, long sY, long sX, int Hs, int Ws, long src_floats,
                                             long out_bytes, bool want_plane, long plane_floats, int max_w, int max_h) {
    SegView s;
    const int64_t D = row[MPN_SEGV_D], H = row[MPN_SEGV_H], W = row[MPN_SEGV_W];
    s.src = row[MPN_SEGV_SRC_OFF]; s.off = row[MPN_SEGV_OUT_OFF]; s.pitch = row[MPN_SEGV_OUT_PITCH]; s.plane = row[MPN_SEGV_PLANE_OFF];
    s.ok = H >= 1 && W >= 1 && H <= max_h && W <= max_w && D >= H && D >= W && D <= 65536;
    s.ok = s.ok && s.src >= 0 && s.src <= src_floats && (long)(Hs - 1) * sY + (long)(Ws - 1) * sX < src_floats - s.src;
    s.ok = s.ok && s.off >= 0 && s.pitch >= W && s.off <= out_bytes && s.pitch <= out_bytes && (H - 1) * s.pitch + W <= out_bytes - s.off;
    if (want_plane) s.ok = s.ok && s.plane >= 0 && s.plane <= plane_floats && H * W <= plane_floats - s.plane;
    s.D = s.ok ? (int)D : 1; s.H = s.ok ? (int)H : 1; s.W = s.ok ? (int)W : 1;
    return s;
}

// workgroup = 64 columns x 16 rows of one image; 16 lanes x 4 pixels are the 64 bytes of one mask row, a wave stores four rows
__global__ void __launch_bounds__(SGI_THREADS) seg_masks_kernel(const float* __restrict__ src, long sY, long sX, int Hs, int Ws, long src_floats,
                                                                const int64_t* __restrict__ imgs, int max_w, int max_h, float thr,
                                                                uint8_t* __restrict__ out, long out_bytes, float* __restrict__ planes,
                                                                long plane_floats) {
    const SegView im = load_view(imgs + (long)blockIdx.z * MPN_SEGV_COLS, sY, sX, Hs, Ws, src_floats, out_bytes, planes != nullptr,
                                 plane_floats, max_w, max_h);
    const int x = blockIdx.x * SGI_TILE_W + (threadIdx.x & 15) * SGI_PX, y = blockIdx.y * SGI_TILE_H + (threadIdx.x >> 4);
    if (!im.ok || x >= im.W || y >= im.H) return;
    const float* __restrict__ q = src + im.src;
    const double scale_y = (double)Hs / (double)im.D, scale_x = (double)Ws / (double)im.D;       // dsize form on the D x D grid
    int yi[4]; float yc[4];
    cubic_taps(y, scale_y, Hs, yi, yc);
    float p[SGI_PX];
#pragma unroll
    for (int t = 0; t < SGI_PX; ++t) {
        int xi[4]; float xc[4];
        cubic_taps(x + t, scale_x, Ws, xi, xc);                  // x + t < D: a column past W is computed and not stored
        p[t] = cubic_sample(q, sY, sX, yi, yc, xi, xc);
    }
    uint8_t* plane = out + im.off;
    const bool aligned = (((uintptr_t)plane | (uintptr_t)im.pitch) & 3) == 0;
    store_pixels(p, thr, x, im.W, plane + (long)y * im.pitch, aligned, planes ? planes + im.plane + (long)y * im.W : nullptr);
}

constexpr int SGI_MAX_SCALES = 8;
struct SegTtaTable {
    const float* u[SGI_MAX_SCALES];
    long pitch[SGI_MAX_SCALES];
    int rh[SGI_MAX_SCALES], rw[SGI_MAX_SCALES];
    int n;
};

// tta_merge_kernel (tta.hip) for the one channel of a seg pair map: channel 0 the original pass, channel 1 the mirrored pass read at
// column W - 1 - x; the same rounding points.  Tile and stores as seg_masks_kernel.
__global__ void __launch_bounds__(SGI_THREADS) tta_merge_mask_kernel(SegTtaTable t, int H, int W, float inv_n, float thr, float* __restrict__ plane,
                                                                     uint8_t* __restrict__ mask, long mask_pitch) {
    const int x = blockIdx.x * SGI_TILE_W + (threadIdx.x & 15) * SGI_PX, y = blockIdx.y * SGI_TILE_H + (threadIdx.x >> 4);
    if (x >= W || y >= H) return;
    double a_o[SGI_PX], a_f[SGI_PX];
#pragma unroll
    for (int k = 0; k < SGI_PX; ++k) a_o[k] = a_f[k] = 0.0;
    for (int s = 0; s < t.n; ++s) {
        const float* __restrict__ u = t.u[s];
        const long pitch = t.pitch[s];
        const int rh = t.rh[s], rw = t.rw[s];
        const double scale_y = (double)rh / (double)H, scale_x = (double)rw / (double)W;      // dsize form
        int yi[4]; float yc[4];
        cubic_taps(y, scale_y, rh, yi, yc);
#pragma unroll
        for (int k = 0; k < SGI_PX; ++k) {
            const int xo = x + k < W ? x + k : W - 1;            // a column past W: computed again, not stored
            int xi[4], xfi[4]; float xc[4], xfc[4];
            cubic_taps(xo, scale_x, rw, xi, xc);
            cubic_taps(W - 1 - xo, scale_x, rw, xfi, xfc);
            a_o[k] = a_o[k] + (double)(cubic_sample(u, pitch, 2, yi, yc, xi, xc) * inv_n);
            a_f[k] = a_f[k] + (double)(cubic_sample(u + 1, pitch, 2, yi, yc, xfi, xfc) * inv_n);
        }
    }
    float p[SGI_PX];
#pragma unroll
    for (int k = 0; k < SGI_PX; ++k) p[k] = (float)((a_o[k] + a_f[k]) * 0.5);                  // / 2. in float64: exact either way
    const bool aligned = (((uintptr_t)mask | (uintptr_t)mask_pitch) & 3) == 0;
    store_pixels(p, thr, x, W, mask ? mask + (long)y * mask_pitch : nullptr, aligned, plane ? plane + (long)y * W : nullptr);
}

constexpr int MIOU_ROWS = 32;                                    // rows of one image per workgroup

struct IouImg {
    int H, W;
    const uint8_t* p; const uint8_t* g;
    long pp, gp;
    bool ok;
};

__device__ __forceinline__ IouImg load_iou(const int64_t* __restrict__ row, const uint8_t* pred, long pred_bytes, const uint8_t* gt,
                                           long gt_bytes, int max_h) {
    IouImg s;
    const int64_t H = row[MPN_MIOU_H], W = row[MPN_MIOU_W], po = row[MPN_MIOU_PRED_OFF], pp = row[MPN_MIOU_PRED_PITCH],
                  go = row[MPN_MIOU_GT_OFF], gp = row[MPN_MIOU_GT_PITCH];
    s.ok = H >= 1 && H <= max_h && W >= 1 && W <= 65536;
    s.ok = s.ok && po >= 0 && pp >= W && po <= pred_bytes && pp <= pred_bytes && (H - 1) * pp + W <= pred_bytes - po;
    s.ok = s.ok && go >= 0 && gp >= W && go <= gt_bytes && gp <= gt_bytes && (H - 1) * gp + W <= gt_bytes - go;
    s.H = s.ok ? (int)H : 1; s.W = s.ok ? (int)W : 1;
    s.p = pred + (s.ok ? po : 0); s.g = gt + (s.ok ? go : 0);
    s.pp = s.ok ? pp : 1; s.gp = s.ok ? gp : 1;
    return s;
}

// bit 7 of every non-zero byte of a word
__device__ __forceinline__ unsigned long long nonzero_bytes(unsigned long long w) {
    const unsigned long long lo = 0x7f7f7f7f7f7f7f7full;
    return (((w & lo) + lo) | w) & ~lo;
}

__device__ __forceinline__ void count_word(unsigned long long p, unsigned long long g, unsigned& ni, unsigned& np, unsigned& ng) {
    const unsigned long long a = nonzero_bytes(p), b = nonzero_bytes(g);
    ni += (unsigned)__popcll(a & b); np += (unsigned)__popcll(a); ng += (unsigned)__popcll(b);
}

// workgroup = MIOU_ROWS rows of one image.  A row is V-byte units (V = 16 where the two plane starts and pitches are multiples of 16,
// 8 where of 8, else 1) and a byte tail; units of the tile's rows are dealt to the lanes round-robin, so a wave reads consecutive
// units.  Sums: registers -> wave (shuffles) -> LDS -> one integer atomic add per workgroup and counter.
__global__ void __launch_bounds__(SGI_THREADS) mask_iou_kernel(const uint8_t* __restrict__ pred, long pred_bytes, const uint8_t* __restrict__ gt,
                                                               long gt_bytes, const int64_t* __restrict__ imgs, int max_h,
                                                               unsigned long long* __restrict__ counts) {
    __shared__ unsigned red[SGI_THREADS / 64][3];
    const IouImg im = load_iou(imgs + (long)blockIdx.y * MPN_MIOU_COLS, pred, pred_bytes, gt, gt_bytes, max_h);
    const int y0 = blockIdx.x * MIOU_ROWS;
    if (!im.ok || y0 >= im.H) return;                            // the same for the whole workgroup
    const int rows = im.H - y0 < MIOU_ROWS ? im.H - y0 : MIOU_ROWS;
    const uintptr_t al = (uintptr_t)im.p | (uintptr_t)im.g | (uintptr_t)im.pp | (uintptr_t)im.gp;
    const int V = (al & 15) == 0 ? 16 : ((al & 7) == 0 ? 8 : 1);
    const int full = im.W / V, tail = im.W - full * V, upr = full + (tail ? 1 : 0);              // units per row
    unsigned ni = 0, np = 0, ng = 0;
    for (int i = threadIdx.x; i < rows * upr; i += SGI_THREADS) {
        const int r = i / upr, c = i - r * upr;
        const uint8_t* __restrict__ pr = im.p + (long)(y0 + r) * im.pp + (long)c * V;
        const uint8_t* __restrict__ gr = im.g + (long)(y0 + r) * im.gp + (long)c * V;
        if (c < full && V == 16) {
            const uint4 a = *reinterpret_cast<const uint4*>(pr), b = *reinterpret_cast<const uint4*>(gr);
            count_word((unsigned long long)a.x | ((unsigned long long)a.y << 32), (unsigned long long)b.x | ((unsigned long long)b.y << 32), ni, np, ng);
            count_word((unsigned long long)a.z | ((unsigned long long)a.w << 32), (unsigned long long)b.z | ((unsigned long long)b.w << 32), ni, np, ng);
        } else if (c < full && V == 8) {
            count_word(*reinterpret_cast<const unsigned long long*>(pr), *reinterpret_cast<const unsigned long long*>(gr), ni, np, ng);
        } else {
            const int nb = c < full ? 1 : tail;
            for (int k = 0; k < nb; ++k) {
                const unsigned a = pr[k] != 0, b = gr[k] != 0;
                ni += a & b; np += a; ng += b;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ni += __shfl_down(ni, d); np += __shfl_down(np, d); ng += __shfl_down(ng, d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = ni; red[wave][1] = np; red[wave][2] = ng; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < SGI_THREADS / 64; ++w) s += red[w][threadIdx.x];
        if (s) atomicAdd(counts + (long)blockIdx.y * 3 + threadIdx.x, s);
    }
}

// [a, a + na) and [b, b + nb) share no byte
static inline bool disjoint(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + (uintptr_t)na <= y || y + (uintptr_t)nb <= x;
}

}  // namespace

extern "C" int mpn_seg_masks(const float* src, int64_t sY, int64_t sX, int Hs, int Ws, int64_t src_floats, const int64_t* imgs, int n_img,
                             int max_w, int max_h, float thr, uint8_t* out, int64_t out_bytes, float* planes, int64_t plane_floats,
                             void* stream) {
    MPN_CHECK_ARG(src && imgs && out && Hs > 0 && Ws > 0 && sY > 0 && sX > 0 && n_img >= 1 && n_img <= 65535);
    MPN_CHECK_ARG(max_w >= 1 && max_w <= 65536 && max_h >= 1 && max_h <= 65536 && out_bytes >= 1 && out_bytes <= (1L << 40));
    MPN_CHECK_ARG(src_floats >= 1 && src_floats <= (1L << 40) && sY <= src_floats && sX <= src_floats &&
                  (int64_t)(Hs - 1) * sY + (int64_t)(Ws - 1) * sX < src_floats);
    MPN_CHECK_ARG(planes ? (plane_floats >= 1 && plane_floats <= (1L << 40)) : plane_floats == 0);
    MPN_CHECK_ARG((uintptr_t)imgs % 8 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)planes % 4 == 0);
    MPN_CHECK_ARG(disjoint(src, 4 * src_floats, out, out_bytes));
    MPN_CHECK_ARG(!planes || (disjoint(planes, 4 * plane_floats, out, out_bytes) && disjoint(planes, 4 * plane_floats, src, 4 * src_floats)));
    dim3 grid((unsigned)((max_w + SGI_TILE_W - 1) / SGI_TILE_W), (unsigned)((max_h + SGI_TILE_H - 1) / SGI_TILE_H), (unsigned)n_img);
    hipLaunchKernelGGL(seg_masks_kernel, grid, dim3(SGI_THREADS), 0, (hipStream_t)stream, src, (long)sY, (long)sX, Hs, Ws, (long)src_floats, imgs,
                       max_w, max_h, thr, out, (long)out_bytes, planes, (long)plane_floats);
    return mpn_launch_status();
}

extern "C" int mpn_tta_merge_mask(const MpnTtaScale* scales, int n_scales, int H, int W, float thr, float* plane, uint8_t* mask,
                                  int64_t mask_pitch, void* stream) {
    MPN_CHECK_ARG(scales && (plane || mask) && n_scales >= 1 && n_scales <= SGI_MAX_SCALES && H > 0 && W > 0 && H <= 65536 && W <= 65536);
    MPN_CHECK_ARG((long)H * W < 0x7fffffffL && (uintptr_t)plane % 4 == 0 && (!mask || mask_pitch >= W));
    MPN_CHECK_ARG(!plane || !mask || disjoint(plane, 4L * H * W, mask, (int64_t)(H - 1) * mask_pitch + W));
    SegTtaTable t;
    for (int s = 0; s < SGI_MAX_SCALES; ++s) { t.u[s] = nullptr; t.pitch[s] = 0; t.rh[s] = 0; t.rw[s] = 0; }
    t.n = n_scales;
    for (int s = 0; s < n_scales; ++s) {
        MPN_CHECK_ARG(scales[s].u && scales[s].rh > 0 && scales[s].rw > 0 && scales[s].pitch >= (int64_t)scales[s].rw * 2);
        MPN_CHECK_ARG((int64_t)scales[s].rw * 2 < 0x7fffffffL);
        t.u[s] = scales[s].u; t.pitch[s] = (long)scales[s].pitch; t.rh[s] = scales[s].rh; t.rw[s] = scales[s].rw;
    }
    const float inv_n = (float)(1.0 / (double)n_scales);
    dim3 grid((unsigned)((W + SGI_TILE_W - 1) / SGI_TILE_W), (unsigned)((H + SGI_TILE_H - 1) / SGI_TILE_H));
    hipLaunchKernelGGL(tta_merge_mask_kernel, grid, dim3(SGI_THREADS), 0, (hipStream_t)stream, t, H, W, inv_n, thr, plane, mask, (long)mask_pitch);
    return mpn_launch_status();
}

extern "C" int mpn_mask_iou(const uint8_t* pred, int64_t pred_bytes, const uint8_t* gt, int64_t gt_bytes, const int64_t* imgs, int n_img,
                            int max_h, int64_t* counts, void* stream) {
    MPN_CHECK_ARG(pred && gt && imgs && counts && n_img >= 1 && n_img <= 65535 && max_h >= 1 && max_h <= 65536);
    MPN_CHECK_ARG(pred_bytes >= 1 && pred_bytes <= (1L << 40) && gt_bytes >= 1 && gt_bytes <= (1L << 40));
    MPN_CHECK_ARG((uintptr_t)imgs % 8 == 0 && (uintptr_t)counts % 8 == 0);
    MPN_CHECK_ARG(disjoint(counts, 24L * n_img, pred, pred_bytes) && disjoint(counts, 24L * n_img, gt, gt_bytes));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)n_img * 3 * sizeof(int64_t), st) != hipSuccess) return mpn_launch_status();
    dim3 grid((unsigned)((max_h + MIOU_ROWS - 1) / MIOU_ROWS), (unsigned)n_img);
    hipLaunchKernelGGL(mask_iou_kernel, grid, dim3(SGI_THREADS), 0, st, pred, (long)pred_bytes, gt, (long)gt_bytes, imgs, max_h,
                       (unsigned long long*)counts);
    return mpn_launch_status();
}
