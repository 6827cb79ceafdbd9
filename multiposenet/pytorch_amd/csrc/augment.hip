// augment.hip — training augmentation of a batch on the device, from raw uint8 sources (datasets/augment.py).
//
// Replaces the pixel side of datasets/coco_data/ImageAugmentation.py:25-231 (aug_scale, aug_rotate, aug_croppad, aug_flip), the
// mask's second resize of COCO_data_pipeline.py:211-215 and preprocessing.py:15-26.  ONE pass: every output element is mapped
// through the composed inverse transform (flip -> crop origin on the rotated canvas -> inverse of the warpAffine matrix -> inverse of
// the resize) to a source coordinate and sampled once with the 4x4 cubic kernel (A = -0.75, OpenCV's interpolateCubic), the taps
// clamped to the source (replicate).  No intermediate image exists and nothing is rounded to uint8.
//
// Arithmetic split: every coordinate up to and including floor and fraction is float64 in a fixed operation order (this file is
// built with -ffp-contract=off), so a float64 restatement takes identical inside/outside decisions and identical taps; the cubic
// weights and the 16-term sum are float32.
//
// One launch covers the batch: blockIdx.z is the image, so every read of the per-sample table (MPN_AUG_* columns, doubles) is
// wave-uniform.  Traffic: sources of <= ~1 MB each gathered through L2; 12 bytes per image pixel / 72 bytes per mask cell out.
//
// mpn_augment_boxes (detection batches) samples the same way from packed instance-mask rectangles, but writes no pixel: a scan
// launch reduces the extents of the ON pixels to one int32 record per (instance, tile), a finalize launch folds them into the
// [B][N][5] box tensor.  Both reductions are min / max over integers in a fixed order: no atomics, the same bytes every time.
#include "common.h"

namespace {

struct Geo {
    long off, pitch;                 // bytes
    int H, W;
    double scale, nw, nh, cw, ch, m00, m01, m02, m10, m11, m12, ox, oy;
    bool flip, ok;
};
struct Rect { int x0, y0, w, h; };   // an instance's bounding rectangle inside its H x W source

// Table row -> registers.  `ok` guards the gather: a row whose source does not lie inside the packed buffer is never dereferenced
// (the element is written as NaN instead); the host wrapper never produces such a row.  What lies at the offset is the whole H x W
// source, or, for an instance row of mpn_augment_boxes (`rect` given: a sample row whose MASK_OFF / MASK_PITCH address the packed
// rectangle, plus the MPN_AUGB_* columns), the rectangle, which must itself lie inside the source.
__device__ __forceinline__ Geo load_geo(const double* __restrict__ row, bool mask, long src_bytes, int bytes_per_pixel, Rect* rect = nullptr) {
    Geo g;
    g.off = (long)row[mask ? MPN_AUG_MASK_OFF : MPN_AUG_IMG_OFF];
    g.pitch = (long)row[mask ? MPN_AUG_MASK_PITCH : MPN_AUG_IMG_PITCH];
    const double H = row[MPN_AUG_H], W = row[MPN_AUG_W];
    g.ok = H >= 1.0 && H <= 65536.0 && W >= 1.0 && W <= 65536.0;
    g.H = g.ok ? (int)H : 1;
    g.W = g.ok ? (int)W : 1;
    int rows = g.H, cols = g.W;
    if (rect) {
        const double x0 = row[MPN_AUGB_RX0], y0 = row[MPN_AUGB_RY0], w = row[MPN_AUGB_RW], h = row[MPN_AUGB_RH];
        g.ok = g.ok && x0 >= 0.0 && y0 >= 0.0 && w >= 1.0 && h >= 1.0 && x0 + w <= W && y0 + h <= H;
        rect->x0 = g.ok ? (int)x0 : 0; rect->y0 = g.ok ? (int)y0 : 0;
        rect->w = cols = g.ok ? (int)w : 1; rect->h = rows = g.ok ? (int)h : 1;
    }
    // the buffer guard: `rows` rows of `row_bytes` bytes, `pitch` bytes apart from byte `off`, lie inside the `src_bytes` of the buffer
    const long row_bytes = (long)cols * bytes_per_pixel;
    g.ok = g.ok && g.off >= 0 && g.pitch >= row_bytes && g.off <= src_bytes && g.pitch <= src_bytes &&
           (long)(rows - 1) * g.pitch + row_bytes <= src_bytes - g.off;
    g.scale = row[MPN_AUG_SCALE];
    g.nw = row[MPN_AUG_NW]; g.nh = row[MPN_AUG_NH]; g.cw = row[MPN_AUG_CW]; g.ch = row[MPN_AUG_CH];
    g.m00 = row[MPN_AUG_MINV + 0]; g.m01 = row[MPN_AUG_MINV + 1]; g.m02 = row[MPN_AUG_MINV + 2];
    g.m10 = row[MPN_AUG_MINV + 3]; g.m11 = row[MPN_AUG_MINV + 4]; g.m12 = row[MPN_AUG_MINV + 5];
    g.ox = row[MPN_AUG_OX]; g.oy = row[MPN_AUG_OY];
    g.flip = row[MPN_AUG_FLIP] != 0.0;
    return g;
}

struct Taps {
    bool inside;
    int x[4], y[4];
    float wx[4], wy[4];
};

// canvas point (xr, yr) [the crop point already un-flipped and moved by the crop origin] -> taps and weights in the source.
// The canvas pixel k covers [k - 0.5, k + 0.5): for the integer points of the image this is the reference's 0 <= k < n.
__device__ __forceinline__ Taps map_point(const Geo& g, double xr, double yr) {
    Taps t;
    t.inside = false;
    if (!(xr >= -0.5 && xr < g.cw - 0.5 && yr >= -0.5 && yr < g.ch - 0.5)) return t;
    const double xs = (g.m00 * xr + g.m01 * yr) + g.m02;
    const double ys = (g.m10 * xr + g.m11 * yr) + g.m12;
    if (!(xs >= -0.5 && xs < g.nw - 0.5 && ys >= -0.5 && ys < g.nh - 0.5)) return t;
    const double sx = (xs + 0.5) / g.scale - 0.5;
    const double sy = (ys + 0.5) / g.scale - 0.5;
    const double fx = floor(sx), fy = floor(sy);
    cubic_coeffs((float)(sx - fx), t.wx);
    cubic_coeffs((float)(sy - fy), t.wy);
    // every tap is clamped to the source below, so limiting the base index first changes nothing and keeps the int conversion in range
    const int ix = (int)fmin(fmax(fx, -4.0), (double)g.W + 4.0);
    const int iy = (int)fmin(fmax(fy, -4.0), (double)g.H + 4.0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t.x[k] = min(max(ix - 1 + k, 0), g.W - 1);
        t.y[k] = min(max(iy - 1 + k, 0), g.H - 1);
    }
    t.inside = true;
    return t;
}

// The 16-term float32 sum of C channels: fetch(k, l, p) supplies the tap of row t.y[k], column t.x[l].  Fixed operation order:
// row = p * wx[0]; row += p * wx[l]; acc = row * wy[0]; acc += row * wy[k].
template <int C, typename Fetch>
__device__ __forceinline__ void cubic_sum(const Taps& t, Fetch fetch, float (&acc)[C]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float row[C];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            float p[C];
            fetch(k, l, p);
#pragma unroll
            for (int c = 0; c < C; ++c) row[c] = l == 0 ? p[c] * t.wx[0] : row[c] + p[c] * t.wx[l];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = k == 0 ? row[c] * t.wy[0] : acc[c] + row[c] * t.wy[k];
    }
}

__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.0f), 255.0f); }

struct Norm { float mean[3], stdv[3]; };

__global__ void __launch_bounds__(256) augment_image_kernel(const uint8_t* __restrict__ src, long src_bytes, const double* __restrict__ table,
                                                            float* __restrict__ out, int crop_y, int crop_x, Norm nm) {
    // block = 64 x 4 output pixels of image blockIdx.z; a wave is 64 consecutive pixels of one output row
    const int u = blockIdx.x * 64 + threadIdx.x, v = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (u >= crop_x || v >= crop_y) return;
    const Geo g = load_geo(table + (long)b * MPN_AUG_COLS, false, src_bytes, 3);
    const long plane = (long)crop_y * crop_x;
    float* o = out + (long)b * 3 * plane + (long)v * crop_x + u;
    float bgr[3] = {128.0f, 128.0f, 128.0f};
    if (!g.ok) {
        bgr[0] = bgr[1] = bgr[2] = __builtin_nanf("");
    } else {
        const int up = g.flip ? crop_x - 1 - u : u;
        const Taps t = map_point(g, g.ox + (double)up, g.oy + (double)v);
        if (t.inside) {
            const uint8_t* base = src + g.off;
            float acc[3];
            cubic_sum(t, [&](int k, int l, float (&p)[3]) {
                const uint8_t* q = base + (long)t.y[k] * g.pitch + t.x[l] * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = (float)q[c];
            }, acc);
#pragma unroll
            for (int c = 0; c < 3; ++c) bgr[c] = clamp255(acc[c]);
        }
    }
    // preprocessing.py:15-26: RGB plane c = (BGR[2 - c] / 255 - mean[c]) / std[c]
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = (bgr[2 - c] / 255.0f - nm.mean[c]) / nm.stdv[c];
}

// CH output channels, all holding the one sample: 18 for mask_miss (mpn_augment_mask, outside = 255), 1 for any other plane
// (mpn_augment_plane, the outside value of the caller's).
template <int CH>
__global__ void __launch_bounds__(256) augment_mask_kernel(const uint8_t* __restrict__ src, long src_bytes, const double* __restrict__ table,
                                                           float* __restrict__ out, int gh, int gw, double stride, double flip_w,
                                                           float outside) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.z;
    if (c >= gh * gw) return;
    const int j = c % gw, i = c / gw;
    const Geo g = load_geo(table + (long)b * MPN_AUG_COLS, true, src_bytes, 1);
    float val = outside;
    if (!g.ok) {
        val = __builtin_nanf("");
    } else {
        // source coordinate of cv2.resize(fx = 1 / stride) in the (crop + 1)-wide mask crop, which the reference flips over its own width
        const double px = ((double)j + 0.5) * stride - 0.5, py = ((double)i + 0.5) * stride - 0.5;
        const double pf = g.flip ? flip_w - px : px;
        const Taps t = map_point(g, g.ox + pf, g.oy + py);
        if (t.inside) {
            const uint8_t* base = src + g.off;
            float acc[1];
            cubic_sum(t, [&](int k, int l, float (&p)[1]) { p[0] = (float)base[(long)t.y[k] * g.pitch + t.x[l]]; }, acc);
            val = clamp255(acc[0]);
        }
    }
    val = val / 255.0f;
    const long cells = (long)gh * gw;
    float* o = out + (long)b * CH * cells + c;
#pragma unroll
    for (int k = 0; k < CH; ++k) o[k * cells] = val;
}

// ---- boxes of instance masks (mpn_augment_boxes) -------------------------------------------------------------------------------
// The reference warps every instance mask through the chain and reads its box off the final (crop + 1)^2 mask with np.any
// (COCO_data_pipeline.py:382-405).  Here no warped mask exists: every pixel of that frame is sampled once from the instance's own
// bounding rectangle of the binary source mask, thresholded at 0.5, and only the extents of the ON pixels leave the workgroup.
constexpr int BOX_ROWS = 4;                   // rows per lane: a workgroup of 64 x 4 lanes covers a 64 x 16 tile
constexpr int BOX_TILE_Y = 4 * BOX_ROWS;
constexpr int BOX_REC = 5;                    // int32 per partial record: min x, max x, min y, max y, flag (0 none, 1 any, -1 bad row)
constexpr int BOX_EMPTY_MIN = 0x7fffffff;

template <typename Op>
__device__ __forceinline__ int wave_reduce(int v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int imin(int a, int b) { return min(a, b); }
__device__ __forceinline__ int imax(int a, int b) { return max(a, b); }

// extents of a set of ON pixels; x_hi < 0 = empty.  Every fold is integer min / max in a fixed order.
struct Extent {
    int x_lo, x_hi, y_lo, y_hi;
    __device__ static Extent none() { return {BOX_EMPTY_MIN, -1, BOX_EMPTY_MIN, -1}; }
    __device__ void merge(const Extent& e) {
        x_lo = min(x_lo, e.x_lo); x_hi = max(x_hi, e.x_hi); y_lo = min(y_lo, e.y_lo); y_hi = max(y_hi, e.y_hi);
    }
    __device__ void add(int u, int v) { merge({u, u, v, v}); }
    __device__ void wave_fold() {
        x_lo = wave_reduce(x_lo, imin); x_hi = wave_reduce(x_hi, imax); y_lo = wave_reduce(y_lo, imin); y_hi = wave_reduce(y_hi, imax);
    }
};

__global__ void __launch_bounds__(256) augment_box_scan_kernel(const uint8_t* __restrict__ src, long src_bytes, const double* __restrict__ table,
                                                               int32_t* __restrict__ partial, int crop_y, int crop_x) {
    // block = 64 x 16 pixels of the (crop_y + 1) x (crop_x + 1) mask frame of instance blockIdx.z; a wave is 64 consecutive pixels
    // of one row and walks BOX_ROWS rows.  Lanes past the frame stay OFF: no early return, every lane takes part in the reduction.
    __shared__ Extent red[4];
    const int u = blockIdx.x * 64 + threadIdx.x, inst = blockIdx.z;
    Rect rc;
    const Geo g = load_geo(table + (long)inst * MPN_AUGB_COLS, true, src_bytes, 1, &rc);
    Extent e = Extent::none();
    if (g.ok && u <= crop_x) {
        const uint8_t* base = src + g.off;
        const int up = g.flip ? crop_x - u : u;                       // the mask is flipped over its OWN width, crop_x + 1
#pragma unroll 1
        for (int j = 0; j < BOX_ROWS; ++j) {
            const int v = blockIdx.y * BOX_TILE_Y + j * 4 + threadIdx.y;
            if (v > crop_y) break;
            const Taps t = map_point(g, g.ox + (double)up, g.oy + (double)v);
            if (!t.inside) continue;                                  // border 0, pad 0
            // a tap outside the rectangle reads 0 (the mask is 0 there) and is not dereferenced.  cubic_sum's order, written out: as a
            // per-tap fetch the rectangle test forms the row address per tap and measures 6 % slower (profiles/augment_one_sampler_ab.txt)
            int cx[4];
            bool inx[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                cx[l] = t.x[l] - rc.x0;
                inx[l] = cx[l] >= 0 && cx[l] < rc.w;
            }
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cy = t.y[k] - rc.y0;
                const bool iny = cy >= 0 && cy < rc.h;
                const uint8_t* r = base + (long)(iny ? cy : 0) * g.pitch;
                float p[4];
#pragma unroll
                for (int l = 0; l < 4; ++l) p[l] = (iny && inx[l] && r[cx[l]] != 0) ? 1.0f : 0.0f;
                float row = p[0] * t.wx[0];
#pragma unroll
                for (int l = 1; l < 4; ++l) row = row + p[l] * t.wx[l];
                acc = k == 0 ? row * t.wy[0] : acc + row * t.wy[k];
            }
            if (acc >= 0.5f) e.add(u, v);
        }
    }
    // stage 1: in the wave; stage 2: the four waves through LDS; one record per (instance, tile), ordinary stores
    e.wave_fold();
    if (threadIdx.x == 0) red[threadIdx.y] = e;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) e.merge(red[w]);
        const long tiles = (long)gridDim.x * gridDim.y;
        int32_t* o = partial + ((long)inst * tiles + (long)blockIdx.y * gridDim.x + blockIdx.x) * BOX_REC;
        o[0] = e.x_lo; o[1] = e.x_hi; o[2] = e.y_lo; o[3] = e.y_hi;
        o[4] = !g.ok ? -1 : (e.x_hi >= 0 ? 1 : 0);
    }
}

// one wave per output row (b, r) of the [B][N][5] box tensor: folds the tiles of its instance (row_inst, -1 = padding row)
__global__ void __launch_bounds__(64) augment_box_finalize_kernel(const int32_t* __restrict__ partial, const int32_t* __restrict__ row_inst,
                                                                  float* __restrict__ out, int n_inst, int tiles) {
    const int row = blockIdx.x, inst = row_inst[row];
    float* o = out + (long)row * 5;
    if (inst < 0 || inst >= n_inst) {
        // bbox_collater pads with -1; a map entry that names no instance cannot come from the host wrapper: NaN
        if (threadIdx.x < 5) o[threadIdx.x] = inst < 0 ? -1.0f : __builtin_nanf("");
        return;
    }
    Extent e = Extent::none();
    int bad = 0;
    const int32_t* p = partial + (long)inst * tiles * BOX_REC;
    for (int t = threadIdx.x; t < tiles; t += 64) {
        const int32_t* q = p + (long)t * BOX_REC;
        if (q[4] > 0) e.merge({q[0], q[1], q[2], q[3]});
        bad = max(bad, q[4] < 0 ? 1 : 0);
    }
    e.wave_fold();
    bad = wave_reduce(bad, imax);
    if (threadIdx.x == 0) {
        if (bad) {
            for (int k = 0; k < 5; ++k) o[k] = __builtin_nanf("");
        } else if (e.x_hi >= 0) {
            // COCO_data_pipeline.py:393-398: x2 and y2 are not part of the box, class 0
            o[0] = (float)e.x_lo; o[1] = (float)e.y_lo; o[2] = (float)(e.x_hi + 1); o[3] = (float)(e.y_hi + 1); o[4] = 0.0f;
        } else {
            for (int k = 0; k < 5; ++k) o[k] = -1.0f;                 // :399-402: warped out of the crop
        }
    }
}

}  // namespace

extern "C" int mpn_augment_image(const uint8_t* src, int64_t src_bytes, const double* table, int B, float* out, int crop_y, int crop_x,
                                 const float* mean_std, void* stream) {
    MPN_CHECK_ARG(src && table && out && mean_std && src_bytes > 0 && B > 0 && B <= 65535 && crop_y > 0 && crop_x > 0);
    MPN_CHECK_ARG(crop_y <= 65535 * 4);
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean_std[c];
        nm.stdv[c] = mean_std[3 + c];
        MPN_CHECK_ARG(nm.stdv[c] > 0.0f);
    }
    dim3 grid((unsigned)((crop_x + 63) / 64), (unsigned)((crop_y + 3) / 4), (unsigned)B);
    hipLaunchKernelGGL(augment_image_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, src, (long)src_bytes, table, out, crop_y, crop_x, nm);
    return mpn_launch_status();
}

template <int CH>
static int launch_augment_mask(const uint8_t* src, int64_t src_bytes, const double* table, int B, float* out, int gh, int gw, int stride,
                               int crop_x, float outside, void* stream) {
    MPN_CHECK_ARG(src && table && out && src_bytes > 0 && B > 0 && B <= 65535 && gh > 0 && gw > 0 && stride > 0 && crop_x > 0);
    MPN_CHECK_ARG((long)gh * gw <= 0x7fffffffL);
    dim3 grid((unsigned)(((long)gh * gw + 255) / 256), 1u, (unsigned)B);
    // the mask crop is crop_x + 1 wide (ImageAugmentation.py:93): its flip maps x to (crop_x + 1) - 1 - x
    hipLaunchKernelGGL(augment_mask_kernel<CH>, grid, dim3(256), 0, (hipStream_t)stream, src, (long)src_bytes, table, out, gh, gw,
                       (double)stride, (double)crop_x, outside);
    return mpn_launch_status();
}

extern "C" int mpn_augment_mask(const uint8_t* src, int64_t src_bytes, const double* table, int B, float* out, int gh, int gw, int stride,
                                int crop_x, void* stream) {
    return launch_augment_mask<18>(src, src_bytes, table, B, out, gh, gw, stride, crop_x, 255.0f, stream);
}

extern "C" int mpn_augment_plane(const uint8_t* src, int64_t src_bytes, const double* table, int B, float* out, int gh, int gw, int stride,
                                 int crop_x, float outside, void* stream) {
    MPN_CHECK_ARG(outside >= 0.0f && outside <= 255.0f);                  // also refuses NaN
    MPN_CHECK_ARG((uintptr_t)table % 8 == 0 && (uintptr_t)out % 4 == 0);
    return launch_augment_mask<1>(src, src_bytes, table, B, out, gh, gw, stride, crop_x, outside, stream);
}

// 64 x BOX_TILE_Y tiles over the (crop_y + 1) x (crop_x + 1) mask frame: the scan's grid, one partial record per tile
static inline dim3 box_grid(int crop_y, int crop_x, int n_inst) {
    return dim3((unsigned)((crop_x + 1 + 63) / 64), (unsigned)((crop_y + 1 + BOX_TILE_Y - 1) / BOX_TILE_Y), (unsigned)n_inst);
}

extern "C" int64_t mpn_augment_boxes_workspace_bytes(int n_inst, int crop_y, int crop_x) {
    if (n_inst < 0 || n_inst > 65535 || crop_y <= 0 || crop_x <= 0 || crop_y > 65535 || crop_x > 65535) return 0;
    const dim3 grid = box_grid(crop_y, crop_x, n_inst);
    return (int64_t)grid.z * grid.x * grid.y * BOX_REC * (int64_t)sizeof(int32_t);
}

extern "C" int mpn_augment_boxes(const uint8_t* src, int64_t src_bytes, const double* table, int n_inst, const int32_t* row_inst, int n_rows,
                                 float* out, int crop_y, int crop_x, void* workspace, void* stream) {
    MPN_CHECK_ARG(n_inst >= 0 && n_inst <= 65535 && n_rows >= 0 && crop_y > 0 && crop_x > 0 && crop_y <= 65535 && crop_x <= 65535);
    MPN_CHECK_ARG(n_inst == 0 || (src && table && workspace && src_bytes > 0));
    MPN_CHECK_ARG(n_rows == 0 || (row_inst && out));
    const dim3 grid = box_grid(crop_y, crop_x, n_inst);
    const long tiles = (long)grid.x * grid.y;
    MPN_CHECK_ARG(tiles <= 0x7fffffffL / BOX_REC);
    if (n_inst > 0) {
        hipLaunchKernelGGL(augment_box_scan_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, src, (long)src_bytes, table,
                           (int32_t*)workspace, crop_y, crop_x);
    }
    if (n_rows > 0)
        hipLaunchKernelGGL(augment_box_finalize_kernel, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream,
                           (const int32_t*)workspace, row_inst, out, n_inst, (int)tiles);
    return (n_inst > 0 || n_rows > 0) ? mpn_launch_status() : 0;
}
