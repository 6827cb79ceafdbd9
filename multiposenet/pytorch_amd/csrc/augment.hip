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
#include "common.h"

namespace {

struct Geo {
    long off, pitch;                 // bytes
    int H, W;
    double scale, nw, nh, cw, ch, m00, m01, m02, m10, m11, m12, ox, oy;
    bool flip, ok;
};

// Table row -> registers.  `ok` guards the gather: a row whose source does not lie inside the packed buffer is never dereferenced
// (the element is written as NaN instead); the host wrapper never produces such a row.
__device__ __forceinline__ Geo load_geo(const double* __restrict__ row, bool mask, long src_bytes, int bytes_per_pixel) {
    Geo g;
    g.off = (long)row[mask ? MPN_AUG_MASK_OFF : MPN_AUG_IMG_OFF];
    g.pitch = (long)row[mask ? MPN_AUG_MASK_PITCH : MPN_AUG_IMG_PITCH];
    const double H = row[MPN_AUG_H], W = row[MPN_AUG_W];
    g.ok = H >= 1.0 && H <= 65536.0 && W >= 1.0 && W <= 65536.0;
    g.H = g.ok ? (int)H : 1;
    g.W = g.ok ? (int)W : 1;
    g.ok = g.ok && g.off >= 0 && g.pitch >= (long)g.W * bytes_per_pixel && g.off <= src_bytes &&
           g.pitch <= src_bytes && (long)(g.H - 1) * g.pitch + (long)g.W * bytes_per_pixel <= src_bytes - g.off;
    g.scale = row[MPN_AUG_SCALE];
    g.nw = row[MPN_AUG_NW]; g.nh = row[MPN_AUG_NH]; g.cw = row[MPN_AUG_CW]; g.ch = row[MPN_AUG_CH];
    g.m00 = row[MPN_AUG_MINV + 0]; g.m01 = row[MPN_AUG_MINV + 1]; g.m02 = row[MPN_AUG_MINV + 2];
    g.m10 = row[MPN_AUG_MINV + 3]; g.m11 = row[MPN_AUG_MINV + 4]; g.m12 = row[MPN_AUG_MINV + 5];
    g.ox = row[MPN_AUG_OX]; g.oy = row[MPN_AUG_OY];
    g.flip = row[MPN_AUG_FLIP] != 0.0;
    return g;
}

// OpenCV interpolateCubic (imgproc/resize.cpp), float32, A = -0.75
__device__ __forceinline__ void cubic_coeffs(float x, float* c) {
    const float A = -0.75f;
    c[0] = ((A * (x + 1.0f) - 5.0f * A) * (x + 1.0f) + 8.0f * A) * (x + 1.0f) - 4.0f * A;
    c[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    c[2] = ((A + 2.0f) * (1.0f - x) - (A + 3.0f)) * (1.0f - x) * (1.0f - x) + 1.0f;
    c[3] = 1.0f - c[0] - c[1] - c[2];
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
            float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* r = base + (long)t.y[k] * g.pitch;
                float row[3];
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const uint8_t* p = r + t.x[l] * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) row[c] = l == 0 ? (float)p[c] * t.wx[0] : row[c] + (float)p[c] * t.wx[l];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = k == 0 ? row[c] * t.wy[0] : acc[c] + row[c] * t.wy[k];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) bgr[c] = clamp255(acc[c]);
        }
    }
    // preprocessing.py:15-26: RGB plane c = (BGR[2 - c] / 255 - mean[c]) / std[c]
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = (bgr[2 - c] / 255.0f - nm.mean[c]) / nm.stdv[c];
}

__global__ void __launch_bounds__(256) augment_mask_kernel(const uint8_t* __restrict__ src, long src_bytes, const double* __restrict__ table,
                                                           float* __restrict__ out, int gh, int gw, double stride, double flip_w) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.z;
    if (c >= gh * gw) return;
    const int j = c % gw, i = c / gw;
    const Geo g = load_geo(table + (long)b * MPN_AUG_COLS, true, src_bytes, 1);
    float val = 255.0f;
    if (!g.ok) {
        val = __builtin_nanf("");
    } else {
        // source coordinate of cv2.resize(fx = 1 / stride) in the (crop + 1)-wide mask crop, which the reference flips over its own width
        const double px = ((double)j + 0.5) * stride - 0.5, py = ((double)i + 0.5) * stride - 0.5;
        const double pf = g.flip ? flip_w - px : px;
        const Taps t = map_point(g, g.ox + pf, g.oy + py);
        if (t.inside) {
            const uint8_t* base = src + g.off;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* r = base + (long)t.y[k] * g.pitch;
                float row = (float)r[t.x[0]] * t.wx[0];
#pragma unroll
                for (int l = 1; l < 4; ++l) row = row + (float)r[t.x[l]] * t.wx[l];
                acc = k == 0 ? row * t.wy[0] : acc + row * t.wy[k];
            }
            val = clamp255(acc);
        }
    }
    val = val / 255.0f;
    const long cells = (long)gh * gw;
    float* o = out + (long)b * 18 * cells + c;
#pragma unroll
    for (int k = 0; k < 18; ++k) o[k * cells] = val;
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

extern "C" int mpn_augment_mask(const uint8_t* src, int64_t src_bytes, const double* table, int B, float* out, int gh, int gw, int stride,
                                int crop_x, void* stream) {
    MPN_CHECK_ARG(src && table && out && src_bytes > 0 && B > 0 && B <= 65535 && gh > 0 && gw > 0 && stride > 0 && crop_x > 0);
    MPN_CHECK_ARG((long)gh * gw <= 0x7fffffffL);
    dim3 grid((unsigned)(((long)gh * gw + 255) / 256), 1u, (unsigned)B);
    // the mask crop is crop_x + 1 wide (ImageAugmentation.py:93): its flip maps x to (crop_x + 1) - 1 - x
    hipLaunchKernelGGL(augment_mask_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, (long)src_bytes, table, out, gh, gw,
                       (double)stride, (double)crop_x);
    return mpn_launch_status();
}
