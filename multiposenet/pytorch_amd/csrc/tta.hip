// tta.hip — the element-wise ends of the multi-scale + flip test-time augmentation (evaluate/tester.py: infer_image_multiscale_fused).
//
//   mpn_tta_input : decoded image -> the network input of ONE scale for the pair {original, mirrored}: crop_with_factor's bilinear
//                   fx/fy-form resize + pad to (hp, wp) with 128, then resnet_preprocess (BGR -> RGB, 1/255, mean, std, planar).
//   mpn_tta_merge : the x4-upsampled, cropped pair maps of every scale -> the final averaged [H, W, 18] maps: dsize-form bicubic
//                   resize to the image, division by the scale count, float64 sums per stream, mirror + channel swap of the
//                   flipped stream, halving, ONE rounding to float32 (_get_outputs twice, _handle_heat, .float()).
//
// Both restate the op sequence of the unfused path value for value: the bilinear and bicubic sums are resize_kernel's (peaks.hip)
// in the same left-to-right form; built with -ffp-contract=off like it.  A float32 tensor divided by a host scalar is a
// multiplication by the rounded reciprocal in the tensor library's device kernel (x / 255., maps / 5); a division of two
// tensors ((x - mean) / std) is a correctly rounded division.
#include "common.h"
#include "resize_taps.h"

namespace {

constexpr int TTA_THREADS = 256;
constexpr int TTA_CH = 18;                                       // heat-map channels of one pass; a pair map holds 2 * TTA_CH

// one thread per (image of the pair, y, x) of the padded input, lanes along x: the three planar stores of a wave are contiguous
__global__ void __launch_bounds__(TTA_THREADS) tta_input_kernel(const float* __restrict__ src, long sY, long sX, long sC, int Hs, int Ws,
                                                                 float* __restrict__ dst, int h, int w, int hp, int wp, double inv_f) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long plane = (long)hp * wp;
    if (i >= 2 * plane) return;
    const int n = (int)(i / plane);                              // 0: original, 1: mirrored (reads source column Ws - 1 - x')
    const int dy = (int)((i - (long)n * plane) / wp);
    const int dx = (int)(i % wp);
    float v[3] = {128.f, 128.f, 128.f};                          // pad value outside (h, w)
    if (dy < h && dx < w) {
        // resize_kernel's linear branch, fx / fy form: scale = 1 / f exactly, on both axes
        float fx = (float)(((double)dx + 0.5) * inv_f - 0.5), fy = (float)(((double)dy + 0.5) * inv_f - 0.5);
        int sx = (int)floorf(fx), sy = (int)floorf(fy);
        fx -= (float)sx; fy -= (float)sy;
        if (sx < 0) { fx = 0.f; sx = 0; }
        if (sx >= Ws - 1) { fx = 0.f; sx = Ws - 1; }
        if (sy < 0) { fy = 0.f; sy = 0; }
        if (sy >= Hs - 1) { fy = 0.f; sy = Hs - 1; }
        const int sx1 = sx + 1 < Ws ? sx + 1 : Ws - 1, sy1 = sy + 1 < Hs ? sy + 1 : Hs - 1;
        const long c0 = (long)(n ? Ws - 1 - sx : sx) * sX, c1 = (long)(n ? Ws - 1 - sx1 : sx1) * sX;
        const float* __restrict__ p0 = src + (long)sy * sY;
        const float* __restrict__ p1 = src + (long)sy1 * sY;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r0 = p0[c0 + c * sC] * (1.f - fx) + p0[c1 + c * sC] * fx;
            const float r1 = p1[c0 + c * sC] * (1.f - fx) + p1[c1 + c * sC] * fx;
            v[c] = r0 * (1.f - fy) + r1 * fy;
        }
    }
    const float inv255 = (float)(1.0 / 255.0);
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};      // RGB
    float* __restrict__ o = dst + (long)n * 3 * plane + (long)dy * wp + dx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int p = 2 - c;                                     // BGR source channel c is RGB plane 2 - c
        float t = v[c] * inv255;
        t = t - mean[p];
        o[(long)p * plane] = __fdiv_rn(t, stdv[p]);
    }
}

constexpr int TTA_MAX_SCALES = 8;
struct TtaTable {
    const float* u[TTA_MAX_SCALES];
    long pitch[TTA_MAX_SCALES];
    int rh[TTA_MAX_SCALES], rw[TTA_MAX_SCALES];
    int n;
};
struct TtaSwap { unsigned long long lo, hi; };                   // 18 five-bit entries: 0..8 in lo, 9..17 in hi

__device__ __forceinline__ float cubic_sample(const float* __restrict__ u, long pitch, int ch, const int (&yi)[4], const float (&yc)[4],
                                              const int (&xi)[4], const float (&xc)[4]) {
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* __restrict__ row = u + (long)yi[k] * pitch + ch;
        float a = row[xi[0] * (2 * TTA_CH)] * xc[0];
        a = a + row[xi[1] * (2 * TTA_CH)] * xc[1];
        a = a + row[xi[2] * (2 * TTA_CH)] * xc[2];
        a = a + row[xi[3] * (2 * TTA_CH)] * xc[3];
        r[k] = a;
    }
    float v = r[0] * yc[0];
    v = v + r[1] * yc[1];
    v = v + r[2] * yc[2];
    v = v + r[3] * yc[3];
    return v;
}

// one thread per output element, flat over [H][W][18]: the 18 channels of consecutive pixels are consecutive lanes, so the store and
// every tap load of the original stream cover consecutive addresses; the flipped stream reads the same 72-byte pixel groups in
// descending pixel order with the channels permuted inside a group.
__global__ void __launch_bounds__(TTA_THREADS) tta_merge_kernel(TtaTable t, TtaSwap sw, float* __restrict__ out, int H, int W, float inv_n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)H * W * TTA_CH) return;
    const int c = (int)(i % TTA_CH);
    const int x = (int)((i / TTA_CH) % W);
    const int y = (int)(i / ((long)TTA_CH * W));
    const int cf = TTA_CH + (int)((c < 9 ? sw.lo >> (5 * c) : sw.hi >> (5 * (c - 9))) & 31);
    const int xf = W - 1 - x;
    double a_o = 0.0, a_f = 0.0;
    for (int s = 0; s < t.n; ++s) {
        const float* __restrict__ u = t.u[s];
        const long pitch = t.pitch[s];
        const int rh = t.rh[s], rw = t.rw[s];
        const double scale_y = (double)rh / (double)H, scale_x = (double)rw / (double)W;      // dsize form
        int yi[4], xi[4], xfi[4]; float yc[4], xc[4], xfc[4];
        cubic_taps(y, scale_y, rh, yi, yc);
        cubic_taps(x, scale_x, rw, xi, xc);
        cubic_taps(xf, scale_x, rw, xfi, xfc);
        a_o = a_o + (double)(cubic_sample(u, pitch, c, yi, yc, xi, xc) * inv_n);
        a_f = a_f + (double)(cubic_sample(u, pitch, cf, yi, yc, xfi, xfc) * inv_n);
    }
    out[i] = (float)((a_o + a_f) * 0.5);                         // / 2. in float64: exact either way
}

}  // namespace

extern "C" int mpn_tta_input(const float* img, int64_t sY, int64_t sX, int64_t sC, int H, int W, float* out, int h, int w, int hp, int wp,
                             double inv_scale, void* stream) {
    MPN_CHECK_ARG(img && out && H > 0 && W > 0 && h > 0 && w > 0 && h <= hp && w <= wp && inv_scale > 0.0);
    const long n = 2L * hp * wp;
    MPN_CHECK_ARG(3 * n < 0x7fffffffL);
    hipLaunchKernelGGL(tta_input_kernel, dim3((unsigned)((n + TTA_THREADS - 1) / TTA_THREADS)), dim3(TTA_THREADS), 0, (hipStream_t)stream, img,
                       (long)sY, (long)sX, (long)sC, H, W, out, h, w, hp, wp, inv_scale);
    return mpn_launch_status();
}

extern "C" int mpn_tta_merge(const MpnTtaScale* scales, int n_scales, const int32_t* swap, float* out, int H, int W, void* stream) {
    MPN_CHECK_ARG(scales && swap && out && n_scales >= 1 && n_scales <= TTA_MAX_SCALES && H > 0 && W > 0);
    MPN_CHECK_ARG((long)H * W * TTA_CH < 0x7fffffffL);
    TtaTable t;
    for (int s = 0; s < TTA_MAX_SCALES; ++s) { t.u[s] = nullptr; t.pitch[s] = 0; t.rh[s] = 0; t.rw[s] = 0; }
    t.n = n_scales;
    for (int s = 0; s < n_scales; ++s) {
        MPN_CHECK_ARG(scales[s].u && scales[s].rh > 0 && scales[s].rw > 0 && scales[s].pitch >= (int64_t)scales[s].rw * 2 * TTA_CH);
        MPN_CHECK_ARG((int64_t)scales[s].rw * 2 * TTA_CH < 0x7fffffffL);
        t.u[s] = scales[s].u; t.pitch[s] = (long)scales[s].pitch; t.rh[s] = scales[s].rh; t.rw[s] = scales[s].rw;
    }
    TtaSwap sw = {0ull, 0ull};
    unsigned seen = 0;
    for (int c = 0; c < TTA_CH; ++c) {
        MPN_CHECK_ARG(swap[c] >= 0 && swap[c] < TTA_CH && !(seen & (1u << swap[c])));          // a permutation of 0..17
        seen |= 1u << swap[c];
        if (c < 9) sw.lo |= (unsigned long long)swap[c] << (5 * c);
        else sw.hi |= (unsigned long long)swap[c] << (5 * (c - 9));
    }
    const long n = (long)H * W * TTA_CH;
    const float inv_n = (float)(1.0 / (double)n_scales);
    hipLaunchKernelGGL(tta_merge_kernel, dim3((unsigned)((n + TTA_THREADS - 1) / TTA_THREADS)), dim3(TTA_THREADS), 0, (hipStream_t)stream, t, sw,
                       out, H, W, inv_n);
    return mpn_launch_status();
}
