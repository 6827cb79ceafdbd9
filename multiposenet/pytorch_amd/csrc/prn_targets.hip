// prn_targets.hip — PRN training pairs on the device, from raw COCO annotations (datasets/prn_data.py).
//
// Replaces PRN_CocoDataset.get_data (datasets/coco_data/prn_data_pipeline.py:33-111): per sample a Python triple loop over
// people x joints, 17 skimage gaussians (sigma 1, 'nearest') and one multichannel gaussian (sigma 2, 'constant') on the host.
// Here ONE launch renders a batch: a workgroup per (output channel, sample, tensor) sets the one-hot cells of its joint plane with
// the reference's float64 cell arithmetic (int() truncation, the one-branch clamp chain, Python's negative-index wrap, the label's
// try/except), blurs it separably (axis 0, then axis 1) in scipy.ndimage.correlate1d's symmetric-kernel summation order and
// writes the float32 [B][H][W][17] tensors that prn_forward and the BCE kernel consume; channel c holds COCO joint our_order[c]
// (:108-110).  Compiled with -ffp-contract=off: the float64 result equals the numpy / scipy arithmetic bit for bit and is rounded
// to float32 once.
//
// Cells only ever become 1 and carry no id, so the lanes scatter in parallel (equal byte stores to one LDS cell are benign).
// LDS: the one-hot plane as bytes plus ONE float64 plane for the first-pass result: 4 536 + 36 288 bytes at coeff 3.
//
// Samples for which the reference raises leave BOTH maps zero in every channel and set err[b] (MPN_PRN_ERR_*), so every
// workgroup of a sample scans all of that sample's keypoints for the raising cases before it renders its own plane.
#include "common.h"

namespace {

constexpr int kMaxCells = 84 * 54;       // coeff 3
constexpr int kThreads = 256;

__constant__ int kOurOrder[17] = {0, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3};

// The chain of prn_data_pipeline.py:56-72 (label) / :90-103 (input) for the truncated cell coordinates, kept as doubles until they
// are known to be in range.  Returns the cell y * W + x, or -1 where the reference raises IndexError.
template <bool LABEL>
__device__ __forceinline__ int chain_cell(double x0, double y0, int H, int W) {
    const double dW = (double)W, dH = (double)H;
    if (x0 >= dW && y0 >= dH) return (H - 1) * W + (W - 1);
    if (x0 >= dW) {                                      // output[y0, W - 1]: y0 < H; a negative y0 wraps once
        if (y0 < -dH) return -1;
        int y = (int)y0;
        if (y < 0) y += H;
        return y * W + (W - 1);
    }
    if (y0 >= dH) {                                      // output[H - 1, x0]: x0 < W
        if (x0 < -dW) return LABEL ? (H - 1) * W : -1;   // the label's try/except (:61-64); the input has none
        int x = (int)x0;
        if (x < 0) x += W;
        return (H - 1) * W + x;
    }
    if (x0 < 0.0 && y0 < 0.0) return 0;
    if (x0 < 0.0) return (int)y0 * W;
    if (y0 < 0.0) return (int)x0;
    return (int)y0 * W + (int)x0;
}

// One separable gaussian of the byte plane `hot` through the float64 plane `mid`, written as channel c of out[b].
// CONSTANT: taps beyond the border read 0 ('constant', cval 0); otherwise the border cell ('nearest').
template <int R, bool CONSTANT>
__device__ __forceinline__ void blur_plane(const unsigned char* hot, double* mid, const double* __restrict__ taps, int H, int W,
                                           float* __restrict__ out) {
    const int n = H * W;
    double w[2 * R + 1];
#pragma unroll
    for (int k = 0; k < 2 * R + 1; ++k) w[k] = taps[k];
    // axis 0 (rows); scipy's symmetric-kernel order: centre, then pairs from the far tap inwards
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int y = i / W, x = i - y * W;
        double tmp = (double)hot[i] * w[R];
#pragma unroll
        for (int jj = -R; jj < 0; ++jj) {
            const int ya = y + jj, yb = y - jj;
            double a, b;
            if (CONSTANT) {
                a = ya < 0 ? 0.0 : (double)hot[ya * W + x];
                b = yb >= H ? 0.0 : (double)hot[yb * W + x];
            } else {
                a = (double)hot[(ya < 0 ? 0 : ya) * W + x];
                b = (double)hot[(yb >= H ? H - 1 : yb) * W + x];
            }
            tmp += (a + b) * w[R + jj];
        }
        mid[i] = tmp;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int y = i / W, x = i - y * W;
        double tmp = mid[i] * w[R];
#pragma unroll
        for (int jj = -R; jj < 0; ++jj) {
            const int xa = x + jj, xb = x - jj;
            double a, b;
            if (CONSTANT) {
                a = xa < 0 ? 0.0 : mid[y * W + xa];
                b = xb >= W ? 0.0 : mid[y * W + xb];
            } else {
                a = mid[y * W + (xa < 0 ? 0 : xa)];
                b = mid[y * W + (xb >= W ? W - 1 : xb)];
            }
            tmp += (a + b) * w[R + jj];
        }
        out[(long)i * 17] = (float)tmp;
    }
}

__global__ void __launch_bounds__(kThreads) prn_train_maps_kernel(const double* __restrict__ box,         // [B][4] raw x, y, w, h
                                                                  const double* __restrict__ own_kp,      // [B][17][3]
                                                                  const double* __restrict__ img_kp,      // [P][17][3]
                                                                  const int* __restrict__ person_off,     // [B + 1] into img_kp
                                                                  int P, int H, int W, double threshold,
                                                                  const double* __restrict__ taps9, const double* __restrict__ taps17,
                                                                  float* __restrict__ input, float* __restrict__ label,   // [B][H][W][17]
                                                                  int* __restrict__ err) {                                // [B]
    __shared__ unsigned char hot[kMaxCells];
    __shared__ double mid[kMaxCells];
    __shared__ int err_s;
    const int c = blockIdx.x, b = blockIdx.y;
    const bool is_label = blockIdx.z == 1;
    const int j = kOurOrder[c];
    const int n = H * W;
    for (int i = threadIdx.x; i < n; i += kThreads) hot[i] = 0;
    if (threadIdx.x == 0) err_s = 0;
    __syncthreads();

    const double b0 = box[b * 4 + 0], b1 = box[b * 4 + 1], b2 = box[b * 4 + 2], b3 = box[b * 4 + 3];
    int code = 0;                                                       // wave-uniform: the box-level cases
    if (!(isfinite(b0) && isfinite(b1) && isfinite(b2) && isfinite(b3))) code = MPN_PRN_ERR_NONFINITE;      // int() / math.ceil raise
    else if (ceil(b2) == 0.0 || ceil(b3) == 0.0) code = MPN_PRN_ERR_ZERODIV;                                // :43-44
    if (code == 0) {
        const double x = trunc(b0), y = trunc(b1);                                                          // int(bbox[0]), int(bbox[1])
        const double x_scale = (double)W / ceil(b2), y_scale = (double)H / ceil(b3);
        const double one_t = 1.0 + threshold;                                                               // formed first (:85-86)
        const double lo_x = b0 - b2 * threshold, hi_x = b0 + b2 * one_t;
        const double lo_y = b1 - b3 * threshold, hi_y = b1 + b3 * one_t;
        int p0 = person_off[b], p1 = person_off[b + 1];
        p0 = p0 < 0 ? 0 : (p0 > P ? P : p0);                                                                // never index outside img_kp
        p1 = p1 < p0 ? p0 : (p1 > P ? P : p1);
        const int total = 17 + (p1 - p0) * 17;
        int mine = 0;
        for (int e = threadIdx.x; e < total; e += kThreads) {
            const bool own = e < 17;
            const double* kp = own ? own_kp + ((long)b * 17 + e) * 3 : img_kp + ((long)p0 * 17 + (e - 17)) * 3;
            const int jt = own ? e : (e - 17) % 17;
            const double kx = kp[0], ky = kp[1], kv = kp[2];
            if (!(kv > 0.0)) continue;
            if (!own && !(kx > lo_x && kx < hi_x && ky > lo_y && ky < hi_y)) continue;                      // raw float bbox (:85-86)
            const double fx = (kx - x) * x_scale, fy = (ky - y) * y_scale;
            if (!(isfinite(fx) && isfinite(fy))) { mine |= MPN_PRN_ERR_NONFINITE; continue; }               // int(nan) / int(inf) raise
            const double x0 = trunc(fx), y0 = trunc(fy);
            const int cell = own ? chain_cell<true>(x0, y0, H, W) : chain_cell<false>(x0, y0, H, W);
            if (cell < 0) { mine |= MPN_PRN_ERR_INDEX; continue; }
            if (jt == j && own == is_label) hot[cell] = 1;
        }
        if (mine) atomicOr(&err_s, mine);
    }
    __syncthreads();
    if (code == 0) code = err_s;
    if (c == 0 && !is_label && threadIdx.x == 0) err[b] = code;
    float* out = (is_label ? label : input) + (long)b * n * 17 + c;
    if (code != 0) {
        for (int i = threadIdx.x; i < n; i += kThreads) out[(long)i * 17] = 0.0f;
        return;
    }
    if (is_label) blur_plane<8, true>(hot, mid, taps17, H, W, out);
    else blur_plane<4, false>(hot, mid, taps9, H, W, out);
}

}  // namespace

extern "C" int mpn_prn_train_maps(const double* box, const double* own_kp, const double* img_kp, const int32_t* person_off, int B, int P,
                                  int coeff, double threshold, const double* taps9, const double* taps17, float* input, float* label,
                                  int32_t* err, void* stream) {
    MPN_CHECK_ARG(box && own_kp && img_kp && person_off && taps9 && taps17 && input && label && err);
    MPN_CHECK_ARG(B > 0 && B <= 65535 && P >= 0 && coeff >= 1 && coeff <= 3);
    MPN_CHECK_ARG(((uintptr_t)box | (uintptr_t)own_kp | (uintptr_t)img_kp | (uintptr_t)taps9 | (uintptr_t)taps17) % 8 == 0);
    MPN_CHECK_ARG(((uintptr_t)person_off | (uintptr_t)input | (uintptr_t)label | (uintptr_t)err) % 4 == 0);
    const int H = 28 * coeff, W = 18 * coeff;
    static_assert(84 * 54 <= kMaxCells, "coeff 3 must fit the LDS planes");
    hipLaunchKernelGGL(prn_train_maps_kernel, dim3(17, (unsigned)B, 2), dim3(kThreads), 0, (hipStream_t)stream, box, own_kp, img_kp,
                       person_off, P, H, W, threshold, taps9, taps17, input, label, err);
    return mpn_launch_status();
}
