// grad_clip.hip — gradient clipping by the infinity norm on the device (the reference Trainer's max_grad_norm option,
// training/trainer.py:254-257: clip_grad_norm(model.parameters(), max_grad_norm, float('inf'))).
//
// torch (nn/utils/clip_grad.py) computes, in f32 on the device:
//   total = max over grads of max |g|                        (NaN anywhere -> NaN)
//   coef  = min(reciprocal(total + 1e-6f) * max_norm, 1)     (Tensor.__rdiv__ is reciprocal * scalar; clamp keeps a NaN)
//   g    *= coef                                              (also when coef == 1)
// Here: mpn_grad_absmax_partial reduces one contiguous run of the gradient arena to one partial per workgroup, one launch per run
// into consecutive slots of a workspace; mpn_grad_clip_finalize (one workgroup) reduces the partials and writes total and coef to
// device scalars.  max is order-independent, so the result does not depend on the grid, and two launches need no inter-workgroup
// counter: the pair is valid under replay and graph capture.  mpn_scale_by_dev scales the gradients in place; for trainable runs
// mpn_adam_step_clip_dev (weight_prep.hip) runs it right before the unchanged Adam update.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr long kPerPart = (long)kThreads * 4 * 4;   // floats per partial before the grid is capped (4 float4 per thread)
constexpr long kMaxParts = 1024;                    // partials per run; beyond it every thread strides further

inline long absmax_parts(long n) {
    const long p = (n + kPerPart - 1) / kPerPart;
    return p < kMaxParts ? p : kMaxParts;
}

// max that propagates NaN (fmaxf drops it; torch's max-abs reduction does not)
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

// 64-lane shuffle tree, then one value per wave through LDS; thread 0 returns the workgroup's max
__device__ __forceinline__ float block_max_nan(float m) {
    __shared__ float wave_max[kThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max_nan(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) m = max_nan(m, wave_max[w]);
    }
    return m;
}

__global__ __launch_bounds__(kThreads) void grad_absmax_partial_kernel(const float* __restrict__ g, long n, float* __restrict__ partials) {
    const long nvec = n >> 2;
    const long stride = (long)gridDim.x * kThreads;
    float m = 0.f;
    for (long j = (long)blockIdx.x * kThreads + threadIdx.x; j < nvec; j += stride) {
        const float4 x = *reinterpret_cast<const float4*>(g + 4 * j);
        m = max_nan(m, max_nan(max_nan(fabsf(x.x), fabsf(x.y)), max_nan(fabsf(x.z), fabsf(x.w))));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = max_nan(m, fabsf(g[4 * nvec + threadIdx.x]));
    m = block_max_nan(m);
    if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

__global__ __launch_bounds__(kThreads) void grad_clip_finalize_kernel(const float* __restrict__ partials, long nparts,
                                                                      const float* __restrict__ max_norm, float* __restrict__ total,
                                                                      float* __restrict__ coef) {
    float m = 0.f;
    for (long j = threadIdx.x; j < nparts; j += kThreads) m = max_nan(m, partials[j]);
    m = block_max_nan(m);
    if (threadIdx.x == 0) {
        const float r = 1.0f / (m + 1e-6f);        // correctly rounded division (hipcc's default for f32), as torch.reciprocal
        const float c = r * *max_norm;
        *total = m;
        *coef = (c > 1.f) ? 1.f : c;               // clamp(max=1): a NaN stays NaN
    }
}

__global__ void scale_by_kernel(float* __restrict__ x, long n, const float* __restrict__ s) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float c = *s;
    if (i + 3 < n) {
        float4 v = *reinterpret_cast<float4*>(x + i);
        v.x = v.x * c; v.y = v.y * c; v.z = v.z * c; v.w = v.w * c;
        *reinterpret_cast<float4*>(x + i) = v;
    } else {
        for (long k = i; k < n; ++k) x[k] = x[k] * c;
    }
}

}  // namespace

extern "C" int64_t mpn_grad_absmax_workspace_bytes(int64_t n) {
    if (n <= 0) return MPN_E_BADARG;
    return (int64_t)sizeof(float) * absmax_parts((long)n);
}

extern "C" int mpn_grad_absmax_partial(const float* grad, int64_t n, float* partials, void* stream) {
    MPN_CHECK_ARG(grad && partials && n > 0);
    MPN_CHECK_ARG((uintptr_t)grad % 16 == 0 && (uintptr_t)partials % 4 == 0);
    hipLaunchKernelGGL(grad_absmax_partial_kernel, dim3((unsigned)absmax_parts((long)n)), dim3(kThreads), 0, (hipStream_t)stream, grad,
                       (long)n, partials);
    return mpn_launch_status();
}

extern "C" int mpn_grad_clip_finalize(const float* partials, int64_t nparts, const float* max_norm, float* total, float* coef,
                                      void* stream) {
    MPN_CHECK_ARG(partials && max_norm && total && coef && nparts > 0);
    MPN_CHECK_ARG(((uintptr_t)partials | (uintptr_t)max_norm | (uintptr_t)total | (uintptr_t)coef) % 4 == 0);
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, partials, (long)nparts, max_norm, total,
                       coef);
    return mpn_launch_status();
}

extern "C" int mpn_scale_by_dev(float* x, int64_t n, const float* s, void* stream) {
    MPN_CHECK_ARG(x && s && n > 0);
    MPN_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)s % 4 == 0);
    const long blocks = (n + 1023) / 1024;
    hipLaunchKernelGGL(scale_by_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long)n, s);
    return mpn_launch_status();
}
