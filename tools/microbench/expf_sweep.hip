// Dense sweep of the device's expf against float64 exp on [-10, 10]: worst error in float32 ulps.  The source of EXPF_ULP_MEASURED in
// tests/postproc_ref.py (the expf allowance of the box-decode bound); the kernel only calls expf on a ramp.  Built like csrc/nms.hip:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/microbench/expf_sweep.hip -o tools/microbench/expf_sweep
// MI355X, ROCm 7.0: "134217728 points on [-10, 10], worst 0.8576 ulp at x = 3.72555065, mean 0.2568 ulp, points above 1 ulp: 0".
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

__global__ void sweep_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = expf(x[i]);
}

int main() {
    const long chunk = 1L << 24, chunks = 8;                       // 2^27 points: step 20 / 2^27 = 1.5e-7
    const long total = chunk * chunks;
    std::vector<float> hx(chunk), hy(chunk);
    float *dx = nullptr, *dy = nullptr;
    CK(hipMalloc(&dx, chunk * sizeof(float)));
    CK(hipMalloc(&dy, chunk * sizeof(float)));
    double worst = 0.0, worst_x = 0.0, sum = 0.0;
    long over1 = 0;
    for (long c = 0; c < chunks; ++c) {
        for (long i = 0; i < chunk; ++i) hx[i] = (float)(-10.0 + 20.0 * (double)(c * chunk + i) / (double)(total - 1));
        CK(hipMemcpy(dx, hx.data(), chunk * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(sweep_kernel, dim3((unsigned)((chunk + 255) / 256)), dim3(256), 0, 0, dx, dy, chunk);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(hy.data(), dy, chunk * sizeof(float), hipMemcpyDeviceToHost));
        for (long i = 0; i < chunk; ++i) {
            const double ref = std::exp((double)hx[i]);
            int e;
            std::frexp(ref, &e);                                    // ref = m * 2^e, m in [0.5, 1): ulp32 = 2^(e - 24)
            const double ulp = std::ldexp(1.0, e - 24);
            const double err = std::fabs((double)hy[i] - ref) / ulp;
            sum += err;
            if (err > 1.0) ++over1;
            if (err > worst) { worst = err; worst_x = hx[i]; }
        }
    }
    std::printf("expf sweep: %ld points on [-10, 10], worst %.4f ulp at x = %.9g, mean %.4f ulp, points above 1 ulp: %ld\n", total, worst,
                worst_x, sum / (double)total, over1);
    CK(hipFree(dx));
    CK(hipFree(dy));
    return 0;
}
