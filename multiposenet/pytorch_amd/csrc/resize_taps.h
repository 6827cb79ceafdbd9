// resize_taps.h — the tap rule of the restated cv2.resize(INTER_CUBIC), shared by peaks.hip (resize_kernel, peak refinement) and
// tta.hip (mpn_tta_merge).  Users are built with -ffp-contract=off.
#pragma once
#include "common.h"

__device__ __forceinline__ void cubic_taps(int d, double scale, int n_src, int (&idx)[4], float (&co)[4]) {
    const float fx = (float)(((double)d + 0.5) * scale - 0.5);
    const int sx = (int)floorf(fx);
    cubic_coeffs(fx - (float)sx, co);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int s = sx - 1 + k;
        idx[k] = s < 0 ? 0 : (s > n_src - 1 ? n_src - 1 : s);
    }
}
