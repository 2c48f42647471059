// The feature weight of include/pt_hip.h (pt_denoise_host, step 2), the one copy the denoiser's and the upsampler's kernels share.
// Device code only; every step is one correctly rounded float operation (the including file sets fp contract off).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace pt {

// w * w_n * w_p of a tap q for a centre p on a triangle: w_n = max(0, n_p . n_q)^(2^k) by k squarings,
// w_p = 1 / (1 + (|n_p . (P_q - P_p)| / sigma_plane)^2).  b = normal.xyz (+ hit flag), c = position.xyz.
__device__ __forceinline__ float feature_weight(float w, const float4 &bp, const float4 &cp, const float4 &bq, const float4 &cq,
                                                float sigma_plane, int k) {
    const float dn = (bp.x * bq.x + bp.y * bq.y) + bp.z * bq.z;
    float wn = dn > 0.0f ? dn : 0.0f;
    for (int i = 0; i < k; ++i) wn = wn * wn;
    const float ex = cq.x - cp.x, ey = cq.y - cp.y, ez = cq.z - cp.z;
    const float dist = __builtin_fabsf((bp.x * ex + bp.y * ey) + bp.z * ez);
    const float up = dist / sigma_plane;
    const float wp = 1.0f / (1.0f + up * up);
    return (w * wn) * wp;
}

}  // namespace pt
