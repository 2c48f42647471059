// Temporal accumulation by reprojection (include/pt_hip.h: pt_temporal_push_host).  The header states the arithmetic; everything
// here is one correctly rounded float operation per step in that order, nothing fused (the Makefile builds with
// -ffp-contract=off and IEEE divide), so tests/temporal_restatement.py reproduces the results bit for bit in numpy.
//
// The history of a frame is four 16-byte records per pixel:
//   sum_n     Hs.xyz  + Hn  (sums of the contributions and their effective number)
//   sum2_age  Hs2.xyz + HL  (sums of the squares and the history's age in frames)
//   normal    N'.xyz  + hit flag (1 = a triangle, 0 = a miss)
//   position  P'.xyz  + 0
// so a history tap is four 16-byte loads, and a pixel reads at most the 2 x 2 taps around the place it was seen at in the
// previous frame.  The records are ping-pong: a push reads one set and writes the other, since a pixel's old record is another
// pixel's tap.  A workgroup is 32 x 8 pixels as in the a-trous filter; neighbouring pixels reproject to neighbouring taps, so a
// wave's taps are a few contiguous row segments of each record plane.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_temporal.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__global__ __launch_bounds__(256) void temporal_merge_kernel(TemporalArgs a) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= a.width || y >= a.height) return;
    const size_t p = static_cast<size_t>(y) * a.width + x;
    const bool hit = a.hit_index[p] >= 0;
    const float Nx = a.normal[3 * p], Ny = a.normal[3 * p + 1], Nz = a.normal[3 * p + 2];
    const float Px = a.position[3 * p], Py = a.position[3 * p + 1], Pz = a.position[3 * p + 2];
    const float4 *HA = static_cast<const float4 *>(a.prev.sum_n), *HB = static_cast<const float4 *>(a.prev.sum2_age);
    const float4 *HN = static_cast<const float4 *>(a.prev.normal), *HP = static_cast<const float4 *>(a.prev.position);

    // the history part h = (h_s, h_n), (h_s2, h_L)
    float4 ha = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool have = false;
    if (a.mode == kTemporalStatic) {
        const float4 qa = HA[p];
        if (qa.w > 0.0f) {
            ha = qa;
            hb = HB[p];
            have = true;
        }
    } else if (a.mode == kTemporalReproject) {
        float ex, ey, ez;
        if (hit) {
            ex = Px - a.prev_origin[0]; ey = Py - a.prev_origin[1]; ez = Pz - a.prev_origin[2];
        } else {   // the sky: a direction, reprojected by rotation only
            const float u = static_cast<float>(static_cast<double>(x) / a.width - 0.5);
            const float v = static_cast<float>(-static_cast<double>(y) / a.height + 0.5);
            const float *c = a.cam;
            ex = (u * c[3] + v * c[6]) + c[9];
            ey = (u * c[4] + v * c[7]) + c[10];
            ez = (u * c[5] + v * c[8]) + c[11];
        }
        const float *m = a.prev_inverse;
        const float ca = dot3(m[0], m[1], m[2], ex, ey, ez), cb = dot3(m[3], m[4], m[5], ex, ey, ez), cg = dot3(m[6], m[7], m[8], ex, ey, ez);
        if (cg > 0.0f) {
            const float fw = static_cast<float>(a.width), fh = static_cast<float>(a.height);
            const float fx = (ca / cg + 0.5f) * fw, fy = (0.5f - cb / cg) * fh;
            if (fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {   // false for a NaN; checked before any conversion
                const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
                const float tx = fx - x0f, ty = fy - y0f;
                const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
                float wt = 0.0f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int yq = y0 + j;
                    if (yq < 0 || yq >= a.height) continue;
                    const float wy = j ? ty : 1.0f - ty;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int xq = x0 + i;
                        if (xq < 0 || xq >= a.width) continue;
                        const size_t q = static_cast<size_t>(yq) * a.width + xq;
                        const float4 qa = HA[q], qn = HN[q];
                        if (!(qa.w > 0.0f) || (qn.w != 0.0f) != hit) continue;
                        if (hit) {
                            const float4 qp = HP[q];
                            if (!(dot3(Nx, Ny, Nz, qn.x, qn.y, qn.z) >= a.min_normal_dot)) continue;
                            const float dist = __builtin_fabsf(dot3(Nx, Ny, Nz, qp.x - Px, qp.y - Py, qp.z - Pz));
                            if (!(dist <= a.sigma_plane)) continue;
                        }
                        const float4 qb = HB[q];
                        const float w = (i ? tx : 1.0f - tx) * wy;
                        wt = wt + w;
                        ha.x = ha.x + w * qa.x; ha.y = ha.y + w * qa.y; ha.z = ha.z + w * qa.z; ha.w = ha.w + w * qa.w;
                        hb.x = hb.x + w * qb.x; hb.y = hb.y + w * qb.y; hb.z = hb.z + w * qb.z; hb.w = hb.w + w * qb.w;
                    }
                }
                if (wt > kTemporalMinWeight) {
                    ha.x = ha.x / wt; ha.y = ha.y / wt; ha.z = ha.z / wt; ha.w = ha.w / wt;
                    hb.x = hb.x / wt; hb.y = hb.y / wt; hb.z = hb.z / wt; hb.w = hb.w / wt;
                    have = true;
                }
            }
        }
    }
    if (have && hb.w > a.max_frames) {   // the cap: an old history weighs as one of max_frames frames
        const float k = a.max_frames / hb.w;
        ha.x = ha.x * k; ha.y = ha.y * k; ha.z = ha.z * k; ha.w = ha.w * k;
        hb.x = hb.x * k; hb.y = hb.y * k; hb.z = hb.z * k; hb.w = hb.w * k;
    }

    const float s0 = a.sum[3 * p], s1 = a.sum[3 * p + 1], s2 = a.sum[3 * p + 2];
    const float q0 = a.sum2[3 * p], q1 = a.sum2[3 * p + 1], q2 = a.sum2[3 * p + 2];
    const int32_t c = a.count[p];
    const float cf = static_cast<float>(c);
    float4 na = make_float4(s0, s1, s2, cf), nb = make_float4(q0, q1, q2, 1.0f);
    float o0 = s0, o1 = s1, o2 = s2, r0 = q0, r1 = q1, r2 = q2;
    int32_t n_i = 0;
    if (have) {
        na = make_float4(s0 + ha.x, s1 + ha.y, s2 + ha.z, cf + ha.w);
        nb = make_float4(q0 + hb.x, q1 + hb.y, q2 + hb.z, 1.0f + hb.w);
        // the outputs carry an integer count: the history's mean and second moment survive the rounding of its count
        if (ha.w > 0.0f) {
            n_i = static_cast<int32_t>(ha.w + 0.5f);
            n_i = n_i > 1 ? n_i : 1;
        }
        const float r = n_i ? static_cast<float>(n_i) / ha.w : 1.0f;
        o0 = s0 + ha.x * r; o1 = s1 + ha.y * r; o2 = s2 + ha.z * r;
        r0 = q0 + hb.x * r; r1 = q1 + hb.y * r; r2 = q2 + hb.z * r;
    }
    static_cast<float4 *>(a.next.sum_n)[p] = na;
    static_cast<float4 *>(a.next.sum2_age)[p] = nb;
    static_cast<float4 *>(a.next.normal)[p] = make_float4(Nx, Ny, Nz, hit ? 1.0f : 0.0f);
    static_cast<float4 *>(a.next.position)[p] = make_float4(Px, Py, Pz, 0.0f);
    a.sum_out[3 * p] = o0; a.sum_out[3 * p + 1] = o1; a.sum_out[3 * p + 2] = o2;
    a.sum2_out[3 * p] = r0; a.sum2_out[3 * p + 1] = r1; a.sum2_out[3 * p + 2] = r2;
    a.count_out[p] = c + n_i;
    a.history_frames[p] = nb.w;
}

}  // namespace

hipError_t launch_temporal_merge(const TemporalArgs &a, hipStream_t stream) {
    const dim3 tiles((a.width + 31) / 32, (a.height + 7) / 8);
    hipLaunchKernelGGL(temporal_merge_kernel, tiles, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace pt
