// The primary ray of a non-perspective projection (include/pt_hip.h: pt_projection), spelled once: the integrator's projection
// kernels (pt_kernels.hip: integrate_kernel_projection, through pt_integrator_body.inc) and the first-hit feature pass
// (pt_kernels.hip: projection_rays_kernel) both call it, so that the feature buffers, the denoiser and the upsampler see the view
// the integrator traced.  Float arithmetic, one correctly rounded operation per step in the order the header states, nothing fused
// (the Makefile builds with -ffp-contract=off and IEEE divide / sqrt): tests/projection_composition.py restates it in numpy.
//
// A small forceinline function like portable_sincos, not a shared kernel body: it is called from the one place of each kernel
// where a primary ray is made.  The caller passes what differs between its two users:
//   c       the camera, 12 floats (origin, right, up, forward), read where a component is consumed
//   ax      r^, u^, f^: right, up, forward as unit vectors (normalised in double, rounded once, as pt_lens defines them), 9 floats
//   span    span_x, span_y of the projection, 2 floats
//   sincos  portable_sincos (domain [0, 2 pi]);  normalize  normalize3 of the bounce code
// `kind` is a kernel argument, hence wave-uniform: the branches on it are scalar branches and a wave runs one of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pt {

constexpr int32_t kProjectionPerspective = 0, kProjectionOrthographic = 1, kProjectionFisheye = 2, kProjectionEquirectangular = 3;

// x with its sign bit flipped if s is negative: puts the sign of an angle back on the sine of its absolute value
__device__ __forceinline__ float projection_sign_from(float x, float s) {
    return __uint_as_float(__float_as_uint(x) ^ (__float_as_uint(s) & 0x80000000u));
}

// (u, v): the pixel's image coordinates as pt_camera forms them.  Writes the origin one component at a time (into the ray slot)
// and the unit direction.  kind is one of the three non-perspective kinds.
template <class Cam, class Axes, class Span, class SinCos, class Normalize>
__device__ __forceinline__ void projection_primary_ray(int32_t kind, float u, float v, Cam c, Axes ax, Span span, SinCos sincos, Normalize normalize,
                                                       float &ox, float &oy, float &oz, float &dx, float &dy, float &dz) {
    if (kind == kProjectionOrthographic) {
        // parallel rays along forward from the plane right and up span around the origin
        ox = c[0] + (u * c[3] + v * c[6]);
        oy = c[1] + (u * c[4] + v * c[7]);
        oz = c[2] + (u * c[5] + v * c[8]);
        dx = c[9]; dy = c[10]; dz = c[11];
    } else {
        float wr, wu, wf;   // the direction's weights of r^, u^, f^
        if (kind == kProjectionFisheye) {
            // equidistant: the angle from forward is the distance from the image centre; sin(theta) / theta scales (a, b)
            const float a = u * span[0], b = v * span[1];
            const float theta = __builtin_sqrtf(a * a + b * b);
            float sn, cs;
            sincos(theta, sn, cs);
            const float k = theta == 0.0f ? 1.0f : sn / theta;
            wr = k * a; wu = k * b; wf = cs;
        } else {
            // longitude phi from forward towards right, latitude psi towards up
            const float phi = u * span[0], psi = v * span[1];
            float s_phi, c_phi, s_psi, c_psi;
            sincos(__builtin_fabsf(phi), s_phi, c_phi);
            s_phi = projection_sign_from(s_phi, phi);
            sincos(__builtin_fabsf(psi), s_psi, c_psi);
            s_psi = projection_sign_from(s_psi, psi);
            wr = c_psi * s_phi; wu = s_psi; wf = c_psi * c_phi;
        }
        ox = c[0];
        dx = (wr * ax[0] + wu * ax[3]) + wf * ax[6];
        oy = c[1];
        dy = (wr * ax[1] + wu * ax[4]) + wf * ax[7];
        oz = c[2];
        dz = (wr * ax[2] + wu * ax[5]) + wf * ax[8];
    }
    normalize(dx, dy, dz);
}

}  // namespace pt
