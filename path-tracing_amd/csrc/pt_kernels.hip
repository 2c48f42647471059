// Radiance-integrator kernel for gfx950 (MI355X).  One lane = one pixel's path, one wave = an 8x8 pixel tile,
// all passes x segments x triangles of a row band in one launch.
//
// Per path segment a wave does three things:
//   1. CULL   triangles are listed in SLOT order (pt_scene.hpp): the table builder groups them spatially, whatever order the
//             OBJ lists them in.  Large triangles (walls) get a barycentric test, wave-uniformly, records through scalar
//             loads and used straight from SGPRs.  Small triangles hang under a hierarchy: in scenes of up to 2048 triangles
//             an 8-ary tree of bounding spheres per connected group, in bigger ones ONE tree of quantised boxes (64-byte
//             nodes) over all of them.  Either tree is walked with a wave-wide LIFO of (ray, node) work items in LDS, dealt out
//             evenly: lane l expands the l-th item whoever's ray it is; the queues are filled through a DPP prefix sum over the
//             lanes' survivor counts (one LDS store per entry, totals for the capacity checks for free).  The box walk also drops nodes entered beyond the
//             ray's best hit so far.  Every test is CONSERVATIVE with respect to the reference's Triangle::Intersect
//             (triangles.h:48-73): it may only say "cannot be a hit".  Survivors become (ray, slot) pairs in a second LDS queue.
//   2. EXACT  the pairs (about 1.5 per ray) are dealt out evenly as well; each runs the reference's arithmetic operation
//             for operation (same association, no FMA contraction, IEEE divide and sqrt), and the closest hit per ray is
//             taken with one LDS atomic-min on (distance, original triangle index), so `t`, the hit decision and the
//             closest-hit choice are bit-identical to the CPU path.
//   3. SHADE  Material::Process + the three lobes (material.h:36-102), Ray::Reflect (ray.h:45-50), the tile's accumulators
//             (material.h:74-77) in LDS, counter-based Philox4x32-10 randoms keyed by (seed | pixel, pass, segment).
//
// The kernel is bound by instruction issue -- its time follows the number of instructions its waves execute, vector or scalar
//  -- so the code below is written for few instructions, not for few memory accesses or many waves.
//
// Everything that decides a result is plain IEEE binary32/binary64 arithmetic (float sqrt and reciprocal through
// pt_fastfp.hpp: shorter sequences, verified against the correctly rounded result for every float of their range); only
// step 1 uses fused multiply-adds and raw v_rcp_f32 results, and step 1 cannot change a result (DESIGN.md "Culling: why it
// cannot reject a hit"; the verification build, -DPT_VERIFY_BRUTE, re-checks every segment against the all-triangles loop).
#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <cstddef>
#include <type_traits>
#include <utility>

#include "pt_fastfp.hpp"
#include "pt_kernels.hpp"
#include "pt_projection.hpp"
#include "pt_environment.hpp"
#include "pt_texture.hpp"
#include "pt_smooth.hpp"
#include "pt_rough.hpp"
#include "pt_direct.hpp"
#include "pt_envdirect.hpp"
#include "pt_roulette.hpp"

#pragma clang fp contract(off)

namespace pt {

namespace {

#ifndef PT_WAVES_PER_SIMD
#define PT_WAVES_PER_SIMD 6
#endif
constexpr int kBlock = 64;                // one wave = one 8x8 pixel tile per workgroup (all LDS below is wave-private)
// Capacity of the two wave-private work queues.  Small scenes (Tor.obj) keep them small so that 5 KB of LDS per wave
// leaves room for 6+ waves per SIMD; scenes with thousands of triangles get deep queues (fuller rounds) and pay with
// occupancy, which matters less there.
#ifndef PT_SMALL_NODES
#define PT_SMALL_NODES 160   // 96 / 144: 4 x the rounds that do not fit (partial commits), -0.9 %; LDS still allows 6 waves per SIMD
#endif
#ifndef PT_SMALL_PAIRS
#define PT_SMALL_PAIRS 256
#endif
struct SmallQueues { static constexpr int kNodeStack = PT_SMALL_NODES, kPairQueue = PT_SMALL_PAIRS, kFiltered = 1; };
// the same for the small-scene kernel with two rays per lane (twice the items per wave-segment)
#ifndef PT_SMALL2_NODES
#define PT_SMALL2_NODES 160
#endif
#ifndef PT_SMALL2_PAIRS
#define PT_SMALL2_PAIRS 256
#endif
struct SmallQueues2 { static constexpr int kNodeStack = PT_SMALL2_NODES, kPairQueue = PT_SMALL2_PAIRS, kFiltered = 1; };
#ifndef PT_BIG_NODES
#define PT_BIG_NODES 384      // measured on the 16 398- and 49 934-triangle scenes: 832 / 512 (4 waves per SIMD) is 4 % slower,
#endif
#ifndef PT_BIG_PAIRS
#define PT_BIG_PAIRS 256      // 256 / 160 (6 waves per SIMD) 7 % slower than this (5 waves per SIMD)
#endif
#ifndef PT_BIG_FILTERED
#define PT_BIG_FILTERED 128
#endif
#ifndef PT_BIG_EXACT_AT
#define PT_BIG_EXACT_AT 64    // big scenes: pre-filtered pairs waiting before an exact round runs (fewer = earlier pruning, emptier rounds)
#endif
#ifndef PT_BOX_SCHED
#define PT_BOX_SCHED 1        // box tree's child test: a scheduling barrier after every PT_BOX_SCHED children (9 = none)
#endif
#ifndef PT_BIG_WAVES
#define PT_BIG_WAVES (PT_WAVES_PER_SIMD - 2)   // waves per SIMD the big-scene instantiations are compiled for (they fit 6: 77 VGPRs)
#endif
#ifndef PT_SKY_WAVES
// ... and the skybox instantiations: 5 since round 4 (96 VGPRs, no scratch; at 4 the compiler took 102-117): +9.6 % on the open
// scenes (Tor.obj without its back wall 6 950 -> 7 620 Msamples/s at 64 spp, the torus x9 3 585 -> 3 915; r04_ab_logs.txt sky5).
// At 6 (80 VGPRs) the lookup's double arithmetic spills 30 registers.
#define PT_SKY_WAVES (PT_WAVES_PER_SIMD - 1)
#endif
struct BigQueues { static constexpr int kNodeStack = PT_BIG_NODES, kPairQueue = PT_BIG_PAIRS, kFiltered = PT_BIG_FILTERED; };
// the box-tree kernel's adaptive instantiations keep one 16-bit word per pixel of their tile (128 / 256 pixels) in LDS: the node stack
// gives up that much, so that the wave stays within five 1 280-byte granules (six waves per SIMD)
#ifndef PT_BIG_ADAPT_NODES
#define PT_BIG_ADAPT_NODES(pixels_per_lane) ((PT_BIG_NODES + 46 - 32 * (pixels_per_lane)) > 64 ? (PT_BIG_NODES + 46 - 32 * (pixels_per_lane)) : 64)   // (the tiny-queue test build)
#endif
template <int OWN> struct BigQueuesAdapt { static constexpr int kNodeStack = PT_BIG_ADAPT_NODES(OWN), kPairQueue = PT_BIG_PAIRS, kFiltered = PT_BIG_FILTERED; };

// ---------------------------------------------------------------------------------------------------------------
// Counter RNG (layout shared with the CPU oracle; see DESIGN.md "Counter RNG")
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t &o0, uint32_t &o1, uint32_t &o2, uint32_t &o3) {
    // The ten round keys are wave-uniform and loop-invariant; hoisted out of the path loops they would sit in ten
    // spilled SGPRs (a v_readlane + hazard nop each).  Opaque here, they are rebuilt with one scalar add per round.
    asm volatile("" : "+s"(k0));
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = static_cast<unsigned long long>(c0) * 0xD2511F53u;   // one v_mad_u64_u32 each
        const unsigned long long p1 = static_cast<unsigned long long>(c2) * 0xCD9E8D57u;
        const uint32_t h0 = static_cast<uint32_t>(p0 >> 32), l0 = static_cast<uint32_t>(p0);
        const uint32_t h1 = static_cast<uint32_t>(p1 >> 32), l1 = static_cast<uint32_t>(p1);
        c0 = __builtin_amdgcn_bitop3_b32(h1, c1, k0, 0x96);   // three-way xor in one instruction (the compiler emits two v_xor_b32)
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1; o2 = c2; o3 = c3;
}
__device__ __forceinline__ float unit_float(uint32_t w) {   // (0,1), never 0 or 1
    return static_cast<float>(((w >> 9) << 1) | 1u) * 5.9604644775390625e-08f;
}
__device__ __forceinline__ double jitter_double(uint32_t w) {   // (-0.5,0.5)
    return (static_cast<double>(w) + 0.5) * 2.3283064365386962890625e-10 - 0.5;
}

// sin/cos of a float angle in [0, 2pi]: double +,-,* only, so the result is the same on every IEEE machine.
// The sixteen double constants come from one table through the scalar cache (two s_load_dwordx16): as immediates each
// costs two s_mov_b32, a third of this function's instructions.
__constant__ double kSinCosTab[16] = {
    0.63661977236758138, 1.57079632673412561417e+00, 6.07710050650619224932e-11, 0.5,
    -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
    -2.50507602534068634195e-08, 1.58969099521155010221e-10,
    4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
    2.08757232129817482790e-09, -1.13596475577881948265e-11};
__device__ __forceinline__ void portable_sincos(float a, float &s_out, float &c_out) {
    typedef const __attribute__((address_space(4))) double *ConstD;
    ConstD t = (ConstD)reinterpret_cast<uintptr_t>(kSinCosTab);
    asm volatile("" : "+s"(t));   // keeps the compiler from folding the table back into immediates
    const double x = static_cast<double>(a);
    const int k = static_cast<int>(x * t[0] + t[3]);
    const double kd = static_cast<double>(k);
    const double r = (x - kd * t[1]) - kd * t[2];
    const double z = r * r;
    const double ps = t[4] + z * (t[5] + z * (t[6] + z * (t[7] + z * (t[8] + z * t[9]))));
    const double sn = r + r * (z * ps);
    const double pc = t[10] + z * (t[11] + z * (t[12] + z * (t[13] + z * (t[14] + z * t[15]))));
    const double cs = (1.0 - t[3] * z) + (z * z) * pc;
    // Quadrant k & 3 = 0: (sn, cs), 1: (cs, -sn), 2: (-sn, -cs), 3: (-cs, sn).  Rounding to float commutes with negation, so the
    // pair is narrowed first and then swapped / sign-flipped with integer operations.
    const uint32_t q = static_cast<uint32_t>(k);
    const float sf = static_cast<float>(sn), cf = static_cast<float>(cs);
    const bool odd = (q & 1u) != 0u;
    const uint32_t ua = __float_as_uint(odd ? cf : sf), ub = __float_as_uint(odd ? sf : cf);
    s_out = __uint_as_float(ua ^ ((q & 2u) << 30));
    c_out = __uint_as_float(ub ^ (((q + 1u) & 2u) << 30));
}

// Portable atan / atan2 / acos for the skybox lookup (scene.cpp:127-128): double +,-,*,/,sqrt only, the same
// sequence as the CPU oracle's, so that texel coordinates agree bit for bit.
__device__ __forceinline__ double portable_atan_pos(double x) {   // x >= 0, finite or +inf
    int id;
    double hi = 0.0, lo = 0.0;
    if (x < 0.4375) {
        id = -1;
    } else if (x < 1.1875) {
        if (x < 0.6875) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17; }
        else { id = 1; x = (x - 1.0) / (x + 1.0); hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17; }
    } else if (x < 2.4375) {
        id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17;
    } else {
        id = 3; x = -1.0 / x; hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17;
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02
                    + w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02
                    + w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (id < 0) return x - x * (s1 + s2);
    return hi - ((x * (s1 + s2) - lo) - x);
}
__device__ __forceinline__ float portable_atan2f(float yf, float xf) {
    const double y = static_cast<double>(yf), x = static_cast<double>(xf);
    if (y != y || x != x) return __builtin_nanf("");
    const double pi = 3.14159265358979311600e+00, pi_2 = 1.57079632679489655800e+00;
    const double ay = y < 0 ? -y : y, ax = x < 0 ? -x : x;
    double r;
    if (ay == 0.0) r = (x < 0 || (x == 0 && __builtin_signbit(xf))) ? pi : 0.0;
    else if (ax == 0.0) r = pi_2;
    else {
        const double t = portable_atan_pos(ay / ax);
        r = x < 0 ? pi - t : t;
    }
    return static_cast<float>((y < 0 || (y == 0 && __builtin_signbit(yf))) ? -r : r);
}
__device__ __forceinline__ float portable_acosf(float vf) {
    const double v = static_cast<double>(vf);
    const double s = __builtin_sqrt((1.0 - v) * (1.0 + v));   // NaN for |v| > 1, like acosf
    if (s != s) return __builtin_nanf("");
    const double pi = 3.14159265358979311600e+00, pi_2 = 1.57079632679489655800e+00;
    double r;
    if (v == 0.0) r = pi_2;
    else {
        const double t = portable_atan_pos(s / (v < 0 ? -v : v));
        r = v < 0 ? pi - t : t;
    }
    return static_cast<float>(r);
}

// ---------------------------------------------------------------------------------------------------------------
// 1. CULL: may only answer "this triangle cannot be accepted by Triangle::Intersect for this ray".
// ---------------------------------------------------------------------------------------------------------------
struct Ray {
    float ox, oy, oz, dx, dy, dz;
};

typedef const __attribute__((address_space(4))) float *ConstF;
__device__ __forceinline__ CullRec load_cull(ConstF p) {
    CullRec r;
    r.n[0] = p[0]; r.n[1] = p[1]; r.n[2] = p[2]; r.w = p[3];
    r.au[0] = p[4]; r.au[1] = p[5]; r.au[2] = p[6]; r.cu = p[7];
    r.av[0] = p[8]; r.av[1] = p[9]; r.av[2] = p[10]; r.cv = p[11];
    return r;
}
typedef const __attribute__((address_space(4))) uint32_t *ConstU;

// Keep the node iff the ray (not the whole line) comes within sqrt(r2) of the centre.  Written so that a NaN keeps.
__device__ __forceinline__ bool sphere_keep(float cx, float cy, float cz, float r2, const Ray &q) {
    const float mx = cx - q.ox, my = cy - q.oy, mz = cz - q.oz;
    const float b = __builtin_fmaf(mx, q.dx, __builtin_fmaf(my, q.dy, mz * q.dz));
    const float m2 = __builtin_fmaf(mx, mx, __builtin_fmaf(my, my, mz * mz));
    const float bb = __builtin_fmaxf(b, 0.0f);
    const float disc = __builtin_fmaf(-bb, bb, m2);
    return !(disc > r2);
}

// A quad record = the two halves of a parallelogram in one stored plane (pt_scene.hpp: ClusterDesc): the plane rows
// as in a triangle record, then alpha and beta rows.  Half A keeps iff min(beta, alpha-beta, 1-alpha) >= -mg,
// half B iff min(alpha, beta-alpha, 1-beta) >= -mg.  Returns bit 0 = reject A, bit 1 = reject B.
__device__ __forceinline__ uint32_t cull_reject_quad(const CullRec r, const Ray &q, float k1, float k2, float a_max, float m0q,
                                                     float t_guard) {
    const float num = __builtin_fmaf(q.ox, r.n[0], __builtin_fmaf(q.oy, r.n[1], __builtin_fmaf(q.oz, r.n[2], r.w)));
    const float den = __builtin_fmaf(q.dx, r.n[0], __builtin_fmaf(q.dy, r.n[1], q.dz * r.n[2]));
    const float rden = __builtin_amdgcn_rcpf(den);
    const float t = -num * rden;
    const float px = __builtin_fmaf(t, q.dx, q.ox), py = __builtin_fmaf(t, q.dy, q.oy), pz = __builtin_fmaf(t, q.dz, q.oz);
    const float al = __builtin_fmaf(px, r.au[0], __builtin_fmaf(py, r.au[1], __builtin_fmaf(pz, r.au[2], r.cu)));
    const float be = __builtin_fmaf(px, r.av[0], __builtin_fmaf(py, r.av[1], __builtin_fmaf(pz, r.av[2], r.cv)));
    const float d = al - be;
    const float ea = __builtin_fminf(__builtin_fminf(be, d), 1.0f - al);
    const float eb = __builtin_fminf(__builtin_fminf(al, -d), 1.0f - be);
    const float et = __builtin_fmaf(k1, __builtin_fabsf(t), k2) * __builtin_fabsf(rden);
    const float mg = __builtin_fmaf(a_max, et, m0q);
    const bool behind = t < -et;
    const bool trusted = __builtin_fabsf(t) < t_guard;
    return ((trusted & ((ea < -mg) | behind)) ? 1u : 0u) | ((trusted & ((eb < -mg) | behind)) ? 2u : 0u);
}

__device__ __forceinline__ bool cull_reject(const CullRec r, const Ray &q, float k1, float k2, float a_max, float m0,
                                            float t_guard) {
    const float num = __builtin_fmaf(q.ox, r.n[0], __builtin_fmaf(q.oy, r.n[1], __builtin_fmaf(q.oz, r.n[2], r.w)));
    const float den = __builtin_fmaf(q.dx, r.n[0], __builtin_fmaf(q.dy, r.n[1], q.dz * r.n[2]));
    const float rden = __builtin_amdgcn_rcpf(den);
    const float t = -num * rden;
    const float px = __builtin_fmaf(t, q.dx, q.ox), py = __builtin_fmaf(t, q.dy, q.oy), pz = __builtin_fmaf(t, q.dz, q.oz);
    const float u = __builtin_fmaf(px, r.au[0], __builtin_fmaf(py, r.au[1], __builtin_fmaf(pz, r.au[2], r.cu)));
    const float v = __builtin_fmaf(px, r.av[0], __builtin_fmaf(py, r.av[1], __builtin_fmaf(pz, r.av[2], r.cv)));
    const float w = (1.0f - u) - v;
    const float e = __builtin_fminf(__builtin_fminf(u, v), w);
    // |t - t_reference| <= et ; a point the reference accepts has every barycentric coordinate >= -mg
    const float et = __builtin_fmaf(k1, __builtin_fabsf(t), k2) * __builtin_fabsf(rden);
    const float mg = __builtin_fmaf(a_max, et, m0);
    const bool outside = e < -mg;
    const bool behind = t < -et;                           // then t_reference < 0 < eps (triangles.h:51)
    const bool trusted = __builtin_fabsf(t) < t_guard;     // false for NaN/inf and for grazing rays
    return trusted & (outside | behind);                   // bitwise on purpose: no divergent branches in the cull loop
}

// ---------------------------------------------------------------------------------------------------------------
// 2. EXACT: Triangle::Intersect (triangles.h:48-73) with PlaneIntersect (:10-13) and ParallelogramSquare (:15-17).
// Every operation is written in the reference's order; GLM's cross/length association is kept.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float area2_of(float ax, float ay, float az, float bx, float by, float bz) {   // |a x b|^2
    const float cx = ay * bz - by * az;
    const float cy = az * bx - bz * ax;
    const float cz = ax * by - bx * ay;
    return cx * cx + cy * cy + cz * cz;
}
// Stages B-D of Triangle::Intersect for one (ray, triangle) pair, without the running `distance`:
// returns new_distance if the point passes the area tests, -inf otherwise (then stage A rejects it: -inf < eps).
__device__ __forceinline__ float exact_inside(const ExactRec *__restrict__ rec, const Ray &q, float eps, uint32_t &orig) {
    const float4 r0 = reinterpret_cast<const float4 *>(rec)[0];   // plane
    const float4 r1 = reinterpret_cast<const float4 *>(rec)[1];   // v0, square
    const float4 r2 = reinterpret_cast<const float4 *>(rec)[2];   // v1, material
    const float4 r3 = reinterpret_cast<const float4 *>(rec)[3];   // v2, original triangle index
    orig = __float_as_uint(r3.w);
    const float signed_dist = q.dx * r0.x + q.dy * r0.y + q.dz * r0.z;
    const float nd = -(q.ox * r0.x + q.oy * r0.y + q.oz * r0.z + r0.w) / signed_dist;
    const float px = q.ox + q.dx * nd, py = q.oy + q.dy * nd, pz = q.oz + q.dz * nd;
    const float f0x = px - r1.x, f0y = py - r1.y, f0z = pz - r1.z;
    const float f1x = px - r2.x, f1y = py - r2.y, f1z = pz - r2.z;
    const float f2x = px - r3.x, f2y = py - r3.y, f2z = pz - r3.z;
    const float sq = r1.w;
    const float q1 = area2_of(f0x, f0y, f0z, f1x, f1y, f1z);
    const float q2 = area2_of(f0x, f0y, f0z, f2x, f2y, f2z);
    const float q3 = area2_of(f2x, f2y, f2z, f1x, f1y, f1z);
    float s1, s2, s3;
    // one range check for the three roots: min and max of the squared areas decide for all of them
    if (__all(fast_fp_ok(__builtin_fminf(__builtin_fminf(q1, q2), q3)) & fast_fp_ok(__builtin_fmaxf(__builtin_fmaxf(q1, q2), q3)))) {
        s1 = sqrt_rn_normal(q1); s2 = sqrt_rn_normal(q2); s3 = sqrt_rn_normal(q3);
    } else {
        s1 = __builtin_sqrtf(q1); s2 = __builtin_sqrtf(q2); s3 = __builtin_sqrtf(q3);
    }
    const bool stage_b = !(s1 > sq + eps);
    const bool stage_c = !(s1 + s2 > sq + eps);
    const bool stage_d = !(__builtin_fabsf(sq - s1 - s2 - s3) > eps);
    return (stage_b && stage_c && stage_d) ? nd : -__builtin_inff();
}

// Inclusive prefix sum over the 64 lanes in six DPP additions: within rows of 16 lanes (row_shr 1, 2, 4, 8), then row 0
// into row 1 and row 2 into row 3 (row_bcast:15), then rows 0-1 into rows 2-3 (row_bcast:31).  Lane 63 holds the total.
// The work queues are filled with it: a lane's entries go to [base + exclusive prefix, ...), one ds_write per entry,
// instead of one wave-wide ballot round per bit plane (which cost a fifth of the big-scene kernel's instructions,
// profiles/r02_blockprof_*.txt) -- and the total, which the capacity checks need, comes for free.
__device__ __forceinline__ uint32_t wave_scan_inclusive(uint32_t v) {
    int x = static_cast<int>(v);
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, true);
    return static_cast<uint32_t>(x);
}
__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63)); }
// Minimum over the 64 lanes, wave-uniform: the same six DPP steps with min instead of + (a lane without a source keeps ~0).
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    int x = static_cast<int>(v);
    auto step = [&](int moved) { x = static_cast<int>(min(static_cast<uint32_t>(x), static_cast<uint32_t>(moved))); };
    step(__builtin_amdgcn_update_dpp(-1, x, 0x111, 0xF, 0xF, false));
    step(__builtin_amdgcn_update_dpp(-1, x, 0x112, 0xF, 0xF, false));
    step(__builtin_amdgcn_update_dpp(-1, x, 0x114, 0xF, 0xF, false));
    step(__builtin_amdgcn_update_dpp(-1, x, 0x118, 0xF, 0xF, false));
    step(__builtin_amdgcn_update_dpp(-1, x, 0x142, 0xA, 0xF, false));
    step(__builtin_amdgcn_update_dpp(-1, x, 0x143, 0xC, 0xF, false));
    return wave_last(static_cast<uint32_t>(x));
}
// One LDS store per set bit of `bits`: entry = ebase + (bit index << shift), at queue[pos], queue[pos + 1], ...
__device__ __forceinline__ void emit_bits(uint32_t *queue, uint32_t pos, uint32_t bits, uint32_t ebase, uint32_t shift = 0) {
    while (bits != 0) {
        const uint32_t j = __builtin_ctz(bits);
        bits &= bits - 1;
        queue[pos++] = ebase + (j << shift);
    }
}
// LDS traffic between lanes of ONE wave: the hardware executes a wave's LDS instructions in order, so only the
// compiler has to be stopped from moving them across the hand-off.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void normalize3(float &x, float &y, float &z) {   // glm::normalize(vec4(x,y,z,0))
    const float d = (x * x + y * y) + z * z;
    float inv;
    if (__all(fast_fp_ok(d))) inv = rcp_rn_normal(sqrt_rn_normal(d));   // the root of an in-range number is in range
    else inv = 1.0f / __builtin_sqrtf(d);
    x = x * inv; y = y * inv; z = z * inv;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// Closest hit of every lane's ray: Scene::TraceRay's loop (scene.cpp:114-120) for one wave.  Wave-uniform control
// flow: all 64 lanes must call it together; lanes with valid == false take part in the shared work only.
// ---------------------------------------------------------------------------------------------------------------
// R = rays per lane.  A wave owns 64 R pixels (an 8R x 8 tile) and a wave-segment searches 64 R rays: lane l carries rays
// l, l + 64, ...  Everything wave-uniform about a segment (the scalar half of the large-class loop, the cluster loop, queue
// bookkeeping) is then shared by R times the rays, and the lane-balanced rounds (sphere-tree items, exact pairs) are that much
// fuller -- for Tor.obj, where 9 % of the rays come near the torus and a segment yields 1.5 pairs per ray, that is where a sixth
// of the instructions went.  Big scenes keep R = 1 (their rounds are full anyway, their registers are not).
template <int N> struct AccPlanes { float v[7][N]; };
template <> struct AccPlanes<0> {};
template <int N> struct FlagWords { uint16_t v[N]; };
template <> struct FlagWords<0> {};
#ifndef PT_MATS_IN_LDS
#define PT_MATS_IN_LDS 16   // two-pixel kernels: a scene's materials, if it has at most this many, are read from a copy in LDS
#endif
template <int N> struct InvPlanes { float v[3][N]; };
template <> struct InvPlanes<0> {};
template <int N> struct MatCache { float4 v[3 * N]; };
template <> struct MatCache<0> {};
template <class Q, int R, int FLAGS = 0>
struct WaveLds {
    static constexpr int kRays = R, kSlots = 64 * R;
    static constexpr int kNodeStack = Q::kNodeStack, kPairQueue = Q::kPairQueue;
    static constexpr bool kPrefilter = Q::kFiltered > 1;   // big scenes: thin the pairs with the barycentric test first
    static_assert(R == 1 || R == 2, "ray ids take 6 or 7 bits of a work item");
    // work-item layouts: sphere-tree stack entries = ray << kNodeSrcShift | level << kNodeLevShift | node index within its level;
    // pairs = slot | ray << 24 (| kUnfiltered << 24 with the pre-filter)
    static constexpr uint32_t kSrcMask = kSlots - 1, kNodeSrcShift = R == 1 ? 26 : 25, kNodeLevShift = kNodeSrcShift - 3;
    // The code that fills the queues relies on these minima (see push_pairs_any, drain_pairs and the tree walk):
    static_assert(Q::kPairQueue >= 128, "push_pairs_any publishes slices of up to 128 pairs");
    static_assert(!kPrefilter || Q::kFiltered >= 128, "the pre-filter appends up to 64 survivors to up to 63 waiting ones");
    static_assert(!kPrefilter || Q::kFiltered >= PT_BIG_EXACT_AT - 1 + 64, "up to PT_BIG_EXACT_AT - 1 pairs wait when 64 survivors are appended");
    static_assert(Q::kNodeStack >= 64, "a round pops up to 64 nodes");
    uint32_t filtered[Q::kFiltered];   // pairs that survived the pre-filter, waiting for a full exact round
    unsigned long long best[kSlots];   // per ray: (order-preserving bits of t) << 32 | triangle index; smaller is closer
    float ray[6][kSlots];          // this segment's rays, readable by every lane
    // big scenes: 1 / direction of every ray, taken once per segment instead of at every node visit (three quarter-rate v_rcp_f32
    // per visit, six visits per ray: +1.4 % / +0.9 % on the replicas, ab68)
    InvPlanes<kPrefilter ? kSlots : 0> rinv;
    uint32_t nodes[kNodeStack + 64];// LIFO of tree nodes to expand (layout above; the box tree: ray << 26 | node)
    uint32_t pairs[kPairQueue];    // (ray, triangle) work items
    uint32_t level_off[kMaxLevels];// sphere offset of each level of the cluster being walked
    uint32_t level_cnt[kMaxLevels];// number of real nodes of each level
    // The tile's accumulators (sum rgb, sum2 rgb, count as int bits) live here for the small-scene kernels with one ray per lane;
    // the two-rays-per-lane kernel and the big-scene kernels leave them in memory (integrate_kernel: "Where the tile's
    // accumulators live"): the LDS is worth a wave per SIMD to them.
    static constexpr bool kAccInLds = R == 1 && !kPrefilter;
    AccPlanes<kAccInLds ? kSlots : 0> acc;
    // adaptive-sampling instantiations of the two-pixel kernel: one 16-bit word per pixel of the tile (FLAGS per lane: pixel lane +
    // 64 j) -- the pixel's next pass << 1 | the cached "variance is low" answer (launches whose passes end beyond kMaxBatchPass
    // run the plain kernel); any lane may be the one that traces it, see "Batches" in integrate_kernel.  (16 bits: with 32-bit
    // words the 32 x 8 instantiation's 7 888 B of LDS round up to seven 1 280-byte granules and cost it its fifth wave per SIMD:
    // +13 % frame time, profiles/r04_ab_logs.txt adapt2)
    FlagWords<64 * FLAGS> low;
    // Shading reads the hit's record and then, through its material index, the material: two dependent loads.  The two-pixel
    // kernels take the second from a copy in LDS when the scene has at most kMatCache materials (Tor.obj: 5): +0.8 % (256 spp:
    // 73.2 -> 72.6 ms; with adaptive sampling +1.3 %); the box-tree kernel gains nothing from it (ab64) and does without.
    static constexpr int kMatCache = (R == 2 && !kPrefilter) ? PT_MATS_IN_LDS : 0;
    MatCache<kMatCache> mat;
};
struct WaveStats {
    uint32_t n_exact = 0, w_segments = 0, w_node_rounds = 0, w_exact_iters = 0, w_partial = 0;   // wave-uniform, live in SGPRs
#ifdef PT_VERIFY_BRUTE
    uint32_t v_checked = 0, v_bad = 0;   // verification build: segments compared with the brute-force loop / differing
#endif
#ifdef PT_PHASE_TIMERS
    // diagnostic build only: shader-clock cycles per phase (never compiled into the shipped library)
    unsigned long long phase[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long last = 0;
#endif
};
// Launches that do not ask for pt_render_stats run an instantiation without any of the counters (they cost ~3 %:
// nine more wave-uniform values alive across the whole kernel push the scalar register file into spilling).
struct Ignored {
    __host__ __device__ Ignored() {}
    __host__ __device__ Ignored(uint32_t) {}
    template <class T> __host__ __device__ Ignored &operator+=(T) { return *this; }
    __host__ __device__ Ignored &operator++() { return *this; }
};
struct NoStats {
    Ignored n_exact, w_segments, w_node_rounds, w_exact_iters, w_partial;
#ifdef PT_VERIFY_BRUTE
    Ignored v_checked, v_bad;   // keeps the verification build compiling; it always launches the STATS instantiations
#endif
#ifdef PT_PHASE_TIMERS
    unsigned long long phase[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = 0;   // keeps the diagnostic build compiling; never launched there
#endif
};
#ifdef PT_PHASE_TIMERS
#define PT_STAMP(st, idx)                                              \
    do {                                                               \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();  \
        (st).phase[idx] += now_ - (st).last;                           \
        (st).last = now_;                                              \
    } while (0)
#else
#define PT_STAMP(st, idx) do { } while (0)
#endif

constexpr uint32_t kUnfiltered = 128u;  // added to the ray id of a pair (bit 31 of the work item): the pre-filter must not judge it

// float -> uint32 whose unsigned order is the float order (for ds_min_u64 keys)
__device__ __forceinline__ uint32_t ordered_bits(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(uint32_t b) {
    return __uint_as_float(b ^ ((b >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
// hides a value from loop-invariant code motion (see the accumulator addresses and the camera ray)
__device__ __forceinline__ uint32_t opaque(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}
// number of set bits of `mask` below this lane
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}


// ---------------------------------------------------------------------------------------------------------------
// Box tree of big scenes (pt_scene.hpp: BvhNode): which of a node's (up to 8) children can hold a hit of ray r that
// beats t_best?  Slab test against the 8-bit child boxes, dequantised on the fly: along axis x the planes of child c are
// t = (org.x + q step - o.x) / d.x = A q + B with A = step / d.x, B = (org.x - o.x) / d.x, one fma per plane.
// CONSERVATIVE: every computed t is within E = err (|B| + 255 |A|) of its exact value (rcp 1 ulp, one product, the
// subtraction of the allowance, one fma: < 3.6e-7 relative to the operands' magnitudes; err = 5e-7), the boxes were
// rounded outward on the host, and a child is dropped only if its interval misses [0, t_best] by more than 2E.  A direction
// component of exactly zero (or too small for its reciprocal) makes A and B infinite: the allowance becomes infinite, every entry
// plane -inf or NaN, and every child of the node is kept (max / min skip NaNs, the final comparison is written so that a NaN keeps)
// -- conservative, and rare enough (no camera ray, no sampled direction has an exactly zero component) not to be worth the nine
// instructions per node that clamping the component to 1e-30 cost.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float byte_to_float(uint32_t w, int k) { return static_cast<float>((w >> (8 * k)) & 0xFFu); }   // v_cvt_f32_ubyteK
// PER = 8: all children of the node.  PER = 4, 2, 1: the node's children are spread over 2, 4, 8 lanes (under-filled rounds) and
// this lane tests children sub * PER ... sub * PER + PER - 1; the result has its bits at those positions.
template <int PER = 8>
__device__ __forceinline__ uint32_t box_children_kept(const uint4 q0, const uint4 q1, const uint4 q2, const uint4 q3, const Ray &r,
                                                      float ix, float iy, float iz, float t_best, float err, uint32_t sub = 0) {
    // ix, iy, iz = v_rcp_f32 of the ray's direction components (the caller holds them per ray)
    const float step = __uint_as_float((q0.w & 0xFFu) << 23);
    const float ax = step * ix, ay = step * iy, az = step * iz;
    const float bx = (__uint_as_float(q0.x) - r.ox) * ix, by = (__uint_as_float(q0.y) - r.oy) * iy, bz = (__uint_as_float(q0.z) - r.oz) * iz;
    const float bmax = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(bx), __builtin_fabsf(by)), __builtin_fabsf(bz));
    const float amax = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(ax), __builtin_fabsf(ay)), __builtin_fabsf(az));
    const float e2 = 2.0f * err * __builtin_fmaf(255.0f, amax, bmax);
    // The allowance goes into the ENTRY planes once per node (entry - 2E against exit) instead of into every comparison.
    const float nbx = bx - e2, nby = by - e2, nbz = bz - e2, t_min = -e2;
    // The ray enters a slab through its lower plane if it travels upwards along that axis, else through the upper one:
    // pick the byte rows of the entry (n) and exit (f) planes once per node.  q -> fma(A, q, B) is monotone, so
    // entry <= exit per axis holds in float arithmetic too.
    const bool sx = ix < 0.0f, sy = iy < 0.0f, sz = iz < 0.0f;
    uint32_t nx0 = sx ? q2.z : q1.x, nx1 = sx ? q2.w : q1.y, fx0 = sx ? q1.x : q2.z, fx1 = sx ? q1.y : q2.w;
    uint32_t ny0 = sy ? q3.x : q1.z, ny1 = sy ? q3.y : q1.w, fy0 = sy ? q1.z : q3.x, fy1 = sy ? q1.w : q3.y;
    uint32_t nz0 = sz ? q3.z : q2.x, nz1 = sz ? q3.w : q2.y, fz0 = sz ? q2.x : q3.z, fz1 = sz ? q2.y : q3.w;
    if constexpr (PER < 8) {
        // this lane's children sit in one word per row (children 0-3 in the first, 4-7 in the second), from byte (sub * PER) & 3 on:
        // bring them to byte 0 of the "first" words, so that the byte indices below stay compile-time constants
        const uint32_t c0 = sub * PER;
        const bool up = c0 >= 4u;
        const uint32_t sh = 8u * (c0 & 3u);
        nx0 = (up ? nx1 : nx0) >> sh; fx0 = (up ? fx1 : fx0) >> sh;
        ny0 = (up ? ny1 : ny0) >> sh; fy0 = (up ? fy1 : fy0) >> sh;
        nz0 = (up ? nz1 : nz0) >> sh; fz0 = (up ? fz1 : fz0) >> sh;
    }
    uint32_t m = 0;
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const int k = c & 3;
        const bool up = c >= 4;
        const float tnx = __builtin_fmaf(ax, byte_to_float(up ? nx1 : nx0, k), nbx), tfx = __builtin_fmaf(ax, byte_to_float(up ? fx1 : fx0, k), bx);
        const float tny = __builtin_fmaf(ay, byte_to_float(up ? ny1 : ny0, k), nby), tfy = __builtin_fmaf(ay, byte_to_float(up ? fy1 : fy0, k), by);
        const float tnz = __builtin_fmaf(az, byte_to_float(up ? nz1 : nz0, k), nbz), tfz = __builtin_fmaf(az, byte_to_float(up ? fz1 : fz0, k), bz);
        const float t_in = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), __builtin_fmaxf(tnz, t_min));
        const float t_out = __builtin_fminf(__builtin_fminf(tfx, tfy), __builtin_fminf(tfz, t_best));
        m |= !(t_in > t_out) ? (1u << c) : 0u;   // a NaN keeps
        // One child at a time.  Left alone, the compiler interleaves the eight children's conversions, multiply-adds and
        // comparisons into one long schedule; a scheduling barrier after every child -- the same instructions, 222 per node visit,
        // the same registers -- makes the x64 / x195 replicas 3.8 % / 2.9 % faster (2 152 -> 2 234, 1 447 -> 1 492 Msamples/s;
        // after 2 or 4 children: +0.9 % / 0; r04_ab_logs.txt sched).  Nothing else in the kernels reacted to such barriers.
        if ((c + 1) % PT_BOX_SCHED == 0) __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (PER < 8) m <<= sub * PER;
    return m;
}

// Scene::TraceRay's triangle loop exactly as the reference runs it (scene.cpp:116-120): every triangle, in index order,
// through Triangle::Intersect for this lane's ray; returns the closest-hit key (~0 = miss).  Wave-uniform control flow.
// Only the verification build calls it.
__device__ __forceinline__ unsigned long long brute_force_key(const RenderArgs &a, const Ray &q, float eps) {
    unsigned long long best = ~0ull;
    for (int i = 0; i < a.n_tri; ++i) {
        uint32_t orig;
        const float nd = exact_inside(a.exact + i, q, eps, orig);
        if (nd >= eps && nd < __builtin_inff()) {
            const unsigned long long k = (static_cast<unsigned long long>(ordered_bits(nd)) << 32) | static_cast<uint32_t>(i);
            best = k < best ? k : best;
        }
    }
    return best;
}

// emis_flag (wave-uniform, honoured only by instantiations with EMIS): search only where emitters are (RenderArgs::emis_*) --
// the closest hit among a SUPERSET of the emitters, which is all the caller needs to know whether the ray's closest hit can be
// one (see the last segment in the kernel).
// DYN (the adaptive-sampling instantiation of the two-rays-per-lane kernel): `two` (wave-uniform) says whether any lane's second
// ray slot is in use this pass; when it is not, everything per-ray about slot 1 is skipped by scalar branches and the segment
// costs about what a one-ray-per-lane segment costs (PT_SLOT_ON).  Without DYN the guards fold away.
// ROOM (the room instantiations of the statistics-free plain small-scene kernel, launched only for scenes whose tables say
// CullTables::room, pt_scene.hpp): the cull stage is one straight sequence -- the single all-quad word of the large class, then the
// one sphere-tree cluster if there is one -- instead of the loops over clusters, class words and record kinds.  The same tests on the
// same records, so the same candidates; only wave-uniform control flow and the scalar registers that carried it are gone.
#define PT_SLOT_ON(k) ((k) == 0 || k1_on)
template <bool ENV, bool EMIS, bool DYN = false, bool ROOM = false, class Lds, class Stats>
__device__ __forceinline__ void closest_hit(const RenderArgs &a, Lds &lds, const Ray (&q)[Lds::kRays], const bool (&live)[Lds::kRays],
                                            const bool (&in_envelope)[Lds::kRays], int lane, float eps, float (&best)[Lds::kRays],
                                            int (&hit)[Lds::kRays], const ExactRec *(&hit_rec)[Lds::kRays], Stats &st, bool emis_flag = false,
                                            bool two = true) {
    constexpr int R = Lds::kRays;   // rays per lane: ray k of lane l has the id l + 64 k
    const bool emis_only = EMIS && emis_flag;
    const bool k1_on = !DYN || two;   // (slot 1 of a lane is never live when `two` is false: the guards only save its instructions)
    // `valid` below = rays that go through the culling hierarchy; live rays outside the envelope its margins were derived
    // for get every slot as a candidate instead (rare: see the caller).
    bool valid[R];
#pragma unroll
    for (int k = 0; k < R; ++k) valid[k] = live[k] && in_envelope[k];
    auto any_ray = [&](const bool (&b)[R]) {   // wave-uniform: does any ray of the wave-segment have the flag?
        bool x = b[0];
#pragma unroll
        for (int k = 1; k < R; ++k) x = x || b[k];
        return __any(x);
    };
    constexpr uint32_t kNodeStack = Lds::kNodeStack, kPairQueue = Lds::kPairQueue;
    // Small scenes (CullTables::big == false: at most kSmallSceneMaxTriangles triangles and slots, so 16 bits each): the closest-hit key carries the SLOT
    // below the original index, and shading reads the slot-ordered record the exact test has just pulled through the
    // caches.  Big scenes look the hit up in the table kept in the original order.
    constexpr bool kPackSlot = !Lds::kPrefilter;
    static_assert(kSmallSceneMaxTriangles < 32768, "packed (original index, slot) key: 16 bits each, slots padded to at most twice the triangles");
    ++st.w_segments;
    PT_STAMP(st, 0);   // everything since the last stamp: ray generation / loop control
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (!PT_SLOT_ON(k)) continue;
        const int id = lane + 64 * k;
        lds.best[id] = ~0ull;
        lds.ray[0][id] = q[k].ox; lds.ray[1][id] = q[k].oy; lds.ray[2][id] = q[k].oz;
        lds.ray[3][id] = q[k].dx; lds.ray[4][id] = q[k].dy; lds.ray[5][id] = q[k].dz;
        if constexpr (Lds::kPrefilter) {
            lds.rinv.v[0][id] = __builtin_amdgcn_rcpf(q[k].dx); lds.rinv.v[1][id] = __builtin_amdgcn_rcpf(q[k].dy); lds.rinv.v[2][id] = __builtin_amdgcn_rcpf(q[k].dz);
        }
    }
    uint32_t n_pairs = 0;   // wave-uniform fill level of lds.pairs
    wave_sync();

    // ---- 2. exact.  (ray, triangle) pairs are spread evenly over the lanes (a lane works on other lanes' rays).
    // The reference keeps, in triangle order, every accepted triangle with new_distance < distance
    // (scene.cpp:116-120, triangles.h:51), i.e. the lexicographic minimum of (new_distance, index) over the triangles
    // that pass Triangle::Intersect with eps <= new_distance < inf: that minimum is taken with one LDS atomic per pair.
    uint32_t n_filtered = 0;   // wave-uniform fill level of lds.filtered (big scenes)
    auto exact_round = [&](uint32_t e, bool active, uint32_t cnt) {
        ++st.w_exact_iters;
        st.n_exact += cnt;
        if (active) {
            const uint32_t src = (e >> 24) & Lds::kSrcMask, tri = e & 0xFFFFFFu;
            Ray r;
            r.ox = lds.ray[0][src]; r.oy = lds.ray[1][src]; r.oz = lds.ray[2][src];
            r.dx = lds.ray[3][src]; r.dy = lds.ray[4][src]; r.dz = lds.ray[5][src];
            uint32_t orig;   // the pair names a SLOT; the closest-hit key carries the original triangle index (tie-break)
            const float nd = exact_inside(a.exact_slot + tri, r, eps, orig);   // -inf unless stages B-D pass
            if (nd >= eps && nd < __builtin_inff())
                atomicMin(&lds.best[src], (static_cast<unsigned long long>(ordered_bits(nd)) << 32) | (kPackSlot ? (orig << 16) | tri : orig));
        }
    };
    auto drain_pairs = [&](uint32_t keep_below) {
        while (n_pairs > keep_below) {
            const uint32_t cnt = min(64u, n_pairs);
            n_pairs -= cnt;
            const bool active = static_cast<uint32_t>(lane) < cnt;
            const uint32_t e = active ? lds.pairs[n_pairs + lane] : 0u;
            if constexpr (!Lds::kPrefilter) {
                exact_round(e, active, cnt);
            } else {
                // A scene with thousands of small triangles yields ~8 sphere survivors per ray; the 30-instruction
                // barycentric test (conservative, like every cull) removes most of them before the 170-instruction exact
                // test, and the survivors are re-packed so that exact rounds stay full.
                bool keep = false;
                if (active) {
                    const uint32_t src = (e >> 24) & Lds::kSrcMask, tri = e & 0xFFFFFFu;
                    Ray r;
                    r.ox = lds.ray[0][src]; r.oy = lds.ray[1][src]; r.oz = lds.ray[2][src];
                    r.dx = lds.ray[3][src]; r.dy = lds.ray[4][src]; r.dz = lds.ray[5][src];
                    const float4 *rp = reinterpret_cast<const float4 *>(a.bary_all + tri);
                    const float4 c0 = rp[0], c1 = rp[1], c2 = rp[2];
                    CullRec rec;
                    rec.n[0] = c0.x; rec.n[1] = c0.y; rec.n[2] = c0.z; rec.w = c0.w;
                    rec.au[0] = c1.x; rec.au[1] = c1.y; rec.au[2] = c1.z; rec.cu = c1.w;
                    rec.av[0] = c2.x; rec.av[1] = c2.y; rec.av[2] = c2.z; rec.cv = c2.w;
                    keep = !cull_reject(rec, r, a.k1, a.k2, a.a_max_all, a.m0_all, a.t_guard_all) || (e >> 31) != 0u;   // bit 31: never filtered
                }
                const unsigned long long ball = __ballot(keep);
                if (keep) lds.filtered[n_filtered + lanes_below(ball)] = e;
                n_filtered += __builtin_popcountll(ball);
                wave_sync();
                if (n_filtered >= static_cast<uint32_t>(PT_BIG_EXACT_AT)) {
                    const uint32_t take = min(64u, n_filtered);
                    n_filtered -= take;
                    const bool on = static_cast<uint32_t>(lane) < take;
                    exact_round(on ? lds.filtered[n_filtered + lane] : 0u, on, take);
                    wave_sync();
                }
            }
            wave_sync();
        }
    };
    // Append one pair per set bit of `bits[k]` (bit j = triangle tri0 + j of this lane's ray k): a prefix sum over the lanes'
    // counts gives every lane its place in the queue (and the total).  `flag` is or-ed into the ray id (kUnfiltered).
    auto emit_lane_pairs = [&](const uint32_t (&bits)[R], uint32_t tri0, uint32_t flag, uint32_t excl, uint32_t total) {
        uint32_t pos = n_pairs + excl;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (!PT_SLOT_ON(k)) continue;
            emit_bits(lds.pairs, pos, bits[k], tri0 | ((static_cast<uint32_t>(lane + 64 * k) | flag) << 24));
            pos += __builtin_popcount(bits[k]);
        }
        n_pairs += total;
        wave_sync();
    };
    // the same for entries of other lanes' rays (root round): one mask per lane, ray id `src`
    auto emit_pairs = [&](uint32_t bits, uint32_t tri0, uint32_t src, uint32_t excl, uint32_t total) {
        emit_bits(lds.pairs, n_pairs + excl, bits, tri0 | (src << 24));
        n_pairs += total;
        wave_sync();
    };
    // for masks of any width: makes room first, and slices the masks if one batch could exceed the queue
    auto push_pairs_any = [&](const uint32_t (&bits)[R], uint32_t tri0, uint32_t flag) {
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (PT_SLOT_ON(k)) cnt += __builtin_popcount(bits[k]);
        const uint32_t incl = wave_scan_inclusive(cnt), total = wave_last(incl);
        if (total == 0) return;
        if (n_pairs + total > kPairQueue) drain_pairs(0);
        if (total <= kPairQueue) {
            emit_lane_pairs(bits, tri0, flag, incl - cnt, total);
            return;
        }
        constexpr uint32_t kSlice = 2u / R;   // bits of every ray's mask per slice: <= 128 pairs
        for (uint32_t lo = 0; lo < 32u; lo += kSlice) {
            uint32_t part[R], pc2 = 0;
            bool some = false;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                part[k] = PT_SLOT_ON(k) ? bits[k] & (((1u << kSlice) - 1u) << lo) : 0u;
                pc2 += __builtin_popcount(part[k]);
                some = some || part[k] != 0;
            }
            if (!__any(some)) continue;
            if (n_pairs + 128u > kPairQueue) drain_pairs(0);
            const uint32_t in2 = wave_scan_inclusive(pc2);
            emit_lane_pairs(part, tri0, flag, in2 - pc2, wave_last(in2));
        }
    };

    // Candidate masks of runs that need no tree walk (large-triangle words, runs of at most 8 small triangles) are
    // collected in a window of 32 consecutive triangle indices and published together: adjacent short runs (the walls
    // and the light of a room, split by the file order into three clusters) then cost one publication, not three.
    uint32_t pend[R], pend_tri0 = 0;    // per-ray bits; wave-uniform window start
#pragma unroll
    for (int k = 0; k < R; ++k) pend[k] = 0;
    bool pend_open = false;             // wave-uniform
    auto flush_pending = [&]() {
        if (pend_open) push_pairs_any(pend, pend_tri0, 0u);
#pragma unroll
        for (int k = 0; k < R; ++k) pend[k] = 0;
        pend_open = false;
    };
    auto add_pending = [&](const uint32_t (&bits)[R], uint32_t tri0, uint32_t width) {   // tri0, width wave-uniform
        if (pend_open && tri0 >= pend_tri0 && tri0 + width <= pend_tri0 + 32u) {
#pragma unroll
            for (int k = 0; k < R; ++k)
                if (PT_SLOT_ON(k)) pend[k] |= bits[k] << (tri0 - pend_tri0);
        } else {
            flush_pending();
#pragma unroll
            for (int k = 0; k < R; ++k) pend[k] = PT_SLOT_ON(k) ? bits[k] : 0u;
            pend_tri0 = tri0;
            pend_open = true;
        }
    };

    // ---- 0. rays outside the envelope: all slots are candidates (padding slots carry NaN planes and are never accepted);
    // their pairs carry bit 30 = "skip the barycentric pre-filter", whose margins assume the envelope as well
    if constexpr (ENV) {
        bool far[R];
#pragma unroll
        for (int k = 0; k < R; ++k) far[k] = live[k] && !in_envelope[k];
        if (__builtin_expect(any_ray(far), 0)) {
            for (uint32_t base = 0; base < a.n_slots; base += 32u) {
                const uint32_t left = a.n_slots - base;
                const uint32_t all = left >= 32u ? 0xFFFFFFFFu : ((1u << left) - 1u);
                uint32_t bits[R];
#pragma unroll
                for (int k = 0; k < R; ++k) bits[k] = far[k] ? all : 0u;
                push_pairs_any(bits, base, Lds::kPrefilter ? kUnfiltered : 0u);
            }
        }
    }

    // ---- 1. cull
    const ConstF clusters = (ConstF)reinterpret_cast<uintptr_t>(a.clusters);
    const ConstF spheres = (ConstF)reinterpret_cast<uintptr_t>(a.spheres);
    const ConstF bary = (ConstF)reinterpret_cast<uintptr_t>(a.bary);
    constexpr int kDescWords = sizeof(ClusterDesc) / 4;
    if constexpr (ROOM) {
        static_assert(EMIS && !ENV && !DYN && !Lds::kPrefilter, "the room instantiations are forms of the statistics-free plain small-scene kernel");
        {
            // ---- the large class: the LAST cluster (the table builder appends it after the sphere trees), one word of quad records.
            // Its records are whole quads, so the class has an even number of slots and every bit a record sets is a real triangle's:
            // no mask for a ragged end.
            const ConstF cp = clusters + kDescWords * (a.n_clusters - 1);
            const uint32_t first_tri = ((ConstU)cp)[4], n_tri = ((ConstU)cp)[5], off = ((ConstU)cp)[7];
            float k1 = a.k1, k2 = a.k2, a_max = a.a_max, m0q = a.m0_quad, t_guard = a.t_guard;   // (in VGPRs: see the generic loop)
            asm volatile("" : "+v"(k1), "+v"(k2), "+v"(a_max), "+v"(m0q), "+v"(t_guard));
            const ConstF bp = bary + 12 * static_cast<size_t>(off);
            uint32_t m[R];
#pragma unroll
            for (int k = 0; k < R; ++k) m[k] = 0;
            auto quad = [&](uint32_t k0) {
                const CullRec rec = load_cull(bp + 12 * k0);
#pragma unroll
                for (int k = 0; k < R; ++k) m[k] |= (~cull_reject_quad(rec, q[k], k1, k2, a_max, m0q, t_guard) & 3u) << k0;
            };
            if (emis_only) {   // only the records that hold an emitter (the light of a room: one quad)
                for (uint32_t rest = (a.emis_large_w0 | (a.emis_large_w0 >> 1)) & 0x55555555u; rest != 0; rest &= rest - 1) quad(__builtin_ctz(rest));
#pragma unroll
                for (int k = 0; k < R; ++k) m[k] &= a.emis_large_w0;
            } else {
                for (uint32_t k0 = 0; k0 < n_tri; k0 += 2) quad(k0);
            }
#pragma unroll
            for (int k = 0; k < R; ++k) m[k] = valid[k] ? m[k] : 0u;
            add_pending(m, first_tri, n_tri);
            flush_pending();   // (published now: the window's masks would be held in vector registers across the walk below)
        }
        // ---- the one sphere-tree cluster, if the room has an object in it: cluster 0
        if (a.n_clusters > 1 && !(emis_only && !(a.emis_clusters & 1u))) {
            constexpr int cl = 0;
            const ConstF cp = clusters;
            const uint32_t first_tri = ((ConstU)cp)[4], n_tri = ((ConstU)cp)[5], off = ((ConstU)cp)[7];
            bool pc[R];
#pragma unroll
            for (int k = 0; k < R; ++k) pc[k] = valid[k] & sphere_keep(cp[0], cp[1], cp[2], cp[3], q[k]);
            if (any_ray(pc)) {
#include "pt_sphere_tree_walk.inc"
            }
        }
    } else
    for (int cl = 0; cl < a.n_clusters; ++cl) {
        const ConstF cp = clusters + kDescWords * cl;
        if (emis_only && cl < 32 && !((a.emis_clusters >> cl) & 1u)) continue;   // no emitter in this cluster
        const uint32_t first_tri = ((ConstU)cp)[4], n_tri = ((ConstU)cp)[5], kind = ((ConstU)cp)[6], off = ((ConstU)cp)[7];
        // (the large class is tested triangle by triangle anyway, and its bounding sphere is the scene's: nothing to gain from it)
        // (big scenes have no sphere-tree clusters -- all their small triangles sit under the box tree, pt_scene.cpp --: their
        // instantiations leave that code out, which spares them its registers)
        constexpr bool kSphereTrees = !Lds::kPrefilter;
        if (!kSphereTrees && kind == 0) continue;
        bool pc[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            pc[k] = false;
            if (PT_SLOT_ON(k)) pc[k] = (kSphereTrees && kind == 0) ? valid[k] & sphere_keep(cp[0], cp[1], cp[2], cp[3], q[k]) : valid[k];
        }
        if (!any_ray(pc)) continue;
        if (kSphereTrees && kind == 0) {
#include "pt_sphere_tree_walk.inc"
        } else {
            // ---- large triangles: barycentric cull, wave-uniform over the triangles.
            // The margins go to VGPRs here: a VALU instruction can name only one SGPR, so an SGPR-resident
            // constant next to an SGPR-resident triangle coefficient would cost a v_mov per use.
            float k1 = a.k1, k2 = a.k2, a_max = a.a_max, m0 = a.m0, m0q = a.m0_quad, t_guard = a.t_guard;
            asm volatile("" : "+v"(k1), "+v"(k2), "+v"(a_max), "+v"(m0), "+v"(m0q), "+v"(t_guard));
            const int n_words = static_cast<int>((n_tri + kChunk - 1) / kChunk);
            for (int w = 0; w < n_words; ++w) {
                const uint32_t left = n_tri - kChunk * w;
                const ConstF bp = bary + 12 * (static_cast<size_t>(off) + kChunk * w);
                const uint32_t quads = w < kMaxLevels - 1 ? ((ConstU)cp)[9 + w] : 0u;   // bit k: slots k, k+1 are one quad record
                uint32_t m[R];
#pragma unroll
                for (int k = 0; k < R; ++k) m[k] = 0;
                const uint32_t cnt32 = min(left, 32u);
                const uint32_t pair_bits = 0x55555555u & (cnt32 >= 32u ? 0xFFFFFFFFu : ((1u << cnt32) - 1u));
                // one record (wave-uniform, in scalar registers) against this lane's R rays
                auto quad = [&](uint32_t k0) {
                    const CullRec rec = load_cull(bp + 12 * k0);
#pragma unroll
                    for (int k = 0; k < R; ++k)
                        if (PT_SLOT_ON(k)) m[k] |= (~cull_reject_quad(rec, q[k], k1, k2, a_max, m0q, t_guard) & 3u) << k0;
                };
                auto single = [&](uint32_t slot) {
                    const CullRec rec = load_cull(bp + 12 * slot);
#pragma unroll
                    for (int k = 0; k < R; ++k)
                        if (PT_SLOT_ON(k)) m[k] |= cull_reject(rec, q[k], k1, k2, a_max, m0, t_guard) ? 0u : (1u << slot);
                };
                if (emis_only && n_words == 1) {   // only the records that hold an emitter (the light of a room: one quad)
                    for (uint32_t rest = (a.emis_large_w0 | (a.emis_large_w0 >> 1)) & pair_bits; rest != 0; rest &= rest - 1) {
                        const uint32_t k0 = __builtin_ctz(rest);
                        if ((quads >> k0) & 1u) {
                            quad(k0);
                        } else {
                            single(k0);
                            single(k0 + 1);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < R; ++k) m[k] &= a.emis_large_w0;
                } else
                if (quads == pair_bits) {   // every record of the word is a quad (the walls of a room): no per-record dispatch
                    // Big scenes take the records two at a time -- both records' scalar loads named before the first one's
                    // arithmetic.  The compiler still waits per record, but this form leaves the box-tree kernel with 31 instead of
                    // 37 spilled scalar registers: +1.7 % on the x64 replica (ab58).  For the small-scene kernels it changes nothing
                    // in pairs and costs 5 % in fours (spills).  The table is padded by more than a record: the load past an odd
                    // class's end is harmless.
                    constexpr int kWallGroup = Lds::kPrefilter ? 2 : 1;
                    if constexpr (kWallGroup > 1) {
                        for (uint32_t k0 = 0; k0 < cnt32; k0 += 2 * kWallGroup) {
                            CullRec r[kWallGroup];
#pragma unroll
                            for (int g = 0; g < kWallGroup; ++g) r[g] = load_cull(bp + 12 * (k0 + 2 * g));
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int g = 0; g < kWallGroup; ++g) {
                                if (k0 + 2 * g < cnt32) {
#pragma unroll
                                    for (int k = 0; k < R; ++k) m[k] |= (~cull_reject_quad(r[g], q[k], k1, k2, a_max, m0q, t_guard) & 3u) << (k0 + 2 * g);
                                }
                            }
                        }
                    } else {
                        for (uint32_t k0 = 0; k0 < cnt32; k0 += 2) quad(k0);
                    }
                } else
                for (uint32_t k0 = 0; k0 < cnt32; k0 += 2) {   // records are padded to whole words
                    if ((quads >> k0) & 1u) {   // wave-uniform
                        quad(k0);
                    } else {
                        single(k0);
                        single(k0 + 1);
                    }
                }
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    m[k] = pc[k] ? m[k] : 0u;
                    m[k] &= left >= 32u ? 0xFFFFFFFFu : ((1u << left) - 1u);
                }
                PT_STAMP(st, 3);   // barycentric cull of the large triangles
                add_pending(m, first_tri + kChunk * w, min(left, 32u));
                PT_STAMP(st, 4);   // pair publication
            }
        }
    }
    PT_STAMP(st, 1);
    if constexpr (Lds::kPrefilter) {
        // ---- big scenes: ONE box tree over all small triangles, walked with the wave-wide LIFO of (ray, node) items.
        // The large class above went first and is tested right away, so that lds.best already holds a hit (the wall behind
        // everything, in a closed room) when the walk starts: a node whose box the ray enters beyond its best hit so far is
        // dropped, and because pairs are tested as soon as 64 are waiting, closer hits keep shrinking the rest of the walk.
        if (a.n_bvh > 0 && !(emis_only && a.emis_bvh == 0u)) {
            flush_pending();
            drain_pairs(0);
            if (n_filtered > 0) {
                const bool active = static_cast<uint32_t>(lane) < n_filtered;
                exact_round(active ? lds.filtered[lane] : 0u, active, n_filtered);
                n_filtered = 0;
                wave_sync();
            }
            uint32_t n_nodes;
            {
                n_nodes = 0;
#pragma unroll
                for (int k = 0; k < R; ++k) {   // the root, for every live ray
                    const unsigned long long vb = __ballot(valid[k]);
                    if (valid[k]) lds.nodes[n_nodes + lanes_below(vb)] = static_cast<uint32_t>(lane + 64 * k) << Lds::kNodeSrcShift;
                    n_nodes += __builtin_popcountll(vb);
                }
                wave_sync();
            }
            while (n_nodes > 0) {
                ++st.w_node_rounds;
                const uint32_t cnt = min(64u, n_nodes);
                // One lane per item: shift is always 0.  (Spreading the items of an under-filled round -- the tail of every walk: 1.3 of
                // the x64 replica's 9.1 rounds per wave-segment hold at most 32 -- over 2, 4 or 8 lanes each, like the sphere-tree walk,
                // was measured at +-0 on the x64 replica and -1 % on x195: those rounds wait for their node loads, not for issue slots;
                // r03_ab_logs.txt ab62.  The switch is gone; the walk keeps the shape the compiler was given then, because any other
                // spelling of it moved the code of the box-tree kernels, profiles/r07_kernel_cleanup.txt.)
                uint32_t shift = 0u;
                uint32_t m8, src, base, kids, keep, packed, incl, tot;
                bool leaf;
                for (;;) {
                m8 = 0; src = 0; base = 0;
                leaf = false;
                const uint32_t item = static_cast<uint32_t>(lane) >> shift, sub = static_cast<uint32_t>(lane) & ((1u << shift) - 1u);
                if (item < cnt) {
                    const uint32_t e = lds.nodes[n_nodes - 1 - item];
                    src = e >> Lds::kNodeSrcShift;
                    const uint32_t node = e & ((1u << Lds::kNodeSrcShift) - 1u);
                    Ray r;
                    r.ox = lds.ray[0][src]; r.oy = lds.ray[1][src]; r.oz = lds.ray[2][src];
                    r.dx = lds.ray[3][src]; r.dy = lds.ray[4][src]; r.dz = lds.ray[5][src];
                    const uint32_t bh = reinterpret_cast<const uint32_t *>(&lds.best[src])[1];   // high word: ordered bits of t
                    const float t_best = bh == 0xFFFFFFFFu ? __builtin_inff() : from_ordered_bits(bh);
                    const uint4 *np = reinterpret_cast<const uint4 *>(a.bvh + node);
                    const uint4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
                    const float ix = lds.rinv.v[0][src], iy = lds.rinv.v[1][src], iz = lds.rinv.v[2][src];
                    if (shift == 0u) m8 = box_children_kept<8>(q0, q1, q2, q3, r, ix, iy, iz, t_best, a.bvh_err);
                    else if (shift == 1u) m8 = box_children_kept<4>(q0, q1, q2, q3, r, ix, iy, iz, t_best, a.bvh_err, sub);
                    else if (shift == 2u) m8 = box_children_kept<2>(q0, q1, q2, q3, r, ix, iy, iz, t_best, a.bvh_err, sub);
                    else m8 = box_children_kept<1>(q0, q1, q2, q3, r, ix, iy, iz, t_best, a.bvh_err, sub);
                    m8 &= (2u << ((q0.w >> 8) & 7u)) - 1u;   // children that exist
                    leaf = ((q0.w >> 11) & 1u) != 0u;                       // BvhNode::meta
                    base = leaf ? (q0.w >> 12) * kFan : (q0.w >> 12);      // a leaf's first slot / an inner node's first child
                }
                kids = __builtin_popcount(m8);
                keep = cnt;
                // Children of inner nodes go back on the stack, triangles of leaves into the pair queue.  One prefix sum serves both
                // (inner lanes count in the low half of the word, leaf lanes in the high half): its last lane says whether everything
                // fits, its other lanes where each lane's entries go.
                packed = leaf ? kids << 16 : kids;
                incl = wave_scan_inclusive(packed);
                tot = wave_last(incl);
                if (n_pairs + (tot >> 16) > kPairQueue) drain_pairs(0);
                if (n_pairs + (tot >> 16) <= kPairQueue && n_nodes - cnt + (tot & 0xFFFFu) <= kNodeStack) break;
                if (shift != 0u) { shift = 0u; continue; }   // rare: redo the round one lane per item
                {
                    // Rare: not everything fits.  Commit the longest prefix of lanes (= the top of the stack) whose children do;
                    // the top item always commits (its children are one level deeper; the 64 slots of slack absorb them).
                    const bool fits = static_cast<uint32_t>(lane) < cnt && n_pairs + (incl >> 16) <= kPairQueue &&
                                      (n_nodes - (lane + 1)) + (incl & 0xFFFFu) <= kNodeStack;
                    const unsigned long long fb = __ballot(fits);
                    keep = (fb == ~0ull) ? 64u : static_cast<uint32_t>(__builtin_ctzll(~fb));
                    if (keep == 0) keep = 1;
                    ++st.w_partial;
                    if (static_cast<uint32_t>(lane) >= keep) m8 = 0;
                    kids = __builtin_popcount(m8);
                    packed = leaf ? kids << 16 : kids;
                    incl = wave_scan_inclusive(packed);
                    tot = wave_last(incl);
                }
                break;
                }
                n_nodes -= keep;
                wave_sync();   // every lane has read its item before the stack is written
                // (Measured and dropped: pushing the children of the far half of a node first, right-aligned over the push steps so
                // that the next round is the near front of all rays.  Pruning is already within 10 % of what knowing the final hit
                // from the start would give -- the walls are tested first and pairs as soon as 64 wait -- and the ordering's 25
                // instructions per round cost as much as it saved.)
                {
                    const uint32_t excl = incl - packed;
                    emit_bits(leaf ? lds.pairs : lds.nodes, leaf ? n_pairs + (excl >> 16) : n_nodes + (excl & 0xFFFFu), m8,
                              leaf ? (base | (src << 24)) : ((src << Lds::kNodeSrcShift) | base));
                    n_nodes += tot & 0xFFFFu;
                    n_pairs += tot >> 16;
                }
                wave_sync();
                PT_STAMP(st, 2);   // box-tree rounds
                if (n_pairs >= 64u) drain_pairs(63);
                PT_STAMP(st, 6);   // pre-filter + exact rounds inside the walk
            }
            PT_STAMP(st, 2);
        }
    }
    flush_pending();
    drain_pairs(0);
    if constexpr (Lds::kPrefilter) {
        if (n_filtered > 0) {
            const bool active = static_cast<uint32_t>(lane) < n_filtered;
            exact_round(active ? lds.filtered[lane] : 0u, active, n_filtered);
            n_filtered = 0;
            wave_sync();
        }
    }
    PT_STAMP(st, 5);   // exact rounds
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (!PT_SLOT_ON(k)) {   // (nobody's ray)
            hit[k] = -1;
            hit_rec[k] = a.exact;
            best[k] = __builtin_inff();
            continue;
        }
        const unsigned long long key = lds.best[lane + 64 * k];
        const uint32_t key_lo = static_cast<uint32_t>(key);
        hit[k] = (key == ~0ull) ? -1 : static_cast<int>(kPackSlot ? key_lo >> 16 : key_lo);
        hit_rec[k] = kPackSlot ? a.exact_slot + (key_lo & 0xFFFFu) : a.exact + key_lo;   // dereferenced only if hit >= 0
#ifdef PT_VERIFY_BRUTE
        // Verification build (libpt_verify.so, never the shipped library): Scene::TraceRay's loop as written -- every
        // triangle through Triangle::Intersect for this lane's own ray -- and a comparison of the two closest hits.
        {
            const unsigned long long brute = brute_force_key(a, q[k], eps);
            st.v_checked += static_cast<uint32_t>(__builtin_popcountll(__ballot(live[k])));
            const unsigned long long mine = (key == ~0ull) ? ~0ull : ((key & 0xFFFFFFFF00000000ull) | static_cast<uint32_t>(hit[k]));
            st.v_bad += static_cast<uint32_t>(__builtin_popcountll(__ballot(live[k] && brute != mine)));
            if (live[k] && brute != mine && a.stats) {   // one example for the host to print (any of them)
                a.stats[11] = brute;
                a.stats[12] = mine;
                a.stats[13] = (static_cast<unsigned long long>(__float_as_uint(q[k].ox)) << 32) | __float_as_uint(q[k].oy);
                a.stats[14] = (static_cast<unsigned long long>(__float_as_uint(q[k].oz)) << 32) | __float_as_uint(q[k].dx);
                a.stats[15] = (static_cast<unsigned long long>(__float_as_uint(q[k].dy)) << 32) | __float_as_uint(q[k].dz);
            }
        }
#endif
        best[k] = (key == ~0ull) ? __builtin_inff() : from_ordered_bits(static_cast<uint32_t>(key >> 32));
    }
    wave_sync();
}

// ---------------------------------------------------------------------------------------------------------------
// The kernel
// ---------------------------------------------------------------------------------------------------------------
// SKY = the scene has a skybox (scene.cpp:126-154).  A separate instantiation: the lookup's double arithmetic raises
// the register peak, and the no-skybox kernel (every BASELINE configuration) should not pay for it.
// BIG = deep work queues for scenes with thousands of triangles (see SmallQueues / BigQueues).
// STATS = the caller asked for pt_render_stats.
// ENV = some triangle of the scene can be "hit" outside the envelope the culling margins are derived for (near-degenerate
// triangles; CullTables::may_leave_envelope): every segment's origin is then checked.  A compile-time choice because the
// mere presence of the rare path costs the common scenes 2 % (measured), whether or not it ever runs.
#ifndef PT_RAYS_PER_LANE
#define PT_RAYS_PER_LANE 2   // pixels (rays) per lane of the small-scene, statistics-free, skybox-free kernel; 1 = one 8 x 8 tile per wave
#endif
constexpr int kMaxBatchPass = 32766;   // adaptive instantiations: a pixel's next pass (at most one past the launch's last) << 1 | a flag in 16 bits
#ifndef PT_ADAPT_TWO_AT
#define PT_ADAPT_TWO_AT 100   // adaptive kernels: pixels with a pass to run from which a batch takes up to 128, two per lane (80 ... 112 within 1 %, adapt3)
#endif
#ifndef PT_BIG_RAYS_PER_LANE
#define PT_BIG_RAYS_PER_LANE 1   // the same for the statistics-free, skybox-free big-scene kernel
#endif
// The camera of a camera-twin launch (RenderArgs::cam: origin, right, up, forward), read where a primary ray is made.  The
// address is made opaque there, so that the twelve scalar loads are not hoisted to the head of the kernel, where their
// registers would be held -- spilled -- for the whole launch (the kernel's only argument sits at the start of its kernarg segment).
using CameraView = const __attribute__((address_space(4))) float *;
__device__ __forceinline__ CameraView camera_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, cam);
    asm volatile("" : "+s"(p));
    return reinterpret_cast<CameraView>(p);
}
// The lens of a lens-kernel launch (RenderArgs::lns: radius, focus distance, r^, u^, f^), read the same way.
using LensView = const __attribute__((address_space(4))) float *;
__device__ __forceinline__ LensView lens_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, lns);
    asm volatile("" : "+s"(p));
    return reinterpret_cast<LensView>(p);
}
// The camera motion of a motion-twin launch (RenderArgs::cam_d: end pose - cam; RenderArgs::lns_d: the same for r^, u^, f^), likewise.
using MotionView = const __attribute__((address_space(4))) float *;
__device__ __forceinline__ MotionView camera_delta_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, cam_d);
    asm volatile("" : "+s"(p));
    return reinterpret_cast<MotionView>(p);
}
__device__ __forceinline__ MotionView lens_delta_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, lns_d);
    asm volatile("" : "+s"(p));
    return reinterpret_cast<MotionView>(p);
}
// The projection of a projection-kernel launch (RenderArgs::projection, prj_span), likewise; its r^, u^, f^ are lens_view() + 2.
struct ProjectionView {
    uint64_t p;
    __device__ __forceinline__ int32_t kind() const { return *reinterpret_cast<const __attribute__((address_space(4))) int32_t *>(p); }
    __device__ __forceinline__ const __attribute__((address_space(4))) float *span() const {
        return reinterpret_cast<const __attribute__((address_space(4))) float *>(p + (offsetof(RenderArgs, prj_span) - offsetof(RenderArgs, projection)));
    }
};
__device__ __forceinline__ ProjectionView projection_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, projection);
    asm volatile("" : "+s"(p));
    return {p};
}
// The environment of an environment-kernel launch (RenderArgs::env_map, env_n), likewise: read where a ray has missed.
struct EnvironmentView {
    uint64_t p;
    __device__ __forceinline__ const EnvTexel *map() const { return *reinterpret_cast<const EnvTexel *const __attribute__((address_space(4))) *>(p); }
    __device__ __forceinline__ int32_t n() const {
        return *reinterpret_cast<const __attribute__((address_space(4))) int32_t *>(p + (offsetof(RenderArgs, env_n) - offsetof(RenderArgs, env_map)));
    }
};
__device__ __forceinline__ EnvironmentView environment_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, env_map);
    asm volatile("" : "+s"(p));
    return {p};
}
// The dielectric table of a dielectric-kernel launch (RenderArgs::glass), likewise: read where a ray has hit a triangle.
__device__ __forceinline__ const GlassRec *glass_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, glass);
    asm volatile("" : "+s"(p));
    return *reinterpret_cast<const GlassRec *const __attribute__((address_space(4))) *>(p);
}
// The textures of a texture-kernel launch (RenderArgs::tex_recs, tex_uv, tex_texels), likewise: read where a ray has hit a triangle.
struct TextureView {
    uint64_t p;
    __device__ __forceinline__ const TexRec *recs() const { return *reinterpret_cast<const TexRec *const __attribute__((address_space(4))) *>(p); }
    __device__ __forceinline__ const float *uv() const {
        return *reinterpret_cast<const float *const __attribute__((address_space(4))) *>(p + (offsetof(RenderArgs, tex_uv) - offsetof(RenderArgs, tex_recs)));
    }
    __device__ __forceinline__ const TexBary *bary() const {
        return *reinterpret_cast<const TexBary *const __attribute__((address_space(4))) *>(p + (offsetof(RenderArgs, tex_bary) - offsetof(RenderArgs, tex_recs)));
    }
    __device__ __forceinline__ const TexTexel *texels() const {
        return *reinterpret_cast<const TexTexel *const __attribute__((address_space(4))) *>(p + (offsetof(RenderArgs, tex_texels) - offsetof(RenderArgs, tex_recs)));
    }
};
__device__ __forceinline__ TextureView texture_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, tex_recs);
    asm volatile("" : "+s"(p));
    return {p};
}
// The corner normals of a smooth-kernel launch (RenderArgs::smooth_normals), likewise: read where a ray that scatters has hit a triangle.
__device__ __forceinline__ const SmoothCorner *smooth_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, smooth_normals);
    asm volatile("" : "+s"(p));
    return *reinterpret_cast<const SmoothCorner *const __attribute__((address_space(4))) *>(p);
}
// The roughness table of a rough-kernel launch (RenderArgs::rough_alpha), likewise: one float per material, read where the glossy lobe
// of a ray that scatters has been chosen.
__device__ __forceinline__ const float *rough_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, rough_alpha);
    asm volatile("" : "+s"(p));
    return *reinterpret_cast<const float *const __attribute__((address_space(4))) *>(p);
}
// The light table of a direct-kernel launch (RenderArgs::lights, n_lights, light_area), likewise: read where the diffuse lobe of a ray
// that scatters has been chosen.
struct DirectView {
    uint64_t p;
    __device__ __forceinline__ const LightRec *lights() const { return *reinterpret_cast<const LightRec *const __attribute__((address_space(4))) *>(p); }
    __device__ __forceinline__ int32_t n() const {
        return *reinterpret_cast<const __attribute__((address_space(4))) int32_t *>(p + (offsetof(RenderArgs, n_lights) - offsetof(RenderArgs, lights)));
    }
    __device__ __forceinline__ float area() const {
        return *reinterpret_cast<const __attribute__((address_space(4))) float *>(p + (offsetof(RenderArgs, light_area) - offsetof(RenderArgs, lights)));
    }
};
__device__ __forceinline__ DirectView direct_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, lights);
    asm volatile("" : "+s"(p));
    return {p};
}
// The alias table of an environment-sampling launch (RenderArgs::env_alias, env_cells, env_share), likewise: read where the diffuse lobe
// of a ray that scatters has been chosen.
struct EnvDirectView {
    uint64_t p;
    __device__ __forceinline__ const EnvAliasRec *table() const { return *reinterpret_cast<const EnvAliasRec *const __attribute__((address_space(4))) *>(p); }
    __device__ __forceinline__ int32_t cells() const {
        return *reinterpret_cast<const __attribute__((address_space(4))) int32_t *>(p + (offsetof(RenderArgs, env_cells) - offsetof(RenderArgs, env_alias)));
    }
    __device__ __forceinline__ float share() const {
        return *reinterpret_cast<const __attribute__((address_space(4))) float *>(p + (offsetof(RenderArgs, env_share) - offsetof(RenderArgs, env_alias)));
    }
};
__device__ __forceinline__ EnvDirectView envdirect_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, env_alias);
    asm volatile("" : "+s"(p));
    return {p};
}
// The roulette parameters of a roulette launch (RenderArgs::rr_start, rr_floor), likewise: read at the end of a scattering step.
struct RouletteView {
    uint64_t p;
    __device__ __forceinline__ int32_t start() const { return *reinterpret_cast<const __attribute__((address_space(4))) int32_t *>(p); }
    __device__ __forceinline__ float floor() const {
        return *reinterpret_cast<const __attribute__((address_space(4))) float *>(p + (offsetof(RenderArgs, rr_floor) - offsetof(RenderArgs, rr_start)));
    }
};
__device__ __forceinline__ RouletteView roulette_view() {
    uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(RenderArgs, rr_start);
    asm volatile("" : "+s"(p));
    return {p};
}

// What the launch planner (pt_launch_plan.hpp) has to know of this build.  Statistics kernels: the diagnostic builds that count
// in every launch run them always; PT_VERIFY_SHIPPED / PT_ADAPT_COUNT never -- the kernels a caller without pt_render_stats
// gets; args.stats only receives the verdict.
constexpr plan::Build kBuild = {kTileW, kTileH, PT_RAYS_PER_LANE, PT_BIG_RAYS_PER_LANE, PT_WAVES_PER_SIMD, kMaxBatchPass,
#if defined(PT_BLOCK_PROFILE)
                                plan::Stats::kAsAsked, true};
#elif defined(PT_PHASE_TIMERS) || defined(PT_VERIFY_BRUTE)
                                plan::Stats::kAlways, false};
#elif defined(PT_VERIFY_SHIPPED) || defined(PT_ADAPT_COUNT)
                                plan::Stats::kNever, false};
#else
                                plan::Stats::kAsAsked, false};
#endif

// rays per lane of an instantiation: the launch geometry (tile width) follows from it on the host as well
template <bool SKY, bool BIG, bool STATS>
constexpr int rays_per_lane() { return plan::rays_per_lane(kBuild, SKY, BIG, STATS); }

// NARROW = the statistics-free small-scene kernel with ONE pixel per lane (8 x 8 tiles): for launches with too few pixels to
// fill the chip with 16 x 8 tiles (small previews, thin row bands) -- half as many waves would leave wave slots empty.
// waves per SIMD an instantiation is compiled for
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW>
constexpr int integrator_waves() {
    return SKY ? ((BIG && STATS && ENV) ? PT_BIG_WAVES /* (that one spills at 5) */ : PT_SKY_WAVES)
               : BIG ? PT_BIG_WAVES : (STATS || (!NARROW && rays_per_lane<SKY, BIG, STATS>() > 1)) ? PT_WAVES_PER_SIMD - 1 : PT_WAVES_PER_SIMD;
}
// ADAPT = ROOM | POOL | CAM.  ROOM (bit 3, alone: ADAPT == 8) = the room instantiation of the statistics-free plain small-scene
// kernel, wide or NARROW (closest_hit<..., ROOM>; Variant::room; instantiated in pt_room_kernels.hip).  POOL (bits 1-2) = the two-pixel kernel for launches with adaptive sampling on (error >= 0), with tiles of
// 64 POOL pixels (2: 16 x 8, 4: 32 x 8): see "Batches" in the pass loop.  CAM (bit 0) = the camera twin: primary rays from the
// scene handle's pt_camera (RenderArgs::cam) instead of the reference's fixed eye.  (One template argument for both, so that the
// camera-free kernels keep their names: tests/test_kernel_resources.py pins them by mangled name.)  On the host a kernel is a
// plan::Variant (pt_launch_plan.hpp): POOL = Variant::pool, CAM = Variant::view != 0; kernel_of below is the one place that maps them.
// The body (pt_integrator_body.inc) is shared with integrate_kernel_lens TEXTUALLY, not through a device function: with the body
// in a forceinline function that both kernels call, the compiler scheduled and spilled 30 of these 44 kernels differently.
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW = false, int ADAPT = 0>
__global__ __launch_bounds__(kBlock, (integrator_waves<SKY, BIG, STATS, ENV, NARROW>())) void integrate_kernel(const RenderArgs a) {
    constexpr bool LENS = false, MOTION = false, PROJ = false, ENVMAP = false, GLASS = false, TEX = false, SMOOTH = false, ROUGH = false, DIRECT = false, ENVDIRECT = false, ROULETTE = false;
#include "pt_integrator_body.inc"
}
// The lens kernel of camera twin integrate_kernel<SKY, BIG, STATS, ENV, NARROW, ADAPT> (ADAPT odd): the same, with each primary ray
// from a point of the thin lens (RenderArgs::lns, pt_hip.h: pt_lens) through the focal plane.  A kernel of its own rather than a
// branch in the twin: such a branch spilled vector registers in the skybox / regeneration twins, which sit at 96 VGPRs for 5 waves.
// Waves per SIMD: the twin's, except for six skybox (path regeneration) kernels, which at the twins' 5 waves and 96 VGPRs spilled
// 6 VGPRs to scratch whatever the order of the lens code (every skybox kernel but the statistics-free, envelope-test-free box-tree one,
// and the one compiled for 4 anyway): they are compiled for 4 ("Lens"; tests/test_lens_host.py pins them).
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW>
constexpr int lens_waves() {
    constexpr int w = integrator_waves<SKY, BIG, STATS, ENV, NARROW>();
    return (SKY && w == PT_SKY_WAVES && !(BIG && !STATS && !ENV)) ? w - 1 : w;
}
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW, int ADAPT>
__global__ __launch_bounds__(kBlock, (lens_waves<SKY, BIG, STATS, ENV, NARROW>())) void integrate_kernel_lens(const RenderArgs a) {
    constexpr bool LENS = true, MOTION = false, PROJ = false, ENVMAP = false, GLASS = false, TEX = false, SMOOTH = false, ROUGH = false, DIRECT = false, ENVDIRECT = false, ROULETTE = false;
#include "pt_integrator_body.inc"
}
// The motion twins (pt_hip.h: camera motion): the camera twin and its lens kernel with the camera -- and the lens axes -- interpolated
// between the handle's camera and its end pose at a time t drawn per path, RenderArgs::cam + t * RenderArgs::cam_d.  Kernels of
// their own for the reason the lens kernel is one.  Waves per SIMD: motion_waves (tests/test_motion_resources.py pins them).
// The parent's (the camera twin's, the lens kernel's) -- except for the lens twin of the two-pixel small-scene kernel with the
// envelope test, which at its parent's 5 waves and 96 VGPRs spilled one VGPR (68 spilled SGPRs no longer fit the lanes set aside
// for them): it is compiled for 4.
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW, bool LENS_>
constexpr int motion_waves() {
    constexpr int w = LENS_ ? lens_waves<SKY, BIG, STATS, ENV, NARROW>() : integrator_waves<SKY, BIG, STATS, ENV, NARROW>();
    return (LENS_ && !SKY && !BIG && !STATS && ENV && !NARROW) ? w - 1 : w;
}
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW, int ADAPT>
__global__ __launch_bounds__(kBlock, (motion_waves<SKY, BIG, STATS, ENV, NARROW, false>())) void integrate_kernel_motion(const RenderArgs a) {
    constexpr bool LENS = false, MOTION = true, PROJ = false, ENVMAP = false, GLASS = false, TEX = false, SMOOTH = false, ROUGH = false, DIRECT = false, ENVDIRECT = false, ROULETTE = false;
#include "pt_integrator_body.inc"
}
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW, int ADAPT>
__global__ __launch_bounds__(kBlock, (motion_waves<SKY, BIG, STATS, ENV, NARROW, true>())) void integrate_kernel_motion_lens(const RenderArgs a) {
    constexpr bool LENS = true, MOTION = true, PROJ = false, ENVMAP = false, GLASS = false, TEX = false, SMOOTH = false, ROUGH = false, DIRECT = false, ENVDIRECT = false, ROULETTE = false;
#include "pt_integrator_body.inc"
}
// The projection kernel of camera twin integrate_kernel<SKY, BIG, STATS, ENV, NARROW, ADAPT> (ADAPT odd): the same, with each primary
// ray from the handle's non-perspective projection (pt_hip.h: pt_projection; pt_projection.hpp spells it once, for this kernel and
// for the first-hit feature pass below).  One kernel for the three kinds: the kind is a kernel argument and primary_dir branches on
// it with scalar branches.  A kernel of its own for the reason the lens kernel is one.  Waves per SIMD: projection_waves, the twin's
// for every kernel (tests/test_projection_resources.py pins them, with the twin's LDS) -- which is why the launch
// planner may ask integrator_waves_per_cu for the TWIN's wave slots: the runtime's answer depends on nothing else.
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW>
constexpr int projection_waves() {
    return integrator_waves<SKY, BIG, STATS, ENV, NARROW>();
}
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW, int ADAPT>
__global__ __launch_bounds__(kBlock, (projection_waves<SKY, BIG, STATS, ENV, NARROW>())) void integrate_kernel_projection(const RenderArgs a) {
    constexpr bool LENS = false, MOTION = false, PROJ = true, ENVMAP = false, GLASS = false, TEX = false, SMOOTH = false, ROUGH = false, DIRECT = false, ENVDIRECT = false, ROULETTE = false;
#include "pt_integrator_body.inc"
}

// launch_surface_integrator's seven halves: each surface unit's translation unit defines its own
template <int UNIT>
hipError_t launch_surface_unit(const RenderArgs &args, const plan::Variant &v, hipStream_t stream);
#define PT_UNIT_HALF(U) template <> hipError_t launch_surface_unit<U>(const RenderArgs &, const plan::Variant &, hipStream_t);
PT_UNIT_HALF(kGlassUnit) PT_UNIT_HALF(kTextureUnit) PT_UNIT_HALF(kSmoothUnit) PT_UNIT_HALF(kRoughUnit) PT_UNIT_HALF(kDirectUnit) PT_UNIT_HALF(kEnvDirectUnit) PT_UNIT_HALF(kRouletteUnit)
#undef PT_UNIT_HALF

#ifdef PT_ENVIRONMENT_UNIT
// ---------------------------------------------------------------------------------------------------------------
// The environment kernels (pt_environment_kernels.hip: this file compiled with PT_ENVIRONMENT_UNIT, a translation unit of its own,
// so that the build of the kernels above takes no longer).  One per skybox kernel (BIG, STATS, ENV) and VIEW: plan views 0 .. 4 and
// 5 = the projection kernel of view 1.  The body with SKY = true (path regeneration, the sky chunking, no last-segment filter) and
// ENVMAP = true: a miss adds throughput x the octahedral map's radiance (pt_environment.hpp) instead of the skybox texel.
// Waves per SIMD: the skybox twin's -- the lookup (a division, a dozen float operations, four 16-byte loads) peaks below the
// skybox's double-precision acos and atan2 -- except where environment_waves says otherwise (tests/test_environment_resources.py
// pins the list).
template <bool BIG, bool STATS, bool ENV, int VIEW>
constexpr int environment_waves() {
    constexpr bool kLens = VIEW == 2 || VIEW == 4;
    if constexpr (VIEW == 5) return projection_waves<true, BIG, STATS, ENV, false>();
    else if constexpr (VIEW >= 3) return motion_waves<true, BIG, STATS, ENV, false, kLens>();
    else if constexpr (VIEW == 2) return lens_waves<true, BIG, STATS, ENV, false>();
    else return integrator_waves<true, BIG, STATS, ENV, false>();
}
template <bool BIG, bool STATS, bool ENV, int VIEW>
__global__ __launch_bounds__(kBlock, (environment_waves<BIG, STATS, ENV, VIEW>())) void integrate_kernel_environment(const RenderArgs a) {
    constexpr bool SKY = true, NARROW = false;
    constexpr int ADAPT = VIEW != 0 ? 1 : 0;
    constexpr bool LENS = VIEW == 2 || VIEW == 4, MOTION = VIEW == 3 || VIEW == 4, PROJ = VIEW == 5, ENVMAP = true, GLASS = false, TEX = false, SMOOTH = false, ROUGH = false, DIRECT = false, ENVDIRECT = false, ROULETTE = false;
#include "pt_integrator_body.inc"
}
namespace {
using Kernel = void (*)(const RenderArgs);
constexpr int kEnvironmentViews = plan::kViews + 1;
template <int I>
Kernel environment_kernel_of() {   // I = VIEW * 8 + (big, stats, env) as bits 2..0
    return &integrate_kernel_environment<(I & 4) != 0, (I & 2) != 0, (I & 1) != 0, I / 8>;
}
template <int... I>
std::array<Kernel, sizeof...(I)> environment_kernel_table(std::integer_sequence<int, I...>) { return {environment_kernel_of<I>()...}; }
const auto kEnvironmentKernels = environment_kernel_table(std::make_integer_sequence<int, 8 * kEnvironmentViews>());
}  // namespace
hipError_t launch_environment_integrator(const RenderArgs &args, const plan::Variant &v, hipStream_t stream) {
    if (!v.sky || v.narrow || v.pool || args.env_map == nullptr || args.env_n < kEnvMinSize || args.env_n > kEnvMaxSize || args.sky != nullptr)
        return hipErrorInvalidValue;
    if (args.projection != 0 && v.view != 1) return hipErrorInvalidDeviceFunction;
    const int view = args.projection != 0 ? 5 : v.view;
    const Kernel kernel = kEnvironmentKernels[view * 8 + (v.big ? 4 : 0) + (v.stats ? 2 : 0) + (v.env ? 1 : 0)];
    hipLaunchKernelGGL(kernel, dim3(args.n_tiles * args.n_chunks), dim3(kBlock), 0, stream, args);
    return hipGetLastError();
}
#elif defined(PT_ROOM_UNIT)
// ---------------------------------------------------------------------------------------------------------------
// The room kernels (pt_room_kernels.hip: this file compiled with PT_ROOM_UNIT, a translation unit of its own, like the units above and
// below): integrate_kernel<false, false, false, false, NARROW, 8>, the plain statistics-free small-scene kernel whose search has no
// generic loops (closest_hit<..., ROOM>), for scenes whose tables say CullTables::room.  They have no camera twin, lens, motion or
// projection kernels -- launches with any of those keep the generic body (plan::plan_tiles) -- and their own resources report
// (lib/asm/room_resource_usage.txt, tests/test_room_kernel_resources.py).
void (*room_kernel(bool narrow))(const RenderArgs) {
    if (!narrow) return &integrate_kernel<false, false, false, false, false, 8>;
    if constexpr (plan::variant_exists({false, false, false, false, true, 0, 0, true}, kBuild)) return &integrate_kernel<false, false, false, false, true, 8>;
    else return nullptr;
}
#elif defined(PT_SURFACE_UNIT)
// A surface unit (pt_kernels.hpp: SurfaceUnit; pt_glass_kernels.hip ... pt_roulette_kernels.hip each compile this file with its number as
// PT_SURFACE_UNIT): this one section, as integrate_kernel_<name>, with the flag of every unit up to this one on.
#define PT_UNIT_NAME_1 glass
#define PT_UNIT_NAME_2 texture
#define PT_UNIT_NAME_3 smooth
#define PT_UNIT_NAME_4 rough
#define PT_UNIT_NAME_5 direct
#define PT_UNIT_NAME_6 envdirect
#define PT_UNIT_NAME_7 roulette
#define PT_PASTE_(a, b) a##b
#define PT_PASTE(a, b) PT_PASTE_(a, b)
#define PT_UNIT_KERNEL PT_PASTE(integrate_kernel_, PT_PASTE(PT_UNIT_NAME_, PT_SURFACE_UNIT))
static_assert(PT_SURFACE_UNIT >= kGlassUnit && PT_SURFACE_UNIT <= kRouletteUnit, "PT_SURFACE_UNIT: a SurfaceUnit");
// (the roulette unit holds the direct unit's kernels AND the environment-sampling unit's: there ENVDIRECT is a parameter of the kernel,
// PT_UNIT_ENVD below, and not a function of the unit's number)
constexpr bool kUnitTex = PT_SURFACE_UNIT >= kTextureUnit, kUnitSmooth = PT_SURFACE_UNIT >= kSmoothUnit, kUnitRough = PT_SURFACE_UNIT >= kRoughUnit,
               kUnitDirect = PT_SURFACE_UNIT >= kDirectUnit, kUnitEnvDirect = PT_SURFACE_UNIT == kEnvDirectUnit, kUnitRoulette = PT_SURFACE_UNIT == kRouletteUnit;
#if PT_SURFACE_UNIT == 7
#define PT_UNIT_TEMPLATE template <int MISS, bool BIG, bool STATS, int FORM, int VIEW, bool ENVD>
#define PT_UNIT_ENVD ENVD
#else
#define PT_UNIT_TEMPLATE template <int MISS, bool BIG, bool STATS, int FORM, int VIEW>
#define PT_UNIT_ENVD kUnitEnvDirect
#endif
// ---------------------------------------------------------------------------------------------------------------
// The dielectric kernels (pt_glass_kernels.hip: this file compiled with PT_SURFACE_UNIT 1, a translation unit of its own).  The body
// with GLASS = true: a hit on a material the handle's table marks (RenderArgs::glass, pt_hip.h: pt_dielectric) reflects or refracts.
// One per kernel a launch can be planned as, and VIEW (plan views 0 .. 4 and 5 = the projection kernel of view 1):
//   MISS  0 = no miss shader, 1 = skybox, 2 = environment (the body with SKY and ENVMAP as in integrate_kernel_environment)
//   FORM  0 = the wide kernel, 1 = its 8 x 8 form, 2 / 3 = the batch kernel over 16 x 8 / 32 x 8 tiles (forms 1 - 3: MISS 0, no statistics)
// The envelope test is not a parameter: forms 0 and 1 always carry it (ENV = true).  A launch planned as the twin without it runs
// the kernel with it -- the same tiles, one compare per segment more, and nothing is culled for an origin outside the envelope, so the
// closest hit is the same by construction.  The batch kernels are not built with the test (plan::variant_exists) and never planned
// for a scene that needs it.  Waves per SIMD: the twin's (with ENV as instantiated here) minus glass_fewer_waves
// (tests/test_glass_resources.py pins every kernel).
template <bool SKY, bool BIG, bool STATS, bool ENV, bool NARROW, int VIEW>
constexpr int view_waves() {
    constexpr bool kLens = VIEW == 2 || VIEW == 4;
    if constexpr (VIEW == 5) return projection_waves<SKY, BIG, STATS, ENV, NARROW>();
    else if constexpr (VIEW >= 3) return motion_waves<SKY, BIG, STATS, ENV, NARROW, kLens>();
    else if constexpr (VIEW == 2) return lens_waves<SKY, BIG, STATS, ENV, NARROW>();
    else return integrator_waves<SKY, BIG, STATS, ENV, NARROW>();
}
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW>
constexpr int glass_fewer_waves() {
    // At their twins' 5 waves and 96 VGPRs these spilled vector registers to scratch: the skybox kernels that are not compiled for 4
    // anyway (6 VGPRs: the dielectric's operands meet the skybox lookup's double-precision registers), and the lens, motion and
    // projection forms of the two-pixel small-scene kernel (1 VGPR).  They are compiled for a wave fewer.
    if constexpr (MISS == 1 && !(BIG && STATS)) return (VIEW == 0 || VIEW == 1 || VIEW == 3 || VIEW == 5) ? 1 : 0;
    else if constexpr (MISS == 0 && !BIG && !STATS && FORM == 0) return (VIEW == 2 || VIEW == 3 || VIEW == 5) ? 1 : 0;
    else return 0;
}
// The texture kernels (pt_hip.h: pt_texture): the same set with TEX = true too -- a hit on a triangle of a material
// the handle's texture table marks (RenderArgs::tex_recs) multiplies the throughput by the texel before the emissive or the diffuse
// lobe runs.  A textured handle without dielectrics runs them with an all-zero dielectric table.  The twin of a texture kernel is the
// dielectric kernel of the same arguments; waves per SIMD: that twin's minus texture_fewer_waves (tests/test_texture_resources.py
// pins every kernel).
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW>
constexpr int texture_fewer_waves() {
    // At the dielectric twin's 5 waves and 96 VGPRs these spilled vector registers to scratch (1 and 2 VGPRs: the barycentrics'
    // operands on top of the second pixel's state): the two-pixel small-scene kernel without a miss shader, fixed eye and camera twin.
    return (MISS == 0 && !BIG && !STATS && FORM == 0 && (VIEW == 0 || VIEW == 1)) ? 1 : 0;
}
// The smooth kernels (pt_hip.h: shading normals): the same set with SMOOTH = true too -- the glossy lobe, the diffuse
// lobe and the dielectric step run with the interpolated normal of the hit point (RenderArgs::smooth_normals), falling back to the
// stored one.  A handle without textures or dielectrics runs them with all-zero tables.  The twin of a smooth kernel is the texture
// kernel of the same arguments; waves per SIMD: that twin's minus smooth_fewer_waves (tests/test_smooth_resources.py pins every kernel).
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW>
constexpr int smooth_fewer_waves() {
    return 0;
}
// The rough kernels (pt_hip.h: rough specular): the same set with ROUGH = true too -- the glossy lobe of a material
// the handle's roughness table marks (RenderArgs::rough_alpha) reflects about a microfacet normal drawn from the GGX distribution of
// visible normals (pt_rough.hpp) and takes Ks x G1.  A handle without shading normals, textures or dielectrics runs them with all-zero
// tables.  The twin of a rough kernel is the smooth kernel of the same arguments; waves per SIMD: that twin's minus rough_fewer_waves
// (tests/test_rough_resources.py pins every kernel).
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW>
constexpr int rough_fewer_waves() {
    // At the smooth twin's 5 waves and 96 VGPRs these spilled 27 vector registers to scratch (the GGX step's two frames on top of the
    // pool's state): the small-scene batch kernel over 16 x 8 tiles with a fixed eye, with the moving lens and under a projection.
    return (MISS == 0 && !BIG && !STATS && FORM == 2 && (VIEW == 0 || VIEW == 4 || VIEW == 5)) ? 1 : 0;
}
// The direct kernels (pt_hip.h: direct lighting): the same set with DIRECT = true too -- a path collects its
// radiance and is counted once when it ends, and a scattering diffuse hit sends a shadow ray to a sampled point of the handle's light
// table (RenderArgs::lights; pt_direct.hpp) through the same closest-hit search.  A handle without the other tables runs them with
// all-zero ones.  The twin of a direct kernel is the rough kernel of the same arguments; waves per SIMD: that twin's minus
// direct_fewer_waves (tests/test_direct_resources.py pins every kernel).
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW>
constexpr int rough_unit_waves() {
    return view_waves<MISS != 0, BIG, STATS, FORM < 2, FORM == 1, VIEW>() - glass_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() -
           texture_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() - smooth_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() -
           rough_fewer_waves<MISS, BIG, STATS, FORM, VIEW>();
}
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW>
constexpr int direct_fewer_waves() {
    // The path's radiance, the pending shadow ray's direction, its term and its light are ten vector registers per ray slot on top of
    // the rough twin's.  Every twin compiled for 5 waves (96 VGPRs) or 6 (80: the 8 x 8 form) either spilled vector registers to scratch
    // (1 to 93 of them) or was given more registers than its bound by the compiler, which is a wave fewer unsaid: every direct kernel is
    // compiled for 4 waves per SIMD.
    constexpr int twin = rough_unit_waves<MISS, BIG, STATS, FORM, VIEW>();
    return twin > 4 ? twin - 4 : 0;
}
// The environment-sampling kernels (pt_hip.h: environment sampling): the direct kernels of an environment
// (MISS == 2, the wide form alone: an environment launch is planned as a skybox launch, which has no other form) with ENVDIRECT = true
// too -- the shadow ray of a diffuse hit goes to the handle's emitters or, by the share, to a direction drawn from the environment's
// alias table (RenderArgs::env_alias; pt_envdirect.hpp), and a miss after a diffuse step adds nothing.  The twin of such a kernel is
// the direct kernel of the same arguments; waves per SIMD: that twin's minus envdirect_fewer_waves (tests/test_envdirect_resources.py
// pins every kernel).
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW>
constexpr int envdirect_fewer_waves() {
    return 0;
}
// The roulette kernels (pt_hip.h: Russian roulette): the direct kernels and the environment-sampling kernels
// (ENVD) with ROULETTE = true too -- from RenderArgs::rr_start on every scattering step ends with the roulette step (pt_roulette.hpp),
// and the closed-room wide and 8 x 8 forms regenerate paths as the skybox kernels do.  The twin of such a kernel is the direct or the
// environment-sampling kernel of the same arguments; waves per SIMD: that twin's minus roulette_fewer_waves
// (tests/test_roulette_resources.py pins every kernel).
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW, bool ENVD>
constexpr int roulette_fewer_waves() {
    // At the direct twin's 4 waves and 128 VGPRs these spilled one vector register to scratch (the regeneration state, cur_pass and
    // next_pass of two ray slots, on top of the twin's 123 to 128): the two-pixel small-scene kernel without a miss shader under the
    // lens, the moving camera and the moving lens.  They are compiled for a wave fewer.
    return (MISS == 0 && !BIG && !STATS && FORM == 0 && !ENVD && (VIEW == 2 || VIEW == 3 || VIEW == 4)) ? 1 : 0;
}
template <int MISS, bool BIG, bool STATS, int FORM, int VIEW, bool ENVD>
constexpr int unit_waves() {
    return view_waves<MISS != 0, BIG, STATS, FORM < 2, FORM == 1, VIEW>() - glass_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() -
           (kUnitTex ? texture_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() : 0) - (kUnitSmooth ? smooth_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() : 0) -
           (kUnitRough ? rough_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() : 0) - (kUnitDirect ? direct_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() : 0) -
           (ENVD ? envdirect_fewer_waves<MISS, BIG, STATS, FORM, VIEW>() : 0) - (kUnitRoulette ? roulette_fewer_waves<MISS, BIG, STATS, FORM, VIEW, ENVD>() : 0);
}
PT_UNIT_TEMPLATE
__global__ __launch_bounds__(kBlock, (unit_waves<MISS, BIG, STATS, FORM, VIEW, PT_UNIT_ENVD>()))
void PT_UNIT_KERNEL(const RenderArgs a) {
    constexpr bool SKY = MISS != 0, ENV = FORM < 2, NARROW = FORM == 1;
    constexpr int ADAPT = (FORM == 2 ? 2 : FORM == 3 ? 4 : 0) | (VIEW != 0 ? 1 : 0);
    constexpr bool LENS = VIEW == 2 || VIEW == 4, MOTION = VIEW == 3 || VIEW == 4, PROJ = VIEW == 5, ENVMAP = MISS == 2, GLASS = true, TEX = kUnitTex, SMOOTH = kUnitSmooth, ROUGH = kUnitRough, DIRECT = kUnitDirect, ENVDIRECT = PT_UNIT_ENVD, ROULETTE = kUnitRoulette;
#include "pt_integrator_body.inc"
}
namespace {
using Kernel = void (*)(const RenderArgs);
constexpr int kGlassViews = plan::kViews + 1, kGlassPerView = 3 * 2 * 2 * 4;
// does the build have the twin of that kernel?  (the 8 x 8 form and the batch kernels: plan::variant_exists)
template <int MISS, bool BIG, bool STATS, int FORM, bool ENVD>
constexpr bool glass_kernel_exists() {
    if constexpr (ENVD) return MISS == 2 && FORM == 0;   // (environment sampling needs an environment)
    else if constexpr (FORM == 0) return true;
    else if constexpr (MISS != 0 || STATS) return false;
    else return plan::variant_exists({false, BIG, false, FORM == 1, FORM == 1, FORM == 2 ? 2 : FORM == 3 ? 4 : 0, 1}, kBuild);
}
constexpr int kGlassTable = kGlassPerView * kGlassViews;
template <int J>
Kernel glass_kernel_of() {   // I = (VIEW * 3 + MISS) * 16 + (big, stats) as bits 3..2 + FORM; the roulette unit: J = I, and kGlassTable + I with ENVD
    constexpr int I = J % kGlassTable;
    constexpr int kMiss = (I / 16) % 3, kForm = I & 3;
    constexpr bool kBig = (I & 8) != 0, kStats = (I & 4) != 0;
    [[maybe_unused]] constexpr bool kEnvd = kUnitRoulette ? J >= kGlassTable : kUnitEnvDirect;
    if constexpr (!glass_kernel_exists<kMiss, kBig, kStats, kForm, kEnvd>()) return nullptr;
#if PT_SURFACE_UNIT == 7
    else return &PT_UNIT_KERNEL<kMiss, kBig, kStats, kForm, I / 48, kEnvd>;
#else
    else return &PT_UNIT_KERNEL<kMiss, kBig, kStats, kForm, I / 48>;
#endif
}
template <int... I>
std::array<Kernel, sizeof...(I)> glass_kernel_table(std::integer_sequence<int, I...>) { return {glass_kernel_of<I>()...}; }
const auto kGlassKernels = glass_kernel_table(std::make_integer_sequence<int, kGlassTable * (kUnitRoulette ? 2 : 1)>());
}  // namespace
template <>
hipError_t launch_surface_unit<PT_SURFACE_UNIT>(const RenderArgs &args, const plan::Variant &v, hipStream_t stream) {
    // (the roulette unit: env_alias picks the environment-sampling kernels, and the launch is then checked as that unit's)
    const bool envd = kUnitRoulette ? args.env_alias != nullptr : kUnitEnvDirect;
    if (surface_unit_of(args) != PT_SURFACE_UNIT || (kUnitDirect && (envd ? args.n_lights < 0 : args.n_lights <= 0))) return hipErrorInvalidValue;
    if (kUnitRoulette && (args.rr_start < 1 || !roulette_params_ok(args.rr_start, args.rr_floor) || args.lights == nullptr)) return hipErrorInvalidValue;
    if (envd && (args.env_map == nullptr || args.env_cells < 1 || args.env_cells > kEnvSampleMaxCells || args.env_cells > args.env_n ||
                           !(args.env_share > 0.0f && args.env_share <= 1.0f) || (args.n_lights == 0 && args.env_share != 1.0f) || args.lights == nullptr))
        return hipErrorInvalidValue;
    if ((kUnitRough && args.rough_alpha == nullptr) || (kUnitSmooth && args.smooth_normals == nullptr)) return hipErrorInvalidValue;
    if (kUnitTex && (args.tex_recs == nullptr || args.tex_uv == nullptr || args.tex_texels == nullptr || args.tex_bary == nullptr)) return hipErrorInvalidValue;
    if (args.glass == nullptr || (args.env_map != nullptr && (!v.sky || args.sky != nullptr))) return hipErrorInvalidValue;
    if (args.projection != 0 && v.view != 1) return hipErrorInvalidDeviceFunction;
    const int view = args.projection != 0 ? 5 : v.view;
    const int miss = args.env_map != nullptr ? 2 : v.sky ? 1 : 0, form = v.narrow ? 1 : v.pool == 2 ? 2 : v.pool == 4 ? 3 : 0;
    const Kernel kernel = kGlassKernels[(kUnitRoulette && envd ? kGlassTable : 0) + (view * 3 + miss) * 16 + (v.big ? 8 : 0) + (v.stats ? 4 : 0) + form];
    if (!kernel) return hipErrorInvalidDeviceFunction;
    hipLaunchKernelGGL(kernel, dim3(args.n_tiles * args.n_chunks), dim3(kBlock), 0, stream, args);
    return hipGetLastError();
}
#undef PT_UNIT_KERNEL
#undef PT_UNIT_TEMPLATE
#undef PT_UNIT_ENVD
#else
// First-hit feature pass under a projection (pt_hip.h: pt_render_features_host): the ray pt_projection states for pixel (x, y) with
// jitter 0, for launch_trace_rays.  (Here and not beside the pinhole's feature_rays_kernel in pt_denoise.hip: the ray needs this
// file's portable_sincos and normalize3.)
__global__ __launch_bounds__(256) void projection_rays_kernel(const RenderArgs a, int width, int height, int row_begin, int n,
                                                              float *__restrict__ origins, float *__restrict__ directions) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int y = row_begin + p / width, x = p % width;
    const float u = static_cast<float>(static_cast<double>(x) / width - 0.5);
    const float v = static_cast<float>(-static_cast<double>(y) / height + 0.5);
    float ox, oy, oz, dx, dy, dz;
    projection_primary_ray(a.projection, u, v, a.cam, a.lns + 2, a.prj_span,
                           [](float ang, float &sn, float &cs) { portable_sincos(ang, sn, cs); },
                           [](float &vx, float &vy, float &vz) { normalize3(vx, vy, vz); }, ox, oy, oz, dx, dy, dz);
    const size_t o = 3 * static_cast<size_t>(p);
    origins[o] = ox; origins[o + 1] = oy; origins[o + 2] = oz;
    directions[o] = dx; directions[o + 1] = dy; directions[o + 2] = dz;
}
hipError_t launch_projection_rays(const RenderArgs &args, int width, int height, int row_begin, int rows, float *d_origins, float *d_directions,
                                  hipStream_t stream) {
    const int n = rows * width;
    if (n <= 0) return hipSuccess;
    if (args.projection == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(projection_rays_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, args, width, height, row_begin, n, d_origins, d_directions);
    return hipGetLastError();
}

// Closest hit for caller-supplied rays (the intersection half of Scene::TraceRay, scene.cpp:114-120).
template <bool BIG>
__global__ __launch_bounds__(kBlock, BIG ? PT_BIG_WAVES : PT_WAVES_PER_SIMD) void trace_rays_kernel(const RenderArgs a, const float *__restrict__ origins,
                                                                              const float *__restrict__ directions, int n_rays,
                                                                              int32_t *__restrict__ hit_index, float *__restrict__ hit_t) {
    __shared__ WaveLds<std::conditional_t<BIG, BigQueues, SmallQueues>, 1> lds;
    const int lane = threadIdx.x;
    const int i = blockIdx.x * kBlock + lane;
    const bool valid = i < n_rays;
    Ray q;
    q.ox = q.oy = q.oz = 0.0f; q.dx = q.dy = 0.0f; q.dz = 1.0f;
    if (valid) {
        q.ox = origins[3 * i]; q.oy = origins[3 * i + 1]; q.oz = origins[3 * i + 2];
        q.dx = directions[3 * i]; q.dy = directions[3 * i + 1]; q.dz = directions[3 * i + 2];
    }
    // Rays outside the envelope the culling margins were derived for (pt_hip.h: pt_trace_rays_host) get every triangle as
    // a candidate for the exact test instead; written so that NaNs count as outside.
    const float d2 = (q.dx * q.dx + q.dy * q.dy) + q.dz * q.dz;
    const bool inside = __builtin_fabsf(q.ox) <= a.r_org && __builtin_fabsf(q.oy) <= a.r_org && __builtin_fabsf(q.oz) <= a.r_org &&
                        __builtin_fabsf(d2 - 1.0f) <= 1.0e-5f;
    float best[1];
    int hit[1];
    const ExactRec *hit_rec[1];
    WaveStats st;
    const Ray qs[1] = {q};
    const bool lives[1] = {valid}, insides[1] = {inside};
    closest_hit<true, false>(a, lds, qs, lives, insides, lane, a.eps, best, hit, hit_rec, st);
    if (valid) {
        hit_index[i] = hit[0];
        hit_t[i] = best[0];
    }
}

// Diagnostic (test builds call it through pt_test_box_masks): the box tree's child test on caller-supplied
// (node, ray, t_best) items, one item per lane -- out[i] = box_children_kept of item i, children that do not exist masked off.
__global__ __launch_bounds__(kBlock) void box_masks_kernel(const BvhNode *__restrict__ nodes, const float *__restrict__ rays,
                                                           const float *__restrict__ t_best, float err, int n, uint32_t *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint4 *np = reinterpret_cast<const uint4 *>(nodes + i);
    const uint4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3];
    Ray r;
    r.ox = rays[6 * i]; r.oy = rays[6 * i + 1]; r.oz = rays[6 * i + 2];
    r.dx = rays[6 * i + 3]; r.dy = rays[6 * i + 4]; r.dz = rays[6 * i + 5];
    const float ix = __builtin_amdgcn_rcpf(r.dx), iy = __builtin_amdgcn_rcpf(r.dy), iz = __builtin_amdgcn_rcpf(r.dz);
    const uint32_t exists = (2u << ((q0.w >> 8) & 7u)) - 1u;
    out[i] = box_children_kept<8>(q0, q1, q2, q3, r, ix, iy, iz, t_best[i], err) & exists;
}
hipError_t launch_box_masks(const BvhNode *d_nodes, const float *d_rays, const float *d_t_best, float err, int n, uint32_t *d_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(box_masks_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, d_nodes, d_rays, d_t_best, err, n, d_out);
    return hipGetLastError();
}

hipError_t launch_trace_rays(const RenderArgs &args, const float *d_origins, const float *d_directions, int n_rays,
                             int32_t *d_hit_index, float *d_hit_t, hipStream_t stream) {
    if (n_rays <= 0) return hipSuccess;
    const unsigned grid = static_cast<unsigned>((n_rays + kBlock - 1) / kBlock);
    if ((args.big != 0))
        hipLaunchKernelGGL(trace_rays_kernel<true>, dim3(grid), dim3(kBlock), 0, stream, args, d_origins, d_directions, n_rays, d_hit_index, d_hit_t);
    else
        hipLaunchKernelGGL(trace_rays_kernel<false>, dim3(grid), dim3(kBlock), 0, stream, args, d_origins, d_directions, n_rays, d_hit_index, d_hit_t);
    return hipGetLastError();
}

#ifdef PT_BLOCK_PROFILE
// the instantiations the instrumented code object must contain (nothing in this build references them)
#define PT_INST(S, B) \
    template __global__ void integrate_kernel<S, B, false, false, false>(const RenderArgs); \
    template __global__ void integrate_kernel<S, B, true, false, false>(const RenderArgs);  \
    template __global__ void integrate_kernel<S, B, false, true, false>(const RenderArgs);  \
    template __global__ void integrate_kernel<S, B, true, true, false>(const RenderArgs);
PT_INST(false, false) PT_INST(false, true) PT_INST(true, false) PT_INST(true, true)
#undef PT_INST
}  // namespace pt
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
namespace pt {
// Diagnostic build (libpt_blockprof.so): the integrator is launched from an INSTRUMENTED copy of this file's code object
// (tools/asm_profile.py inserts an execution counter in front of every straight-line run of instructions of the compiler's
// own assembly) and the counters are written to $PT_BLOCKPROF_OUT.<kernel> after every launch.  Never part of the product.
hipError_t launch_integrator(const RenderArgs &args0, const plan::Variant &v, hipStream_t stream) {
    constexpr size_t kCounters = 4096;
    static hipModule_t mod = nullptr;
    static uint32_t *d_cnt = nullptr;
    const int rows = args0.row_end - args0.row_begin;
    if (rows <= 0 || args0.width <= 0) return hipSuccess;
    if (!plan::variant_exists(v, kBuild) || args0.projection != 0 || args0.env_map != nullptr || surface_unit_of(args0) != kNoSurfaceUnit) return hipErrorNotSupported;   // (the instrumented code object holds no camera-twin, lens or projection kernel: refuse rather than run another)
    if (!mod) {
        const char *path = std::getenv("PT_BLOCKPROF_HSACO");
        if (!path) return hipErrorInvalidValue;
        hipError_t e = hipModuleLoad(&mod, path);
        if (e != hipSuccess) return e;
        e = hipMalloc(reinterpret_cast<void **>(&d_cnt), kCounters * sizeof(uint32_t));
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipMemsetAsync(d_cnt, 0, kCounters * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    RenderArgs args = args0;
    args.blockprof = d_cnt;
    char name[128];
    std::snprintf(name, sizeof name, "_ZN2pt16integrate_kernelILb%dELb%dELb%dELb%dELb%dELi%dEEEvNS_10RenderArgsE", v.sky, v.big, v.stats, v.env, v.narrow,
                  v.pool | v.view);
    hipFunction_t f;
    e = hipModuleGetFunction(&f, mod, name);
    if (e != hipSuccess) return e;
    size_t size = sizeof args;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    e = hipModuleLaunchKernel(f, args.n_tiles * args.n_chunks, 1, 1, kBlock, 1, 1, 0, stream, nullptr, config);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    std::vector<uint32_t> h(kCounters);
    e = hipMemcpy(h.data(), d_cnt, kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    if (const char *out = std::getenv("PT_BLOCKPROF_OUT")) {
        if (FILE *fp = std::fopen((std::string(out) + "." + name + ".txt").c_str(), "w")) {
            for (size_t i = 0; i < kCounters; ++i) if (h[i]) std::fprintf(fp, "%zu %u\n", i, h[i]);
            std::fclose(fp);
        }
    }
    return hipSuccess;
}
hipError_t integrator_waves_per_cu(const plan::Variant &, int *waves) {
    *waves = 24;
    return hipSuccess;
}
#else
namespace {
using Kernel = void (*)(const RenderArgs);
// The kernel of variant I of this build, nullptr if the build has none: the one place where a plan::Variant becomes template arguments.
template <int I>
Kernel kernel_of() {
    constexpr plan::Variant v = plan::variant_of(I);
    if constexpr (!plan::variant_exists(v, kBuild)) return nullptr;
    else if constexpr (v.room) return room_kernel(v.narrow);   // (pt_room_kernels.hip)
    else if constexpr (plan::view_has_motion(v.view) && plan::view_has_lens(v.view)) return &integrate_kernel_motion_lens<v.sky, v.big, v.stats, v.env, v.narrow, v.pool | 1>;
    else if constexpr (plan::view_has_motion(v.view)) return &integrate_kernel_motion<v.sky, v.big, v.stats, v.env, v.narrow, v.pool | 1>;
    else if constexpr (plan::view_has_lens(v.view)) return &integrate_kernel_lens<v.sky, v.big, v.stats, v.env, v.narrow, v.pool | 1>;
    else return &integrate_kernel<v.sky, v.big, v.stats, v.env, v.narrow, v.pool | v.view>;
}
template <int... I>
std::array<Kernel, sizeof...(I)> kernel_table(std::integer_sequence<int, I...>) { return {kernel_of<I>()...}; }
const auto kKernels = kernel_table(std::make_integer_sequence<int, plan::kKernelIds>());   // by plan::variant_id
static_assert(plan::variant_id({true, true, true, true, false, 0, plan::kViews - 1}) < plan::kAllVariants, "every view's ids fit the table");
// The projection kernels have no ids in the plan (a projection launch is planned as its camera twin, view 1): a table of their
// own, indexed by the twin's id within its view.
template <int R>
Kernel projection_kernel_of() {
    constexpr plan::Variant v = plan::variant_of(plan::kVariantsPerView + R);
    if constexpr (!plan::variant_exists(v, kBuild)) return nullptr;
    else return &integrate_kernel_projection<v.sky, v.big, v.stats, v.env, v.narrow, v.pool | 1>;
}
template <int... R>
std::array<Kernel, sizeof...(R)> projection_kernel_table(std::integer_sequence<int, R...>) { return {projection_kernel_of<R>()...}; }
const auto kProjectionKernels = projection_kernel_table(std::make_integer_sequence<int, plan::kVariantsPerView>());
// the kernel of a launch: variant v's, or with a projection the projection kernel of camera twin v
Kernel kernel_for(const plan::Variant &v, bool projection) {
    if (!projection) return kKernels[plan::variant_id(v)];
    return v.view == 1 ? kProjectionKernels[plan::variant_id(v) - plan::kVariantsPerView] : nullptr;
}
}  // namespace

hipError_t launch_integrator(const RenderArgs &args, const plan::Variant &v, hipStream_t stream) {
    const int rows = args.row_end - args.row_begin;
    if (rows <= 0 || args.width <= 0) return hipSuccess;
    if (v.room && (surface_unit_of(args) != kNoSurfaceUnit || args.env_map != nullptr || args.projection != 0)) return hipErrorInvalidDeviceFunction;   // (never planned: plan::Launch::room)
    if (const int unit = surface_unit_of(args)) return launch_surface_integrator(unit, args, v, stream);
    if (args.env_map != nullptr) return launch_environment_integrator(args, v, stream);   // (pt_environment_kernels.hip)
    const Kernel kernel = kernel_for(v, args.projection != 0);
    if (!kernel) return hipErrorInvalidDeviceFunction;
    hipLaunchKernelGGL(kernel, dim3(args.n_tiles * args.n_chunks), dim3(kBlock), 0, stream, args);
    return hipGetLastError();
}

// Waves (= workgroups: one wave each) of that kernel one compute unit holds at a time, from the runtime's occupancy
// calculation (registers, LDS, launch bounds): the scheduler's count of wave slots.  Asked once per kernel and device.
hipError_t integrator_waves_per_cu(const plan::Variant &v, int *waves) {
    constexpr int kDevices = 16;
    static std::atomic<int> cache[kDevices][plan::kKernelIds];   // 0 = not asked yet
    const Kernel kernel = kKernels[plan::variant_id(v)];
    if (!kernel) return hipErrorInvalidDeviceFunction;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<int> *cached = dev < kDevices ? &cache[dev][plan::variant_id(v)] : nullptr;
    int n = cached ? cached->load(std::memory_order_relaxed) : 0;
    if (n == 0) {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kBlock, 0);
        if (e == hipSuccess && n > 0) {
            // The runtime's calculator divides the CU's LDS by the kernel's bytes; the hardware hands LDS out in granules of 1 280
            // bytes (tools/lds_granule_probe.hip, profiles/r04_lds_granule.txt: 7 888 B -> 18 workgroups run, the runtime says 20).
            hipFuncAttributes fa;
            hipDeviceProp_t prop;
            if (hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(kernel)) == hipSuccess && fa.sharedSizeBytes > 0 &&
                hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.maxSharedMemoryPerMultiProcessor > 0) {
                constexpr size_t kLdsGranule = 1280;
                const size_t per_wave = (fa.sharedSizeBytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule;
                const size_t by_lds = std::max<size_t>(prop.maxSharedMemoryPerMultiProcessor, prop.sharedMemPerBlock) / per_wave;
                if (by_lds >= 1 && by_lds < static_cast<size_t>(n)) n = static_cast<int>(by_lds);
            }
        }
        if (e != hipSuccess || n <= 0) n = 0;
        else if (cached) cached->store(n, std::memory_order_relaxed);
    }
    if (n > 0) *waves = n;
    return e;
}
#endif

hipError_t launch_surface_integrator(int unit, const RenderArgs &args, const plan::Variant &v, hipStream_t stream) {
#if defined(PT_PHASE_TIMERS) || defined(PT_BLOCK_PROFILE)
    return hipErrorNotSupported;   // the diagnostic builds are linked without the surface units: a handle with one of their tables is refused (PT_ERR_UNSUPPORTED)
#else
    constexpr decltype(&launch_surface_unit<kGlassUnit>) kLaunch[] = {&launch_surface_unit<kGlassUnit>, &launch_surface_unit<kTextureUnit>, &launch_surface_unit<kSmoothUnit>,
                                                                      &launch_surface_unit<kRoughUnit>, &launch_surface_unit<kDirectUnit>, &launch_surface_unit<kEnvDirectUnit>,
                                                                      &launch_surface_unit<kRouletteUnit>};
    return unit >= kGlassUnit && unit <= kRouletteUnit ? kLaunch[unit - kGlassUnit](args, v, stream) : hipErrorInvalidValue;
#endif
}

const plan::Build &integrator_build() { return kBuild; }
#endif   // PT_ENVIRONMENT_UNIT

}  // namespace pt
