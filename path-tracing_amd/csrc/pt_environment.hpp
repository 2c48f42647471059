// Environment lighting (include/pt_hip.h: pt_environment_*), the one copy of its arithmetic: the octahedral map's lookup, which the
// environment kernels (pt_kernels.hip: integrate_kernel_environment) run per miss and pt_environment_lookup runs on the host, the apron
// rule and the conversion of an equirectangular picture into the map (host only, double).  The lookup is float, every operation
// rounded once, nothing fused; no trigonometry, no double.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pt_grade.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

constexpr int kEnvMinSize = 8, kEnvMaxSize = 4096;           // N of an octahedral map
constexpr int kEnvMaxSourceW = 16384, kEnvMaxSourceH = 8192;   // the largest equirectangular picture a map is made from

struct alignas(16) EnvTexel { float r, g, b, pad; };   // 16 bytes: one load

// Texel (i, j), -1 <= i, j <= N, of the (N + 2) x (N + 2) array with its one-texel apron.
PT_GRADE_FN size_t env_index(int n, int i, int j) { return static_cast<size_t>(j + 1) * static_cast<size_t>(n + 2) + static_cast<size_t>(i + 1); }

// f = (q * 0.5 + 0.5) * N - 0.5 split into the texel below (clamped to -1 .. N - 1; a NaN goes to -1) and the weight of the next one.
PT_GRADE_FN void env_cell(float q, int n, int &i0, float &w) {
    const float f = (q * 0.5f + 0.5f) * static_cast<float>(n) - 0.5f;
    const float fl = __builtin_floorf(f);
    i0 = fl >= -1.0f ? (fl <= static_cast<float>(n - 1) ? static_cast<int>(fl) : n - 1) : -1;
    w = f - static_cast<float>(i0);
}

// The radiance the map holds for unit direction d (y is the pole axis): pt_hip.h states every step.
template <class Texels>
PT_GRADE_FN void env_lookup(const Texels map, int n, float dx, float dy, float dz, float &lr, float &lg, float &lb) {
    const float s = (__builtin_fabsf(dx) + __builtin_fabsf(dy)) + __builtin_fabsf(dz);
    const float px = dx / s, pz = dz / s;
    float qx = px, qz = pz;
    if (dy < 0.0f) {   // the lower hemisphere folds outwards; both from the unfolded px, pz
        qx = __builtin_copysignf(1.0f - __builtin_fabsf(pz), px);
        qz = __builtin_copysignf(1.0f - __builtin_fabsf(px), pz);
    }
    int x0, y0;
    float ax, ay;
    env_cell(qx, n, x0, ax);
    env_cell(qz, n, y0, ay);
    const size_t at = env_index(n, x0, y0), row = static_cast<size_t>(n + 2);
    const EnvTexel t00 = map[at], t10 = map[at + 1], t01 = map[at + row], t11 = map[at + row + 1];
    const float bx = 1.0f - ax, by = 1.0f - ay;
    lr = (t00.r * bx + t10.r * ax) * by + (t01.r * bx + t11.r * ax) * ay;
    lg = (t00.g * bx + t10.g * ax) * by + (t01.g * bx + t11.g * ax) * ay;
    lb = (t00.b * bx + t10.b * ax) * by + (t01.b * bx + t11.b * ax) * ay;
}

// Host only from here on.
// The (N + 2)^2 array of an N x N x 3 map: the interior, then the apron by the octahedral fold (a point just outside an edge is the
// point mirrored about that edge's midpoint); the corners by the two rules in turn, columns first.
inline std::vector<EnvTexel> env_with_apron(int n, const float *rgb) {
    std::vector<EnvTexel> t(static_cast<size_t>(n + 2) * (n + 2));
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const float *p = rgb + 3 * (static_cast<size_t>(j) * n + i);
            t[env_index(n, i, j)] = {p[0], p[1], p[2], 0.0f};
        }
    for (int j = 0; j < n; ++j) {
        t[env_index(n, -1, j)] = t[env_index(n, 0, n - 1 - j)];
        t[env_index(n, n, j)] = t[env_index(n, n - 1, n - 1 - j)];
    }
    for (int i = -1; i <= n; ++i) {   // (with the two apron columns: the corners)
        const int m = n - 1 - i;      // -1 <-> n
        t[env_index(n, i, -1)] = t[env_index(n, m, 0)];
        t[env_index(n, i, n)] = t[env_index(n, m, n - 1)];
    }
    return t;
}

// Default N for a picture h rows high: the smallest power of two >= h, clamped to 8 .. 2048.
inline int env_default_size(int h) {
    int n = 8;
    while (n < h && n < 2048) n *= 2;
    return n;
}

// The conversion (pt_hip.h: pt_environment_from_equirect): all in double, one rounding to float at the end.
inline void env_from_equirect(int w, int h, const float *src, double gain, double rotate_degrees, int n, float *map_rgb) {
    const double pi = 3.14159265358979323846;
    const int k = std::min(8, std::max(1, (w + n - 1) / n));
    const double ang = rotate_degrees * pi / 180.0, ca = std::cos(ang), sa = std::sin(ang);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int sj = 0; sj < k; ++sj)
                for (int si = 0; si < k; ++si) {
                    // the sub-cell's centre in [-1, 1]^2, the inverse of the direction-to-map rule, normalised
                    const double qx = 2.0 * ((i + (si + 0.5) / k) / n) - 1.0, qz = 2.0 * ((j + (sj + 0.5) / k) / n) - 1.0;
                    double dx, dz;
                    const double dy = 1.0 - std::fabs(qx) - std::fabs(qz);
                    if (dy >= 0.0) {
                        dx = qx; dz = qz;
                    } else {
                        dx = std::copysign(1.0 - std::fabs(qz), qx);
                        dz = std::copysign(1.0 - std::fabs(qx), qz);
                    }
                    const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
                    const double ux = dx / len, uy = dy / len, uz = dz / len;
                    // rotated about +y by the caller's angle
                    const double rx = ca * ux + sa * uz, rz = -sa * ux + ca * uz;
                    // the skybox's convention: theta down the rows, phi along the columns
                    const double theta = std::acos(std::min(1.0, std::max(-1.0, uy))) / pi;
                    const double phi = std::atan2(rz, -rx) / (2.0 * pi) + 0.5;
                    const double fx = phi * w, fy = theta * h;   // (texel x's full weight at fx = x, as in the skybox lookup)
                    const double flx = std::floor(fx), fly = std::floor(fy);
                    const double ax = fx - flx, ay = fy - fly;
                    const long long x0 = static_cast<long long>(flx), y0 = static_cast<long long>(fly);
                    const int xa = static_cast<int>(((x0 % w) + w) % w), xb = static_cast<int>((((x0 + 1) % w) + w) % w);   // wraps in x
                    const int ya = static_cast<int>(std::min<long long>(h - 1, std::max<long long>(0, y0)));                // clamps in y
                    const int yb = static_cast<int>(std::min<long long>(h - 1, std::max<long long>(0, y0 + 1)));
                    for (int c = 0; c < 3; ++c) {
                        const double t00 = src[3 * (static_cast<size_t>(ya) * w + xa) + c], t10 = src[3 * (static_cast<size_t>(ya) * w + xb) + c];
                        const double t01 = src[3 * (static_cast<size_t>(yb) * w + xa) + c], t11 = src[3 * (static_cast<size_t>(yb) * w + xb) + c];
                        acc[c] += (t00 * (1.0 - ax) + t10 * ax) * (1.0 - ay) + (t01 * (1.0 - ax) + t11 * ax) * ay;
                    }
                }
            for (int c = 0; c < 3; ++c) map_rgb[3 * (static_cast<size_t>(j) * n + i) + c] = static_cast<float>(acc[c] / (k * k) * gain);
        }
}
}  // namespace pt
