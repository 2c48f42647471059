// Environment sampling (include/pt_hip.h: environment sampling), the one copy of its arithmetic: the sampling table's record, the table's
// construction from an octahedral map (host only, double), the draw of a direction from the table and the term a diffuse hit adds for it
// before visibility.  The environment-sampling kernels (pt_kernels.hip: integrate_kernel_envdirect) run the sample per scattering
// diffuse hit that chose the sky, and pt_envdirect_term runs it on the host.  The sample and the term are float, every operation rounded
// once in the order written, nothing fused; roots and quotients are the correctly rounded ones.  `normalize` is the caller's normalize3.
//
// The Jacobian.  A point of the map's square q = (qx, qz) unfolds to p = (px, 1 - |px| - |pz|, pz) on the octahedron |x| + |y| + |z| = 1
// (upper half: px = qx, pz = qz; the lower half is the reflection of q in the nearest edge of the inner diamond, which preserves area),
// and the direction is p / |p|.  With a = dp/dpx = (1, -sgn px, 0) and b = dp/dpz = (0, -sgn pz, 1), a x b = (-sgn px, -1, -sgn pz)
// and p . (a x b) = -(|px| + py + |pz|) = -1, so d omega = |p . (a x b)| / |p|^3 dq = dq / |p|^3.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "pt_environment.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pt {

// The fourth Philox counter word of the environment sample's words (e0 .. e3); 3 is the direct term's (pt_direct.hpp).
constexpr uint32_t kEnvDirectStream = 4u;
constexpr int kEnvSampleMaxCells = 256;   // S = min(N, 256)

// One cell of the alias table (RenderArgs::env_alias; pt_hip.h: pt_env_sample_record has the same layout): 16 bytes, one load.
struct alignas(16) EnvAliasRec {
    float accept;      // the cell keeps a draw whose unit_float(e1) < accept; any other goes to `alias`
    int32_t alias;
    float pdf_self;    // probability per unit q-area of this cell, P_c * S^2 / 4
    float pdf_alias;   // the same of cell `alias`
};
static_assert(sizeof(EnvAliasRec) == 16, "one 16-byte load");

// The direction drawn by the words e0 .. e3 from a table of S x S cells: the cell by e0, kept or replaced by its alias by u1 =
// unit_float(e1), the point in the cell by u2, u3; its unfold p, w = normalize3(p) and the density per solid angle.
template <class Table, class Normalize, class Sqrt>
PT_GRADE_FN void envdirect_sample(const Table table, int32_t s, uint32_t e0, float u1, float u2, float u3, Normalize normalize, Sqrt sqrt_rn,
                                  int32_t &cell, float &wx, float &wy, float &wz, float &pdf_w) {
    const uint32_t cells = static_cast<uint32_t>(s) * static_cast<uint32_t>(s);
    const int32_t drawn = static_cast<int32_t>((static_cast<uint64_t>(e0) * cells) >> 32);
    const EnvAliasRec rec = table[drawn];
    const bool keep = u1 < rec.accept;
    const int32_t c = keep ? drawn : rec.alias;
    const float pdf_q = keep ? rec.pdf_self : rec.pdf_alias;
    cell = c;
    const int32_t cj = c / s, ci = c - cj * s;
    const float cw = 2.0f / static_cast<float>(s);
    const float qx = (static_cast<float>(ci) + u2) * cw - 1.0f;
    const float qz = (static_cast<float>(cj) + u3) * cw - 1.0f;
    const float ax = __builtin_fabsf(qx), az = __builtin_fabsf(qz);
    const float py = (1.0f - ax) - az;
    float px = qx, pz = qz;
    if (!(py >= 0.0f)) {   // the lower hemisphere: the fold, both from the folded qx, qz
        px = __builtin_copysignf(1.0f - az, qx);
        pz = __builtin_copysignf(1.0f - ax, qz);
    }
    const float len = sqrt_rn((px * px + py * py) + pz * pz);
    wx = px; wy = py; wz = pz;
    normalize(wx, wy, wz);
    pdf_w = pdf_q * ((len * len) * len);
}

// The term of direction w (density pdf_w, radiance L) for a diffuse hit with stored normal N, shading normal n, throughput T (after the
// texel step) and albedo Kd, where the environment is chosen with probability `share`.  Returns whether there is one.
PT_GRADE_FN bool envdirect_term(float wx, float wy, float wz, float pdf_w, float share, float lr, float lg, float lb, float Nx, float Ny, float Nz,
                                float nx, float ny, float nz, float tr, float tg, float tb, float kdr, float kdg, float kdb, float &cr, float &cg,
                                float &cb) {
    const float cn = (Nx * wx + Ny * wy) + Nz * wz;
    const float cs = (nx * wx + ny * wy) + nz * wz;
    cr = cg = cb = 0.0f;
    if (!(cn > 0.0f && cs > 0.0f && pdf_w > 0.0f && pdf_w < __builtin_inff())) return false;
    const float g = (cs * __builtin_fabsf(wz)) / ((3.141593f * pdf_w) * share);
    cr = ((tr * kdr) * lr) * g;
    cg = ((tg * kdg) * lg) * g;
    cb = ((tb * kdb) * lb) * g;
    return true;
}

// Host only from here on.
inline int envdirect_cells(int n) { return n < kEnvSampleMaxCells ? n : kEnvSampleMaxCells; }
inline double envdirect_lum(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }

// The table of an N x N map (its texels with the apron, env_with_apron): S = min(N, 256) cells a side; W_c = the cell's area in q times
// the mean over k x k sub-points, k = max(2, ceil(2 N / S)), of lum(max(L, 0)) / |p|^3 with L from env_lookup at the sub-point's
// direction (rows of sub-points, then columns, as env_from_equirect runs them); phi = the sum of W in cell order (row-major, qz the
// row); every cell then at least mean(W) / 16; P_c = W_c / sum.  The alias table by Vose's method on P_c S^2: the cells below 1 and
// the others on two stacks in ascending cell order; while both hold one, the top s of the small and the top l of the large are taken,
// accept_s = p_s, alias_s = l, p_l = (p_l + p_s) - 1, and l goes back on the stack its new p_l belongs to; every cell left has accept 1
// and is its own alias.  Returns false, with nothing built, where phi is zero or not finite.
inline bool envdirect_build(int n, const std::vector<EnvTexel> &texels, std::vector<EnvAliasRec> &out, double &phi) {
    const int s = envdirect_cells(n), k = std::max(2, (2 * n + s - 1) / s);
    const size_t cells = static_cast<size_t>(s) * s;
    std::vector<double> w(cells);
    phi = 0.0;
    for (int cj = 0; cj < s; ++cj)
        for (int ci = 0; ci < s; ++ci) {
            double acc = 0.0;
            for (int sj = 0; sj < k; ++sj)
                for (int si = 0; si < k; ++si) {
                    const double qx = 2.0 * ((ci + (si + 0.5) / k) / s) - 1.0, qz = 2.0 * ((cj + (sj + 0.5) / k) / s) - 1.0;
                    double dx, dz;
                    const double dy = 1.0 - std::fabs(qx) - std::fabs(qz);
                    if (dy >= 0.0) {
                        dx = qx; dz = qz;
                    } else {
                        dx = std::copysign(1.0 - std::fabs(qz), qx);
                        dz = std::copysign(1.0 - std::fabs(qx), qz);
                    }
                    const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
                    float lr, lg, lb;
                    env_lookup(texels.data(), n, static_cast<float>(dx / len), static_cast<float>(dy / len), static_cast<float>(dz / len), lr, lg, lb);
                    const double r = lr > 0.0f ? lr : 0.0, g = lg > 0.0f ? lg : 0.0, b = lb > 0.0f ? lb : 0.0;
                    acc += envdirect_lum(r, g, b) / ((len * len) * len);
                }
            const double wc = (4.0 / static_cast<double>(cells)) * (acc / (k * k));
            w[static_cast<size_t>(cj) * s + ci] = wc;
            phi += wc;
        }
    if (!(phi > 0.0) || !std::isfinite(phi)) return false;
    const double floor_w = phi / static_cast<double>(cells) / 16.0;
    double total = 0.0;
    for (double &x : w) {
        if (x < floor_w) x = floor_w;
        total += x;
    }
    std::vector<double> prob(cells), p(cells);
    std::vector<int32_t> small, large;
    for (size_t c = 0; c < cells; ++c) {
        prob[c] = w[c] / total;
        p[c] = prob[c] * static_cast<double>(cells);
        (p[c] < 1.0 ? small : large).push_back(static_cast<int32_t>(c));
    }
    const double per_q = static_cast<double>(cells) / 4.0;
    out.assign(cells, EnvAliasRec{1.0f, 0, 0.0f, 0.0f});
    for (size_t c = 0; c < cells; ++c) {
        out[c].alias = static_cast<int32_t>(c);
        out[c].pdf_self = out[c].pdf_alias = static_cast<float>(prob[c] * per_q);
    }
    while (!small.empty() && !large.empty()) {
        const int32_t sm = small.back(), lg = large.back();
        small.pop_back(); large.pop_back();
        out[sm].accept = static_cast<float>(p[sm]);
        out[sm].alias = lg;
        out[sm].pdf_alias = out[lg].pdf_self;
        p[lg] = (p[lg] + p[sm]) - 1.0;
        (p[lg] < 1.0 ? small : large).push_back(lg);
    }
    return true;
}

}  // namespace pt
