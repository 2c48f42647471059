// The normal generator (include/pt_hip.h: pt_smooth_normals): per-corner normals of a triangle soup.  Corners whose positions are
// bit-identical are one vertex; a corner's normal is the angle-weighted sum of the geometric face normals of the triangles at its
// vertex that lie within the crease angle of the corner's own face, normalised.  Host only, plain C++, accumulated in double.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "pt_smooth_normals.hpp"

namespace pt {

namespace {

struct Key {
    uint32_t b[3];
    bool operator<(const Key &o) const { return std::memcmp(b, o.b, sizeof b) < 0; }
};

struct Face {
    double n[3];       // unit geometric normal
    double angle[3];   // the interior angle at each corner
    bool ok;           // false: degenerate -- contributes nothing, receives zeros
};

double dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

Face face_of(const float *v) {
    Face f{};
    double p[3][3];
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) p[c][k] = v[3 * c + k];
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double len = std::sqrt(dot(c, c));
    f.ok = std::isfinite(len) && len > 0.0;
    if (!f.ok) return f;
    for (int k = 0; k < 3; ++k) f.n[k] = c[k] / len;
    for (int i = 0; i < 3; ++i) {
        const double *a = p[i], *b = p[(i + 1) % 3], *d = p[(i + 2) % 3];
        const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {d[0] - a[0], d[1] - a[1], d[2] - a[2]};
        double cs = dot(u, w) / std::sqrt(dot(u, u) * dot(w, w));
        cs = cs < -1.0 ? -1.0 : cs > 1.0 ? 1.0 : cs;
        f.angle[i] = std::acos(cs);
        if (!std::isfinite(f.angle[i])) f.ok = false;
    }
    return f;
}

}  // namespace

void smooth_normals(int32_t n_tri, const float *vertices, double crease_degrees, float *out) {
    const size_t n = static_cast<size_t>(n_tri);
    std::vector<Face> faces(n);
    std::map<Key, std::vector<uint32_t>> at;   // vertex -> the corners (3 * triangle + corner) that lie on it
    for (size_t t = 0; t < n; ++t) {
        faces[t] = face_of(vertices + 9 * t);
        if (!faces[t].ok) continue;
        for (int c = 0; c < 3; ++c) {
            Key k;
            std::memcpy(k.b, vertices + 9 * t + 3 * c, sizeof k.b);
            at[k].push_back(static_cast<uint32_t>(3 * t + c));
        }
    }
    const double limit = std::cos(crease_degrees * (3.14159265358979323846 / 180.0));
    for (size_t i = 0; i < 9 * n; ++i) out[i] = 0.0f;
    for (const auto &vertex : at) {
        const std::vector<uint32_t> &corners = vertex.second;
        for (const uint32_t mine : corners) {
            const Face &f = faces[mine / 3];
            double sum[3] = {0.0, 0.0, 0.0};
            for (const uint32_t other : corners) {
                const Face &g = faces[other / 3];
                if (other / 3 != mine / 3 && !(dot(f.n, g.n) >= limit)) continue;   // (a corner's own face always counts)
                for (int k = 0; k < 3; ++k) sum[k] += g.angle[other % 3] * g.n[k];
            }
            const double len = std::sqrt(dot(sum, sum));
            if (std::isfinite(len) && len > 0.0)
                for (int k = 0; k < 3; ++k) out[3 * static_cast<size_t>(mine) + k] = static_cast<float>(sum[k] / len);
        }
    }
}

}  // namespace pt
