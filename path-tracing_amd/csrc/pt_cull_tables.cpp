// The culling hierarchy (host side, plain C++): which triangles are culled how, the slot order, the sphere trees of small scenes,
// the box tree of big ones, the barycentric records of the large class and the margins that make every test conservative
// (DESIGN.md "Culling").  build_cull_tables at the end of the file is the list of the stages.
#include "pt_scene.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pt {

// PT_KNOB: a knob of the test build (pt_scene.hpp: CullMutation) and what the shipped library has in its place.
#ifdef PT_TEST_HOOKS
CullMutation g_cull_mutation;
#define PT_KNOB(field, shipped) (g_cull_mutation.field)
#else
#define PT_KNOB(field, shipped) (shipped)
#endif

namespace {

struct V3 {
    double x, y, z;
};
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 crs(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dt(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline double nrm(V3 a) { return std::sqrt(dt(a, a)); }

// What an accepted hit point of one triangle can be, in exact arithmetic (DESIGN.md "Culling"):
// barycentric coordinates >= -m_geo, distance from the triangle's own plane <= h_max.
struct TriGeo {
    V3 v[3];
    double area2;    // parallelogram area S
    double diam;     // longest edge
    double m_geo;    // (eps + E_fp) / (2 S)
    double h_max;    // sqrt(2 S E + E^2) / perimeter
    double a_max;    // largest barycentric gradient
    bool degenerate;
};

const double kU = 5.9604644775390625e-08;   // unit roundoff of binary32

TriGeo tri_geometry(const float *r, double eps) {
    TriGeo g;
    g.v[0] = {r[4], r[5], r[6]};
    g.v[1] = {r[7], r[8], r[9]};
    g.v[2] = {r[10], r[11], r[12]};
    const V3 e1 = sub(g.v[1], g.v[0]), e2 = sub(g.v[2], g.v[0]), e3 = sub(g.v[2], g.v[1]);
    g.area2 = nrm(crs(e1, e2));
    g.diam = std::max(nrm(e1), std::max(nrm(e2), nrm(e3)));
    const double perim = nrm(e1) + nrm(e2) + nrm(e3);
    // float error of the reference's |S - s1 - s2 - s3| for a point near the triangle: three cross products of
    // vectors no longer than ~diam, three lengths, three subtractions
    const double e_fp = 48.0 * kU * (g.diam + 1e-3) * (g.diam + 1e-3);   // first-order worst case 37 u, largest seen 32 u (tests/test_cull_margins_host.py)
    const double big_e = std::fabs(eps) + e_fp;
    // A triangle whose area is within a few eps of zero is accepted by the reference for points that have nothing to
    // do with it (all three computed sub-areas can vanish far away): never cull it.
    g.degenerate = !(g.area2 > 4.0 * big_e) || !std::isfinite(g.area2) || !std::isfinite(g.diam);
    if (g.degenerate) {
        g.m_geo = g.h_max = g.a_max = INFINITY;
    } else {
        g.m_geo = big_e / (2.0 * g.area2);
        g.h_max = std::sqrt(2.0 * g.area2 * big_e + big_e * big_e) / perim;
        g.a_max = g.diam / g.area2;   // gradients of the barycentric functions are 1/height; smallest height = S/diam
    }
    return g;
}

// One step of Ritter's algorithm: the smallest sphere that holds the sphere (c, rad) and the point p.
inline void ritter_grow(V3 &c, double &rad, V3 p) {
    const V3 d = sub(p, c);
    const double dist = nrm(d);
    if (dist > rad) {
        const double nr = (rad + dist) / 2, k = (nr - rad) / dist;
        c = {c.x + d.x * k, c.y + d.y * k, c.z + d.z * k};
        rad = nr;
    }
}

void push_vertices(const HostScene &s, int t, std::vector<V3> &out) {
    for (int v = 0; v < 3; ++v) {
        const float *p = &s.tri[14 * static_cast<size_t>(t) + 4 + 3 * v];
        out.push_back({p[0], p[1], p[2]});
    }
}

// Ritter's bounding sphere of a point set, then grown to cover every point exactly.
void bounding_sphere(const std::vector<V3> &pts, V3 &c, double &rad) {
    if (pts.empty()) { c = {0, 0, 0}; rad = 0; return; }
    auto far_from = [&](V3 p) {
        size_t best = 0; double bd = -1;
        for (size_t i = 0; i < pts.size(); ++i) { const double d = nrm(sub(pts[i], p)); if (d > bd) { bd = d; best = i; } }
        return best;
    };
    const V3 a = pts[far_from(pts[0])];
    const V3 b = pts[far_from(a)];
    c = {(a.x + b.x) / 2, (a.y + b.y) / 2, (a.z + b.z) / 2};
    rad = nrm(sub(a, b)) / 2;
    for (int it = 0; it < 2; ++it)
        for (const V3 &p : pts) ritter_grow(c, rad, p);
    for (const V3 &p : pts) rad = std::max(rad, nrm(sub(p, c)));
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// Slot order: which triangles are culled how, and in what order the tables list them
// ---------------------------------------------------------------------------------------------------
namespace {

struct Centroid {
    double c[3];
};

// Total order on triangles that depends on their GEOMETRY only (the file order enters last, for exact duplicates), so
// that a shuffled OBJ gives the same hierarchy.
struct GeoLess {
    const HostScene *s;
    const std::vector<Centroid> *cen;
    int axis;
    bool operator()(int a, int b) const {
        for (int k = 0; k < 3; ++k) {
            const double x = (*cen)[a].c[(axis + k) % 3], y = (*cen)[b].c[(axis + k) % 3];
            if (x != y) return x < y;
        }
        const int m = std::memcmp(&s->tri[14 * static_cast<size_t>(a)], &s->tri[14 * static_cast<size_t>(b)], 14 * sizeof(float));
        if (m != 0) return m < 0;
        return a < b;
    }
};

int longest_axis(const std::vector<int> &ids, size_t b, size_t e, const std::vector<Centroid> &cen) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = b; i < e; ++i)
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], cen[ids[i]].c[k]);
            hi[k] = std::max(hi[k], cen[ids[i]].c[k]);
        }
    int ax = 0;
    for (int k = 1; k < 3; ++k)
        if (hi[k] - lo[k] > hi[ax] - lo[ax]) ax = k;
    return ax;
}

// Reorders ids[b, e) into `sizes.size()` consecutive groups of the given sizes, each spatially compact: recursive
// bisection of the group list along the longest axis of the centroids.
void partition_groups(std::vector<int> &ids, size_t b, const std::vector<size_t> &sizes, size_t g0, size_t g1, const HostScene &s,
                      const std::vector<Centroid> &cen) {
    if (g1 - g0 <= 1) return;
    const size_t gm = g0 + (g1 - g0) / 2;
    size_t left = 0, total = 0;
    for (size_t g = g0; g < g1; ++g) {
        if (g < gm) left += sizes[g];
        total += sizes[g];
    }
    // the cut that leaves the two most compact halves: smallest sum of (bounding-sphere radius)^2 x triangles over the
    // three axes (a ray meets a sphere with probability ~ r^2)
    int best_axis = longest_axis(ids, b, b + total, cen);
    if (total <= 4096) {
        double best_cost = INFINITY;
        std::vector<int> tmp(ids.begin() + b, ids.begin() + b + total);
        for (int axis = 0; axis < 3; ++axis) {
            std::nth_element(tmp.begin(), tmp.begin() + left, tmp.end(), GeoLess{&s, &cen, axis});
            double cost = 0;
            for (int half = 0; half < 2; ++half) {
                const size_t h0 = half ? left : 0, h1 = half ? total : left;
                std::vector<V3> pts;
                for (size_t i = h0; i < h1; ++i) push_vertices(s, tmp[i], pts);
                std::sort(pts.begin(), pts.end(), [](const V3 &x, const V3 &y) { return x.x != y.x ? x.x < y.x : x.y != y.y ? x.y < y.y : x.z < y.z; });
                V3 c; double rad;
                bounding_sphere(pts, c, rad);
                cost += rad * rad * static_cast<double>(h1 - h0);
            }
            if (cost < best_cost) { best_cost = cost; best_axis = axis; }
        }
    }
    const GeoLess less{&s, &cen, best_axis};
    std::nth_element(ids.begin() + b, ids.begin() + b + left, ids.begin() + b + total, less);
    partition_groups(ids, b, sizes, g0, gm, s, cen);
    partition_groups(ids, b + left, sizes, gm, g1, s, cen);
}

// Surface-area-heuristic version for the box tree of big scenes: splits ids[b, e) into k consecutive children of AT MOST
// `cap` triangles each (sizes appended to `sizes`), by recursive bisection: each cut goes, along the best of the three
// axes, where area(left) * n_left + area(right) * n_right of the triangles' bounding boxes is smallest among the
// positions the capacities allow -- so children follow the objects of the scene (the gaps between them) instead of
// cutting through them at equal counts.
struct Box {
    double lo[3], hi[3];
    void grow(const Box &b) { for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], b.lo[k]); hi[k] = std::max(hi[k], b.hi[k]); } }
    double area() const {
        const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
        return x < 0 ? 0.0 : 2.0 * (x * y + y * z + z * x);
    }
};
const Box kEmptyBox = {{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
void split_sah(std::vector<int> &ids, size_t b, size_t e, size_t k, size_t cap, const HostScene &s, const std::vector<Centroid> &cen,
               const std::vector<Box> &tbox, std::vector<size_t> &sizes) {
    const size_t n = e - b;
    if (k <= 1) {
        sizes.push_back(n);
        return;
    }
    const size_t k1 = k / 2, k2 = k - k1;
    // n_left must leave no more than k2 * cap on the right, no more than k1 * cap on the left, and at least k1 / k2
    // triangles on each side (no empty child)
    const size_t lo = std::max(k1, n > k2 * cap ? n - k2 * cap : 0), hi = std::min(n - k2, k1 * cap);
    double best_cost = INFINITY;
    int best_axis = 0;
    size_t best_at = (lo + hi) / 2;
    std::vector<int> sorted(ids.begin() + b, ids.begin() + e), best_order;
    std::vector<double> right_area(n + 1);
    for (int axis = 0; axis < 3; ++axis) {
        const GeoLess less{&s, &cen, axis};
        std::sort(sorted.begin(), sorted.end(), less);
        Box acc = kEmptyBox;
        right_area[n] = 0;
        for (size_t i = n; i-- > 0;) {
            acc.grow(tbox[sorted[i]]);
            right_area[i] = acc.area();
        }
        acc = kEmptyBox;
        for (size_t i = 1; i < n; ++i) {   // left = sorted[0, i)
            acc.grow(tbox[sorted[i - 1]]);
            if (i < lo || i > hi) continue;
            const double cost = acc.area() * static_cast<double>(i) + right_area[i] * static_cast<double>(n - i);
            if (cost < best_cost) {
                best_cost = cost;
                best_axis = axis;
                best_at = i;
            }
        }
        if (best_axis == axis && best_cost < INFINITY) best_order = sorted;
    }
    if (!best_order.empty()) std::copy(best_order.begin(), best_order.end(), ids.begin() + b);
    split_sah(ids, b, b + best_at, k1, cap, s, cen, tbox, sizes);
    split_sah(ids, b + best_at, e, k2, cap, s, cen, tbox, sizes);
}

// Orders ids[b, e) so that every aligned run of 8^L consecutive entries (L = 1, 2, ...) is spatially compact: the
// implicit 8-ary sphere tree of a small-scene cluster is laid over this order.
void arrange_implicit(std::vector<int> &ids, size_t b, size_t e, const HostScene &s, const std::vector<Centroid> &cen) {
    const size_t n = e - b;
    if (n <= static_cast<size_t>(kFan)) {   // a leaf group: canonical order, whatever order the triangles arrived in
        std::sort(ids.begin() + b, ids.begin() + e, GeoLess{&s, &cen, 0});
        return;
    }
    size_t cap = kFan;   // capacity of one child subtree
    while (cap * kFan < n) cap *= kFan;
    std::vector<size_t> sizes;
    for (size_t left = n; left > 0; left -= std::min(left, cap)) sizes.push_back(std::min(left, cap));
    partition_groups(ids, b, sizes, 0, sizes.size(), s, cen);
    size_t at = b;
    for (size_t sz : sizes) {
        arrange_implicit(ids, at, at + sz, s, cen);
        at += sz;
    }
}

// Alternative arrangement for small clusters: compact PATCHES instead of axis-aligned cells.  Items (triangles, then
// groups of 8, then groups of 64, ...) are peeled off from the outside in: the item farthest from the centre of what is
// left seeds a group, its 7 nearest remaining items join it.  Surfaces (a torus, a sphere) pack tighter this way than
// under planar cuts.  Reorders ids[b, e); the last group of every level is the partial one, as the implicit tree needs.
void arrange_patches(std::vector<int> &ids, size_t b, size_t e, const HostScene &s, const std::vector<Centroid> &cen) {
    struct Item { std::vector<int> tris; double c[3]; };
    std::vector<Item> items;
    for (size_t i = b; i < e; ++i) items.push_back({{ids[i]}, {cen[ids[i]].c[0], cen[ids[i]].c[1], cen[ids[i]].c[2]}});
    const GeoLess less{&s, &cen, 0};
    while (items.size() > 1) {
        std::vector<uint8_t> used(items.size(), 0);
        std::vector<Item> next;
        size_t left = items.size();
        while (left > 0) {
            double m[3] = {0, 0, 0};
            for (size_t i = 0; i < items.size(); ++i)
                if (!used[i]) for (int k = 0; k < 3; ++k) m[k] += items[i].c[k] / static_cast<double>(left);
            auto d2 = [](const double *p, const double *q) { return (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2]); };
            // the seed: farthest from the centre of the remaining items (geometry breaks ties, not the file order)
            size_t seed = items.size();
            for (size_t i = 0; i < items.size(); ++i) {
                if (used[i]) continue;
                if (seed == items.size()) { seed = i; continue; }
                const double a = d2(items[i].c, m), z = d2(items[seed].c, m);
                if (a > z || (a == z && less(items[i].tris[0], items[seed].tris[0]))) seed = i;
            }
            const size_t take = std::min<size_t>(kFan, left);
            // grow the group by the item that enlarges its bounding sphere least (on a curved surface that follows the
            // curvature -- a half ring of a tube fits a smaller sphere than a flat-looking patch of the same area)
            std::vector<size_t> member = {seed};
            used[seed] = 1;
            auto verts_of = [&](const Item &it, std::vector<V3> &out) {
                for (int t : it.tris) push_vertices(s, t, out);
            };
            std::vector<V3> pts;
            verts_of(items[seed], pts);
            V3 gc; double gr;
            bounding_sphere(pts, gc, gr);
            for (size_t k = 1; k < take; ++k) {
                size_t best = items.size();
                double best_r = INFINITY;
                for (size_t i = 0; i < items.size(); ++i) {
                    if (used[i]) continue;
                    std::vector<V3> q;
                    verts_of(items[i], q);
                    double r = gr;   // Ritter-style growth of (gc, gr) over the candidate's vertices
                    V3 c = gc;
                    for (const V3 &p : q) ritter_grow(c, r, p);
                    if (r < best_r || (r == best_r && (best == items.size() || less(items[i].tris[0], items[best].tris[0])))) { best_r = r; best = i; }
                }
                used[best] = 1;
                member.push_back(best);
                verts_of(items[best], pts);
                bounding_sphere(pts, gc, gr);
            }
            left -= take;
            Item g;
            g.c[0] = g.c[1] = g.c[2] = 0;
            std::sort(member.begin(), member.end(), [&](size_t x, size_t y) { return less(items[x].tris[0], items[y].tris[0]); });
            for (size_t i : member) {
                g.tris.insert(g.tris.end(), items[i].tris.begin(), items[i].tris.end());
                for (int k = 0; k < 3; ++k) g.c[k] += items[i].c[k] / static_cast<double>(member.size());
            }
            next.push_back(std::move(g));
        }
        // the partial group (if any) was formed last: it already sits at the end.  But a group of full SUBGROUPS must not
        // follow a partial subgroup inside one parent: partial items can only be the very last item of the level, which
        // holds because only the last-formed group can contain the (single) partial item... unless the peeling picked it
        // earlier: move the item with the fewest triangles to the end of its level.
        size_t small = 0;
        for (size_t i = 1; i < next.size(); ++i) if (next[i].tris.size() < next[small].tris.size()) small = i;
        if (next[small].tris.size() < next.back().tris.size()) std::swap(next[small], next.back());
        items.swap(next);
    }
    std::copy(items[0].tris.begin(), items[0].tris.end(), ids.begin() + b);
}

struct UnionFind {
    std::vector<int> p;
    explicit UnionFind(int n) : p(n) { for (int i = 0; i < n; ++i) p[i] = i; }
    int find(int x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; }
    void unite(int a, int b) { a = find(a); b = find(b); if (a != b) p[std::max(a, b)] = std::min(a, b); }
};

// Axis-aligned box of every point Triangle::Intersect can accept for this triangle (DESIGN.md "Culling"): barycentric
// coordinates >= -m_geo (the triangle grown about its centroid: vertex k moves to v_k + m (2 v_k - v_i - v_j)), at most
// h_max off the triangle's own plane (displacement h_max |n_axis| per axis), plus the float rounding of
// P* = o + d t* (eps_line).
Box acceptance_box(const TriGeo &g, double eps_line) {
    Box b = kEmptyBox;
    const double m = g.m_geo;
    for (int k = 0; k < 3; ++k) {
        const V3 &v = g.v[k], &a = g.v[(k + 1) % 3], &c = g.v[(k + 2) % 3];
        const double p[3] = {v.x + m * (2 * v.x - a.x - c.x), v.y + m * (2 * v.y - a.y - c.y), v.z + m * (2 * v.z - a.z - c.z)};
        for (int x = 0; x < 3; ++x) { b.lo[x] = std::min(b.lo[x], p[x]); b.hi[x] = std::max(b.hi[x], p[x]); }
    }
    const V3 nn = crs(sub(g.v[1], g.v[0]), sub(g.v[2], g.v[0]));
    const double len = nrm(nn);
    const double n[3] = {std::fabs(nn.x) / len, std::fabs(nn.y) / len, std::fabs(nn.z) / len};
    for (int x = 0; x < 3; ++x) {
        const double pad = g.h_max * n[x] * (1.0 + 1e-9) + eps_line;
        b.lo[x] -= pad;
        b.hi[x] += pad;
#ifdef PT_TEST_HOOKS
        // mutation testing: scale the box about its centre (1 = as shipped)
        const double c = 0.5 * (b.lo[x] + b.hi[x]), h = 0.5 * (b.hi[x] - b.lo[x]) * g_cull_mutation.box;
        b.lo[x] = c - h;
        b.hi[x] = c + h;
#endif
    }
    return b;
}

// ---------------------------------------------------------------------------------------------------
// Box tree of big scenes
// ---------------------------------------------------------------------------------------------------
#ifndef PT_BVH_MODE
#define PT_BVH_MODE 1   // box-tree builder of big scenes: 0 = uniform depth (uniform_topology), 1 = binary SAH collapsed to 8-wide nodes (sah_topology)
#endif

// One node of the box tree from its own box and its children's: the children as 8-bit boxes in the node's frame, rounded outward.
// `base`: an inner node's first child node (its children are consecutive), a leaf's first slot / 8.
void quantise_node(BvhNode &q, const Box &nb, const Box *kids, size_t k, bool leaf, uint32_t base) {
    std::memset(&q, 0, sizeof q);
    double extent = 0;
    for (int x = 0; x < 3; ++x) {
        float f = static_cast<float>(nb.lo[x]);
        if (static_cast<double>(f) > nb.lo[x]) f = std::nextafterf(f, -INFINITY);
        q.org[x] = f;
        extent = std::max(extent, nb.hi[x] - static_cast<double>(f));
    }
    int e = extent > 0 ? static_cast<int>(std::ceil(std::log2(extent / 255.0))) : -100;
    e = std::max(-100, std::min(100, e));
    while (std::ceil(extent / std::ldexp(1.0, e)) > 255.0) ++e;
    const double step = std::ldexp(1.0, e);
    for (size_t c = 0; c < k; ++c)
        for (int x = 0; x < 3; ++x) {
            const double lo = std::floor((kids[c].lo[x] - static_cast<double>(q.org[x])) / step);
            const double hi = std::ceil((kids[c].hi[x] - static_cast<double>(q.org[x])) / step);
            q.lo[x][c] = static_cast<uint8_t>(std::max(0.0, std::min(255.0, lo)));
            q.hi[x][c] = static_cast<uint8_t>(std::max(0.0, std::min(255.0, hi)));
        }
    // (base: an inner node's first child or a leaf's ordinal -- the tree's slots are the FIRST slots of the global order, so a
    // leaf's first slot / 8 is its ordinal among the leaves --: below the node count either way, which check_table_limits bounds
    // by 2^20 before any table reaches a device; a tree beyond that is still built, with the field wrapped, and then refused)
    q.meta = static_cast<uint32_t>(e + 127) | (static_cast<uint32_t>(k - 1) << 8) | (leaf ? 1u << 11 : 0u) | ((base & 0xFFFFFu) << 12);
}

// What a tree builder decides: the topology.  Nodes are numbered so that a node's children are consecutive and come after
// it (the root is node 0); a leaf is the range [b, e) of the builder's triangle list, an inner node its first child and
// their number.
struct TreeNode {
    size_t b, e;
    uint32_t first_child, n_kids;   // n_kids == 0: a leaf
};

// Uniform depth, up to 8 children per node, every node's triangles split into spatially compact children of (nearly) equal
// size.  Levels are listed from the top, the leaves last.
std::vector<TreeNode> uniform_topology(const HostScene &s, const std::vector<Centroid> &cen, const std::vector<Box> &tbox, std::vector<int> &ids) {
    const size_t n = ids.size();
    int top = 1;
    for (size_t cap = kFan; cap < n; cap *= kFan) ++top;
    std::vector<TreeNode> nodes = {{0, n, 0, 0}};
    size_t level_begin = 0;
    for (int L = top; L >= 2; --L) {   // level 1 = leaves
        size_t cap = 1;
        for (int k = 0; k < L - 1; ++k) cap *= kFan;       // capacity of a child
        const size_t level_end = nodes.size();
        for (size_t w = level_begin; w < level_end; ++w) {
            // as many children as keeps them at most half full -- in effect eight wherever the count allows: a uniform-depth
            // tree over n triangles has room for up to 8x n anyway, and nodes with few, full children only add levels
            // whose boxes prune little (x195 replica: 14.1 instead of 17.4 box rounds per wave-segment, +13 %; fill
            // factors from 0.25 to 0.5 build the same trees for the replicas, 0.55 and above lose) --
            // never fewer than the capacity demands
            const size_t b = nodes[w].b, e = nodes[w].e, cnt = e - b, k_min = (cnt + cap - 1) / cap;
            const double fill = PT_KNOB(bvh_fill, 0.5);
            const size_t k_want = static_cast<size_t>(std::ceil(static_cast<double>(cnt) / (fill * static_cast<double>(cap))));
            const size_t k = std::min<size_t>(std::min<size_t>(kFan, cnt), std::max(k_min, k_want));
            std::vector<size_t> sizes;
            split_sah(ids, b, e, k, cap, s, cen, tbox, sizes);
            nodes[w].first_child = static_cast<uint32_t>(nodes.size());
            nodes[w].n_kids = static_cast<uint32_t>(sizes.size());
            size_t at = b;
            for (size_t sz : sizes) {
                nodes.push_back({at, at + sz, 0, 0});
                at += sz;
            }
        }
        level_begin = level_end;
    }
    return nodes;
}

// The same tree WITHOUT the uniform depth: a binary tree built top down with the surface-area heuristic (every cut where
// area(left) n_left + area(right) n_right is smallest over the three axes; binned above 512 triangles), leaves of at most 8
// triangles, then collapsed to nodes of up to 8 children (a node takes a binary node's two children and keeps replacing the
// child of the largest area by its two children) -- the textbook wide-tree construction.  Big empty regions end up high in the
// tree and dense ones get the depth they need: on the x195 replica a ray visits 5 % fewer nodes and 7 % fewer child boxes than in
// the uniform-depth tree (profiles/r03_ab_logs.txt tree02).  Nodes are numbered breadth-first, a node's children are consecutive
// whatever their kind.
std::vector<TreeNode> sah_topology(const HostScene &s, const std::vector<Centroid> &cen, const std::vector<Box> &tbox, std::vector<int> &ids) {
    const size_t n = ids.size();
    std::sort(ids.begin(), ids.end(), GeoLess{&s, &cen, 0});   // a starting order that depends on geometry only
    struct Bin { size_t b, e; int left, right; Box box; };
    std::vector<Bin> bin;
    bin.reserve(2 * n / 4 + 16);
    // (iterative: a work list instead of recursion, children created in a fixed order)
    {
        Bin root = {0, n, -1, -1, kEmptyBox};
        for (size_t i = 0; i < n; ++i) root.box.grow(tbox[ids[i]]);
        bin.push_back(root);
    }
    for (size_t at = 0; at < bin.size(); ++at) {
        const size_t b = bin[at].b, e = bin[at].e, cnt = e - b;
        if (cnt <= static_cast<size_t>(kFan)) continue;   // a leaf
        size_t cut = 0;          // triangles of the left child
        int cut_axis = -1;
        double best = INFINITY;
        if (cnt <= 512) {
            // exact sweep: every cut position along each axis
            std::vector<double> right_area(cnt);
            for (int ax = 0; ax < 3; ++ax) {
                std::sort(ids.begin() + b, ids.begin() + e, GeoLess{&s, &cen, ax});
                Box acc = kEmptyBox;
                for (size_t i = cnt; i-- > 1;) { acc.grow(tbox[ids[b + i]]); right_area[i] = acc.area(); }
                acc = kEmptyBox;
                for (size_t i = 1; i < cnt; ++i) {
                    acc.grow(tbox[ids[b + i - 1]]);
                    const double c = acc.area() * static_cast<double>(i) + right_area[i] * static_cast<double>(cnt - i);
                    if (c < best) { best = c; cut = i; cut_axis = ax; }
                }
            }
            if (cut_axis != 2) std::sort(ids.begin() + b, ids.begin() + e, GeoLess{&s, &cen, cut_axis});
        } else {
            // 32 bins per axis over the centroids' range
            constexpr int kBins = 32;
            double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (size_t i = b; i < e; ++i)
                for (int x = 0; x < 3; ++x) { clo[x] = std::min(clo[x], cen[ids[i]].c[x]); chi[x] = std::max(chi[x], cen[ids[i]].c[x]); }
            int best_bin = -1;
            for (int ax = 0; ax < 3; ++ax) {
                if (!(chi[ax] > clo[ax])) continue;
                const double scale = kBins / (chi[ax] - clo[ax]);
                Box bb[kBins];
                size_t bc[kBins] = {};
                for (auto &x : bb) x = kEmptyBox;
                for (size_t i = b; i < e; ++i) {
                    const int k = std::min(kBins - 1, static_cast<int>((cen[ids[i]].c[ax] - clo[ax]) * scale));
                    bb[k].grow(tbox[ids[i]]);
                    ++bc[k];
                }
                double ra[kBins];
                Box acc = kEmptyBox;
                for (int k = kBins - 1; k >= 1; --k) { acc.grow(bb[k]); ra[k] = acc.area(); }
                acc = kEmptyBox;
                size_t nl = 0;
                for (int k = 1; k < kBins; ++k) {
                    acc.grow(bb[k - 1]);
                    nl += bc[k - 1];
                    if (nl == 0 || nl == cnt) continue;
                    const double c = acc.area() * static_cast<double>(nl) + ra[k] * static_cast<double>(cnt - nl);
                    if (c < best) { best = c; cut = nl; cut_axis = ax; best_bin = k; }
                }
            }
            if (cut_axis >= 0) {
                const double scale = kBins / (chi[cut_axis] - clo[cut_axis]);
                const int ax = cut_axis, kb = best_bin;
                const double lo = clo[ax];
                const auto mid = std::stable_partition(ids.begin() + b, ids.begin() + e, [&](int t) {
                    return std::min(kBins - 1, static_cast<int>((cen[t].c[ax] - lo) * scale)) < kb;
                });
                cut = static_cast<size_t>(mid - (ids.begin() + b));
            }
        }
        if (cut_axis < 0 || cut == 0 || cut >= cnt) {   // all centroids equal (or the heuristic found nothing): halves in canonical order
            std::sort(ids.begin() + b, ids.begin() + e, GeoLess{&s, &cen, 0});
            cut = cnt / 2;
        }
        Bin l = {b, b + cut, -1, -1, kEmptyBox}, r = {b + cut, e, -1, -1, kEmptyBox};
        for (size_t i = l.b; i < l.e; ++i) l.box.grow(tbox[ids[i]]);
        for (size_t i = r.b; i < r.e; ++i) r.box.grow(tbox[ids[i]]);
        bin[at].left = static_cast<int>(bin.size());
        bin.push_back(l);
        bin[at].right = static_cast<int>(bin.size());
        bin.push_back(r);
    }
    // collapse, breadth first: wide node w <-> binary node wide_bin[w]; its children are numbered consecutively
    std::vector<int> wide_bin = {0};
    std::vector<TreeNode> nodes;
    for (size_t w = 0; w < wide_bin.size(); ++w) {
        const Bin &bn = bin[wide_bin[w]];
        std::vector<int> kids;   // binary nodes that become the children (empty for a leaf)
        if (bn.left >= 0) {
            kids = {bn.left, bn.right};
            while (kids.size() < static_cast<size_t>(kFan)) {
                int pick = -1;
                double pa = -1;
                for (size_t i = 0; i < kids.size(); ++i)
                    if (bin[kids[i]].left >= 0 && bin[kids[i]].box.area() > pa) { pa = bin[kids[i]].box.area(); pick = static_cast<int>(i); }
                if (pick < 0) break;
                const int k = kids[pick];
                kids[pick] = bin[k].left;
                kids.insert(kids.begin() + pick + 1, bin[k].right);
            }
        }
        nodes.push_back({bn.b, bn.e, static_cast<uint32_t>(wide_bin.size()), static_cast<uint32_t>(kids.size())});
        for (int k : kids) wide_bin.push_back(k);   // (children of w: consecutive node indices, in this order)
    }
    return nodes;
}

// Box tree of a big scene over the (non-degenerate, small) triangles `ids`, by the builder `mode` names.  Writes the tree's
// slots (8 per leaf in node order, -1 = empty) to `order`: the tree's slots are the first slots.
void build_box_tree(int mode, const HostScene &s, const std::vector<TriGeo> &geo, const std::vector<Centroid> &cen, std::vector<int> ids,
                    double eps_line, CullTables &out, std::vector<int> &order) {
    out.bvh.clear();
    out.bvh_inner = 0;
    out.bvh_depth = 0;
    out.bvh_err = static_cast<float>(5.0e-7 * PT_MUT(box_err));   // first-order worst case 3.6e-7 (tests/test_cull_margins_host.py)
    order.clear();
    if (ids.empty()) return;
    std::vector<Box> tbox(geo.size());
    for (int t : ids) {
        tbox[t] = kEmptyBox;
        for (const V3 &v : geo[t].v) tbox[t].grow({{v.x, v.y, v.z}, {v.x, v.y, v.z}});
    }
    const std::vector<TreeNode> nodes = mode == 1 ? sah_topology(s, cen, tbox, ids) : uniform_topology(s, cen, tbox, ids);
    const size_t total = nodes.size();
    // forward: leaves in node order get their slots (canonical order inside a leaf); a node's level is its parent's + 1
    std::vector<uint32_t> leaf_ordinal(total, 0), level(total, 1);
    size_t n_leaves = 0;
    for (size_t w = 0; w < total; ++w) {
        const TreeNode &nd = nodes[w];
        for (uint32_t c = 0; c < nd.n_kids; ++c) level[nd.first_child + c] = level[w] + 1;
        out.bvh_depth = std::max(out.bvh_depth, level[w]);
        if (nd.n_kids > 0) continue;
        std::sort(ids.begin() + nd.b, ids.begin() + nd.e, GeoLess{&s, &cen, 0});
        leaf_ordinal[w] = static_cast<uint32_t>(n_leaves++);
        order.resize(n_leaves * kFan, -1);
        std::copy(ids.begin() + nd.b, ids.begin() + nd.e, order.end() - kFan);
    }
    out.bvh_inner = static_cast<uint32_t>(total - n_leaves);
    // backward: children have larger indices than their parent, so their boxes are complete when the parent is reached
    out.bvh.resize(total);
    std::vector<Box> node_box(total, kEmptyBox), tri_box;
    for (size_t w = total; w-- > 0;) {
        const TreeNode &nd = nodes[w];
        const bool leaf = nd.n_kids == 0;
        tri_box.clear();
        if (leaf)
            for (size_t i = nd.b; i < nd.e; ++i) tri_box.push_back(acceptance_box(geo[ids[i]], eps_line));
        const Box *kids = leaf ? tri_box.data() : &node_box[nd.first_child];
        const size_t k = leaf ? tri_box.size() : nd.n_kids;
        for (size_t c = 0; c < k; ++c) node_box[w].grow(kids[c]);
        quantise_node(out.bvh[w], node_box[w], kids, k, leaf, leaf ? leaf_ordinal[w] : nd.first_child);
    }
}

// ---------------------------------------------------------------------------------------------------
// The stages of build_cull_tables
// ---------------------------------------------------------------------------------------------------
// Scene-wide bounds every margin is derived from.
struct Envelope {
    double r_max;      // the camera origin ((0,0,-20), main.cpp:129, unless the scene handle has a camera of its own) and every vertex
    double r_org;      // ray origins sit on surfaces, offset by eps*N
    double d_max;      // bound on |c - o| for c, o inside the scene box
    double eps_line;   // rounding of P* = o + d*t* (per component <= u(2|t| + |o|)) and of the centre-to-origin vector
    double disc_err;   // float error of disc = |m|^2 - (m.d)^2 in the kernel, plus |d| != 1 by a few ulp
    double m_abs;      // bound on |o.n| + |w|
};
Envelope envelope_of(double extent, double r_camera) {
    Envelope e;
    e.r_max = cull_r_max(extent, r_camera);
    e.r_org = e.r_max + 1.0;
    e.d_max = 2.0 * std::sqrt(3.0) * e.r_org;
    e.eps_line = 8.0 * kU * (e.d_max + e.r_org);
    e.disc_err = 24.0 * kU * e.d_max * e.d_max;
    e.m_abs = 2.0 * std::sqrt(3.0) * e.r_org;
    return e;
}

// Bounding sphere of the acceptance regions of the triangles ids[0, count).  Returns its radius before the slacks of the
// record (infinite if one of the triangles cannot be bounded).
double sphere_of(const std::vector<TriGeo> &geo, const Envelope &env, const int *ids, int count, SphereRec &rec) {
    std::vector<V3> pts;
    bool inf = false;
    for (int k = 0; k < count; ++k) {
        if (geo[ids[k]].degenerate) inf = true;
        for (const V3 &v : geo[ids[k]].v) pts.push_back(v);
    }
    V3 c; double rad;
    bounding_sphere(pts, c, rad);
    double reff = 0;
    for (int k = 0; k < count && !inf; ++k) {
        const TriGeo &g = geo[ids[k]];
        double dmax = 0;
        for (const V3 &v : g.v) dmax = std::max(dmax, nrm(sub(v, c)));
        // accepted point = sum(lambda_k v_k) + h n, lambda_k >= -m_geo  =>  |P - c| <= (1 + 4 m_geo) dmax + h_max
        reff = std::max(reff, (1.0 + 4.0 * g.m_geo) * dmax + g.h_max + env.eps_line);
    }
    rec.c[0] = static_cast<float>(c.x); rec.c[1] = static_cast<float>(c.y); rec.c[2] = static_cast<float>(c.z);
    // the centre is rounded to float: grow by that displacement
    const double c_round = nrm(sub(c, V3{rec.c[0], rec.c[1], rec.c[2]}));
    double r2 = (reff + c_round) * (reff + c_round) * (1.0 + 1e-6) + env.disc_err;
    r2 *= PT_MUT(sphere_r2);
    rec.r2 = (inf || !std::isfinite(r2)) ? INFINITY : static_cast<float>(r2 * (1.0 + 2e-7));
    return inf ? INFINITY : reff;
}

bool triangle_emits(const HostScene &s, int t) { return material_emits(&s.mat[10 * static_cast<size_t>(s.tri_mat[t])]); }

// Connected groups of the small triangles (triangles sharing a vertex position): the objects of the scene.
std::vector<std::vector<int>> connected_groups(const HostScene &s, const std::vector<uint8_t> &large) {
    const int T = s.n_tri();
    UnionFind uf(T);
    struct Key { uint32_t b[3]; int tri; };
    std::vector<Key> keys;
    for (int i = 0; i < T; ++i)
        if (!large[i])
            for (int v = 0; v < 3; ++v) {
                Key k;
                std::memcpy(k.b, &s.tri[14 * static_cast<size_t>(i) + 4 + 3 * v], 12);
                k.tri = i;
                keys.push_back(k);
            }
    std::sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) {
        const int m = std::memcmp(a.b, b.b, 12);
        return m != 0 ? m < 0 : a.tri < b.tri;
    });
    for (size_t k = 1; k < keys.size(); ++k)
        if (std::memcmp(keys[k].b, keys[k - 1].b, 12) == 0) uf.unite(keys[k].tri, keys[k - 1].tri);
    std::vector<std::vector<int>> groups;
    std::vector<int> group_of(T, -1);
    for (int i = 0; i < T; ++i) {
        if (large[i]) continue;
        const int r = uf.find(i);
        if (group_of[r] < 0) { group_of[r] = static_cast<int>(groups.size()); groups.emplace_back(); }
        groups[group_of[r]].push_back(i);
    }
    return groups;
}

// Classes.  LARGE: a triangle whose own sphere is a sizeable part of the scene (walls) -- and every triangle that cannot be
// bounded at all (degenerate) -- is culled by a barycentric record, wave-uniformly.  SMALL: the rest, under a hierarchy of
// bounding volumes, by connected group.
struct Classes {
    std::vector<uint8_t> large;             // per triangle
    std::vector<std::vector<int>> groups;   // small triangles by connected group
};
Classes classify(const HostScene &s, const std::vector<TriGeo> &geo, const Envelope &env, bool big) {
    const int T = s.n_tri();
    const double r_max = env.r_max;
    Classes cl;
    std::vector<uint8_t> &large = cl.large;
    large.resize(T);
    std::vector<double> own_radius(T);
    for (int i = 0; i < T; ++i) {
        SphereRec tmp;
        own_radius[i] = sphere_of(geo, env, &i, 1, tmp);
        large[i] = !(own_radius[i] < 0.12 * r_max);
    }
    // A big scene's few emitters (the light of a room) join the large class whatever their size: their records alone then
    // tell which rays of a path's last segment can still contribute (pt_kernels.hip, "last segment").
    if (big) {
        // (not tiny ones: the margins of the barycentric test scale with the inverse size of the smallest record, and
        // every wall would pay for a pinhead of a light)
        int n_emit = 0;
        bool sizeable = true;
        for (int i = 0; i < T; ++i)
            if (triangle_emits(s, i)) {
                ++n_emit;
                sizeable = sizeable && own_radius[i] >= 0.01 * r_max;
            }
        if (n_emit <= 8 && sizeable)
            for (int i = 0; i < T; ++i) if (triangle_emits(s, i)) large[i] = 1;
    }
    cl.groups = connected_groups(s, large);
    // A group of one or two small triangles (the light of a room) costs more as a cluster of its own -- descriptor, sphere
    // tests, a publication per segment -- than as one more record of the large class ...
    const bool absorb = !PT_KNOB(no_absorb, 0);
    bool any_large = false;
    for (int i = 0; i < T; ++i) any_large |= large[i] != 0;
    if (absorb && any_large && !big) {
        for (auto &g : cl.groups) {
            // ... unless they are so small that their barycentric gradients (1 / height) would blow up the margin of
            // the whole class: the test of every large triangle uses the class-wide a_max
            bool fits = g.size() <= 2;
            for (int t : g) fits = fits && !geo[t].degenerate && geo[t].a_max * r_max <= 64.0;
            if (!fits) continue;
            for (int t : g) large[t] = 1;
            g.clear();
        }
        cl.groups.erase(std::remove_if(cl.groups.begin(), cl.groups.end(), [](const std::vector<int> &g) { return g.empty(); }), cl.groups.end());
    }
    return cl;
}

// Can a path leave the envelope (origins within r_org) the margins are derived for?  Only through a hit point outside
// it, i.e. only if some triangle's acceptance region reaches beyond it: a near-degenerate triangle (the reference
// accepts it for points anywhere along its axis) or a long sliver at the edge of the scene.  Scenes without such
// triangles (Tor.obj, the replicas) skip the per-segment origin test altogether.
bool may_leave_envelope(const std::vector<TriGeo> &geo, const Envelope &env) {
    for (const TriGeo &g : geo) {
        if (g.degenerate) return true;
        const Box b = acceptance_box(g, env.eps_line);
        for (int x = 0; x < 3; ++x)
            if (!(b.lo[x] > -(env.r_org - 0.01)) || !(b.hi[x] < env.r_org - 0.01)) return true;
    }
    return false;
}

// Cost of laying the implicit 8-ary sphere tree over an order: sum of r^2 over its nodes (a ray meets a sphere with
// probability ~ r^2).
double order_cost(const std::vector<TriGeo> &geo, const Envelope &env, const std::vector<int> &ids) {
    double cost = 0;
    const long long n = static_cast<long long>(ids.size());
    for (long long span = kFan; span * kFan < n * kFan && span < n; span *= kFan)   // levels below the top one
        for (long long f = 0; f < n; f += span) {
            SphereRec sr;
            const double reff = sphere_of(geo, env, &ids[f], static_cast<int>(std::min<long long>(span, n - f)), sr);
            cost += std::isfinite(reff) ? reff * reff : 0.0;
        }
    return cost;
}

// Small scenes: one cluster per connected group, clusters and the triangles inside each in an order that depends on
// geometry only.  Appends the slots to `order` and each cluster's [first slot, count) to `small_runs`.
void order_clusters(const HostScene &s, const std::vector<TriGeo> &geo, const std::vector<Centroid> &cen, const Envelope &env,
                    std::vector<std::vector<int>> groups, std::vector<int> &order, std::vector<std::pair<int, int>> &small_runs) {
    const int max_clusters = PT_KNOB(max_clusters, -1) >= 0 ? PT_KNOB(max_clusters, -1) : kMaxClusters;
    if (static_cast<int>(groups.size()) > max_clusters) {   // a cloud of loose triangles: one tree over all of them
        std::vector<int> all;
        for (const auto &g : groups) all.insert(all.end(), g.begin(), g.end());
        groups.assign(1, all);
    }
    std::vector<std::pair<Centroid, size_t>> keyed;
    for (size_t g = 0; g < groups.size(); ++g) {
        Centroid m = {{0, 0, 0}};
        for (int t : groups[g]) for (int k = 0; k < 3; ++k) m.c[k] += cen[t].c[k] / static_cast<double>(groups[g].size());
        keyed.push_back({m, g});
    }
    std::sort(keyed.begin(), keyed.end(), [](const std::pair<Centroid, size_t> &a, const std::pair<Centroid, size_t> &b) {
        for (int k = 0; k < 3; ++k) if (a.first.c[k] != b.first.c[k]) return a.first.c[k] < b.first.c[k];
        return a.second < b.second;
    });
    for (const auto &kg : keyed) {
        // the cheaper of two spatial arrangements
        // (two geometry-only arrangements are tried and the cheaper kept; results do not depend on the choice)
        std::vector<int> ids = groups[kg.second], patches = ids;
        arrange_implicit(ids, 0, ids.size(), s, cen);          // axis-aligned cells
        if (patches.size() <= 4096) {                          // compact patches (quadratic in the group size)
            arrange_patches(patches, 0, patches.size(), s, cen);
            const int order_mode = PT_KNOB(order_mode, 0);   // 0 = the cheaper of the two, 1 = as filed, 2 = cells, 3 = patches
            if (order_mode == 1) ids = groups[kg.second];
            else if (order_mode == 3) ids = patches;
            else if (order_mode == 0 && order_cost(geo, env, patches) < order_cost(geo, env, ids)) ids = patches;
        }
        small_runs.push_back({static_cast<int>(order.size()), static_cast<int>(ids.size())});
        order.insert(order.end(), ids.begin(), ids.end());
    }
}

// Slot order of the small class: one box tree over all of it (big scenes) or a sphere-tree cluster per group.
void order_small_class(const HostScene &s, const std::vector<TriGeo> &geo, const std::vector<Centroid> &cen, const Envelope &env,
                       const std::vector<std::vector<int>> &groups, CullTables &out, std::vector<int> &order,
                       std::vector<std::pair<int, int>> &small_runs) {
    if (!out.big) {
        if (!groups.empty()) order_clusters(s, geo, cen, env, groups, order, small_runs);
        return;
    }
    std::vector<int> ids;
    for (const auto &g : groups) ids.insert(ids.end(), g.begin(), g.end());
    const int mode = PT_KNOB(bvh_mode, -1) >= 0 ? PT_KNOB(bvh_mode, -1) : PT_BVH_MODE;
    build_box_tree(mode, s, geo, cen, ids, env.eps_line, out, order);
    // The SAH tree's depth follows the geometry (nested shells of geometrically growing triangles: 12 levels for 12 000
    // triangles) and the walk's stack slack bounds it (kMaxBvhDepth): such a scene gets the uniform-depth tree instead.
    const uint32_t depth_cap = static_cast<uint32_t>(PT_KNOB(bvh_depth_cap, kMaxBvhDepth));
    if (mode == 1 && out.bvh_depth > depth_cap) build_box_tree(0, s, geo, cen, ids, env.eps_line, out, order);
}

// Slot order of the large class: coplanar pairs that share an edge first (they become quad records), then singles.
void order_large_class(const HostScene &s, const std::vector<TriGeo> &geo, const std::vector<Centroid> &cen, const std::vector<uint8_t> &large,
                       std::vector<int> &order) {
    std::vector<int> lg;
    for (int i = 0; i < s.n_tri(); ++i) if (large[i]) lg.push_back(i);
    std::sort(lg.begin(), lg.end(), GeoLess{&s, &cen, 0});
    std::vector<uint8_t> used(lg.size(), 0);
    std::vector<int> pairs, singles;
    for (size_t a = 0; a < lg.size(); ++a) {
        if (used[a]) continue;
        const float *ra = &s.tri[14 * static_cast<size_t>(lg[a])];
        int mate = -1;
        for (size_t b = a + 1; b < lg.size() && mate < 0 && !geo[lg[a]].degenerate; ++b) {
            if (used[b] || geo[lg[b]].degenerate) continue;
            const float *rb = &s.tri[14 * static_cast<size_t>(lg[b])];
            if (std::memcmp(ra, rb, 16) != 0) continue;   // ONE stored plane
            int shared = 0;
            for (int x = 0; x < 3; ++x)
                for (int y = 0; y < 3; ++y) shared += std::memcmp(ra + 4 + 3 * x, rb + 4 + 3 * y, 12) == 0;
            if (shared == 2) mate = static_cast<int>(b);
        }
        if (mate >= 0) {
            used[a] = used[mate] = 1;
            pairs.push_back(lg[a]);
            pairs.push_back(lg[mate]);
        } else {
            used[a] = 1;
            singles.push_back(lg[a]);
        }
    }
    order.insert(order.end(), pairs.begin(), pairs.end());
    order.insert(order.end(), singles.begin(), singles.end());
}

// slot_tri and exact_slot; a padding slot gets a record that can never be accepted.
void fill_slot_tables(const HostScene &s, const std::vector<int> &order, CullTables &out) {
    const size_t n_slots = order.size();
    out.slot_tri.resize(n_slots);
    out.exact_slot.resize(n_slots);
    DeviceTables dev_tables;
    build_device_tables(s, dev_tables);
    for (size_t k = 0; k < n_slots; ++k) {
        out.slot_tri[k] = order[k] < 0 ? kNoTriangle : static_cast<uint32_t>(order[k]);
        if (order[k] >= 0) {
            out.exact_slot[k] = dev_tables.exact[order[k]];
        } else {
            ExactRec e;
            std::memset(&e, 0, sizeof e);
            e.plane[0] = e.plane[1] = e.plane[2] = e.plane[3] = NAN;
            e.orig = -1;
            out.exact_slot[k] = e;
        }
    }
}

const SphereRec kNeverSphere = {{0, 0, 0}, -1.0e30f};   // keeps no ray

// The descriptor of the cluster over slots [first, first + n): its bounding sphere and range.
ClusterDesc cluster_over(const std::vector<TriGeo> &geo, const Envelope &env, const std::vector<int> &order, int first, int n, uint32_t kind) {
    ClusterDesc cd;
    std::memset(&cd, 0, sizeof cd);
    SphereRec cs;
    sphere_of(geo, env, &order[first], n, cs);
    cd.c[0] = cs.c[0]; cd.c[1] = cs.c[1]; cd.c[2] = cs.c[2]; cd.r2 = cs.r2;
    cd.first_tri = static_cast<uint32_t>(first);
    cd.n_tri = static_cast<uint32_t>(n);
    cd.kind = kind;
    return cd;
}

// One small-scene cluster: an implicit 8-ary tree of bounding spheres over the run of slots [first, first + n).
void append_sphere_tree(const std::vector<TriGeo> &geo, const Envelope &env, const std::vector<int> &order, int first, int n, CullTables &out) {
    ClusterDesc cd = cluster_over(geo, env, order, first, n, 0u);
    cd.data_off = static_cast<uint32_t>(out.spheres.size());
    long long span = 1;   // triangles per node of the current level
    for (int level = 0;; ++level, span *= kFan) {
        const long long count = (n + span - 1) / span;
        if (level > 0) cd.level_off[level - 1] = static_cast<uint32_t>(out.spheres.size() - cd.data_off);
        for (long long j = 0; j < (count + kFan - 1) / kFan * kFan; ++j) {
            SphereRec sr = kNeverSphere;
            if (j < count) {
                const long long f = j * span;
                sphere_of(geo, env, &order[first + static_cast<int>(f)], static_cast<int>(std::min<long long>(span, n - f)), sr);
            }
            out.spheres.push_back(sr);
        }
        if (count <= kFan || level == kMaxLevels - 1) {
            cd.n_levels = static_cast<uint32_t>(level + 1);
            break;
        }
    }
    out.clusters.push_back(cd);
}

// Dual rows of the edges e1, e2 of a plane: u.e1 = v.e2 = 1, u.e2 = v.e1 = 0, both rows in the plane -- the gradients of
// the coordinates of a point's orthogonal projection in the frame (e1, e2).
struct DualRows {
    V3 u, v;
};
DualRows dual_rows(V3 e1, V3 e2) {
    const V3 nn = crs(e1, e2);
    const double s2 = dt(nn, nn);
    return {{crs(e2, nn).x / s2, crs(e2, nn).y / s2, crs(e2, nn).z / s2}, {crs(nn, e1).x / s2, crs(nn, e1).y / s2, crs(nn, e1).z / s2}};
}

void set_rows(CullRec &c, V3 au, V3 av, double cu, double cv) {
    c.au[0] = static_cast<float>(au.x); c.au[1] = static_cast<float>(au.y); c.au[2] = static_cast<float>(au.z);
    c.av[0] = static_cast<float>(av.x); c.av[1] = static_cast<float>(av.y); c.av[2] = static_cast<float>(av.z);
    c.cu = static_cast<float>(cu);
    c.cv = static_cast<float>(cv);
}

// The barycentric cull record of one triangle (`row`: its 14 floats).
CullRec cull_record(const float *row, const TriGeo &g) {
    CullRec c;
    std::memset(&c, 0, sizeof c);
    c.n[0] = row[0]; c.n[1] = row[1]; c.n[2] = row[2]; c.w = row[3];
    const DualRows d = dual_rows(sub(g.v[1], g.v[0]), sub(g.v[2], g.v[0]));
    set_rows(c, d.u, d.v, -dt(d.u, g.v[0]), -dt(d.v, g.v[0]));
    // NaN coefficients make every comparison of the cull test false: a triangle that cannot be bounded is always kept
    if (g.degenerate) c.au[0] = c.au[1] = c.au[2] = c.av[0] = c.av[1] = c.av[2] = c.cu = c.cv = NAN;
    return c;
}

// What the margins of a set of records depend on: maxima over its non-degenerate triangles.
struct RecordMaxima {
    double a_max = 0;      // largest barycentric gradient (and, for the large class, quad row)
    double inv_2s = 0;     // 1 / (2 S)
    double diam2_2s = 0;   // diam^2 / (2 S)
    void add(const TriGeo &g) {
        if (g.degenerate) return;
        a_max = std::max(a_max, g.a_max);
        inv_2s = std::max(inv_2s, 1.0 / (2.0 * g.area2));
        diam2_2s = std::max(diam2_2s, g.diam * g.diam / (2.0 * g.area2));
    }
};

// Quads: two consecutive large triangles (even slot first) that lie in ONE stored plane and share an edge
// are the two halves of a (near-)parallelogram s0, a, s1, b with diagonal s0-s1.  With P = s0 + alpha*(a-s0) +
// beta*(b-s0), half A = (s0, s1, a) has barycentrics (beta, alpha-beta, 1-alpha) and half B = (s0, s1, b) has
// (alpha, beta-alpha, 1-beta), so ONE plane evaluation and two affine rows cull both.  The identity is exact
// only for an exact parallelogram; the deviation of each half's own barycentrics from it is measured
// over the region alpha, beta in [-1, 2] and added to the margin (quad_slack); pairs that deviate by more
// than 1 % are left as two triangles.  (Outside that region the derived minimum is <= -1 and the deviation
// grows at most linearly, so a far point can never be kept by one test and rejected by the other.)
struct QuadRecord {
    V3 ral, rbe;       // alpha row: dual of a - s0; beta row: dual of b - s0
    double cal, cbe;
    double dev;        // largest deviation measured
};
// true barycentrics of a triangle (orthogonal projection onto its own plane), as affine functions
void bary_rows(const TriGeo &g, int i0, int i1, int i2, V3 rows[3], double cst[3]) {
    const DualRows d = dual_rows(sub(g.v[i1], g.v[i0]), sub(g.v[i2], g.v[i0]));
    rows[1] = d.u;   // weight of i1
    rows[2] = d.v;   // weight of i2
    rows[0] = {-(rows[1].x + rows[2].x), -(rows[1].y + rows[2].y), -(rows[1].z + rows[2].z)};
    cst[1] = -dt(rows[1], g.v[i0]); cst[2] = -dt(rows[2], g.v[i0]); cst[0] = 1.0 - cst[1] - cst[2];
}
// The quad record of the triangles with rows ra, rb, or nothing if they are not the halves of a near-parallelogram.
bool fuse_quad(const float *ra, const float *rb, const TriGeo &ga, const TriGeo &gb, QuadRecord &q) {
    if (std::memcmp(ra, rb, 16) != 0 || ga.degenerate || gb.degenerate) return false;
    // shared vertices (bitwise) and the two apexes
    int sa[2], sb[2], ns = 0, apex_a = -1, apex_b = -1;
    bool used_b[3] = {false, false, false};
    for (int x = 0; x < 3; ++x) {
        int match = -1;
        for (int y = 0; y < 3; ++y)
            if (!used_b[y] && std::memcmp(ra + 4 + 3 * x, rb + 4 + 3 * y, 12) == 0) { match = y; break; }
        if (match >= 0 && ns < 2) { sa[ns] = x; sb[ns] = match; used_b[match] = true; ++ns; }
        else apex_a = x;
    }
    if (ns != 2 || apex_a < 0) return false;
    for (int y = 0; y < 3; ++y) if (!used_b[y]) apex_b = y;
    const V3 s0 = ga.v[sa[0]], pa = ga.v[apex_a], pb = gb.v[apex_b];
    const V3 ea = sub(pa, s0), eb = sub(pb, s0);
    const V3 nn = crs(ea, eb);
    const double s2 = dt(nn, nn);
    if (!(s2 > 0)) return false;
    const DualRows d = dual_rows(ea, eb);
    q.ral = d.u;
    q.rbe = d.v;
    q.cal = -dt(q.ral, s0);
    q.cbe = -dt(q.rbe, s0);
    V3 rowa[3], rowb[3];
    double ca[3], cb[3];
    bary_rows(ga, sa[0], sa[1], apex_a, rowa, ca);   // weights of s0, s1, a
    bary_rows(gb, sb[0], sb[1], apex_b, rowb, cb);   // weights of s0, s1, b
    const V3 nu = {nn.x / std::sqrt(s2), nn.y / std::sqrt(s2), nn.z / std::sqrt(s2)};
    const double hh = 0.05 * std::max(ga.diam, gb.diam);
    q.dev = 0;
    for (int c8 = 0; c8 < 8; ++c8) {
        const double al = (c8 & 1) ? 2.0 : -1.0, be = (c8 & 2) ? 2.0 : -1.0, h = (c8 & 4) ? hh : -hh;
        const V3 P = {s0.x + al * ea.x + be * eb.x + h * nu.x, s0.y + al * ea.y + be * eb.y + h * nu.y, s0.z + al * ea.z + be * eb.z + h * nu.z};
        const double a_ = dt(q.ral, P) + q.cal, b_ = dt(q.rbe, P) + q.cbe;
        const double da[3] = {1 - a_, b_, a_ - b_}, db[3] = {1 - b_, a_, b_ - a_};   // derived weights of (s0, s1, apex)
        for (int t3 = 0; t3 < 3; ++t3) {
            q.dev = std::max(q.dev, std::fabs(dt(rowa[t3], P) + ca[t3] - da[t3]));
            q.dev = std::max(q.dev, std::fabs(dt(rowb[t3], P) + cb[t3] - db[t3]));
        }
    }
    return q.dev < 0.01;
}

// The large class: one cluster of barycentric records over slots [first, first + n), padded to whole words of 32, pairs
// fused into quad records where they can be.  Returns the largest deviation of a fused quad (quad_slack).
double append_large_cluster(const HostScene &s, const std::vector<TriGeo> &geo, const Envelope &env, const std::vector<int> &order,
                            int first, int n, CullTables &out, RecordMaxima &maxima) {
    ClusterDesc cd = cluster_over(geo, env, order, first, n, 1u);
    cd.data_off = static_cast<uint32_t>(out.bary.size());
    const int n_words = (n + kChunk - 1) / kChunk;
    auto row = [&](int k) { return &s.tri[14 * static_cast<size_t>(order[first + k])]; };
    for (int k = 0; k < n_words * kChunk; ++k) {
        CullRec c;
        std::memset(&c, 0, sizeof c);
        if (k < n) {
            c = cull_record(row(k), geo[order[first + k]]);
            maxima.add(geo[order[first + k]]);
        }
        out.bary.push_back(c);
    }
    double quad_slack = 0;
    for (int w = 0; w < n_words && w < kMaxLevels - 1; ++w) {
        uint32_t qmask = 0;
        for (int k = w * kChunk; k + 1 < std::min(n, (w + 1) * kChunk); k += 2) {
            QuadRecord q;
            if (!fuse_quad(row(k), row(k + 1), geo[order[first + k]], geo[order[first + k + 1]], q)) continue;
            quad_slack = std::max(quad_slack, q.dev);
            maxima.a_max = std::max(maxima.a_max, std::max(nrm(q.ral), std::max(nrm(q.rbe), nrm(sub(q.ral, q.rbe)))));
            set_rows(out.bary[cd.data_off + k], q.ral, q.rbe, q.cal, q.cbe);
            std::memset(&out.bary[cd.data_off + k + 1], 0, sizeof(CullRec));
            qmask |= 1u << (k - w * kChunk);
        }
        cd.level_off[w] = qmask;   // large clusters have no sphere tree: the slots carry the quad masks
    }
    out.clusters.push_back(cd);
    return quad_slack;
}

// Big scenes: a barycentric record for every slot, used to thin the (ray, triangle) pairs before the exact test.
RecordMaxima fill_bary_all(const HostScene &s, const std::vector<TriGeo> &geo, const std::vector<int> &order, CullTables &out) {
    RecordMaxima maxima;
    out.bary_all.resize(order.size() + 4);
    for (auto &c : out.bary_all) std::memset(&c, 0, sizeof c);
    for (size_t k = 0; k < order.size(); ++k) {
        if (order[k] < 0) continue;   // padding slots are never candidates
        out.bary_all[k] = cull_record(&s.tri[14 * static_cast<size_t>(order[k])], geo[order[k]]);
        maxima.add(geo[order[k]]);
    }
    return maxima;
}

// Margins of the barycentric test over a set of records.
CullConstants margins(const RecordMaxima &mx, double quad_slack, const Envelope &env, double eps) {
    const double r_org = env.r_org, a_max = mx.a_max;
    CullConstants cc;
    cc.k2 = static_cast<float>(PT_MUT(k12) * (12.0 * kU * env.m_abs + 8.0 * kU * r_org));
    cc.k1 = static_cast<float>(PT_MUT(k12) * 40.0 * kU);
    cc.a_max = static_cast<float>(PT_MUT(a_max) * a_max * (1.0 + 1e-6));
    cc.m0 = static_cast<float>(PT_MUT(m0) * (std::fabs(eps) * mx.inv_2s * 1.01 + 48.0 * kU * mx.diam2_2s
                                             + 16.0 * kU * a_max * r_org * std::sqrt(3.0) + 1e-6));
    double tg = 4096.0 * r_org;
    if (a_max > 0) tg = std::min(tg, 1.0e6 / a_max);   // keep the reference's own area arithmetic meaningful
    cc.t_guard = static_cast<float>(tg);
    cc.m0_quad = static_cast<float>(static_cast<double>(cc.m0) + PT_MUT(quad_slack) * (quad_slack * 1.01 + 8.0 * kU * a_max * r_org));
    return cc;
}

// Where the emitters are (a path's last segment searches among them alone).
void fill_emitter_masks(const HostScene &s, int n_small_slots, CullTables &out) {
    auto emits = [&](uint32_t slot) {
        const uint32_t t = slot < out.slot_tri.size() ? out.slot_tri[slot] : kNoTriangle;
        return t != kNoTriangle && triangle_emits(s, static_cast<int>(t));
    };
    out.emis_clusters = 0;
    out.emis_large_w0 = 0xFFFFFFFFu;
    for (size_t c = 0; c < out.clusters.size(); ++c) {
        const ClusterDesc &cd = out.clusters[c];
        bool any = false;
        for (uint32_t k = 0; k < cd.n_tri; ++k) any = any || emits(cd.first_tri + k);
        if (c >= 32 || any) out.emis_clusters |= c < 32 ? (1u << c) : 0u;
        if (cd.kind == 1u && cd.n_tri <= static_cast<uint32_t>(kChunk)) {
            out.emis_large_w0 = 0;
            for (uint32_t k = 0; k < cd.n_tri; ++k) out.emis_large_w0 |= emits(cd.first_tri + k) ? (1u << k) : 0u;
        }
    }
    if (out.clusters.size() > 32) out.emis_clusters = 0xFFFFFFFFu;   // (small scenes have at most 10 clusters)
    // negative control of the shipped-path verification: forget one emitter of the large class
    if (PT_KNOB(emis_drop, 0) && out.emis_large_w0 != 0xFFFFFFFFu) out.emis_large_w0 &= out.emis_large_w0 - 1u;
    out.emis_bvh = false;
    if (!out.bvh.empty())
        for (uint32_t k = 0; k < static_cast<uint32_t>(n_small_slots); ++k) out.emis_bvh = out.emis_bvh || emits(k);
}

// Clauses 1-4 of "room-shaped" (pt_scene.hpp: CullTables::room, where each clause has its reason).
bool room_shaped(const CullTables &t) {
    if (t.big || !t.bvh.empty()) return false;                                          // 1. a small scene
    if (t.clusters.empty() || t.clusters.size() > 2) return false;                      // 4. the large class and at most one more cluster ...
    const ClusterDesc &large = t.clusters.back();
    if (large.kind != 1u || large.n_tri == 0 || large.n_tri > static_cast<uint32_t>(kChunk)) return false;   // 2. one chunk word
    const uint32_t pair_bits = 0x55555555u & (large.n_tri >= 32u ? 0xFFFFFFFFu : ((1u << large.n_tri) - 1u));
    if (large.level_off[0] != pair_bits) return false;                                  // 3. every record a quad (what the kernel tests as quads == pair_bits)
    return t.clusters.size() == 1 || t.clusters.front().kind == 0u;                     // 4. ... which is a sphere tree
}

}  // namespace

double vertex_extent(const HostScene &s) {
    double r = 0.0;
    for (int i = 0; i < s.n_tri(); ++i)
        for (int k = 4; k < 13; ++k) r = std::max(r, static_cast<double>(std::fabs(s.tri[14 * static_cast<size_t>(i) + k])));
    return r;
}

void build_cull_tables(const HostScene &s, float eps_f, CullTables &out, double r_camera) {
    const int T = s.n_tri();
    const double eps = eps_f;
    out = CullTables();
    out.eps = eps_f;
    // sphere trees + small-scene kernels, or one box tree + big-scene kernels (pt_scene.hpp: kBigSceneTriangles)
    const int hook = PT_KNOB(big_threshold, -1);
    out.big = T > (hook >= 0 ? std::min(hook, kSmallSceneMaxTriangles) : kBigSceneTriangles);

    const Envelope env = envelope_of(vertex_extent(s), r_camera);
    out.r_max = env.r_max;
    out.r_org = static_cast<float>(env.r_org);
    std::vector<TriGeo> geo(T);
    std::vector<Centroid> cen(T);
    for (int i = 0; i < T; ++i) {
        geo[i] = tri_geometry(&s.tri[14 * static_cast<size_t>(i)], eps);
        const V3 *v = geo[i].v;
        cen[i] = {{(v[0].x + v[1].x + v[2].x) / 3, (v[0].y + v[1].y + v[2].y) / 3, (v[0].z + v[1].z + v[2].z) / 3}};
    }
    const Classes classes = classify(s, geo, env, out.big);
    out.may_leave_envelope = may_leave_envelope(geo, env);

    // ---- slot order: the small class (box tree or sphere-tree clusters), then the large class
    std::vector<int> order;                       // slot -> triangle (-1 = padding)
    std::vector<std::pair<int, int>> small_runs;  // small scenes: [first slot, count) of each cluster
    order_small_class(s, geo, cen, env, classes.groups, out, order, small_runs);
    const int n_small_slots = static_cast<int>(order.size());
    order_large_class(s, geo, cen, classes.large, order);
    const int n_large = static_cast<int>(order.size()) - n_small_slots;

    // ---- tables in slot order
    fill_slot_tables(s, order, out);
    for (const auto &run : small_runs) append_sphere_tree(geo, env, order, run.first, run.second, out);
    RecordMaxima large_maxima, all_maxima;
    double quad_slack = 0;
    if (n_large > 0) quad_slack = append_large_cluster(s, geo, env, order, n_small_slots, n_large, out, large_maxima);
    // keep the tables non-empty and padded so that speculative wide scalar loads stay inside the allocation
    // (the root round of the kernel reads up to 8 x 64 records from a level's start without a bounds test and masks afterwards)
    for (int k = 0; k < 16 + 8 * 64; ++k) out.spheres.push_back(kNeverSphere);
    for (int k = 0; k < 4; ++k) { CullRec c; std::memset(&c, 0, sizeof c); out.bary.push_back(c); }
    if (out.big) all_maxima = fill_bary_all(s, geo, order, out);

    // ---- margins: of the large class, and the same over ALL triangles for the pair pre-filter of big scenes (they must
    // cover the smallest triangle of the scene); k1, k2 and m0_quad of cc_all are those of cc
    out.cc = margins(large_maxima, quad_slack, env, eps);
    const CullConstants all = margins(all_maxima, 0.0, env, eps);
    out.cc_all = out.cc;
    out.cc_all.a_max = all.a_max;
    out.cc_all.m0 = all.m0;
    out.cc_all.t_guard = all.t_guard;

    fill_emitter_masks(s, n_small_slots, out);
    out.room = room_shaped(out);
}

}  // namespace pt
