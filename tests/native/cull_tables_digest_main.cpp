// One 64-bit FNV-1a digest of EVERY field of pt::CullTables per case: what tests/test_cull_tables_digest_host.py compares with
// tests/golden/cull_table_digests.json, so that a change of the table builder that moves one byte of one table is seen on the CPU.
//   argv[1] = models directory, argv[2] = directory of the x9 replica (x9.obj), argv[3] = the same with an emissive torus
//   material (all with a trailing slash); an optional argv[4] "-v" adds a summary of each case's tables to its line.
// Built plain and with -DPT_TEST_HOOKS; the hooks build prints the plain cases too (default knobs: the same digests) and then
// one case per knob of pt::g_cull_mutation, which it writes directly.
#include "pt_scene.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <type_traits>

namespace {

// A field added to CullTables must be added to digest() below (and the golden file recorded anew).
static_assert(sizeof(void *) != 8 || sizeof(std::vector<int>) != 24 || sizeof(pt::CullTables) == 264, "CullTables changed: update digest()");

struct Fnv {
    uint64_t h = 14695981039346656037ull;
    void bytes(const void *p, size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    }
    template <class T> void scalar(const T &v) {
        static_assert(std::is_arithmetic<T>::value && !std::is_same<T, bool>::value, "scalars only");
        bytes(&v, sizeof v);
    }
    void flag(bool v) { const unsigned char b = v ? 1 : 0; bytes(&b, 1); }
    template <class T> void vec(const std::vector<T> &v) {   // (every record type is padding-free)
        static_assert(std::is_trivially_copyable<T>::value, "raw bytes");
        const uint64_t n = v.size();
        bytes(&n, sizeof n);
        if (n) bytes(v.data(), n * sizeof(T));
    }
    void constants(const pt::CullConstants &c) { static_assert(sizeof c == 24, "six floats"); bytes(&c, sizeof c); }
};

uint64_t digest(const pt::CullTables &t) {
    Fnv f;
    f.vec(t.slot_tri); f.vec(t.exact_slot); f.vec(t.spheres); f.vec(t.bary); f.vec(t.bary_all);
    f.constants(t.cc_all);
    f.vec(t.clusters); f.vec(t.bvh);
    f.scalar(t.bvh_inner); f.scalar(t.bvh_depth); f.flag(t.big); f.scalar(t.bvh_err);
    f.constants(t.cc);
    f.scalar(t.eps); f.scalar(t.r_org); f.scalar(t.r_max); f.flag(t.may_leave_envelope);
    f.scalar(t.emis_clusters); f.scalar(t.emis_large_w0); f.flag(t.emis_bvh);
    return f.h;
}

bool verbose = false;

void report(const std::string &name, const pt::HostScene &s, float eps, double r_camera = 20.0) {
    pt::CullTables t;
    pt::build_cull_tables(s, eps, t, r_camera);
    std::printf("%s %016llx", name.c_str(), static_cast<unsigned long long>(digest(t)));
    if (verbose) {
        uint32_t quads = 0;
        for (const pt::ClusterDesc &c : t.clusters)
            if (c.kind == 1u) for (uint32_t w : c.level_off) for (; w; w &= w - 1) ++quads;
        std::printf("  # %d tri big %d clusters %zu spheres %zu bary %zu bary_all %zu bvh %zu inner %u depth %u quads %u m0 %g m0_quad %g leave %d emis %08x %08x %d",
                    s.n_tri(), t.big, t.clusters.size(), t.spheres.size(), t.bary.size(), t.bary_all.size(), t.bvh.size(), t.bvh_inner, t.bvh_depth,
                    quads, t.cc.m0, t.cc.m0_quad, t.may_leave_envelope, t.emis_clusters, t.emis_large_w0, t.emis_bvh);
    }
    std::printf("\n");
}

// Floats from the raw 32-bit output of mt19937 (the standard fixes that output, not the distributions built on it).
struct Rand {
    std::mt19937 g;
    explicit Rand(uint32_t seed) : g(seed) {}
    float unit() { return static_cast<float>(g() >> 8) * (1.0f / 16777216.0f); }   // [0, 1), 24 bits: exact
    float in(float lo, float hi) { return lo + (hi - lo) * unit(); }
};

pt::HostScene two_materials() {
    pt::HostScene h;
    h.mat.assign(20, 0.5f);
    h.mat[3] = h.mat[4] = h.mat[5] = 0.0f;                 // material 0: no Ke
    h.mat[10 + 3] = 4.0f; h.mat[10 + 4] = 3.0f; h.mat[10 + 5] = 0.0f;   // material 1: emissive
    return h;
}

// n triangles at random places: most small, every 13th wall-sized, every 7th of zero area; every `emit_every`th emissive
// (`emit_scale`: size of the emissive ones, 0 = as the others).
pt::HostScene random_scene(int n, uint32_t seed, int emit_every = 11, float emit_scale = 0.0f) {
    pt::HostScene h = two_materials();
    Rand r(seed);
    for (int i = 0; i < n; ++i) {
        const bool emits = i % emit_every == 5;
        float p[3], q[3], w[3];
        for (float &c : p) c = r.in(-9.0f, 9.0f);
        float k = (i % 13 == 0) ? 8.0f : (i % 7 == 0 ? 0.0f : 0.4f);
        if (emits && emit_scale > 0.0f) k = emit_scale;
        for (int c = 0; c < 3; ++c) { q[c] = p[c] + k * r.in(-1.0f, 1.0f); w[c] = p[c] + k * r.in(-1.0f, 1.0f); }
        pt::append_triangle(h, p, q, w, nullptr, emits ? 1 : 0);
    }
    return h;
}

// s0, a, s1, b in the plane z = 0 as the halves (s0, s1, a) and (s0, s1, b); `skew` moves b along x off the parallelogram.
pt::HostScene quad_scene(float skew) {
    pt::HostScene h = two_materials();
    const float s0[3] = {-5, -5, 0}, a[3] = {5, -5, 0}, s1[3] = {5, 5, 0}, b[3] = {-5 + skew, 5, 0};
    pt::append_triangle(h, s0, a, s1, nullptr, 0);
    pt::append_triangle(h, s0, s1, b, nullptr, 0);
    return h;
}

// Three closed fans of small triangles (three connected groups: three sphere-tree clusters) in front of one wall quad.
pt::HostScene fans_scene() {
    pt::HostScene h = quad_scene(0.0f);
    Rand r(99);
    const float centre[3][3] = {{-4, 2, -6}, {3, -1, -3}, {0.5f, 4, -9}};
    const int spokes[3] = {12, 20, 5};
    for (int f = 0; f < 3; ++f) {
        std::vector<float> rim;
        for (int k = 0; k < spokes[f]; ++k) {   // the rim goes round a diamond (no libm in a fixture: plain arithmetic only)
            const float t = 4.0f * static_cast<float>(k) / static_cast<float>(spokes[f]), u = t - std::floor(t);
            const float dx = t < 1 ? 1 - u : t < 2 ? -u : t < 3 ? u - 1 : u, dy = t < 1 ? u : t < 2 ? 1 - u : t < 3 ? -u : u - 1;
            rim.push_back(centre[f][0] + dx * r.in(0.8f, 1.2f));
            rim.push_back(centre[f][1] + dy * r.in(0.8f, 1.2f));
            rim.push_back(centre[f][2] + r.in(-0.3f, 0.3f));
        }
        for (int k = 0; k < spokes[f]; ++k)
            pt::append_triangle(h, centre[f], &rim[3 * k], &rim[3 * ((k + 1) % spokes[f])], nullptr, f == 1 ? 1 : 0);
    }
    return h;
}

bool load(const std::string &dir, const char *name, pt::HostScene &s) {
    std::string err;
    bool io = false;
    if (pt::load_obj(dir, name, s, err, io)) return true;
    std::printf("load failed: %s\n", err.c_str());
    return false;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    verbose = argc > 4 && std::strcmp(argv[4], "-v") == 0;
    pt::HostScene tor, x9, x9_emissive;
    if (!load(argv[1], "Tor.obj", tor) || !load(argv[2], "x9.obj", x9) || !load(argv[3], "x9.obj", x9_emissive)) return 1;
    const pt::HostScene r65 = random_scene(65, 1065), r3000 = random_scene(3000, 4000), fans = fans_scene();

    const float eps_values[4] = {1e-4f, 1e-2f, 0.0f, 1e-7f};
    const char *eps_names[4] = {"1e-4", "1e-2", "0", "1e-7"};
    for (int e = 0; e < 4; ++e)
        for (int cam : {20, 55}) report(std::string("tor_eps") + eps_names[e] + "_cam" + std::to_string(cam), tor, eps_values[e], cam);
    report("x9", x9, 1e-4f);
    report("x9_emissive_torus", x9_emissive, 1e-4f);
    for (int n : {0, 1, 7, 9, 65, 513, 1024, 1025, 3000}) report("random_" + std::to_string(n), random_scene(n, 1000 + n), 1e-4f);
    report("random_1100_three_sizeable_emitters", random_scene(1100, 77, 400, 3.0f), 1e-4f);
    report("random_1100_three_tiny_emitters", random_scene(1100, 77, 400, 0.05f), 1e-4f);
    report("quad", quad_scene(0.0f), 1e-4f);
    report("quad_skew_below_1pc", quad_scene(0.03f), 1e-4f);
    report("quad_skew_above_1pc", quad_scene(0.5f), 1e-4f);
    report("fans", fans, 1e-4f);

#ifdef PT_TEST_HOOKS
    pt::CullMutation &m = pt::g_cull_mutation;
    auto hooked = [&](const char *name, const pt::HostScene &s) { report(std::string("hooks:") + name, s, 1e-4f); m = pt::CullMutation(); };
    m.bvh_mode = 0; hooked("x9_bvh_mode0", x9);
    m.bvh_mode = 1; hooked("x9_bvh_mode1", x9);
    m.bvh_depth_cap = 2; hooked("x9_bvh_depth_cap2", x9);
    m.bvh_mode = 0; m.bvh_fill = 0.25; hooked("x9_bvh_mode0_fill0.25", x9);
    m.bvh_mode = 0; m.bvh_fill = 0.75; hooked("x9_bvh_mode0_fill0.75", x9);
    m.bvh_depth_cap = 2; m.bvh_fill = 0.75; hooked("x9_bvh_depth_cap2_fill0.75", x9);
    m.big_threshold = 0; hooked("tor_big_threshold0", tor);
    m.big_threshold = 0; m.bvh_mode = 0; hooked("tor_big_threshold0_bvh_mode0", tor);
    m.big_threshold = 1 << 20; hooked("random_3000_small_path", r3000);
    m.big_threshold = 1 << 20; hooked("random_6500_small_path", random_scene(6500, 6000));
    for (int mode : {1, 2, 3}) {
        m.order_mode = mode; hooked(("tor_order_mode" + std::to_string(mode)).c_str(), tor);
        m.order_mode = mode; hooked(("random_65_order_mode" + std::to_string(mode)).c_str(), r65);
    }
    m.no_absorb = 1; hooked("tor_no_absorb", tor);
    m.max_clusters = 1; hooked("fans_max_clusters1", fans);
    m.max_clusters = 1; m.no_absorb = 1; hooked("tor_no_absorb_max_clusters1", tor);
    m.emis_drop = 1; hooked("tor_emis_drop", tor);
    m.emis_drop = 1; hooked("x9_emis_drop", x9);
    struct Knob { const char *name; double pt::CullMutation::*field; };
    const Knob knobs[] = {{"sphere_r2", &pt::CullMutation::sphere_r2}, {"m0", &pt::CullMutation::m0}, {"k12", &pt::CullMutation::k12},
                          {"a_max", &pt::CullMutation::a_max}, {"quad_slack", &pt::CullMutation::quad_slack}, {"box", &pt::CullMutation::box},
                          {"box_err", &pt::CullMutation::box_err}};
    for (const Knob &k : knobs) {
        m.*k.field = 1.5; hooked((std::string("tor_") + k.name + "1.5").c_str(), tor);
        m.*k.field = 1.5; hooked((std::string("x9_") + k.name + "1.5").c_str(), x9);
    }
    m.quad_slack = 1.5; hooked("quad_skew_below_1pc_quad_slack1.5", quad_scene(0.03f));
#endif
    return 0;
}
