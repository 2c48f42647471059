// The launch planner's ids of the motion views (pt_launch_plan.hpp: view 3 / 4), without HIP: built and run by
// tests/test_motion_host.py.  stdout: one line per id of every view -- id, whether the product has the kernel, whether
// variant_id(variant_of(id)) == id, view, view_has_lens, view_has_motion, SKY BIG STATS ENV NARROW POOL.  stderr: a few launches
// planned for a still view and for its motion twin, "still | moving" (kernel form and tiles; they must be equal).
#include <cstdio>
#include "pt_launch_plan.hpp"
using namespace pt::plan;
constexpr Build kBuild = {8, 8, 2, 1, 6, 32766, Stats::kAsAsked, false};   // the product's constants (pt_kernels.hip)
static void print_plan(FILE *f, const Tiles &t) {
    std::fprintf(f, "%d %d %d %d %d %d %d %d %d %u", t.variant.sky, t.variant.big, t.variant.stats, t.variant.env, t.variant.narrow, t.variant.pool, t.narrow,
                 t.adapt_pool, t.blocks_x, t.n_tiles);
}
int main() {
    static_assert(kAllVariants == kViews * kVariantsPerView && kVariants == 3 * kVariantsPerView, "ids are dense over the views");
    for (int id = 0; id < kAllVariants; ++id) {
        const Variant v = variant_of(id);
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", id, variant_exists(v, kBuild), variant_id(v) == id && variant_of(variant_id(v)) == v, v.view,
                    view_has_lens(v.view), view_has_motion(v.view), v.sky, v.big, v.stats, v.env, v.narrow, v.pool);
    }
    const int sizes[4][2] = {{48, 40}, {24, 16}, {1920, 1080}, {1280, 720}};
    for (const auto &wh : sizes)
        for (int big = 0; big < 2; ++big)
            for (float error : {-1.0f, 0.02f})
                for (int view = 1; view <= 2; ++view) {
                    const Launch still = {wh[0], wh[1], false, big != 0, false, false, error, 0, 16, view, 256};
                    Launch moving = still;
                    moving.view = view + 2;
                    const Tiles a = plan_tiles(still, kBuild), b = plan_tiles(moving, kBuild);
                    if (a.variant.view != view || b.variant.view != view + 2 || !variant_exists(b.variant, kBuild)) return 3;
                    print_plan(stderr, a);
                    std::fprintf(stderr, " | ");
                    print_plan(stderr, b);
                    std::fprintf(stderr, "\n");
                }
    return 0;
}
