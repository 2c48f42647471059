// The launch planner (pt_launch_plan.hpp) on its own, without HIP: built and run by tests/test_launch_plan_host.py.
// "variants": one line per id -- id, whether this build has the kernel, whether variant_id(variant_of(id)) == id, and the kernel's
// template arguments (SKY BIG STATS ENV NARROW ADAPT lens).  Otherwise: launches on stdin, one per line (width band_rows sky big
// want_stats may_leave_envelope error pass_begin pass_count cu_count waves_per_cu view tile_width items_per_slot chunk_min), their
// plans on stdout (id, the template arguments, narrow adapt_pool blocks_x n_tiles n_chunks chunk_passes).
#include <cstdio>
#include <cstring>
#include "pt_launch_plan.hpp"
#ifndef PT_BIG_RAYS_PER_LANE
#define PT_BIG_RAYS_PER_LANE 1
#endif
using namespace pt::plan;
constexpr Build kBuild = {8, 8, 2, PT_BIG_RAYS_PER_LANE, 6, 32766, Stats::kAsAsked, false};   // the product's constants (pt_kernels.hip)
static void print_kernel(const Variant &v) { std::printf("%d %d %d %d %d %d %d", v.sky, v.big, v.stats, v.env, v.narrow, v.pool | (v.view != 0), v.view == 2); }
int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "variants") == 0) {
        for (int id = 0; id < kVariants; ++id) {
            const Variant v = variant_of(id);
            std::printf("%d %d %d ", id, variant_exists(v, kBuild), variant_id(v) == id && variant_of(variant_id(v)) == v);
            print_kernel(v);
            std::printf("\n");
        }
        return 0;
    }
    int width, band_rows, sky, big, stats, env, pass_begin, pass_count, cu, waves, view;
    float error;
    Overrides o;
    while (std::scanf("%d %d %d %d %d %d %f %d %d %d %d %d %d %d %d", &width, &band_rows, &sky, &big, &stats, &env, &error, &pass_begin, &pass_count, &cu, &waves,
                      &view, &o.tile_width, &o.items_per_slot, &o.chunk_min) == 15) {
        const Tiles t = plan_tiles({width, band_rows, sky != 0, big != 0, stats != 0, env != 0, error, pass_begin, pass_count, view, cu}, kBuild, o);
        const Chunks c = plan_chunks(t.n_tiles, static_cast<uint32_t>(cu) * static_cast<uint32_t>(waves), pass_count, sky != 0, t.narrow != 0, stats != 0, o);
        if (!variant_exists(t.variant, kBuild)) return 3;
        std::printf("%d ", variant_id(t.variant));
        print_kernel(t.variant);
        std::printf(" %d %d %d %u %u %d\n", t.narrow, t.adapt_pool, t.blocks_x, t.n_tiles, c.n_chunks, c.chunk_passes);
    }
    return 0;
}
