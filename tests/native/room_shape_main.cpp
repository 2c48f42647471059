// The room-shape flag of the culling tables (pt_scene.hpp: CullTables::room) and what the launch plan makes of it, on the CPU:
// what tests/test_room_shape_host.py reads.
//   argv[1..] = pairs "directory/ file.obj": one line per scene --
//     scene <file> room <0|1> big <0|1> clusters <n> kinds <k0,k1,..> large_slots <n> quads <hex mask of word 0> pair_bits <hex>
//   then one line per launch of a fixed list, planned for a scene WITH the flag --
//     plan <name> room <0|1> narrow <0|1> id <plan::variant_id>
#include "pt_launch_plan.hpp"
#include "pt_scene.hpp"
#include <cstdio>
#include <string>

int main(int argc, char **argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        pt::HostScene s;
        std::string err;
        bool io = false;
        if (!pt::load_obj(argv[i], argv[i + 1], s, err, io)) {
            std::printf("load failed: %s\n", err.c_str());
            return 1;
        }
        pt::CullTables t;
        pt::build_cull_tables(s, 1e-4f, t);
        std::string kinds;
        for (const pt::ClusterDesc &c : t.clusters) kinds += (kinds.empty() ? "" : ",") + std::to_string(c.kind);
        uint32_t n_large = 0, quads = 0;
        if (!t.clusters.empty() && t.clusters.back().kind == 1u) {
            n_large = t.clusters.back().n_tri;
            quads = t.clusters.back().level_off[0];
        }
        const uint32_t pair_bits = 0x55555555u & (n_large >= 32u ? 0xFFFFFFFFu : ((1u << n_large) - 1u));
        std::printf("scene %s room %d big %d clusters %zu kinds %s large_slots %u quads %x pair_bits %x\n", argv[i + 1], t.room, t.big, t.clusters.size(),
                    kinds.empty() ? "-" : kinds.c_str(), n_large, quads, pair_bits);
    }
    using namespace pt::plan;
    const Build build = {8, 8, 2, 1, 6, 32766, Stats::kAsAsked, false};   // the product's constants (pt_kernels.hip: kBuild)
    struct Case { const char *name; Launch l; Overrides o; };
    const Launch plain = {1920, 1080, false, false, false, false, -1.0f, 0, 256, 0, 256, true};
    auto with = [&](auto edit) { Launch l = plain; edit(l); return l; };
    Overrides generic, narrow_tiles, wide_tiles;
    generic.no_room_kernel = 1;
    narrow_tiles.tile_width = 1;
    wide_tiles.tile_width = 2;
    const Case cases[] = {
        {"headline", plain, {}},
        {"small_frame", with([](Launch &l) { l.width = 48; l.band_rows = 24; }), {}},
        {"forced_narrow", plain, narrow_tiles},
        {"small_frame_forced_wide", with([](Launch &l) { l.width = 48; l.band_rows = 24; }), wide_tiles},
        {"flag_off", with([](Launch &l) { l.room = false; }), {}},
        {"override", plain, generic},
        {"skybox", with([](Launch &l) { l.sky = true; }), {}},
        {"statistics", with([](Launch &l) { l.want_stats = true; }), {}},
        {"adaptive", with([](Launch &l) { l.error = 0.001f; }), {}},
        {"adaptive_beyond_batches", with([](Launch &l) { l.error = 0.001f; l.pass_begin = 40000; }), {}},
        {"camera", with([](Launch &l) { l.view = 1; }), {}},
        {"motion", with([](Launch &l) { l.view = 3; }), {}},
        {"lens", with([](Launch &l) { l.view = 2; }), {}},
        {"envelope_test", with([](Launch &l) { l.may_leave_envelope = true; }), {}},
        {"big", with([](Launch &l) { l.big = true; }), {}},
    };
    for (const Case &c : cases) {
        const Tiles t = plan_tiles(c.l, build, c.o);
        if (!variant_exists(t.variant, build) || !(variant_of(variant_id(t.variant)) == t.variant) || variant_id(t.variant) >= kKernelIds) return 3;
        std::printf("plan %s room %d narrow %d id %d\n", c.name, t.variant.room, t.variant.narrow, variant_id(t.variant));
    }
    for (int id = 0; id < kKernelIds; ++id)   // ids and variants are one-to-one over the whole table, the room kernels included
        if (variant_id(variant_of(id)) != id || variant_of(id).room != (id >= kAllVariants)) return 4;
    return 0;
}
