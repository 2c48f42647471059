// The launch plan of the integrator: which kernel variant a launch runs, how its row band is cut into tiles and how its pass
// range is cut into chunks.  Pure host arithmetic: no HIP, no RenderArgs, compiles with a plain C++17 compiler
// (tests/test_launch_plan_host.py pins it case for case).  The constants of the build are an input (Build): they are -D knobs of
// the KERNELS' translation unit, which hands them out through pt::integrator_build() (pt_kernels.hpp).
#pragma once
#include <algorithm>
#include <cstdint>

namespace pt::plan {

enum class Stats { kAsAsked, kAlways, kNever };   // which launches run the statistics kernels: those whose caller wants pt_render_stats / all / none

struct Build {
    int tile_w, tile_h;         // kTileW, kTileH: the 64-pixel block a tile is made of (8 x 8; one, two or four of them side by side)
    int rays_small, rays_big;   // pixels (rays) per lane of the statistics-free, skybox-free small-scene / big-scene kernel (PT_RAYS_PER_LANE, PT_BIG_RAYS_PER_LANE)
    int waves_per_simd;         // PT_WAVES_PER_SIMD
    int max_batch_pass;         // kMaxBatchPass: the last pass number the batch kernels' 16-bit pass words hold
    Stats stats;
    bool wide_only;             // the code object holds the camera-free wide kernels only: no 8 x 8, batch, camera-twin or lens kernels (the PT_BLOCK_PROFILE build's instrumented copy)
};

// One integrator kernel.  view: 0 = camera-free, 1 = its camera twin, 2 = the lens kernel of that twin, 3 / 4 = the motion twins
// of 1 / 2 (pt_hip.h: camera motion -- the camera interpolated between two poses at a time drawn per path).
// pool: 0, or 2 / 4 = the adaptive-sampling kernel that runs batches over 16 x 8 / 32 x 8 tiles.
// room: the room instantiation of the statistics-free plain small-scene kernel (wide or narrow; everything else false / 0): the
// search without its generic loops, for scenes whose tables say CullTables::room (pt_scene.hpp).
struct Variant {
    bool sky, big, stats, env, narrow;
    int pool, view;
    bool room = false;
};
constexpr bool operator==(const Variant &a, const Variant &b) {
    return a.sky == b.sky && a.big == b.big && a.stats == b.stats && a.env == b.env && a.narrow == b.narrow && a.pool == b.pool && a.view == b.view &&
           a.room == b.room;
}

// rays per lane of a kernel's wide form: the launch geometry (tile width) follows from it
constexpr int rays_per_lane(const Build &b, bool sky, bool big, bool stats) { return (!sky && !stats) ? (big ? b.rays_big : b.rays_small) : 1; }

// Ids: per view 0-15 the wide kernels ((sky, big, stats, env) as bits 3..0), 16-19 the 8 x 8 ones ((big, env) as bits 1..0),
// 20-23 the batch kernels ((big, pool == 4) as bits 1..0); the camera twins 24 higher, the lens kernels 48 higher, the motion
// twins of the two 72 and 96 higher.  A table indexed by id (the kernels, the occupancy cache) has kAllVariants entries.
constexpr int kVariantsPerView = 24, kViews = 5, kAllVariants = kViews * kVariantsPerView;
// The ids of the still views 0-2 come first: kStillVariants of them.  NOT a table size.  (kVariants is its name from before the
// motion views, kept because tests/native/launch_plan_main.cpp enumerates the still ids under it; new code says kStillVariants.)
constexpr int kStillVariants = 3 * kVariantsPerView, kVariants = kStillVariants;
// The view of a launch from what its handle has (a lens or a motion implies the camera twin), and back.
constexpr int view_of(bool camera, bool lens, bool motion) { return motion ? (lens ? 4 : 3) : lens ? 2 : camera ? 1 : 0; }
constexpr bool view_has_lens(int view) { return view == 2 || view == 4; }
constexpr bool view_has_motion(int view) { return view == 3 || view == 4; }
// The two room kernels (wide, narrow) have the ids after every view's: a table indexed by id has kKernelIds entries.
constexpr int kRoomVariants = 2, kKernelIds = kAllVariants + kRoomVariants;
constexpr int variant_id(const Variant &v) {
    if (v.room) return kAllVariants + v.narrow;
    return kVariantsPerView * v.view + (v.narrow ? 16 + 2 * v.big + v.env : v.pool ? 20 + 2 * v.big + (v.pool == 4) : ((v.sky * 2 + v.big) * 2 + v.stats) * 2 + v.env);
}
constexpr Variant variant_of(int id) {
    if (id >= kAllVariants) return {false, false, false, false, id - kAllVariants == 1, 0, 0, true};
    const int view = id / kVariantsPerView, r = id % kVariantsPerView;
    if (r < 16) return {(r & 8) != 0, (r & 4) != 0, (r & 2) != 0, (r & 1) != 0, false, 0, view};
    if (r < 20) return {false, (r & 2) != 0, false, (r & 1) != 0, true, 0, view};
    return {false, (r & 2) != 0, false, false, false, (r & 1) ? 4 : 2, view};
}
// Is that kernel part of a build?  The 8 x 8 form exists of the kernels with two pixels per lane; the batch kernels are not
// built with the rare envelope test (one more spilled register there), the small-scene ones only as a form of the two-pixel kernel.
constexpr bool variant_exists(const Variant &v, const Build &b) {
    if (v.room) {   // a form of the plain statistics-free small-scene kernel, where the build has that one
        if (b.wide_only || v.sky || v.big || v.stats || v.env || v.pool || v.view != 0) return false;
        return !v.narrow || rays_per_lane(b, false, false, false) > 1;
    }
    if (b.wide_only && (v.narrow || v.pool || v.view != 0)) return false;
    if (!v.narrow && !v.pool) return true;
    if (v.sky || v.stats || (v.pool && v.env)) return false;
    return (v.pool && v.big) || rays_per_lane(b, false, v.big, false) > 1;
}

// What the test builds override (pt_test_set_mutation); all zero in the product.
struct Overrides {
    int tile_width = 0;       // 1 = always 8 x 8 tiles, 2 = always 16 x 8 where the kernel has them, 3 = the same and 32 x 8 for adaptive launches, 0 = by tile count
    int items_per_slot = 0;   // equal chunks with about that many work items per wave slot (< 0: never equal chunks), 0 = by tile count
    int chunk_min = 0;        // passes the scheduler's last geometric chunk holds at least (0 = the library's)
    int regen_min_dead = 0;   // overrides RenderArgs::regen_min_dead (0 = the library's)
    int no_room_kernel = 0;   // 1 = a room-shaped scene runs the generic kernel too (the A/B and the yardstick of the room kernel's tests), 0 = by the scene's flag
};

struct Launch {
    int width, band_rows;   // band_rows: rows the band's planes hold
    bool sky, big, want_stats, may_leave_envelope;
    float error;
    int pass_begin, pass_count;
    int view;
    int cu_count;
    bool room = false;   // the scene's tables say CullTables::room and its handle has nothing a plain launch does not read (no environment, projection or surface table)
};

struct Tiles {
    Variant variant;
    int narrow, adapt_pool, blocks_x;   // as the kernels read them (RenderArgs)
    uint32_t n_tiles;
};

// Picks the kernel of a launch and cuts its row band into that kernel's tiles.  The statistics-free small-scene kernel owns
// 16 x 8 tiles (two pixels per lane) -- unless that would leave the chip's wave slots underfilled, in which case its 8 x 8
// variant runs (a tile's passes are a serial chain: fewer tiles than slots means idle SIMDs).
inline Tiles plan_tiles(const Launch &l, const Build &b, const Overrides &o = {}) {
    const int force = o.tile_width;
    const bool stats = b.stats == Stats::kAlways || (b.stats == Stats::kAsAsked && l.want_stats);
    const uint32_t rows = static_cast<uint32_t>((l.band_rows + b.tile_h - 1) / b.tile_h);      // tile rows of the band (its planes hold band_rows rows)
    const auto tiles_of = [&](int px) { return static_cast<uint32_t>((l.width + b.tile_w * px - 1) / (b.tile_w * px)) * rows; };   // tiles px column blocks wide
    const auto rounds = [&](int waves, uint32_t num, uint32_t den) { return static_cast<uint32_t>(l.cu_count) * 4u * static_cast<uint32_t>(waves) * num / den; };
    int rays = rays_per_lane(b, l.sky, l.big, stats);
    // adaptive sampling on: the kernels that run batches (not built with the rare envelope test: one more spilled register there)
    const bool batches = !b.wide_only && !l.sky && !stats && l.error >= 0.0f && !l.may_leave_envelope && l.pass_begin >= 0 &&
                         l.pass_begin + l.pass_count <= b.max_batch_pass && (l.big ? rays == 1 && force != 1 : rays > 1);
    Tiles t = {{l.sky, l.big, stats, l.may_leave_envelope, false, 0, l.view}, 0, 0, 0, 0};
    if (rays > 1 && !b.wide_only) {
        // one and a half rounds of its waves (measured, profiles/r03_ab_logs.txt ab53: 7 200 tiles -19 %, 8 160 tiles +3 %, 16 200 +6.6 %);
        // the batch kernel beats the 8 x 8 kernel's sitting out from 1.2 rounds on (1280 x 720: 29.0 against 31.7 ms, r04_ab_logs.txt adapt6)
        uint32_t min_tiles = rounds(b.waves_per_simd - 1, 3u, 2u), min_wide = batches ? rounds(b.waves_per_simd - 1, 6u, 5u) : min_tiles;
        if (force == 1) min_tiles = min_wide = 0xFFFFFFFFu;   // (test builds: always 8 x 8 / always 16 x 8 / always 32 x 8 with adaptive sampling on)
        if (force == 2 || force == 3) min_tiles = min_wide = 0;
        if (tiles_of(rays) < min_wide) {
            rays = 1;
            t.narrow = 1;
        } else if (batches) {   // over 32 x 8 tiles if there are enough of those as well, else over 16 x 8 tiles
            t.adapt_pool = (force != 2 && tiles_of(4) >= min_tiles) ? 4 : 2;
        }
    } else if (batches) {
        // the box-tree kernel (one ray slot per lane, six waves per SIMD) with adaptive sampling on: batches of 64 over 16 x 8 tiles,
        // over 32 x 8 tiles where the frame has one and a half rounds of those
        const uint32_t min_tiles = (force == 2 || force == 3) ? 0u : rounds(b.waves_per_simd, 3u, 2u);
        if (force != 2 && tiles_of(4) >= min_tiles) t.adapt_pool = 4;
        else if (tiles_of(2) >= min_tiles) t.adapt_pool = 2;
    }
    t.variant.narrow = t.narrow != 0;
    t.variant.pool = t.adapt_pool;
    // A room-shaped scene: the room form of the plain statistics-free small-scene kernel, in whichever tile width was picked above.
    // Statistics, adaptive sampling (error >= 0: batches or not), the envelope test and the camera twins keep the generic kernel.
    t.variant.room = l.room && !o.no_room_kernel && !b.wide_only && !l.sky && !l.big && !stats && !l.may_leave_envelope && l.error < 0.0f &&
                     l.view == 0 && t.adapt_pool == 0;
    const int tile_px = t.adapt_pool ? t.adapt_pool : rays;   // tile width in 8-pixel column blocks
    t.blocks_x = (l.width + b.tile_w * tile_px - 1) / (b.tile_w * tile_px);
    t.n_tiles = static_cast<uint32_t>(t.blocks_x) * rows;
    return t;
}

struct Chunks {
    uint32_t n_chunks;
    int32_t chunk_passes;   // passes per chunk; 0 = geometric chunks (see the kernel)
};

// Scheduler: cut the pass range into chunks so that the tail of the launch is balanced with small work items.  A tile's
// chunks run in order and each re-reads and re-writes the tile's accumulators, so there should be few of them: chunk c
// takes 3/4 of the passes that are left, down to single passes (256 passes: 192 + 48 + 12 + 3 + 1; until round 4 the last
// chunk held 8 to 31 passes -- 192 + 48 + 16 -- and launches below 32 passes were one chunk: 16 passes at 1080p 5.26 -> 4.71 ms,
// 64 passes 18.81 -> 18.20, 256 passes 72.70 -> 72.08, profiles/r04_ab_logs.txt chunks2).
// slots: wave slots of the chip FOR THE KERNEL THIS LAUNCH RUNS: its occupancy is the compiler's and the LDS budget's
// business, asked from the runtime once per kernel instead of assumed (pt_kernels.hpp: integrator_waves_per_cu).
inline Chunks plan_chunks(uint32_t n_tiles, uint32_t slots, int32_t pass_count, bool sky, bool narrow, bool want_stats, const Overrides &o = {}) {
    uint32_t n_chunks = 1;
    int32_t chunk_passes = 0;
    // (launches that fill a statistics block keep the old floor of 8: every work item ends with a dozen atomic adds to the same
    // few words, and 65 000 more items cost the 16-pass 1080p frame 6.7 -> 11.2 ms)
    // (and the regenerating kernels under a sky, where a chunk's end is a tail of idle lanes; the 8 x 8 kernel with its accumulators
    // in LDS stops at 2: chunks2)
    const int chunk_min = o.chunk_min > 0 ? o.chunk_min : (want_stats || sky) ? 8 : narrow ? 2 : 1;
    if (n_tiles >= slots / 2u)
        while (n_chunks < 6u && (pass_count >> (2u * n_chunks)) >= chunk_min) ++n_chunks;
    // Between about one and two tiles per wave slot the first of those chunks is too coarse -- all tiles' 3/4 of the passes: the
    // chip runs one full round of them and a second one half empty.  There the pass range is cut into EQUAL chunks, 8 to 32
    // work items per wave slot: Tor.obj 1366 x 768 x 256 spp 47.5 -> 40.2 ms, 960 x 540 25.7 -> 21.9 ms, and the 32 x 8 tiles of
    // adaptive 1080p launches (1.58 per slot) 65.2 -> 55.8 ms; from 2.3 tiles per slot up the 3/4 scheme wins again; the open
    // scene under a sky at 960 x 540 22.2 -> 20.1 ms (profiles/r04_ab_logs.txt, chunks1).
    int items_per_slot = 0;
    const unsigned long long t100 = 100ull * n_tiles;
    if (sky) {   // (regenerating kernels: a chunk's end is a tail of idle lanes, so fewer, longer chunks and a narrower range)
        if (t100 >= 75ull * slots && t100 < 190ull * slots) items_per_slot = 8;
    } else if (t100 >= 75ull * slots && t100 < 230ull * slots) {
        items_per_slot = t100 < 120ull * slots ? 8 : t100 < 190ull * slots ? 16 : 32;
    }
    if (o.items_per_slot != 0) items_per_slot = std::max(0, o.items_per_slot);   // scheduler tuning, test builds only
    if (items_per_slot > 0) {   // equal chunks, about items_per_slot work items per wave slot
        n_chunks = (static_cast<uint32_t>(items_per_slot) * slots + n_tiles - 1u) / n_tiles;
        n_chunks = std::max(1u, std::min(n_chunks, static_cast<uint32_t>(std::max(1, pass_count / 4))));
        chunk_passes = std::max(1, (pass_count + static_cast<int32_t>(n_chunks) - 1) / static_cast<int32_t>(n_chunks));
        n_chunks = static_cast<uint32_t>(std::max(1, (pass_count + chunk_passes - 1) / chunk_passes));
        if (n_chunks == 1u) chunk_passes = 0;
    }
    return {n_chunks, chunk_passes};
}

}  // namespace pt::plan
