// Launch interface of the integrator kernel (pt_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "pt_launch_plan.hpp"
#include "pt_scene.hpp"

namespace pt {

constexpr uint32_t kPhiloxKey1 = 0x50544831u;   // "PTH1": second Philox key word (the first is the seed)
// Path regeneration (pt_kernels.hip: REGEN; skybox instantiations): new paths are started once this many ray slots of the wave
// wait for one.  1 = at once; 64 = only when no ray of the wave is alive, i.e. the passes stay in step.  The crossover is
// between -MRR 3 and -MRR 5 (profiles/r04_regen_sweep.jsonl): short paths leave few lanes idle and the primary-ray code costs a
// third of a segment whenever it runs.  From -MRR 5 up: 4 -- on an open scene 1.3 % behind "at once" (7 517 / 7 617 Msamples/s), and
// a CLOSED room that happens to have a skybox (two thirds of a lane ends per iteration there) keeps its passes in step instead
// of running that code in every other iteration (5 753 against 5 287 at 1, 5 790 at 8; r04_ab_logs.txt regen3).
constexpr uint32_t regen_min_dead_for(int mrr) { return mrr >= 5 ? 4u : 64u; }

// One material's entry of the dielectric table (RenderArgs::glass): ior == 0 = not a dielectric.  inv_ior = 1.0f / ior, formed once on the host.
struct GlassRec {
    float ior, inv_ior, pad0, pad1;
    float tint[3], pad2;
};

struct RenderArgs {
    const ClusterDesc *clusters;   // cull hierarchy (pt_scene.hpp: CullTables), read through the scalar cache
    const SphereRec *spheres;
    const CullRec *bary;
    const CullRec *bary_all;        // big scenes: one record per triangle for the pair pre-filter, else nullptr
    float a_max_all, m0_all, t_guard_all;
    const ExactRec *exact;    // n_tri records in the ORIGINAL triangle order: shading, the reference's all-triangles loop
    const ExactRec *exact_slot;   // the same records in slot order, `orig` = original index: the exact test of (ray, slot) pairs
    const BvhNode *bvh;       // big scenes: box tree over the small triangles, else nullptr
    uint32_t n_bvh;           // number of nodes
    float bvh_err;            // relative rounding allowance of the slab arithmetic
    const MatRec *mats;
    int32_t n_mats;
    const uint8_t *sky;       // skybox texels (B,G,R bytes, top-down rows) or nullptr
    int32_t sky_w, sky_h;
    float *sum, *sum2;        // row band, 3 floats per pixel
    int32_t *count;
    unsigned long long *stats;   // 24 counters (11 used; 16.. = phase timers of diagnostic builds) or nullptr
    int32_t n_clusters, n_tri;
    int32_t big;                 // CullTables::big: the hierarchy is the box tree (big-scene instantiations), not sphere trees
    uint32_t n_slots;            // slots of the hierarchy (>= n_tri: the box tree pads its leaves)
    int32_t width, height, row_begin, row_end;
    int32_t row_stride;                 // 1: the band is rows [row_begin, row_end); n > 1: every n-th tile row (8 image rows) from row_begin on, below row_end
    int32_t band_rows;                  // rows the band's planes hold (= row_end - row_begin without a stride; 8 per tile row with one)
    int32_t pass_begin, pass_count, mrr;
    float eps, error;
    uint32_t seed;
    float k1, k2, a_max, m0, m0_quad, t_guard;   // cull margins (pt_scene.hpp: CullConstants)
    int32_t blocks_x;                   // ceil(width / tile width of the instantiation launched)
    int32_t narrow;                     // 1: the statistics-free small-scene kernel runs its one-pixel-per-lane variant (8 x 8 tiles)
    int32_t adapt_pool;                 // 2 / 4: the adaptive-sampling instantiation over 16 x 8 / 32 x 8 tiles runs (batches); 0: none
    uint32_t *sched;                    // [0] ticket counter, [1 + tile] chunks of that tile already published; zeroed per launch
    uint32_t n_tiles, n_chunks;         // work items = n_tiles * n_chunks, chunk-major
    int32_t chunk_passes;               // passes per chunk; 0 = geometric chunks (see the kernel)
    int32_t vec_ok;                     // sum / sum2 / count are 16-byte aligned and width % 4 == 0: 16-byte write-back allowed
    float r_org;                        // origins with a component beyond this are outside the cull margins' envelope
    int32_t may_leave_envelope;         // 0: no triangle of this scene can be hit outside the envelope, the integrator skips the test
    // A path's last segment (depth + 1 == mrr) can only contribute by hitting an emitter: the statistics-free, skybox-free
    // instantiations search the emitters alone first (CullTables::emis_*) and run the full search only for rays that hit one.
    uint32_t regen_min_dead;            // skybox instantiations (path regeneration): new paths start once this many ray slots of the wave wait for one
    uint32_t last_segment_filter;       // 0 = off
    uint32_t emis_clusters, emis_large_w0, emis_bvh;
    // The scene handle's camera (pt_hip.h: pt_camera), appended so that the fields above keep their offsets.  camera != 0: the
    // launch runs the camera twins (integrate_kernel<..., ADAPT | 1>), which read cam = origin[3], right[3], up[3], forward[3].
    int32_t camera;
    float cam[12];
    // The handle's lens (pt_hip.h: pt_lens), appended likewise.  lens != 0 (only with camera != 0): the launch runs the lens kernels
    // (integrate_kernel_lens), which read lns = radius, focus distance, r^[3], u^[3], f^[3] (right, up, forward as unit vectors).
    int32_t lens;
    float lns[11];
    // The handle's camera motion (pt_hip.h: pt_scene_set_camera_motion), appended likewise.  motion != 0 (only with camera != 0): the
    // launch runs the motion twins (integrate_kernel_motion, integrate_kernel_motion_lens), which interpolate every component they
    // read: cam[j] + t * cam_d[j] with cam_d = end pose - cam, and lns[2 + j] + t * lns_d[j] with lns_d = the end pose's r^, u^, f^
    // minus lns[2 ..] (float differences taken on the host; lns_d is zero without a lens).
    int32_t motion;
    float cam_d[12];
    float lns_d[9];
    // The handle's projection (pt_hip.h: pt_projection), appended likewise.  projection != 0 (only with camera != 0, lens == 0 and
    // motion == 0: the host refuses the combinations): the launch runs the projection kernels (integrate_kernel_projection), planned
    // as their camera twins (plan::Variant::view == 1), which read the kind here, prj_span = span_x, span_y, and r^, u^, f^ from the
    // slots a lens would fill, lns[2 .. 10] (lns[0], lns[1] stay zero).
    int32_t projection;
    float prj_span[2];
    // The handle's environment (pt_hip.h: pt_environment_*), appended likewise.  env_map != nullptr (never with sky): the launch runs
    // the environment kernels (integrate_kernel_environment), planned as the skybox kernels of the same view (plan::Variant::sky;
    // no ids of their own in the plan).  env_map = the (env_n + 2)^2 texels of the octahedral map with its apron, 16 bytes each.
    const void *env_map;
    int32_t env_n;
    // The handle's dielectrics (pt_hip.h: pt_dielectric), appended likewise.  glass != nullptr: the launch runs the dielectric kernels
    // (integrate_kernel_glass, pt_glass_kernels.hip), planned as the kernels the same launch would run without the list (no ids of
    // their own in the plan).  glass = n_mats records of 32 bytes (GlassRec below), read only where a ray has hit a triangle.
    const void *glass;
    // The handle's albedo textures (pt_hip.h: pt_texture), appended likewise.  tex_recs != nullptr: the launch runs the texture kernels
    // (integrate_kernel_texture, pt_texture_kernels.hip: the dielectric kernels with the texel step), planned as the kernels the same
    // launch would run without the list; `glass` is then never null (a handle without dielectrics passes an all-zero table).
    // tex_recs = n_mats records of 16 bytes (pt_texture.hpp: TexRec), tex_uv = 6 floats per triangle in the ORIGINAL triangle order,
    // tex_texels = the list's texels, 16 bytes each, tex_bary = one 32-byte record per triangle (original order) that gives the hit
    // point's barycentrics: all read only where a ray has hit a triangle of a textured material.
    const void *tex_recs;
    const float *tex_uv;
    const void *tex_texels;
    const void *tex_bary;               // 32 bytes per triangle in the original order (pt_texture.hpp: TexBary): the barycentrics' record
    // The handle's shading normals (pt_hip.h: shading normals), appended likewise.  smooth_normals != nullptr: the launch runs the smooth
    // kernels (integrate_kernel_smooth, pt_smooth_kernels.hip: the texture kernels with the interpolated normal), planned as the
    // kernels the same launch would run without them; glass, tex_recs, tex_uv, tex_texels and tex_bary are then never null (a handle
    // without dielectrics or textures passes all-zero tables).  Three 16-byte records per triangle (pt_smooth.hpp: SmoothCorner) in
    // the ORIGINAL triangle order, read only where a ray that scatters has hit a triangle.
    const void *smooth_normals;
    // The handle's roughness list (pt_hip.h: rough specular), appended likewise.  rough_alpha != nullptr: the launch runs the rough kernels
    // (integrate_kernel_rough, pt_rough_kernels.hip: the smooth kernels with the GGX glossy lobe), planned as the kernels the same launch
    // would run without it; smooth_normals, glass and the tex_ pointers are then never null (a handle without them passes all-zero
    // tables).  One float per material: alpha, 0 = the mirror.  Read only where the glossy lobe of a ray that scatters has been chosen.
    const float *rough_alpha;
    // The handle's light table (pt_hip.h: direct lighting), appended likewise.  lights != nullptr: the launch runs the direct kernels
    // (integrate_kernel_direct, pt_direct_kernels.hip: the rough kernels with per-path accounting and a shadow ray at every scattering
    // diffuse hit), planned as the kernels the same launch would run without it; rough_alpha, smooth_normals, glass and the tex_
    // pointers are then never null (a handle without them passes all-zero tables).  n_lights records of 80 bytes (pt_direct.hpp:
    // LightRec) and the table's total area A.
    const void *lights;
    int32_t n_lights;
    float light_area;
    // The handle's environment sampling table (pt_hip.h: environment sampling), appended likewise.  env_alias != nullptr (only with
    // env_map): the launch runs the environment-sampling kernels (integrate_kernel_envdirect, pt_envdirect_kernels.hip: the direct
    // kernels whose shadow ray goes to the emitters or, with probability env_share, to a direction drawn from the environment).  lights
    // is then never null: a handle without emitters passes one all-zero record with n_lights = 0 and env_share = 1.  env_cells^2
    // records of 16 bytes (pt_envdirect.hpp: EnvAliasRec).
    const void *env_alias;
    int32_t env_cells;
    float env_share;
    // The handle's Russian roulette (pt_hip.h: Russian roulette), appended likewise.  rr_start > 0 (only with lights; env_alias may be
    // set too): the launch runs the roulette kernels (integrate_kernel_roulette, pt_roulette_kernels.hip: the direct kernels, or with
    // env_alias the environment-sampling kernels, whose scattering steps end with the roulette step from depth + 1 >= rr_start on
    // under the floor rr_floor in [2^-10, 1]; pt_roulette.hpp).
    int32_t rr_start;
    float rr_floor;
#ifdef PT_BLOCK_PROFILE
    uint32_t *blockprof;                // diagnostic build only (tools/asm_profile.py): execution counters of the instrumented code object
#endif
};

// The constants the kernels of this library were compiled with: what plan::plan_tiles needs to know of the build.
const plan::Build &integrator_build();
// The surface units: translation units of their own (pt_glass_kernels.hip ... pt_roulette_kernels.hip), each the unit below it with
// one more table read where a ray has hit a surface (the roulette unit: the direct and the environment-sampling unit with the step).  A launch needs the unit of the highest table its arguments hold, and every
// table below that one is then never null (a handle without it passes an all-zero table).
enum SurfaceUnit : int { kNoSurfaceUnit = 0, kGlassUnit, kTextureUnit, kSmoothUnit, kRoughUnit, kDirectUnit, kEnvDirectUnit, kRouletteUnit };
inline int surface_unit_of(const RenderArgs &a) {
    return a.rr_start > 0 ? kRouletteUnit : a.env_alias ? kEnvDirectUnit : a.lights ? kDirectUnit : a.rough_alpha ? kRoughUnit : a.smooth_normals ? kSmoothUnit : a.tex_recs ? kTextureUnit : a.glass ? kGlassUnit : kNoSurfaceUnit;
}
// launches kernel `v` (plan::plan_tiles: Tiles::variant, whose tile geometry and chunks args holds) -- with args.projection != 0
// the projection kernel of camera twin `v` (v.view == 1), which has the twin's tiles and chunks and no id of its own in the plan;
// with args.env_map != nullptr the environment kernel of skybox kernel `v` (v.sky), likewise; with surface_unit_of(args) that unit's
// kernel of whichever of those the launch would run
hipError_t launch_integrator(const RenderArgs &args, const plan::Variant &v, hipStream_t stream);
// the environment kernels' translation unit (pt_environment_kernels.hip); launch_integrator calls it, nothing else does
hipError_t launch_environment_integrator(const RenderArgs &args, const plan::Variant &v, hipStream_t stream);
// The room kernel (pt_room_kernels.hip), wide or 8 x 8; nullptr if the build has none.
void (*room_kernel(bool narrow))(const RenderArgs);
// the surface units' translation units, likewise (hipErrorNotSupported from a diagnostic build, which is linked without them)
hipError_t launch_surface_integrator(int unit, const RenderArgs &args, const plan::Variant &v, hipStream_t stream);
// waves of kernel `v` that one compute unit holds at a time (runtime occupancy query, cached).  A projection launch asks for its
// camera twin's: the projection kernels are compiled for their twins' waves per SIMD and LDS (tests/test_projection_resources.py)
hipError_t integrator_waves_per_cu(const plan::Variant &v, int *waves);
// First-hit feature pass under a projection (args.projection != 0; cam, lns and prj_span as for the integrator): the rays through
// the pixels of rows [row_begin, row_begin + rows) with jitter 0, origins / directions 3 floats per pixel.
hipError_t launch_projection_rays(const RenderArgs &args, int width, int height, int row_begin, int rows, float *d_origins, float *d_directions,
                                  hipStream_t stream);
// diagnostic: the box tree's child test on n (node, ray, t_best) items; out[i] = the mask of item i's kept children
hipError_t launch_box_masks(const BvhNode *d_nodes, const float *d_rays, const float *d_t_best, float err, int n, uint32_t *d_out, hipStream_t stream);
hipError_t launch_trace_rays(const RenderArgs &args, const float *d_origins, const float *d_directions, int n_rays,
                             int32_t *d_hit_index, float *d_hit_t, hipStream_t stream);

}  // namespace pt
