// The body of pt::integrate_kernel, pt::integrate_kernel_lens, their motion twins and pt::integrate_kernel_projection (pt_kernels.hip),
// included inside each.  It sees the kernel's template arguments, its argument `a` and `constexpr bool LENS`, `MOTION`, `PROJ` and
// `ENVMAP`, which the including kernel defines.  ENVMAP (only pt::integrate_kernel_environment: false in every other kernel) = a miss
// adds throughput x the handle's environment map (pt_hip.h: pt_environment_*; pt_environment.hpp spells the lookup) instead of the skybox.
// GLASS (only pt::integrate_kernel_glass: false in every other kernel) = a hit on a material the handle's dielectric table marks
// (pt_hip.h: pt_dielectric) reflects or refracts by the Fresnel term instead of running the material's lobes.
// TEX (only pt::integrate_kernel_texture: false in every other kernel) = a hit on a triangle of a material the handle's texture table
// marks (pt_hip.h: pt_texture) multiplies the throughput by the texel before the emissive or the diffuse lobe runs.
// SMOOTH (only pt::integrate_kernel_smooth: false in every other kernel; with GLASS and TEX) = the glossy lobe, the diffuse lobe and
// the dielectric step run with the interpolated shading normal of the hit point (pt_hip.h: shading normals; pt_smooth.hpp spells it).
// ROUGH (only pt::integrate_kernel_rough: false in every other kernel; with SMOOTH) = the glossy lobe of a material the handle's
// roughness table marks reflects about a GGX microfacet normal and takes Ks x G1 (pt_hip.h: rough specular; pt_rough.hpp spells it).
// DIRECT (only pt::integrate_kernel_direct: false in every other kernel; with ROUGH) = a path collects its radiance in L and the
// accumulators take it once, when the path ends; a scattering diffuse hit sends a shadow ray to a sampled point of the handle's light
// table through closest_hit itself, and an emitter reached by the diffuse lobe's own ray adds nothing (pt_hip.h: direct lighting;
// pt_direct.hpp spells the term).
// ENVDIRECT (only pt::integrate_kernel_envdirect: false in every other kernel; with DIRECT and ENVMAP) = the shadow ray of a diffuse hit
// goes, with probability RenderArgs::env_share, to a direction drawn from the environment's alias table, and counts if it misses; a
// miss after a diffuse step adds nothing (pt_hip.h: environment sampling; pt_envdirect.hpp spells the sample and the term).
// ROULETTE (only pt::integrate_kernel_roulette: false in every other kernel; with DIRECT) = from depth + 1 >= RenderArgs::rr_start on,
// every scattering step ends with the roulette step on the throughput: the path ends there with a probability that follows it, and a
// survivor is divided by that probability (pt_hip.h: Russian roulette; pt_roulette.hpp spells the step).  Lanes then die at different
// depths, so these kernels regenerate paths in closed rooms too (REGEN below) and have no last-segment filter.
    constexpr int POOL = ADAPT & 6;
    constexpr bool CAM = (ADAPT & 1) != 0;
    // ROOM (bit 3 of ADAPT; only pt::integrate_kernel<false, false, false, false, NARROW, 8>, pt_room_kernels.hip): the search of a room-shaped scene
    // (pt_scene.hpp: CullTables::room) without its generic loops -- closest_hit<..., ROOM>.  Nothing else of the body differs.
    constexpr bool ROOM = (ADAPT & 8) != 0;
    static_assert(!ROOM || (ADAPT == 8 && !SKY && !BIG && !STATS && !ENV && !LENS && !MOTION && !PROJ && !ENVMAP && !GLASS && !TEX && !SMOOTH && !ROUGH && !DIRECT && !ENVDIRECT && !ROULETTE),
                  "the room instantiations are forms of the statistics-free plain small-scene kernel alone");
    static_assert(!LENS || CAM, "a lens kernel is the lens variant of a camera twin");
    static_assert(!DIRECT || (SMOOTH && ROUGH), "the direct term is written in the smooth scatter step: a direct kernel is a rough kernel with DIRECT");
    static_assert(!ENVDIRECT || (DIRECT && ENVMAP), "an environment-sampling kernel is a direct kernel with an environment");
    static_assert(!ROULETTE || DIRECT, "roulette needs per-path accounting: a roulette kernel is a direct kernel with ROULETTE");
    static_assert(!MOTION || CAM, "a motion kernel is the motion variant of a camera twin or of its lens kernel");
    static_assert(!PROJ || (CAM && !LENS && !MOTION), "a projection kernel is the projection variant of a camera twin; the host refuses a lens or a motion with it");
    static_assert(!NARROW || (!SKY && !STATS), "only the statistics-free, skybox-free kernels have a narrow variant");
    static_assert(!ENVMAP || SKY, "an environment kernel is the environment variant of a skybox kernel: regeneration, no last-segment filter");
    constexpr int R = NARROW ? 1 : rays_per_lane<SKY, BIG, STATS>();   // pixels per lane: the wave's tile is kTileW * R x kTileH
    static_assert(POOL == 0 || ((POOL == 2 || POOL == 4) && (R == 2 || BIG) && !STATS && !SKY), "batches of the tile's pixels (a pixel's number takes 8 bits): the two-pixel kernel and the box-tree kernel");
    // REGEN = path regeneration: a lane whose path has ended starts its pixel's NEXT pass at once instead of idling until the
    // longest path of the wave is done.  The skybox instantiations run this way: a scene with a skybox is an open scene, most
    // paths end on their first or second segment (scene.cpp:125-155: a miss ends the path) -- Tor.obj without its back wall has
    // 32.7 of 64 rays alive per wave-segment at -MRR 8 (profiles/r04_open_scene_probe_before.jsonl), the closed room 63.6.  The
    // frame cannot change: a pixel's passes still run in order on its own lane (its contributions are added in pass order, its
    // adaptive-sampling answer is the one main.cpp:118-125 computes before that pass), and the RNG counter is (pixel, pass,
    // segment) whatever the other lanes are doing.  The closed-room kernels keep the pass loop: there regeneration gains
    // nothing and would cost the last-segment filter, which needs the wave's rays to reach their last segment together.
    // ROULETTE: the paths of a closed room end at different depths too, and a wave without regeneration would still run until its
    // longest path is done: the roulette kernels regenerate in closed rooms as well (one trip of the pass loop runs the chunk's passes
    // inside the segment loop).  The batch forms keep the pass loop: roulette without regeneration, which is correct and only slower.
    constexpr bool REGEN = SKY || (ROULETTE && !POOL);
    static_assert(!REGEN || !POOL, "the compacting instantiation keeps the pass loop");
    // kDynSlots: batches of at most 64 pixels run with the second ray slots switched off (scalar branches around every per-ray piece of
    // the search and of shading).  Only the 16 x 8 kernel (POOL == 2) has them -- a third of its batches are such.  In the 32 x 8 kernel
    // one batch in eleven is, and the branches cost every batch 3-4 % (1080p 56.0 -> 54.1 ms, 3840 x 2160 215.5 -> 207.2,
    // r04_ab_logs.txt adapt5), so it always runs both slots.
    constexpr bool kDynSlots = POOL == 2 && R == 2;
    constexpr int kOwn = POOL ? POOL : R;   // pixels of the tile per lane: pixel j of the tile = column (j % 8) + 8 (j / 64), row (j % 64) / 8
    constexpr int kTW = kTileW * kOwn;
    __shared__ WaveLds<std::conditional_t<BIG, std::conditional_t<POOL != 0, BigQueuesAdapt<POOL>, BigQueues>, std::conditional_t<(R > 1), SmallQueues2, SmallQueues>>, R, POOL> lds;   // one wave per workgroup: all wave-private

    const int lane = threadIdx.x;
    if constexpr (decltype(lds)::kMatCache > 0) {
        if (a.n_mats <= decltype(lds)::kMatCache) {
            const float4 *src = reinterpret_cast<const float4 *>(a.mats);
            for (int i = lane; i < 3 * a.n_mats; i += 64) lds.mat.v[i] = src[i];
            wave_sync();
        }
    }
    // Work item = (pixel tile, chunk of passes), claimed from a ticket counter in chunk-major order: all tiles' first
    // chunk, then all tiles' second chunk, ...  Cutting the pass range into chunks gives the tail of the launch small
    // items to balance with (at 1080p x 64 spp one tile per wave left the last of 5.3 rounds a quarter full).
    // A chunk may only start once the tile's previous chunk has published its accumulators; because tickets are
    // taken in execution order, that chunk was claimed earlier by a wave that is running or done, so the wait below
    // cannot deadlock, and with thousands of tiles between two chunks of one tile it practically never waits.
    uint32_t item = 0;
    if (lane == 0) item = atomicAdd(&a.sched[0], 1u);
    item = __builtin_amdgcn_readfirstlane(item);
    const uint32_t tile = item % a.n_tiles, chunk = item / a.n_tiles;
    // chunk_passes > 0: equal chunks.  chunk_passes == 0: chunk c covers passes [P - (P >> 2c), P - (P >> 2(c+1))) of the launch's P
    // (3/4 of what is left each time, the last chunk takes the rest): the tail of the launch is balanced with small items while a
    // tile's accumulators make few round trips to memory (5 chunks at 256 passes: 192 + 48 + 12 + 3 + 1).
    int pass_first, pass_last;
    if (a.chunk_passes > 0) {
        pass_first = a.pass_begin + static_cast<int>(chunk) * a.chunk_passes;
        pass_last = min(a.pass_begin + a.pass_count, pass_first + a.chunk_passes);
    } else {
        pass_first = a.pass_begin + (a.pass_count - (a.pass_count >> (2u * chunk)));
        pass_last = a.pass_begin + (chunk + 1 < a.n_chunks ? a.pass_count - (a.pass_count >> (2u * (chunk + 1u))) : a.pass_count);
    }
    if (chunk > 0) {
        if (lane == 0) {
            while (__hip_atomic_load(&a.sched[1 + tile], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < chunk) __builtin_amdgcn_s_sleep(8);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // one poll, one agent-scope acquire, then plain loads
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
    // a.blocks_x counts tiles of THIS instantiation's width (the host asks integrator_tile_width)
    // A band is rows [row_begin, row_end) of the image -- or, with row_stride n > 1, every n-th TILE ROW (kTileH image rows) from row_begin
    // on, packed in the band's planes: tile row j of the band is image rows row_begin + j n kTileH ..., plane rows j kTileH ...  (the
    // interleaved split of a frame over several devices, pt_frame.cpp).  acc_y0 = the tile's first row in the band's planes; its first
    // image row follows from it (and is what the camera ray and the RNG's pixel index take).
    int tile_x0 = static_cast<int>(tile % a.blocks_x) * kTW, acc_y0 = static_cast<int>(tile / a.blocks_x) * kTileH;   // wave-uniform
    if constexpr (POOL != 0) {   // (the division runs on the vector unit: say that its results are scalars, or the 16 x 8 kernel spills one of them)
        tile_x0 = __builtin_amdgcn_readfirstlane(tile_x0);
        acc_y0 = __builtin_amdgcn_readfirstlane(acc_y0);
    }
    const int tile_y0 = a.row_begin + acc_y0 * a.row_stride;
    // pixel k of the lane: column (lane % 8) + 8 k of the tile, row lane / 8; its slot in the wave's LDS arrays is lane + 64 k
    int x[R];
    const int y = tile_y0 + (lane / kTileW);
    bool in_image[R];
    uint32_t gpix[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        x[k] = tile_x0 + (lane % kTileW) + kTileW * k;
        in_image[k] = x[k] < a.width && y < a.row_end;
        gpix[k] = static_cast<uint32_t>(static_cast<size_t>(y) * a.width + x[k]);
    }

    // The tile's accumulators live in LDS for the whole launch (read once, written once: exactly the algorithmic
    // 56 B/pixel of HBM traffic).  Keeping them in VGPRs costs a wave per SIMD; read-modify-writing them in HBM at every
    // emitter hit moved 10x the algorithmic bytes, because each hit touches three sparse cache lines.
    // Where the tile's accumulators live.  Small scenes, one ray per lane: in LDS for the whole work item (read once, written
    // once: exactly the algorithmic 56 B/pixel of HBM traffic; keeping them in VGPRs costs a wave per SIMD).  Two rays per lane,
    // and big scenes: in memory, read-modify-written when a path reaches an emitter (1 % of the samples): the LDS they would
    // take (3.5 KB / 1.8 KB per wave) is what separates 4 from 5 waves per SIMD in the first and 5 from 6 in the second, worth
    // 8 % and 3 % of the frame time (profiles/r03_ab_logs.txt, ab52 / ab54), while the extra traffic -- three sparse cache lines
    // in and out per contribution, ~0.4 GB per 256-spp frame -- is 0.08 % of the HBM peak.
    constexpr bool kAccInLds = decltype(lds)::kAccInLds;
    if constexpr (kAccInLds) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (in_image[k]) {
            const size_t p = static_cast<size_t>(acc_y0 + lane / kTileW) * a.width + x[k];
            const int id = lane + 64 * k;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lds.acc.v[c][id] = a.sum[3 * p + c];
                lds.acc.v[3 + c][id] = a.sum2[3 * p + c];
            }
            lds.acc.v[6][id] = __int_as_float(a.count[p]);
        }
    }
    }
    // Adaptive sampling (main.cpp:118-125) asks, before every pass > 10, whether the variance estimate of all three
    // channels is below `error`.  That is a pure function of the accumulators, which change only when this pixel's
    // path reaches an emitter, so the answer is cached in one bit and refreshed there: no per-pass re-reads.
    auto low_variance = [&](float c0, float c1, float c2, float q0, float q1, float q2, int n) {
        const float sc = static_cast<float>(n);
        if (!(sc > 0)) return false;
        const float mr = c0 / sc, mg_ = c1 / sc, mb = c2 / sc;
        const float dr = q0 / sc - mr * mr, dg = q1 / sc - mg_ * mg_, db = q2 / sc - mb * mb;
        return dr < a.error && dg < a.error && db < a.error;
    };
    bool lowvar[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        lowvar[k] = false;
        if constexpr (POOL) {
            // (the answers of this instantiation live in LDS, by pixel: below)
        } else if constexpr (!kAccInLds) {
            if (in_image[k] && a.error >= 0.0f) {   // (adaptive sampling off: nobody asks, and a work item need not read its tile at all)
                const size_t p = static_cast<size_t>(acc_y0 + lane / kTileW) * a.width + x[k];
                lowvar[k] = low_variance(a.sum[3 * p], a.sum[3 * p + 1], a.sum[3 * p + 2], a.sum2[3 * p], a.sum2[3 * p + 1], a.sum2[3 * p + 2], a.count[p]);
            }
        } else {
            const int id = lane + 64 * k;
            if (in_image[k]) lowvar[k] = low_variance(lds.acc.v[0][id], lds.acc.v[1][id], lds.acc.v[2][id], lds.acc.v[3][id], lds.acc.v[4][id],
                                                      lds.acc.v[5][id], __float_as_int(lds.acc.v[6][id]));
        }
    }
    // ADAPT: the pixels of the tile (number j = owner lane | column block << 6) the lane's two ray slots work on in the current
    // batch: slot 0's in bits 0-7, slot 1's in bits 8-15 (see "Batches" in the pass loop).  Everything about a traced pixel --
    // camera ray, RNG counter, accumulator address, pass -- is derived from its number where it is needed.
    uint32_t jobs = 0;
    auto job_of = [&](int k) { return (opaque(jobs) >> (8 * k)) & 0xFFu; };
    auto tile_x_of = [&](uint32_t j) { return tile_x0 + static_cast<int>((j & 63u) % kTileW) + kTileW * static_cast<int>(j >> 6); };
    auto tile_y_of = [&](uint32_t j) { return tile_y0 + static_cast<int>((j & 63u) / kTileW); };
    if constexpr (POOL) {
#pragma unroll
        for (int kb = 0; kb < kOwn; ++kb) {   // the lane's own pixels: next pass | answer
            const uint32_t j = static_cast<uint32_t>(lane) + 64u * kb;
            bool low = false;
            if (tile_x_of(j) < a.width && y < a.row_end) {
                const size_t p = static_cast<size_t>(acc_y0 + lane / kTileW) * a.width + tile_x_of(j);
                low = low_variance(a.sum[3 * p], a.sum[3 * p + 1], a.sum[3 * p + 2], a.sum2[3 * p], a.sum2[3 * p + 1], a.sum2[3 * p + 2], a.count[p]);
            }
            lds.low.v[j] = static_cast<uint16_t>((static_cast<uint32_t>(pass_first) << 1) | (low ? 1u : 0u));
        }
        wave_sync();
    }
    // adds one contribution (material.h:74-77) to pixel k of the lane and refreshes its cached adaptive-sampling answer
    auto contribute = [&](int k, float cr, float cg, float cb) {
        float n0, n1, n2, p0, p1, p2;
        int nn;
        if constexpr (!kAccInLds) {
            // (the pixel's index is rebuilt from the lane number and the tile's wave-uniform corner, like the camera ray's x, y)
            // (opaque: or the addresses are formed at the head of the pass and held -- spilled -- until here)
            uint32_t le = opaque(static_cast<uint32_t>(lane));
            int kb = k;
            if constexpr (POOL) {
                const uint32_t j = job_of(k);
                le = j & 63u;
                kb = static_cast<int>(j >> 6);
            }
            const size_t p = static_cast<size_t>(acc_y0 + static_cast<int>(le / kTileW)) * a.width + (tile_x0 + static_cast<int>(le % kTileW) + kTileW * kb);
            n0 = a.sum[3 * p] + cr; n1 = a.sum[3 * p + 1] + cg; n2 = a.sum[3 * p + 2] + cb;
            p0 = a.sum2[3 * p] + cr * cr; p1 = a.sum2[3 * p + 1] + cg * cg; p2 = a.sum2[3 * p + 2] + cb * cb;
            nn = a.count[p] + 1;
            a.sum[3 * p] = n0; a.sum[3 * p + 1] = n1; a.sum[3 * p + 2] = n2;
            a.sum2[3 * p] = p0; a.sum2[3 * p + 1] = p1; a.sum2[3 * p + 2] = p2;
            a.count[p] = nn;
        } else {
            const int id = lane + 64 * k;   // the pixel's slot in the tile's accumulators
            n0 = lds.acc.v[0][id] + cr; n1 = lds.acc.v[1][id] + cg; n2 = lds.acc.v[2][id] + cb;
            p0 = lds.acc.v[3][id] + cr * cr; p1 = lds.acc.v[4][id] + cg * cg; p2 = lds.acc.v[5][id] + cb * cb;
            nn = __float_as_int(lds.acc.v[6][id]) + 1;
            lds.acc.v[0][id] = n0; lds.acc.v[1][id] = n1; lds.acc.v[2][id] = n2;
            lds.acc.v[3][id] = p0; lds.acc.v[4][id] = p1; lds.acc.v[5][id] = p2;
            lds.acc.v[6][id] = __int_as_float(nn);
        }
        const bool now_low = low_variance(n0, n1, n2, p0, p1, p2, nn);
        if constexpr (POOL) {
            // (the answers live in LDS, by pixel, whoever traces it -- bit 0 of the pixel's word, its next pass above --; the owners
            // read them at the head of every batch)
            const uint32_t pj = job_of(k);
            lds.low.v[pj] = static_cast<uint16_t>((lds.low.v[pj] & ~1u) | (now_low ? 1u : 0u));
        } else {
            lowvar[k] = now_low;
        }
    };
    // statistics are wave-level (uniform) counts: they live in SGPRs
    using Count = std::conditional_t<STATS, uint32_t, Ignored>;
    Count n_traced = 0, n_segments = 0, n_contrib = 0, n_miss = 0;
    std::conditional_t<STATS, WaveStats, NoStats> wst;
#ifdef PT_PHASE_TIMERS
    wst.last = __builtin_amdgcn_s_memtime();
#endif

    const int mrr = a.mrr;
    const float eps = a.eps;
#ifdef PT_VERIFY_SHIPPED
    uint32_t v_checked = 0, v_bad = 0;   // wave-uniform
    uint32_t v_compacted = 0;            // passes a wave ran compacted (ADAPT): reported where this build has no other use for a field
#endif
#ifdef PT_ADAPT_COUNT
    // diagnostic build (make variant DEFS=-DPT_ADAPT_COUNT): what the batches of the adaptive instantiations held, reported in the
    // statistics block's fields: samples_traced = rays, wave_node_rounds / wave_exact_iterations = one- / two-slot batches,
    // segments / wave_segments = segment-loop iterations inside one- / two-slot batches
    uint32_t c_rays = 0, c_one = 0, c_two = 0, c_seg1 = 0, c_seg2 = 0;
#endif
    auto any_of = [&](const bool (&b)[R]) {   // wave-uniform: any ray of the wave
        bool v = b[0];
#pragma unroll
        for (int k = 1; k < R; ++k) v = v || b[k];
        return __any(v);
    };

    // this lane's path state (REGEN: across passes -- a lane is in a pass of its own)
    Ray q[R];
    float tr[R], tg[R], tb[R];   // Ray::color_ (throughput), ray.h:17
    int depth[R];
    int cur_pass[R], next_pass[R];   // REGEN: the pass slot k's path belongs to / the next one its pixel has to run
    // DIRECT: the path's radiance L; the pending shadow ray's direction (its origin is the path ray's), term and light (the triangle's
    // original index); `lit` = the path's last step was a diffuse one, whose emitters the shadow ray has sampled.  A shadow ray is
    // searched in the segment-loop iteration after the one that made it, alone (shadow_phase), so `pending` lives for one iteration.
    [[maybe_unused]] float Lr[R], Lg[R], Lb[R], sdx[R], sdy[R], sdz[R], scr[R], scg[R], scb[R];
    [[maybe_unused]] int slight[R];
    [[maybe_unused]] bool lit[R], pending[R];
    if constexpr (DIRECT) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            Lr[k] = Lg[k] = Lb[k] = 0.0f;
            sdx[k] = sdy[k] = sdz[k] = scr[k] = scg[k] = scb[k] = 0.0f;
            slight[k] = -1;
            lit[k] = pending[k] = false;
        }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        tr[k] = tg[k] = tb[k] = 1.0f;
        depth[k] = mrr;
        cur_pass[k] = next_pass[k] = pass_first;
        q[k].ox = q[k].oy = q[k].oz = 0.0f; q[k].dx = q[k].dy = 0.0f; q[k].dz = 1.0f;
    }
    for (int pass = pass_first; POOL ? true : REGEN ? pass == pass_first : pass < pass_last; ++pass) {   // (REGEN: one trip, the loop inside runs all passes; POOL: one trip per batch)
        // Adaptive skip, main.cpp:118-125.
        bool skip[R], traced[R];
        bool two = true;   // wave-uniform: some lane's second ray slot is in use this pass
        if constexpr (!POOL) {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                skip[k] = !in_image[k] || (pass > 10 && (pass % 4) && lowvar[k]);
                if constexpr (REGEN) skip[k] = true;   // (paths are started inside the segment loop)
                traced[k] = !skip[k];
            }
            if constexpr (!REGEN) {
                if (!any_of(traced)) continue;
            }
        }
        // Batches (ADAPT).  With adaptive sampling on, most pixels of a tile sit out three passes of four in the second half of a
        // frame (Tor.obj, -ERR 0.001, 256 spp: a third of the pixels are still traced at the end), scattered over the tile: a wave
        // that runs the tile pass by pass, two pixels per lane, pays nearly every pass in full for a third of the rays.  So this
        // instantiation does not run passes, it runs BATCHES.  Every pixel of the tile (64 ADAPT of them: twice as many as ray
        // slots with 32 x 8 tiles) has its own next pass (lds.low: pass << 1 | "variance is low"), stepped over the passes it
        // sits out; a batch takes pixels that still have a pass to run in this work item, each at ITS next pass: up to 128, two
        // per lane, if at least PT_ADAPT_TWO_AT wait; otherwise up to 64, one per lane, with the second ray slots switched off
        // (`two`: 0.65 of the cost of a two-slot batch, profiles/r04_ab_logs.txt adapt1).  When more wait than a batch takes,
        // those that are furthest behind go first (all at the smallest next pass, then the others in pixel order), so that
        // the tile's pixels finish together.  The chosen pixels' numbers are compacted into a list (ranks by ballot and prefix
        // over the column blocks); ray slot k of lane l traces entry l + 64 k.
        // A pixel's passes still run in order, one per batch at most: its contributions are added in pass order and its
        // adaptive-sampling answer is the one main.cpp:118-125 computes before that pass (it changes only when the pixel's own
        // path contributes).  A sample does not depend on the lane or the batch that traces it (the counter RNG is keyed by pixel
        // and pass, the search returns the minimum over the same candidates), so the frame does not change.
        // the RNG's pixel index of ray slot k
        auto rng_pixel = [&](int k) {
            if constexpr (POOL) {
                const uint32_t j = job_of(k);
                return static_cast<uint32_t>(static_cast<size_t>(tile_y_of(j)) * a.width + tile_x_of(j));
            }
            return opaque(gpix[k]);
        };
        if constexpr (POOL) {
            wave_sync();   // (the answers written while shading the last batch, by whichever lane traced the pixel)
            uint32_t word[kOwn], np[kOwn];
            bool pend[kOwn], sel[kOwn];
            unsigned long long pb[kOwn];
            const uint32_t le = opaque(static_cast<uint32_t>(lane));   // (or the words' addresses are kept -- spilled -- across the batch)
            uint32_t n_pend = 0, behind = ~0u;
#pragma unroll
            for (int kb = 0; kb < kOwn; ++kb) {
                const uint32_t j = le + 64u * kb;
                word[kb] = lds.low.v[j];
                np[kb] = word[kb] >> 1;
                if (np[kb] > 10u && (np[kb] & 3u) && (word[kb] & 1u)) np[kb] = (np[kb] + 3u) & ~3u;   // sits out until the next multiple of 4
                pend[kb] = tile_x_of(j) < a.width && tile_y_of(j) < a.row_end && static_cast<int>(np[kb]) < pass_last;
                sel[kb] = pend[kb];
                pb[kb] = __ballot(pend[kb]);
                n_pend += __builtin_popcountll(pb[kb]);
                behind = min(behind, pend[kb] ? np[kb] : ~0u);
            }
            if (n_pend == 0) break;
            // (the box-tree kernel has one ray slot per lane; in the 32 x 8 kernel, which has no kDynSlots, a batch costs the same however few it holds)
            const uint32_t quota = (R == 2 && (!kDynSlots || n_pend >= static_cast<uint32_t>(PT_ADAPT_TWO_AT))) ? 128u : 64u;
            if (n_pend > quota) {
                const uint32_t m = wave_min(behind);
                uint32_t at_a = 0, at_b = 0, rank_a[kOwn], rank_b[kOwn];
                bool is_a[kOwn];
#pragma unroll
                for (int kb = 0; kb < kOwn; ++kb) {
                    is_a[kb] = pend[kb] && np[kb] == m;
                    const unsigned long long ab = __ballot(is_a[kb]), bb = pb[kb] & ~ab;
                    rank_a[kb] = at_a + lanes_below(ab);
                    rank_b[kb] = at_b + lanes_below(bb);
                    at_a += __builtin_popcountll(ab);
                    at_b += __builtin_popcountll(bb);
                }
                const uint32_t quota_b = at_a >= quota ? 0u : quota - at_a;
#pragma unroll
                for (int kb = 0; kb < kOwn; ++kb) sel[kb] = is_a[kb] ? rank_a[kb] < quota : (pend[kb] && rank_b[kb] < quota_b);
            }
            uint32_t n_sel = 0;
#pragma unroll
            for (int kb = 0; kb < kOwn; ++kb) {
                const unsigned long long sb = __ballot(sel[kb]);
                if (sel[kb]) lds.pairs[n_sel + lanes_below(sb)] = le + 64u * kb;   // (the queues are empty between two searches)
                n_sel += __builtin_popcountll(sb);
            }
            wave_sync();
            two = n_sel > 64u;
#ifdef PT_ADAPT_COUNT
            c_rays += n_sel;
            if (two) ++c_two; else ++c_one;
#endif
            jobs = 0;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                skip[k] = le + 64u * k >= n_sel;
                traced[k] = !skip[k];
                if (traced[k]) jobs |= lds.pairs[le + 64u * k] << (8 * k);
            }
#ifdef PT_VERIFY_SHIPPED
            if (__any((traced[0] && (jobs & 0xFFu) != le) || (traced[R - 1] && R == 2 && (jobs >> 8) != le + 64u))) ++v_compacted;
#endif
            wave_sync();   // (the list was in the pair queue: read before the search fills that)
#pragma unroll
            for (int kb = 0; kb < kOwn; ++kb)   // the owners: the chosen pixels' next pass
                lds.low.v[le + 64u * kb] = static_cast<uint16_t>(((np[kb] + (sel[kb] ? 1u : 0u)) << 1) | (word[kb] & 1u));
        }
        const bool k1_on = kDynSlots ? two : true;   // (PT_SLOT_ON)

        // Primary ray, main.cpp:126-129 + Ray ctor ray.h:21-25 (double arithmetic, then narrowed).
        // MOTION: every component of the camera (and of the lens axes) is c[j] + t * delta[j] (pt_hip.h: camera motion), formed
        // where it is consumed from the two kernel-argument segments, so that the interpolated camera never sits in registers.
        // Returns t, the path's time within the shutter interval (start_path takes the origin with it), 0 without MOTION.
        auto primary_dir = [&](int k, int pass_k, float &out_dx, float &out_dy, float &out_dz) -> float {
            float t = 0.0f;
            {
                // the time comes first: only t is held across the double-precision jitter below
                if constexpr (MOTION) {
                    uint32_t m0, m1, m2, m3;
                    philox4x32_10(rng_pixel(k), static_cast<uint32_t>(pass_k), 0xFFFFFFFEu, 0u, a.seed, kPhiloxKey1, m0, m1, m2, m3);
                    t = unit_float(m0);
                }
                uint32_t w0, w1, w2, w3;
                philox4x32_10(rng_pixel(k), static_cast<uint32_t>(pass_k), 0xFFFFFFFFu, 0u, a.seed, kPhiloxKey1, w0, w1, w2, w3);
                // LENS: the point of the thin lens (pt_hip.h: pt_lens) from the two words the jitter leaves unused, in polar form
                // (rho cos phi, rho sin phi) on the disc of radius lns[0].  Taken first, so that w2 and w3 are not held across the
                // double-precision jitter below (the skybox kernels, at 96 VGPRs, spilled them).
                float pa = 0.0f, pb = 0.0f;
                if constexpr (LENS) {
                    const float rho = lens_view()[0] * sqrt_rn_normal(unit_float(w2));   // unit_float: a multiple of 2^-24 in [2^-24, 1)
                    float sn, cs;
                    portable_sincos(2 * 3.141593f * unit_float(w3), sn, cs);
                    pa = rho * cs;
                    pb = rho * sn;
                }
                const double jx = jitter_double(w0), jy = jitter_double(w1);
                // x, y are made opaque once per pass so that their int->double conversions (and the doubles of width and
                // height) are redone here instead of being hoisted out of the pass loop, where they would occupy eight
                // VGPRs for the whole kernel (the compiler spilled them to scratch: ~1 GB of memory traffic per frame).
                // (x and y themselves are rebuilt from the lane number and the tile's wave-uniform corner: kept in two VGPRs for the
                // whole kernel they were spilled to scratch, a launch-time cost that doubled the time of a 256 x 256 frame)
                // (the big-scene kernel has the registers to keep them: there the recomputation costs 2.6 %)
                int xi = x[k], yi = y;
                if constexpr (!BIG) {
                    xi = tile_x0 + static_cast<int>(opaque(static_cast<uint32_t>(lane)) % kTileW) + kTileW * k;
                    yi = tile_y0 + static_cast<int>(opaque(static_cast<uint32_t>(lane)) / kTileW);
                }
                if constexpr (POOL) {
                    xi = tile_x_of(job_of(k));
                    yi = tile_y_of(job_of(k));
                }
                int wi = a.width, hi = a.height;
                asm volatile("" : "+v"(xi), "+v"(yi), "+s"(wi), "+s"(hi));
                const float ddx = static_cast<float>((xi + jx) / wi - 0.5f);
                const float ddy = static_cast<float>(-(yi + jy) / hi + 0.5f);
                if constexpr (PROJ) {
                    // a non-perspective projection (pt_hip.h: pt_projection; pt_projection.hpp spells the ray): from here on the
                    // jitter's doubles are dead, so the angular work (sincos, root, divide) does not meet them.  The kind is a kernel
                    // argument: a scalar branch.  The origin goes straight into the ray slot, one component at a time, as the lens's does.
                    const ProjectionView pv = projection_view();
                    projection_primary_ray(pv.kind(), ddx, ddy, camera_view(), lens_view() + 2, pv.span(),
                                           [](float ang, float &sn, float &cs) { portable_sincos(ang, sn, cs); },
                                           [](float &vx, float &vy, float &vz) { normalize3(vx, vy, vz); },
                                           q[k].ox, q[k].oy, q[k].oz, out_dx, out_dy, out_dz);
                } else if constexpr (CAM) {
                    // u right + v up + forward, componentwise, unfused (-ffp-contract=off); with the reference camera every step
                    // is exact (x 1, + 0) and |d|^2 is the sum below, so the twin's frame is the camera-free kernel's bit for bit
                    const CameraView c = camera_view();
                    MotionView cd = nullptr;
                    if constexpr (MOTION) cd = camera_delta_view();
                    const auto cam = [&](int j) -> float {
                        if constexpr (MOTION) return c[j] + t * cd[j];
                        else return c[j];
                    };
                    float dx = (ddx * cam(3) + ddy * cam(6)) + cam(9);
                    float dy = (ddx * cam(4) + ddy * cam(7)) + cam(10);
                    float dz = (ddx * cam(5) + ddy * cam(8)) + cam(11);
                    if constexpr (LENS) {
                        // the lens point L = pa r^ + pb u^ (r^ = lns[2..4], u^ = lns[5..7]); the ray from origin + L through the
                        // point where D meets the focal plane (distance lns[1] along f^ = lns[8..10]).  The origin goes straight
                        // into the ray slot, one component at a time.
                        // (MOTION: r^, u^, f^ interpolated like the camera, not renormalised)
                        const LensView l = lens_view();
                        MotionView ld = nullptr;
                        if constexpr (MOTION) ld = lens_delta_view();
                        const auto axis = [&](int j) -> float {   // j = 2 .. 10
                            if constexpr (MOTION) return l[j] + t * ld[j - 2];
                            else return l[j];
                        };
                        const float s = l[1] / ((dx * axis(8) + dy * axis(9)) + dz * axis(10));
                        const float lx = pa * axis(2) + pb * axis(5);
                        q[k].ox = cam(0) + lx;
                        dx = dx * s - lx;
                        const float ly = pa * axis(3) + pb * axis(6);
                        q[k].oy = cam(1) + ly;
                        dy = dy * s - ly;
                        const float lz = pa * axis(4) + pb * axis(7);
                        q[k].oz = cam(2) + lz;
                        dz = dz * s - lz;
                    }
                    normalize3(dx, dy, dz);
                    out_dx = dx; out_dy = dy; out_dz = dz;
                } else {
                    const float ddz = 1.0f;
                    const float inv = rcp_rn_normal(sqrt_rn_normal((ddx * ddx + ddy * ddy) + (1.0f * 1.0f + 0.0f * 0.0f)));   // 1 <= argument < 2
                    out_dx = ddx * inv; out_dy = ddy * inv; out_dz = ddz * inv;
                }
            }
            return t;
        };
        // starts slot k's path along a primary direction (eye fixed at (0, 0, -20), main.cpp:129 -- or the camera's; Ray::color_ = 1, ray.h:17)
        auto start_path = [&](int k, float ddx, float ddy, float ddz, float t) {
            q[k].dx = ddx; q[k].dy = ddy; q[k].dz = ddz;
            if constexpr (LENS || PROJ) {
                // (the origin, camera origin + lens point -- or the projection's: primary_dir wrote it)
            } else if constexpr (MOTION) {
                const CameraView c = camera_view();
                const MotionView cd = camera_delta_view();
                q[k].ox = c[0] + t * cd[0]; q[k].oy = c[1] + t * cd[1]; q[k].oz = c[2] + t * cd[2];
            } else if constexpr (CAM) {
                const CameraView c = camera_view();
                q[k].ox = c[0]; q[k].oy = c[1]; q[k].oz = c[2];
            } else {
                q[k].ox = 0.0f; q[k].oy = 0.0f; q[k].oz = -20.0f;
            }
            tr[k] = tg[k] = tb[k] = 1.0f;
            depth[k] = 0;
            if constexpr (DIRECT) {
                Lr[k] = Lg[k] = Lb[k] = 0.0f;
                lit[k] = false;
            }
        };
        auto primary_ray = [&](int k, int pass_k) {
            float ddx, ddy, ddz;
            const float t = primary_dir(k, pass_k, ddx, ddy, ddz);
            start_path(k, ddx, ddy, ddz, t);
        };
        // the pass of ray slot k's path: the wave's (a scalar) -- or, with regeneration or batches, the slot's own
        auto pass_of = [&](int k) {
            if constexpr (POOL) {   // (a traced pixel's word holds the pass AFTER this one: read where needed, a register would spill)
                return static_cast<int>(lds.low.v[job_of(k)] >> 1) - 1;
            } else if constexpr (REGEN) {
                return cur_pass[k];
            } else {
                return pass;
            }
        };
        if constexpr (!REGEN) {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                tr[k] = tg[k] = tb[k] = 1.0f;
                depth[k] = mrr;
                if (PT_SLOT_ON(k) && !skip[k]) {
                    primary_ray(k, pass_of(k));
                } else {
                    q[k].ox = q[k].oy = q[k].oz = 0.0f; q[k].dx = q[k].dy = 0.0f; q[k].dz = 1.0f;
                }
                if constexpr (STATS) n_traced += __builtin_popcountll(__ballot(!skip[k]));
            }
        }
        // DIRECT: a path that has ended hands its radiance to the accumulators, once (count = the paths traced)
        [[maybe_unused]] auto path_over = [&](int k) { return !(depth[k] < mrr && (tr[k] != 0.0f || tg[k] != 0.0f || tb[k] != 0.0f)); };
        for (;;) {
            bool valid[R];
#pragma unroll
            for (int k = 0; k < R; ++k) valid[k] = depth[k] < mrr && (tr[k] != 0.0f || tg[k] != 0.0f || tb[k] != 0.0f);   // Ray::IsValid, ray.h:52-54
            // DIRECT: the shadow rays the last iteration's shading left are searched first, alone: the slot's ray takes the shadow
            // direction for this iteration (the origin is the same) and gets its own back below.
            [[maybe_unused]] bool shadow_phase = false;
            if constexpr (DIRECT) {
                shadow_phase = any_of(pending);
                if (shadow_phase) {
#pragma unroll
                    for (int k = 0; k < R; ++k) {
                        valid[k] = pending[k];
                        if (pending[k]) {
                            float t;
                            t = q[k].dx; q[k].dx = sdx[k]; sdx[k] = t;
                            t = q[k].dy; q[k].dy = sdy[k]; sdy[k] = t;
                            t = q[k].dz; q[k].dz = sdz[k]; sdz[k] = t;
                        }
                    }
                }
            }
            if constexpr (REGEN) {
                if (!shadow_phase) {
                // Regeneration: a slot whose path is over takes its pixel's next pass -- after the adaptive skip of
                // main.cpp:118-125, which sits out passes > 10 that are not multiples of 4 while the variance is low: the next
                // one that runs is then the next multiple of 4.
                // The primary-ray code (Philox, two double-precision divisions, a normalisation) costs about a third of a segment
                // however few lanes run it, so it runs only once a.regen_min_dead slots of the wave wait for a path, or when no
                // ray of the wave is alive (a.regen_min_dead = 64: the wave's passes stay in step, as without regeneration).  The
                // host sets it per launch (enqueue_render): 4 from -MRR 5 up, 64 below -- measured on Tor.obj without its back
                // wall, 1080p x 64 spp (profiles/r04_regen_sweep.jsonl; Msamples/s at 1 / 16 / 32 / 64): -MRR 8 6 980 / 6 650 / 6 210 /
                // 5 350, -MRR 5 8 250 / 8 030 / 7 710 / 8 100, -MRR 3 11 260 / 11 360 / 12 740 / 13 390.  Making the rays in advance and
                // in batches (a ray in store per slot) was built and measured too: +1 % at -MRR 8, -16 % at -MRR 3 still -- a slot
                // that ends two paths in a row has nothing in store, and some slot of 64 nearly always does (r04_ab_logs.txt, regen2).
                // Which iteration a path starts in changes nothing about it: the frames are the same for every setting.
                uint32_t n_wait = 0;
                bool wants[R];
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    wants[k] = false;
                    if (!valid[k] && in_image[k]) {
                        int np = next_pass[k];
                        if (np > 10 && (np & 3) && lowvar[k]) np = (np + 3) & ~3;
                        next_pass[k] = np;                 // (the skip is final: lowvar only changes when this slot's own path contributes)
                        wants[k] = np < pass_last;
                    }
                    n_wait += __builtin_popcountll(__ballot(wants[k]));
                }
                if (n_wait >= a.regen_min_dead || (n_wait > 0 && !any_of(valid))) {
#pragma unroll
                    for (int k = 0; k < R; ++k) {
                        if (wants[k]) {
                            cur_pass[k] = next_pass[k];
                            primary_ray(k, next_pass[k]);
                            next_pass[k] = next_pass[k] + 1;
                        }
                        valid[k] = valid[k] || wants[k];
                        if constexpr (STATS) n_traced += __builtin_popcountll(__ballot(wants[k]));
                    }
                }
                }
            }
            if (!any_of(valid)) break;
#ifdef PT_ADAPT_COUNT
            if (two) ++c_seg2; else ++c_seg1;
#endif
            if constexpr (STATS) {
                if (!shadow_phase) {
#pragma unroll
                for (int k = 0; k < R; ++k) n_segments += __builtin_popcountll(__ballot(valid[k]));
                }
            }

            float best[R];
            int hit[R];
            const ExactRec *hit_rec[R];
            // The culling margins hold for origins within r_org of the scene (pt_scene.cpp).  A path can leave that envelope:
            // the reference accepts a near-degenerate triangle for points that have nothing to do with it, at any distance
            // (all three computed sub-areas can vanish), and the next segment then starts millions of units away.  For such
            // a ray nothing is culled: every triangle goes through the exact test.  (A NaN origin counts as outside.)
            // (one v_max3_f32 with |.| modifiers and one compare; an origin here is never NaN: it is o + d t + N eps of finite terms)
            bool inside[R];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                inside[k] = true;
                if constexpr (ENV)
                    inside[k] = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(q[k].ox), __builtin_fabsf(q[k].oy)), __builtin_fabsf(q[k].oz)) <= a.r_org;
            }
            // A path's last segment (depth + 1 == mrr; the live rays of a wave reach it together) can only contribute by hitting
            // an emitter, and whatever else it hits is never looked at (no next ray, statistics not requested, no skybox).  So
            // the search runs among the emitters alone first -- for Tor.obj one quad record instead of seven walls and a torus --
            // and the full search, which decides whether the emitter really is the closest hit, only for rays that hit one.
            bool searched[R], last_or_dead[R];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                searched[k] = valid[k];
                last_or_dead[k] = !valid[k] || depth[k] + 1 >= mrr;
            }
            bool all_last = last_or_dead[0];
#pragma unroll
            for (int k = 1; k < R; ++k) all_last = all_last && last_or_dead[k];
            if constexpr (DIRECT) all_last = all_last && !shadow_phase;   // (a shadow ray is no last segment: the full search decides it)
            // (big scenes: the flag's scalar registers cost more than it saves; ROULETTE: the wave's rays no longer reach their last segment together)
            constexpr bool kLastSegmentFilter = !STATS && !SKY && !BIG && !ROULETTE;
            bool emis_phase = false;
            if constexpr (kLastSegmentFilter) emis_phase = a.last_segment_filter != 0u && __all(all_last);
#ifdef PT_VERIFY_SHIPPED
            bool filtered_last = emis_phase;   // wave-uniform: this segment's search only has to find emitters
#endif
            if constexpr (BIG && !STATS && !SKY) {
                // Big scenes: the same idea without a second search.  The table builder keeps a big scene's emitters in the
                // large class (pt_scene.cpp), so the conservative test of those records alone says which rays of the last
                // segment can reach an emitter at all; only those are searched.
                if (a.last_segment_filter != 0u && a.emis_bvh == 0u && a.n_clusters == 1 && __all(all_last)) {
                    const ConstF cp = (ConstF)reinterpret_cast<uintptr_t>(a.clusters) + (sizeof(ClusterDesc) / 4) * (a.n_clusters - 1);
                    const uint32_t n_large = ((ConstU)cp)[5], kind = ((ConstU)cp)[6], off = ((ConstU)cp)[7], quads = ((ConstU)cp)[9];
                    if (kind == 1u && n_large <= static_cast<uint32_t>(kChunk)) {
                        float k1 = a.k1, k2 = a.k2, a_max = a.a_max, m0 = a.m0, m0q = a.m0_quad, t_guard = a.t_guard;
                        asm volatile("" : "+v"(k1), "+v"(k2), "+v"(a_max), "+v"(m0), "+v"(m0q), "+v"(t_guard));
                        const ConstF bp = (ConstF)reinterpret_cast<uintptr_t>(a.bary) + 12 * static_cast<size_t>(off);
                        uint32_t m = 0;
                        for (uint32_t rest = (a.emis_large_w0 | (a.emis_large_w0 >> 1)) & 0x55555555u; rest != 0; rest &= rest - 1) {
                            const uint32_t k0 = __builtin_ctz(rest);
                            if ((quads >> k0) & 1u) {
                                m |= (~cull_reject_quad(load_cull(bp + 12 * k0), q[0], k1, k2, a_max, m0q, t_guard) & 3u) << k0;
                            } else {
                                for (uint32_t j = 0; j < 2; ++j)
                                    m |= cull_reject(load_cull(bp + 12 * (k0 + j)), q[0], k1, k2, a_max, m0, t_guard) ? 0u : (1u << (k0 + j));
                            }
                        }
                        bool can_reach = (m & a.emis_large_w0) != 0u;
                        if constexpr (ENV) can_reach = can_reach || !inside[0];   // (outside the margins' envelope nothing is culled)
                        searched[0] = valid[0] && can_reach;
#ifdef PT_VERIFY_SHIPPED
                        filtered_last = true;
#endif
                    }
                }
            }
            for (;;) {
                if (BIG && !any_of(searched)) break;
                closest_hit<ENV, kLastSegmentFilter, kDynSlots, ROOM>(a, lds, q, searched, inside, lane, eps, best, hit, hit_rec, wst, emis_phase, two);
                if (!emis_phase) break;
                emis_phase = false;
#pragma unroll
                for (int k = 0; k < R; ++k) searched[k] = searched[k] && hit[k] >= 0;
                if (!any_of(searched)) break;
            }
#pragma unroll
            for (int k = 0; k < R; ++k)
                if (!searched[k]) hit[k] = -1;   // (a ray of the last segment that met no emitter ends like a miss, contributing nothing)
#ifdef PT_VERIFY_SHIPPED
            // Verification of the path that SHIPS (libpt_verify_shipped.so, never the product): this is the statistics-free
            // instantiation with the emitter-first last segment and the big scenes' can-reach filter compiled in.  Every segment's
            // result is compared with Scene::TraceRay's loop as written (scene.cpp:116-120) for the lane's own ray: the same
            // (distance bits, triangle index) -- except that a FILTERED last segment may report a miss where the reference hits
            // something, if and only if that something has no emissive lobe (nothing else of a last segment is ever looked at:
            // Ray::IsValid ray.h:52-54, material.h:67-80).
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const unsigned long long brute = brute_force_key(a, q[k], eps);
                const unsigned long long mine = hit[k] < 0 ? ~0ull : ((static_cast<unsigned long long>(ordered_bits(best[k])) << 32) | static_cast<uint32_t>(hit[k]));
                bool ok = brute == mine;
                if (!ok && filtered_last && mine == ~0ull) {
                    bool emissive = false;
                    if (brute != ~0ull) {
                        const MatRec m = a.mats[a.exact[static_cast<uint32_t>(brute)].material];
                        emissive = (m.n_lobes >= 1 && m.kind0 == 0) || (m.n_lobes >= 2 && m.kind1 == 0);
                    }
                    ok = !emissive;
                }
                v_checked += static_cast<uint32_t>(__builtin_popcountll(__ballot(valid[k])));
                v_bad += static_cast<uint32_t>(__builtin_popcountll(__ballot(valid[k] && !ok)));
                if (valid[k] && !ok && a.stats) {   // one example for the host to print (any of them)
                    a.stats[11] = brute;
                    a.stats[12] = mine;
                    a.stats[13] = (static_cast<unsigned long long>(__float_as_uint(q[k].ox)) << 32) | __float_as_uint(q[k].oy);
                    a.stats[14] = (static_cast<unsigned long long>(__float_as_uint(q[k].oz)) << 32) | __float_as_uint(q[k].dx);
                    a.stats[15] = (static_cast<unsigned long long>(__float_as_uint(q[k].dy)) << 32) | __float_as_uint(q[k].dz);
                }
            }
#endif

            // DIRECT: the shadow rays' verdicts.  The term counts if and only if the closest hit is the sampled light's triangle; the
            // slot's path ray comes back, and a path that had ended with the step (throughput zero) is handed in now.
            if constexpr (DIRECT) {
                if (shadow_phase) {
#pragma unroll
                    for (int k = 0; k < R; ++k) {
                        bool added = false;
                        if (PT_SLOT_ON(k) && pending[k]) {
                            if (hit[k] == slight[k]) {
                                Lr[k] += scr[k]; Lg[k] += scg[k]; Lb[k] += scb[k];
                                added = true;
                            }
                            q[k].dx = sdx[k]; q[k].dy = sdy[k]; q[k].dz = sdz[k];
                            pending[k] = false;
                            if (path_over(k)) contribute(k, Lr[k], Lg[k], Lb[k]);
                        }
                        if constexpr (STATS) n_contrib += __builtin_popcountll(__ballot(added));
                    }
                    continue;
                }
            }
            // ---- 3. shade (Scene::TraceRay scene.cpp:121-156, Material::Process material.h:36-50), ray after ray of the lane
#pragma unroll
            for (int k = 0; k < R; ++k) {
            if constexpr (STATS) n_miss += __builtin_popcountll(__ballot(valid[k] && hit[k] < 0));
            bool contributed = false;
            if (PT_SLOT_ON(k) && valid[k]) {
                if (hit[k] < 0) {
                    if constexpr (ENVMAP) {   // environment miss shader: throughput x L(direction), four 16-byte loads, no double
                        const EnvironmentView ev = environment_view();
                        float lr, lg, lb;
                        env_lookup(ev.map(), ev.n(), q[k].dx, q[k].dy, q[k].dz, lr, lg, lb);
                        if constexpr (ENVDIRECT) {   // (an environment the diffuse step's shadow ray has sampled already adds nothing)
                            if (!lit[k]) {
                                Lr[k] += tr[k] * lr; Lg[k] += tg[k] * lg; Lb[k] += tb[k] * lb;
                                contributed = true;
                            }
                        } else if constexpr (DIRECT) {
                            Lr[k] += tr[k] * lr; Lg[k] += tg[k] * lg; Lb[k] += tb[k] * lb;
                            contributed = true;
                        } else {
                        contribute(k, tr[k] * lr, tg[k] * lg, tb[k] * lb);
                        contributed = true;
                        }
                    } else if (SKY) {   // skybox miss shader, scene.cpp:126-154 (note: the path throughput is NOT applied)
                        const float pi = 3.141593f;
                        const float theta = portable_acosf(q[k].dy) / pi;
                        const float phi = portable_atan2f(q[k].dz, -q[k].dx) / pi / 2 + 0.5f;
                        const uint32_t sw = static_cast<uint32_t>(a.sky_w), sh = static_cast<uint32_t>(a.sky_h);
                        const float sx = phi * static_cast<float>(sw), sy = theta * static_cast<float>(sh);
                        // float -> unsigned is undefined for NaN / out of range in the reference; clamp into the image
                        uint32_t x1 = (sx >= 0.0f) ? (sx < 4294967040.0f ? static_cast<uint32_t>(sx) : 0xFFFFFFFFu) : 0u;
                        uint32_t y1 = (sy >= 0.0f) ? (sy < 4294967040.0f ? static_cast<uint32_t>(sy) : 0xFFFFFFFFu) : 0u;
                        x1 = min(x1, sw - 1u);
                        y1 = min(y1, sh - 1u);
                        const uint32_t x2 = (x1 + 1u) % sw, y2 = (y1 + 1u) % sh;
                        const uint8_t *t1 = a.sky + (static_cast<size_t>(y1) * sw + x1) * 3, *t2 = a.sky + (static_cast<size_t>(y1) * sw + x2) * 3;
                        const uint8_t *t3 = a.sky + (static_cast<size_t>(y2) * sw + x1) * 3, *t4 = a.sky + (static_cast<size_t>(y2) * sw + x2) * 3;
                        const float ax = 1 - sx + static_cast<float>(x1), ay = 1 - sy + static_cast<float>(y1);
                        float c[3];
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {   // r,g,b = bytes 2,1,0
                            const float c1 = static_cast<float>(t1[2 - ch]), c2 = static_cast<float>(t2[2 - ch]);
                            const float c3 = static_cast<float>(t3[2 - ch]), c4 = static_cast<float>(t4[2 - ch]);
                            const float c12 = c1 * (1.0f - ax) + c2 * ax;   // glm::mix(x, y, a) = x*(1-a) + y*a
                            const float c34 = c3 * (1.0f - ax) + c4 * ax;
                            c[ch] = (c12 * (1.0f - ay) + c34 * ay) / 256.f;
                        }
                        if constexpr (DIRECT) {
                            Lr[k] += c[0]; Lg[k] += c[1]; Lb[k] += c[2];
                        } else
                        contribute(k, c[0], c[1], c[2]);
                        contributed = true;
                    }
                    depth[k] = mrr;   // MakeInvalid
                } else {
                    const ExactRec *__restrict__ rec = hit_rec[k];
                    const float4 pl = reinterpret_cast<const float4 *>(rec)[0];
                    const int mi = rec->material;
                    const float px = q[k].ox + q[k].dx * best[k], py = q[k].oy + q[k].dy * best[k], pz = q[k].oz + q[k].dz * best[k];
                    float4 m0v, m1v;   // kd, chance0; ks, chance1
                    int4 m2v;          // n_lobes, kind0, kind1
                    bool mat_cached = false;
                    if constexpr (decltype(lds)::kMatCache > 0) mat_cached = a.n_mats <= decltype(lds)::kMatCache;
                    if (mat_cached) {
                        if constexpr (decltype(lds)::kMatCache > 0) {
                            m0v = lds.mat.v[3 * mi]; m1v = lds.mat.v[3 * mi + 1];
                            const float4 t = lds.mat.v[3 * mi + 2];
                            m2v = make_int4(__float_as_int(t.x), __float_as_int(t.y), __float_as_int(t.z), __float_as_int(t.w));
                        }
                    } else {
                        m0v = reinterpret_cast<const float4 *>(a.mats + mi)[0];
                        m1v = reinterpret_cast<const float4 *>(a.mats + mi)[1];
                        m2v = reinterpret_cast<const int4 *>(a.mats + mi)[2];
                    }
                    // On a path's last segment the random words only matter where they choose between an emissive lobe and
                    // another one (see below: nothing else of that segment survives it).
                    uint32_t w0 = 0, w1 = 0, w2 = 0, w3;
                    if (depth[k] + 1 < mrr || (m2v.x >= 2 && (m2v.y == 0 || m2v.z == 0)))
                        philox4x32_10(rng_pixel(k), static_cast<uint32_t>(pass_of(k)), static_cast<uint32_t>(depth[k]), 0u, a.seed, kPhiloxKey1,
                                      w0, w1, w2, w3);
                    int kind;
                    if (m2v.x == 0) {
                        kind = -1;
                    } else if (m2v.x == 1) {
                        kind = m2v.y;
                    } else {
                        // `while (sample > 0) { ++i; sample -= chance_[i]; }` with sample in (0,1); past the last lobe
                        // the reference reads out of bounds, here the last lobe is kept.
                        const float sample = unit_float(w0);
                        kind = (sample - m0v.w > 0) ? m2v.z : m2v.y;
                    }
                    // GLASS: a material the handle's table marks is a dielectric and nothing else (kind 3; never emissive: the setter
                    // refuses that, so the Philox call above was made under the condition it is made under without the table)
                    [[maybe_unused]] const GlassRec *grec = nullptr;
                    [[maybe_unused]] float g_ior = 0.0f;
                    if constexpr (GLASS) {
                        grec = glass_view() + mi;
                        g_ior = grec->ior;
                        if (g_ior != 0.0f) kind = 3;
                    }
                    // TEX: the emissive and the diffuse lobe of a textured material take the throughput times the texel at the hit
                    // point (pt_hip.h: pt_texture; pt_texture.hpp spells barycentrics, wrap and filters); the glossy lobe and a
                    // dielectric do not.  On a path's last segment only the emissive lobe computes anything.  hit_rec may be a record
                    // of either table: `orig` is the triangle's index in the original order, which the coordinates are stored in.
                    // SMOOTH: the same texel step, with the barycentrics kept for the shading normal below -- one load of the triangle's
                    // record serves both.
                    [[maybe_unused]] float sb1 = 0.0f, sb2 = 0.0f;
                    if constexpr (SMOOTH) {
                        const bool scatters = kind > 0 && depth[k] + 1 < mrr;
                        const TextureView tv = texture_view();
                        const size_t ti = static_cast<size_t>(rec->orig);
                        TexRec tm = {0u, 0, 0, 0};
                        if (kind == 0 || (kind == 2 && scatters)) tm = tv.recs()[mi];
                        if (scatters || tm.w != 0) {
                            const TexBary t = tv.bary()[ti];   // (two 16-byte loads)
                            tex_barycentrics_record(t.a1[0], t.a1[1], t.a1[2], t.c1, t.a2[0], t.a2[1], t.a2[2], t.c2, px, py, pz, sb1, sb2);
                        }
                        if (tm.w != 0) {
                            const float *uv = tv.uv() + 6 * ti;
                            float tu, tvv, xr, xg, xb;
                            tex_interpolate(uv[0], uv[1], uv[2], uv[3], uv[4], uv[5], sb1, sb2, tu, tvv);
                            tex_lookup(tv.texels() + tm.first, tm.w, tm.h, tm.filter, tu, tvv, xr, xg, xb);
                            tr[k] *= xr; tg[k] *= xg; tb[k] *= xb;
                        }
                    } else
                    if constexpr (TEX) {
                        if (kind == 0 || (kind == 2 && depth[k] + 1 < mrr)) {
                            const TextureView tv = texture_view();
                            const TexRec tm = tv.recs()[mi];
                            if (tm.w != 0) {
                                float xr, xg, xb;
#ifdef PT_TEXTURE_VERTICES   // (the form that was measured against the record: DESIGN.md section 27)
                                const float4 r1 = reinterpret_cast<const float4 *>(rec)[1], r2 = reinterpret_cast<const float4 *>(rec)[2];
                                const float4 r3 = reinterpret_cast<const float4 *>(rec)[3];
                                tex_at_hit(tm, tv.texels(), tv.uv() + 6 * static_cast<size_t>(rec->orig), r1.x, r1.y, r1.z, r2.x, r2.y, r2.z,
                                           r3.x, r3.y, r3.z, px, py, pz, xr, xg, xb);
#else
                                const size_t ti = static_cast<size_t>(rec->orig);
                                tex_at_hit_record(tm, tv.texels(), tv.uv() + 6 * ti, tv.bary() + ti, px, py, pz, xr, xg, xb);
#endif
                                tr[k] *= xr; tg[k] *= xg; tb[k] *= xb;
                            }
                        }
                    }
                    if (kind < 0) {
                        depth[k] = mrr;
                    } else if (kind == 0) {   // emissive, material.h:68-79
                        if (!((q[k].dx * pl.x + q[k].dy * pl.y) + q[k].dz * pl.z > 0)) {
                            const float cr = tr[k] * m0v.x, cg = tg[k] * m0v.y, cb = tb[k] * m0v.z;
                            if constexpr (DIRECT) {   // (an emitter the diffuse step's shadow ray has sampled already adds nothing)
                                if (!lit[k]) {
                                    Lr[k] += cr; Lg[k] += cg; Lb[k] += cb;
                                    contributed = true;
                                }
                            } else {
                            contribute(k, cr, cg, cb);
                            contributed = true;
                            }
                        }
                        depth[k] = mrr;
                    } else {
                        // Both scattering lobes end in Ray::Reflect (ray.h:45-50): the lobe-specific part leaves the new direction
                        // (not yet normalised by Reflect) and the throughput factor, the common tail runs once per wave.
                        // A path's last segment (depth + 1 == mrr: all live lanes of a wave reach it together) can only contribute
                        // through the emissive lobe above: the ray a scattering lobe would produce is never traced
                        // (Ray::IsValid, ray.h:52-54), so it is not computed either.
                        if (depth[k] + 1 < mrr) {
                        float rx, ry, rz, fr, fg, fb;
                        [[maybe_unused]] float oe = eps;   // GLASS: +-eps, the side of the surface the next ray starts on
                        bool dielectric = false;
                        if constexpr (GLASS) dielectric = kind == 3;
                        if constexpr (SMOOTH) {
                            // The step with the shading normal Ns (pt_hip.h: shading normals), and the same step with the stored
                            // normal N: the first is kept unless its direction leaves on the other side of the stored plane from
                            // the origin's offset.  Both are computed and one is selected; the diffuse lobe's hemisphere sample,
                            // which no normal enters, is drawn once.  The same w1 .. w3 serve both.
                            const SmoothCorner *__restrict__ sc = smooth_view() + 3 * static_cast<size_t>(rec->orig);
                            const SmoothCorner c0 = sc[0], c1 = sc[1], c2 = sc[2];   // (three 16-byte loads)
                            float sx, sy, sz;
                            smooth_normal(c0.x, c0.y, c0.z, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z, sb1, sb2, pl.x, pl.y, pl.z,
                                          [](float &vx, float &vy, float &vz) { normalize3(vx, vy, vz); }, sx, sy, sz);
                            // DIRECT: the direct term of a diffuse step (pt_hip.h: direct lighting; pt_direct.hpp spells it), from the
                            // words of counter (pixel, pass, depth, 3): the light, the point on it, the shadow ray from the next origin
                            // p + N eps and the term, which waits for the ray's verdict.
                            if constexpr (DIRECT) {
                                lit[k] = !dielectric && kind != 1;
                                if (lit[k]) {
                                    uint32_t l0, l1, l2, l3;
                                    philox4x32_10(rng_pixel(k), static_cast<uint32_t>(pass_of(k)), static_cast<uint32_t>(depth[k]), kDirectStream, a.seed, kPhiloxKey1,
                                                  l0, l1, l2, l3);
                                    // ENVDIRECT: the counter's spare word chooses between the emitters (the term above over 1 - share) and the
                                    // environment: a direction drawn from the alias table by the words of counter (pixel, pass, depth, 4), whose
                                    // term counts if the shadow ray misses -- the slot's "light" is the miss value of the search.
                                    [[maybe_unused]] bool to_sky = false;
                                    [[maybe_unused]] float share = 1.0f;
                                    if constexpr (ENVDIRECT) {
                                        share = envdirect_view().share();
                                        to_sky = unit_float(l3) < share;
                                    }
                                    if (!to_sky) {
                                    const DirectView dv = direct_view();
                                    const LightRec *__restrict__ lr = dv.lights() + direct_pick(dv.lights(), dv.n(), unit_float(l0));
                                    const LightRec lrec = *lr;   // (five 16-byte loads)
                                    float ppx, ppy, ppz;
                                    pending[k] = direct_term(lrec, dv.area(), unit_float(l1), unit_float(l2), px + pl.x * eps, py + pl.y * eps, pz + pl.z * eps,
                                                             pl.x, pl.y, pl.z, sx, sy, sz, tr[k], tg[k], tb[k], m0v.x, m0v.y, m0v.z,
                                                             [](float &vx, float &vy, float &vz) { normalize3(vx, vy, vz); }, ppx, ppy, ppz, sdx[k], sdy[k], sdz[k],
                                                             scr[k], scg[k], scb[k]);
                                    slight[k] = lrec.orig;
                                    if constexpr (ENVDIRECT) {
                                        const float rest = 1.0f - share;
                                        scr[k] = scr[k] / rest; scg[k] = scg[k] / rest; scb[k] = scb[k] / rest;
                                    }
                                    }
                                    if constexpr (ENVDIRECT) {
                                        if (to_sky) {
                                            const EnvDirectView sv = envdirect_view();
                                            uint32_t e0, e1, e2, e3;
                                            philox4x32_10(rng_pixel(k), static_cast<uint32_t>(pass_of(k)), static_cast<uint32_t>(depth[k]), kEnvDirectStream, a.seed,
                                                          kPhiloxKey1, e0, e1, e2, e3);
                                            float pdf_w;
                                            [[maybe_unused]] int32_t cell;
                                            envdirect_sample(sv.table(), sv.cells(), e0, unit_float(e1), unit_float(e2), unit_float(e3),
                                                             [](float &vx, float &vy, float &vz) { normalize3(vx, vy, vz); },
                                                             [](float v) { return sqrt_rn_normal(v); }, cell, sdx[k], sdy[k], sdz[k], pdf_w);
                                            const EnvironmentView ev = environment_view();
                                            float er, eg, eb;
                                            env_lookup(ev.map(), ev.n(), sdx[k], sdy[k], sdz[k], er, eg, eb);   // (four 16-byte loads)
                                            pending[k] = envdirect_term(sdx[k], sdy[k], sdz[k], pdf_w, share, er, eg, eb, pl.x, pl.y, pl.z, sx, sy, sz, tr[k], tg[k],
                                                                        tb[k], m0v.x, m0v.y, m0v.z, scr[k], scg[k], scb[k]);
                                            slight[k] = -1;
                                        }
                                    }
                                }
                            }
                            float hx = 0.0f, hy = 0.0f, hz = 0.0f;
                            if (!dielectric && kind != 1) {   // diffuse, material.h:90-100: the sample
                                const float xi1 = unit_float(w1), xi2 = unit_float(w2);
                                const float ang = 2 * 3.141593f * xi2;
                                float sn, cs;
                                portable_sincos(ang, sn, cs);
                                const float sq = sqrt_rn_normal(xi1);
                                hx = sq * cs; hy = sq * sn; hz = sqrt_rn_normal(1 - xi1);
                                normalize3(hx, hy, hz);
                            }
                            // ROUGH: the material's alpha, 0 = the mirror (RenderArgs::rough_alpha), read where the glossy lobe was chosen
                            [[maybe_unused]] float r_alpha = 0.0f;
                            if constexpr (ROUGH) {
                                if (kind == 1) r_alpha = rough_view()[mi];
                            }
                            auto step = [&](const float nx, const float ny, const float nz, float &ux, float &uy, float &uz, float &ur, float &ug,
                                            float &ub, float &uo) {
                                uo = eps;
                                if (dielectric) {
                                    const float c = (nx * q[k].dx + ny * q[k].dy) + nz * q[k].dz;
                                    const bool entering = c < 0;
                                    const float eta = entering ? grec->inv_ior : g_ior;
                                    float ci = entering ? -c : c;
                                    ci = ci < 1 ? ci : 1;
                                    const float s2 = (eta * eta) * (1 - ci * ci);
                                    const float ec = eta * ci;
                                    float fresnel = 1.0f, ct = 0.0f;
                                    if (s2 < 1) {
                                        ct = sqrt_rn_normal(1 - s2);
                                        const float et = eta * ct;
                                        const float rs = (ec - ct) / (ec + ct), rp = (ci - et) / (ci + et);
                                        fresnel = 0.5f * (rs * rs + rp * rp);
                                    }
                                    float dm, nk;
                                    if (unit_float(w3) < fresnel) {
                                        dm = 1.0f; nk = 2 * ci;
                                        uo = entering ? eps : -eps;
                                        ur = ug = ub = 1.0f;
                                    } else {
                                        dm = eta; nk = ec - ct;
                                        uo = entering ? -eps : eps;
                                        ur = grec->tint[0]; ug = grec->tint[1]; ub = grec->tint[2];
                                    }
                                    if (!entering) nk = -nk;
                                    ux = q[k].dx * dm + nx * nk; uy = q[k].dy * dm + ny * nk; uz = q[k].dz * dm + nz * nk;
                                } else if (kind == 1) {
                                    if constexpr (ROUGH) {   // the GGX lobe of a listed material (pt_hip.h: rough specular; pt_rough.hpp spells it)
                                        if (r_alpha != 0.0f) {
                                            float g1, mhx, mhy, mhz;
                                            rough_step(nx, ny, nz, q[k].dx, q[k].dy, q[k].dz, r_alpha, unit_float(w1), unit_float(w2),
                                                       [](float ang, float &sn, float &cs) { portable_sincos(ang, sn, cs); },
                                                       [](float &vx, float &vy, float &vz) { normalize3(vx, vy, vz); }, ux, uy, uz, g1, mhx, mhy, mhz);
                                            ur = m1v.x * g1; ug = m1v.y * g1; ub = m1v.z * g1;
                                            return;   // (the direction is normalised already)
                                        }
                                    }
                                    const float dn = (nx * q[k].dx + ny * q[k].dy) + nz * q[k].dz;
                                    ux = q[k].dx - nx * dn * 2.0f; uy = q[k].dy - ny * dn * 2.0f; uz = q[k].dz - nz * dn * 2.0f;
                                    ur = m1v.x; ug = m1v.y; ub = m1v.z;
                                } else {
                                    ux = hx; uy = hy; uz = hz;
                                    if ((nx * ux + ny * uy) + nz * uz < 0) { ux *= -1; uy *= -1; uz *= -1; }
                                    float dt = (nx * ux + ny * uy) + nz * uz;
                                    dt = dt > 0.0f ? dt : 0.0f;
                                    ur = m0v.x * dt; ug = m0v.y * dt; ub = m0v.z * dt;
                                }
                                normalize3(ux, uy, uz);
                            };
                            float ax, ay, az, ar, ag, ab, ao;
                            step(sx, sy, sz, ax, ay, az, ar, ag, ab, ao);
                            step(pl.x, pl.y, pl.z, rx, ry, rz, fr, fg, fb, oe);
                            if (smooth_keeps(ax, ay, az, pl.x, pl.y, pl.z, ao)) {
                                rx = ax; ry = ay; rz = az; fr = ar; fg = ag; fb = ab; oe = ao;
                            }
                        } else {
                        if (dielectric) {   // smooth dielectric (pt_hip.h: pt_dielectric states this operation by operation)
                            if constexpr (GLASS) {
                                const float c = (pl.x * q[k].dx + pl.y * q[k].dy) + pl.z * q[k].dz;
                                const bool entering = c < 0;   // n = N entering, -N leaving: below, n's sign rides on the factors of N
                                const float eta = entering ? grec->inv_ior : g_ior;
                                float ci = entering ? -c : c;
                                ci = ci < 1 ? ci : 1;
                                const float s2 = (eta * eta) * (1 - ci * ci);
                                const float ec = eta * ci;
                                float fresnel = 1.0f, ct = 0.0f;
                                if (s2 < 1) {   // (else total internal reflection; 1 - s2 is in [2^-24, 1])
                                    ct = sqrt_rn_normal(1 - s2);
                                    const float et = eta * ct;
                                    const float rs = (ec - ct) / (ec + ct), rp = (ci - et) / (ci + et);
                                    fresnel = 0.5f * (rs * rs + rp * rp);
                                }
                                float dm, nk;   // the new direction d * dm + n * nk
                                if (unit_float(w3) < fresnel) {   // reflected: from the side the ray came from, throughput unchanged
                                    dm = 1.0f; nk = 2 * ci;
                                    oe = entering ? eps : -eps;
                                    fr = fg = fb = 1.0f;
                                } else {   // transmitted: the reference's Refract (main.cpp:35-47) with eta; from the far side, tinted
                                    dm = eta; nk = ec - ct;
                                    oe = entering ? -eps : eps;
                                    fr = grec->tint[0]; fg = grec->tint[1]; fb = grec->tint[2];
                                }
                                if (!entering) nk = -nk;
                                rx = q[k].dx * dm + pl.x * nk; ry = q[k].dy * dm + pl.y * nk; rz = q[k].dz * dm + pl.z * nk;
                            } else {
                                __builtin_unreachable();
                            }
                        } else
                        if (kind == 1) {   // glossy, material.h:83-85
                            const float dn = (pl.x * q[k].dx + pl.y * q[k].dy) + pl.z * q[k].dz;
                            rx = q[k].dx - pl.x * dn * 2.0f; ry = q[k].dy - pl.y * dn * 2.0f; rz = q[k].dz - pl.z * dn * 2.0f;
                            fr = m1v.x; fg = m1v.y; fb = m1v.z;
                        } else {   // diffuse, material.h:90-100
                            const float xi1 = unit_float(w1), xi2 = unit_float(w2);
                            const float ang = 2 * 3.141593f * xi2;
                            float sn, cs;
                            portable_sincos(ang, sn, cs);
                            const float sq = sqrt_rn_normal(xi1);   // xi1 and 1 - xi1 are multiples of 2^-24 in [2^-24, 1)
                            rx = sq * cs; ry = sq * sn; rz = sqrt_rn_normal(1 - xi1);
                            normalize3(rx, ry, rz);
                            if ((pl.x * rx + pl.y * ry) + pl.z * rz < 0) { rx *= -1; ry *= -1; rz *= -1; }
                            float dt = (pl.x * rx + pl.y * ry) + pl.z * rz;
                            dt = dt > 0.0f ? dt : 0.0f;
                            fr = m0v.x * dt; fg = m0v.y * dt; fb = m0v.z * dt;
                        }
                        normalize3(rx, ry, rz);   // Ray::Reflect normalises (again), ray.h:47
                        }
                        if constexpr (GLASS) {   // p + n eps or p - n eps: the sign is exact, N * (-eps) = -(N * eps)
                            q[k].ox = px + pl.x * oe; q[k].oy = py + pl.y * oe; q[k].oz = pz + pl.z * oe;
                        } else {
                        q[k].ox = px + pl.x * eps; q[k].oy = py + pl.y * eps; q[k].oz = pz + pl.z * eps;
                        }
                        q[k].dx = rx; q[k].dy = ry; q[k].dz = rz;
                        tr[k] *= fr; tg[k] *= fg; tb[k] *= fb;
                        // ROULETTE: the step, whatever the lobe was (pt_hip.h: Russian roulette; pt_roulette.hpp spells it), under the
                        // word of counter (pixel, pass, depth, 5), drawn only where it decides.  A path it ends has throughput zero: it is
                        // over by path_over and hands in its L below, or with its pending shadow ray's verdict.
                        if constexpr (ROULETTE) {
                            const RouletteView rv = roulette_view();
                            if (depth[k] + 1 >= rv.start()) {
                                roulette_step(rv.floor(), [&] {
                                    uint32_t r0, r1, r2, r3;
                                    philox4x32_10(rng_pixel(k), static_cast<uint32_t>(pass_of(k)), static_cast<uint32_t>(depth[k]), kRouletteStream, a.seed, kPhiloxKey1,
                                                  r0, r1, r2, r3);
                                    return unit_float(r0);
                                }, tr[k], tg[k], tb[k]);
                            }
                        }
                        }
                        ++depth[k];
                    }
                }
                if constexpr (DIRECT) {
                    if (!pending[k] && path_over(k)) contribute(k, Lr[k], Lg[k], Lb[k]);
                }
            }
            if constexpr (STATS) n_contrib += __builtin_popcountll(__ballot(contributed));
            }
            PT_STAMP(wst, 7);   // shading
        }
    }

    // Write-back.  A tile whose rows are 16-byte aligned in the caller's planes is written with 16-byte stores (a row of
    // the tile is kTW*12 contiguous bytes of sum / sum2 and kTW*4 of count): dword stores at a 12-byte stride made the
    // memory side see about twice the bytes.  Column c of the tile's row r lives in LDS slot r*kTileW + c%kTileW + 64*(c/kTileW).
    if constexpr (kAccInLds) {
    const int tile_x = static_cast<int>(tile % a.blocks_x) * kTW, tile_y = a.row_begin + static_cast<int>(tile / a.blocks_x) * kTileH * a.row_stride;
    const int wb_row0 = a.row_begin + static_cast<int>(tile / a.blocks_x) * kTileH * (a.row_stride - 1);
    const bool whole = a.vec_ok && tile_x + kTW <= a.width && tile_y + kTileH <= a.row_end;   // wave-uniform
    wave_sync();
    auto slot_of = [](int row, int col) { return row * kTileW + (col % kTileW) + 64 * (col / kTileW); };
    if (whole) {
        constexpr int kRowVec = kTW * 3 / 4;          // float4 per tile row of a colour plane
#pragma unroll
        for (int v0 = 0; v0 < kRowVec * kTileH; v0 += kBlock) {
            const int vv = v0 + lane;
            if (vv < kRowVec * kTileH) {
                const int row = vv / kRowVec, v = vv % kRowVec;
                const size_t base = (static_cast<size_t>(tile_y - wb_row0 + row) * a.width + tile_x) * 3 + 4 * v;
                float4 o1, o2;
                float *p1 = &o1.x, *p2 = &o2.x;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * v + j;                   // element of the row: pixel e/3, channel e%3
                    p1[j] = lds.acc.v[e % 3][slot_of(row, e / 3)];
                    p2[j] = lds.acc.v[3 + e % 3][slot_of(row, e / 3)];
                }
                *reinterpret_cast<float4 *>(a.sum + base) = o1;
                *reinterpret_cast<float4 *>(a.sum2 + base) = o2;
            }
        }
        constexpr int kCntVec = kTW / 4;              // int4 per tile row of the count plane
        if (lane < kCntVec * kTileH) {
            const int row = lane / kCntVec, v = lane % kCntVec;
            const size_t base = static_cast<size_t>(tile_y - wb_row0 + row) * a.width + tile_x + 4 * v;
            int4 oc;
            oc.x = __float_as_int(lds.acc.v[6][slot_of(row, 4 * v)]);
            oc.y = __float_as_int(lds.acc.v[6][slot_of(row, 4 * v + 1)]);
            oc.z = __float_as_int(lds.acc.v[6][slot_of(row, 4 * v + 2)]);
            oc.w = __float_as_int(lds.acc.v[6][slot_of(row, 4 * v + 3)]);
            *reinterpret_cast<int4 *>(a.count + base) = oc;
        }
    } else {
        // recomputed from the tile's corner and the lane number: p, x or y kept across the kernel would be spilled
        const uint32_t le = opaque(static_cast<uint32_t>(lane));
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int xe = tile_x + static_cast<int>(le % kTileW) + kTileW * k, ye = tile_y + static_cast<int>(le / kTileW);
            if (xe < a.width && ye < a.row_end) {
                const size_t pe = static_cast<size_t>(ye - wb_row0) * a.width + xe;
                const int id = lane + 64 * k;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    a.sum[3 * pe + c] = lds.acc.v[c][id];
                    a.sum2[3 * pe + c] = lds.acc.v[3 + c][id];
                }
                a.count[pe] = __float_as_int(lds.acc.v[6][id]);
            }
        }
    }
    }
    if (chunk + 1 < a.n_chunks) {   // publish the tile's accumulators to the wave that takes its next chunk
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the fence's own wait can be dropped by the compiler (guide, G16)
        if (lane == 0) __hip_atomic_store(&a.sched[1 + tile], chunk + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#ifdef PT_ADAPT_COUNT
    if (a.stats && lane == 0) {
        atomicAdd(&a.stats[0], static_cast<unsigned long long>(c_rays));
        atomicAdd(&a.stats[6], static_cast<unsigned long long>(c_one));
        atomicAdd(&a.stats[7], static_cast<unsigned long long>(c_two));
        atomicAdd(&a.stats[1], static_cast<unsigned long long>(c_seg1));
        atomicAdd(&a.stats[5], static_cast<unsigned long long>(c_seg2));
    }
#endif
#ifdef PT_VERIFY_SHIPPED
    if (a.stats && lane == 0) {
        atomicAdd(&a.stats[9], static_cast<unsigned long long>(v_checked));
        if (v_bad) atomicAdd(&a.stats[10], static_cast<unsigned long long>(v_bad));
        if (v_compacted) atomicAdd(&a.stats[8], static_cast<unsigned long long>(v_compacted));   // (pt_render_stats::partial_commit_rounds)
    }
#endif
    if constexpr (STATS) if (a.stats && lane == 0) {
        atomicAdd(&a.stats[0], static_cast<unsigned long long>(n_traced));
        atomicAdd(&a.stats[1], static_cast<unsigned long long>(n_segments));
        atomicAdd(&a.stats[2], static_cast<unsigned long long>(n_contrib));
        atomicAdd(&a.stats[3], static_cast<unsigned long long>(wst.n_exact));
        atomicAdd(&a.stats[4], static_cast<unsigned long long>(n_miss));
        atomicAdd(&a.stats[5], static_cast<unsigned long long>(wst.w_segments));
        atomicAdd(&a.stats[6], static_cast<unsigned long long>(wst.w_node_rounds));
        atomicAdd(&a.stats[7], static_cast<unsigned long long>(wst.w_exact_iters));
        if (wst.w_partial) atomicAdd(&a.stats[8], static_cast<unsigned long long>(wst.w_partial));
#ifdef PT_VERIFY_BRUTE
        atomicAdd(&a.stats[9], static_cast<unsigned long long>(wst.v_checked));
        if (wst.v_bad) atomicAdd(&a.stats[10], static_cast<unsigned long long>(wst.v_bad));
#endif
#ifdef PT_PHASE_TIMERS
        for (int k = 0; k < 8; ++k) atomicAdd(&a.stats[16 + k], wst.phase[k]);
#endif
    }
