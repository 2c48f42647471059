// The walk of ONE sphere-tree cluster (kind 0) inside pt::closest_hit (pt_kernels.hip), included where a cluster is walked: in
// the generic loop over clusters, and after the large class of the room instantiation (pt_scene.hpp: CullTables::room).  Shared
// TEXTUALLY, like pt_integrator_body.inc and for the same reason: a function around it moves the registers of kernels that sit at
// their budgets.  It sees closest_hit's locals and, of the cluster: cl (its index), cp (its descriptor), first_tri, n_tri, off, and
// pc[R] (the rays that passed its bounding sphere; some ray of the wave has).
            // ---- small triangles: an 8-ary tree of bounding spheres, walked with a wave-wide LIFO of (ray, node) items
            const uint32_t n_levels = ((ConstU)cp)[8];
            const uint32_t top = n_levels - 1;
            if (lane < static_cast<int>(n_levels)) {
                lds.level_off[lane] = lane == 0 ? 0u : a.clusters[cl].level_off[lane - 1];
                lds.level_cnt[lane] = (n_tri + (1u << (3 * lane)) - 1u) >> (3 * lane);
            }
            wave_sync();
            uint32_t n_nodes = 0;   // wave-uniform fill level of lds.nodes
            uint32_t tmask[R];      // per ray: top-level nodes still to be pushed
#pragma unroll
            for (int k = 0; k < R; ++k) tmask[k] = 0;
            auto any_tmask = [&]() {
                uint32_t x = tmask[0];
#pragma unroll
                for (int k = 1; k < R; ++k) x |= tmask[k];
                return __any(x != 0);
            };
            // pushes one top-level node per ray and step until nothing is left or the stack is full (the rest follows once it has drained)
            auto push_top = [&](uint32_t top) {
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    if (!PT_SLOT_ON(k)) continue;
                    while (__any(tmask[k] != 0)) {   // at most 8 x 64 R items > capacity: drained in the expansion loop before overflow
                        const bool has = tmask[k] != 0;
                        const unsigned long long ball = __ballot(has);
                        if (n_nodes + __builtin_popcountll(ball) > kNodeStack) return;
                        if (has) {
                            const uint32_t j = __builtin_ctz(tmask[k]);
                            tmask[k] &= tmask[k] - 1;
                            lds.nodes[n_nodes + lanes_below(ball)] = (static_cast<uint32_t>(lane + 64 * k) << Lds::kNodeSrcShift) | (top << Lds::kNodeLevShift) | j;
                        }
                        n_nodes += __builtin_popcountll(ball);
                    }
                }
            };
            // (a') Few rays near a small tree: skip its top level.  The (at most 16) lanes that passed the cluster sphere are
            // compacted, each gets 4 to 64 lanes, and together they test ALL nodes of the level below the top (at most 8
            // per lane) in one round -- instead of the wave-uniform top-level tests plus a round that is mostly empty.
            bool rooted = false;
            if (top >= 1) {
                unsigned long long pcb[R];
                uint32_t rcnt = 0;
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    pcb[k] = 0;
                    if (!PT_SLOT_ON(k)) continue;
                    pcb[k] = __ballot(pc[k]);
                    rcnt += __builtin_popcountll(pcb[k]);
                }
                const uint32_t clev = top - 1;
                const uint32_t nchild = (n_tri + (1u << (3 * clev)) - 1u) >> (3 * clev);
                const uint32_t sh = rcnt <= 1u ? 6u : rcnt <= 2u ? 5u : rcnt <= 4u ? 4u : rcnt <= 8u ? 3u : rcnt <= 16u ? 2u : 0u;   // lanes per ray
                const uint32_t per = (nchild + (1u << sh) - 1u) >> sh;                                                           // nodes per lane
                if (rcnt <= 16u && per <= 8u) {
                    ++st.w_node_rounds;
                    {
                        uint32_t at = 0;   // the stack is empty here: the compacted ray ids go to its bottom
#pragma unroll
                        for (int k = 0; k < R; ++k) {
                            if (!PT_SLOT_ON(k)) continue;
                            if (pc[k]) lds.nodes[at + lanes_below(pcb[k])] = static_cast<uint32_t>(lane + 64 * k);
                            at += __builtin_popcountll(pcb[k]);
                        }
                    }
                    wave_sync();
                    // Lane `sub` of a ray's group takes nodes sub, sub + group, sub + 2 group, ...: one load instruction then
                    // reads consecutive records across the group (whole cache lines) instead of one line per lane.  When
                    // the nodes are the triangles themselves the slices stay contiguous (pairs are published as bit masks).
                    const uint32_t item = static_cast<uint32_t>(lane) >> sh, sub = static_cast<uint32_t>(lane) & ((1u << sh) - 1u);
                    const uint32_t c0 = clev == 0 ? sub * per : sub, cstep = clev == 0 ? 1u : (1u << sh);
                    uint32_t m = 0, src = 0;
                    if (item < rcnt) {
                        src = lds.nodes[item];
                        Ray r;
                        r.ox = lds.ray[0][src]; r.oy = lds.ray[1][src]; r.oz = lds.ray[2][src];
                        r.dx = lds.ray[3][src]; r.dy = lds.ray[4][src]; r.dz = lds.ray[5][src];
                        const float4 *cs = reinterpret_cast<const float4 *>(a.spheres) + off + lds.level_off[clev] + c0;
                        auto test = [&](auto per_c) {
                            constexpr uint32_t kPer = decltype(per_c)::value;
#pragma unroll
                            for (uint32_t i = 0; i < kPer; ++i) {   // no bounds test per sphere: the table is padded (pt_scene.cpp) ...
                                const float4 sp = cs[i * cstep];
                                m |= sphere_keep(sp.x, sp.y, sp.z, sp.w, r) ? (1u << i) : 0u;
                            }
                            // ... and the results beyond the level's last node are dropped here
                            const uint32_t left = nchild > c0 ? nchild - c0 : 0u;
                            const uint32_t n_ok = min((left + cstep - 1u) >> (clev == 0 ? 0u : sh), kPer);
                            m &= (1u << n_ok) - 1u;
                        };
                        if (per == 1u) test(std::integral_constant<uint32_t, 1>());
                        else if (per == 2u) test(std::integral_constant<uint32_t, 2>());
                        else if (per <= 4u) test(std::integral_constant<uint32_t, 4>());
                        else test(std::integral_constant<uint32_t, 8>());
                    }
                    wave_sync();   // every lane has read its ray's lane number before the stack is written
                    const uint32_t mc = __builtin_popcount(m);
                    const uint32_t incl = wave_scan_inclusive(mc), tot = wave_last(incl);
                    if (clev == 0) {   // the level below the top is the triangles themselves
                        if (n_pairs + tot > kPairQueue) drain_pairs(0);
                        if (tot <= kPairQueue) {
                            emit_pairs(m, first_tri + c0, src, incl - mc, tot);
                            rooted = true;
                        }
                    } else if (tot <= kNodeStack) {
                        // bit j = node c0 + j * cstep of level clev (cstep = 1 << sh here)
                        emit_bits(lds.nodes, n_nodes + incl - mc, m, (src << Lds::kNodeSrcShift) | (clev << Lds::kNodeLevShift) | c0, sh);
                        n_nodes += tot;
                        wave_sync();
                        rooted = true;
                    }
                    // (more survivors than the queue holds: fall through to the general path below)
                }
            }
            if (!rooted) {
            // (a) wave-uniform: every lane against the (at most 8) top-level spheres, records in SGPRs
            const uint32_t top_off = top == 0 ? 0u : ((ConstU)cp)[8 + top];
            const uint32_t top_cnt = (n_tri + (1u << (3 * top)) - 1u) >> (3 * top);
            const ConstF tp = spheres + 4 * (static_cast<size_t>(off) + top_off);
            for (uint32_t j = 0; j < top_cnt; ++j) {
                const float sx = tp[4 * j], sy = tp[4 * j + 1], sz = tp[4 * j + 2], sr = tp[4 * j + 3];
#pragma unroll
                for (int k = 0; k < R; ++k)
                    if (PT_SLOT_ON(k)) tmask[k] |= sphere_keep(sx, sy, sz, sr, q[k]) ? (1u << j) : 0u;
            }
#pragma unroll
            for (int k = 0; k < R; ++k) tmask[k] = pc[k] ? tmask[k] : 0u;
            PT_STAMP(st, 1);   // cluster + top-level sphere tests
            if (top == 0) {
                add_pending(tmask, first_tri, n_tri);   // the run has at most 8 triangles
#pragma unroll
                for (int k = 0; k < R; ++k) tmask[k] = 0;
            } else {
                push_top(top);
                wave_sync();
            }
            }
            // (b) lane-balanced expansion: lane l takes the l-th item from the top of the stack, tests the node's 8
            // children against that item's ray and pushes the survivors (tree nodes back on the stack, triangles as
            // (ray, triangle) pairs).  A round is committed only for the top k lanes whose children fit.
            while (n_nodes > 0 || any_tmask()) {
                if (n_nodes == 0) {   // top-level items that did not fit earlier
                    push_top(top);
                    wave_sync();
                }
                ++st.w_node_rounds;
                const uint32_t cnt = min(64u, n_nodes);
                // A round with few items spreads each item's 8 children over 2, 4 or 8 lanes (wave-uniform choice).
                uint32_t shift = cnt <= 8u ? 3u : cnt <= 16u ? 2u : cnt <= 32u ? 1u : 0u;
                uint32_t m8, src, level, child0, keep, packed, incl, tot;
                bool leaf;
                for (;;) {
                    m8 = 0; src = 0; level = 1; child0 = 0;
                    const uint32_t item = static_cast<uint32_t>(lane) >> shift, sub = static_cast<uint32_t>(lane) & ((1u << shift) - 1u);
                    if (item < cnt) {
                        const uint32_t e = lds.nodes[n_nodes - 1 - item];
                        src = e >> Lds::kNodeSrcShift;
                        level = (e >> Lds::kNodeLevShift) & 7u;
                        child0 = (e & ((1u << Lds::kNodeLevShift) - 1u)) * kFan;   // index of the first child within level-1
                        Ray r;
                        r.ox = lds.ray[0][src]; r.oy = lds.ray[1][src]; r.oz = lds.ray[2][src];
                        r.dx = lds.ray[3][src]; r.dy = lds.ray[4][src]; r.dz = lds.ray[5][src];
                        const float4 *cs = reinterpret_cast<const float4 *>(a.spheres) + off + lds.level_off[level - 1] + child0;
                        auto test = [&](auto per_c) {
                            constexpr int per = decltype(per_c)::value;
#pragma unroll
                            for (int i = 0; i < per; ++i) {
                                const uint32_t c = sub + (static_cast<uint32_t>(i) << shift);   // interleaved: the item's lanes read consecutive records
                                const float4 sp = cs[c];
                                m8 |= sphere_keep(sp.x, sp.y, sp.z, sp.w, r) ? (1u << c) : 0u;
                            }
                        };
                        if (shift == 0u) test(std::integral_constant<int, 8>());
                        else if (shift == 1u) test(std::integral_constant<int, 4>());
                        else if (shift == 2u) test(std::integral_constant<int, 2>());
                        else test(std::integral_constant<int, 1>());
                        const uint32_t real = lds.level_cnt[level - 1];   // padding spheres are never children
                        const uint32_t left = real > child0 ? real - child0 : 0u;
                        m8 &= left >= 8u ? 0xFFu : ((1u << left) - 1u);
                    }
                    leaf = level == 1;   // children are triangles
                    uint32_t kids = __builtin_popcount(m8);
                    keep = cnt;          // items [0, keep) (from the top of the stack) are committed this round
                    // one prefix sum for both queues: tree nodes count in the low half of the word, triangles in the high half
                    packed = leaf ? kids << 16 : kids;
                    incl = wave_scan_inclusive(packed);
                    tot = wave_last(incl);
                    if (n_pairs + (tot >> 16) > kPairQueue) drain_pairs(0);
                    if (n_pairs + (tot >> 16) <= kPairQueue && n_nodes - cnt + (tot & 0xFFFFu) <= kNodeStack) break;
                    if (shift != 0u) { shift = 0u; continue; }   // rare: redo the round one lane per item
                    // Rare: not everything fits.  Commit the longest prefix of lanes (= the top of the stack) whose
                    // children do; the other items stay where they are.  If not even the top item fits it is committed
                    // anyway: its (at most 8) children replace it, and since they are one level deeper the stack can
                    // outgrow kNodeStack by at most 7 per level, which is what the 64 slots of slack are for.
                    const bool fits = static_cast<uint32_t>(lane) < cnt && n_pairs + (incl >> 16) <= kPairQueue &&
                                      (n_nodes - (lane + 1)) + (incl & 0xFFFFu) <= kNodeStack;
                    const unsigned long long fb = __ballot(fits);
                    keep = (fb == ~0ull) ? 64u : static_cast<uint32_t>(__builtin_ctzll(~fb));
                    if (keep == 0) keep = 1;
                    ++st.w_partial;
                    if (static_cast<uint32_t>(lane) >= keep) m8 = 0;
                    kids = __builtin_popcount(m8);
                    packed = leaf ? kids << 16 : kids;
                    incl = wave_scan_inclusive(packed);
                    tot = wave_last(incl);
                    break;
                }
                n_nodes -= keep;
                wave_sync();
                // node children back on the stack, triangle children into the pair queue: one pass
                {
                    const uint32_t excl = incl - packed;
                    emit_bits(leaf ? lds.pairs : lds.nodes, leaf ? n_pairs + (excl >> 16) : n_nodes + (excl & 0xFFFFu), m8,
                              leaf ? ((first_tri + child0) | (src << 24)) : ((src << Lds::kNodeSrcShift) | ((level - 1) << Lds::kNodeLevShift) | child0));
                    n_nodes += tot & 0xFFFFu;
                    n_pairs += tot >> 16;
                }
                wave_sync();
            }
            PT_STAMP(st, 2);   // balanced tree walk
