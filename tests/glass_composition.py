"""The frame of a scene whose handle carries DIELECTRICS (pt_hip.h: pt_dielectric), composed on the host from the CPU oracle's parts:
tests/environment_composition.compose (every view, an optional environment map) with one more step per segment -- Scene.closest_hits
gives the triangle; rays whose triangle's material is in the list take the restated dielectric step (tests/glass_restatement.py) with
the fourth word of the segment's Philox call; the rest go to Scene.segments as they do there.  Without a map a miss goes to
Scene.segments too, which ends the path (and adds the oracle scene's skybox sample if it has one).

For the fuzz tests compose also reports what its paths met (`events`, the counters of EVENTS) and which pixels had a segment for which
the oracle's plane evaluation gave a NaN (`want_tainted`: the ray lay exactly in some triangle's stored plane, where the library
documents a deviation, so every comparison leaves such pixels out)."""
import numpy as np

import environment_restatement as E
import glass_restatement as G
import motion_composition as M
import oracle_lib as O
import projection_composition as P
import view_composition as V

F32 = np.float32
EVENTS = ("entering",                 # dielectric hits with c < 0
          "leaving",                  # dielectric hits with c >= 0
          "total_reflections",        # s2 >= 1
          "partial_reflections",      # reflected with F < 1
          "transmissions",
          "material_ties",            # dielectric hits where a triangle of ANOTHER material is accepted at the bit-identical distance
          "near_hits",                # segments (of any material) whose hit distance is below 2 eps
          "origins_beyond_vertices",  # transmitted origins with max |component| beyond the largest |vertex coordinate|
          "last_on_glass")            # last segments (depth + 1 == mrr) that end on a dielectric: nothing is computed


def compose(scene, glass, env_map, width, height, pixels, spp, mrr, *, camera=None, projection=(P.PERSPECTIVE, 0.0, 0.0), lens=None, motion_end=None,
            seed=42, eps=1e-4, error=-1.0, pass_begin=0, stats=None, events=None, want_tainted=False, step=G.step, tie_highest=False):
    """sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)) after passes pass_begin ..
    pass_begin + spp - 1.  `glass`: {material index: (ior, (tr, tg, tb))}.  `env_map`: an (N, N, 3) octahedral map or None.
    `stats`: a dict that receives samples_traced, segments, misses and contributing of these pixels.  `events`: a dict that receives
    the counters of EVENTS over these pixels.  want_tainted: a fourth result, tainted [n] -- some segment of the pixel had the
    oracle's nan_seen.  `step` (another dielectric step) and tie_highest (the triangle a dielectric decision looks at is the HIGHEST
    index at the closest distance) exist for tests/test_glass_fuzz_host.py, which composes with deliberate errors."""
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    n = len(px)
    gpix = (px[:, 1] * width + px[:, 0]).astype(np.uint32)
    s, s2, cnt = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, np.int32)
    tri, tri_mat = scene.triangles()
    normals = np.ascontiguousarray(tri[:, 0:3], F32)
    ior_of, tint_of = np.zeros(scene.n_mat, F32), np.ones((scene.n_mat, 3), F32)
    for m, (ior, tint) in (glass or {}).items():
        ior_of[m], tint_of[m] = F32(ior), np.asarray(tint, F32)
    tally = dict(samples_traced=0, segments=0, misses=0, contributing=0)
    ev = dict.fromkeys(EVENTS, 0)
    tainted = np.zeros(n, bool)
    vertex_bound = np.abs(tri[:, 4:13]).max()
    for p in range(pass_begin, pass_begin + spp):
        skip = O.adaptive_skip(np.full(n, p, np.int32), s, s2, cnt, error)
        act = np.nonzero(~skip)[0]
        if len(act) == 0:
            continue
        tally["samples_traced"] += len(act)
        words = V.philox(gpix[act], p, 0xFFFFFFFF, seed)
        if motion_end is not None:
            o, d = M.primary_rays(px[act, 0], px[act, 1], width, height, words, M.shutter_time(gpix[act], p, seed), camera, motion_end, lens=lens)
        elif lens is not None:
            o, d = V.primary_rays(px[act, 0], px[act, 1], width, height, words, camera, lens)
        else:
            o, d = P.primary_rays(px[act, 0], px[act, 1], width, height, words, camera, projection)
        o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
        col = np.ones((len(act), 3), F32)
        depth = np.zeros(len(act), np.int32)
        live = np.arange(len(act))
        while len(live):
            tally["segments"] += len(live)
            hit, t, nan_seen = scene.closest_hits(o[live], d[live], eps=eps)
            tainted[act[live[nan_seen]]] = True
            miss = hit < 0
            if tie_highest:
                hit = scene.closest_hit_ties(o[live], d[live], eps=eps)[2]
            ev["near_hits"] += int((~miss & (t < F32(2.0) * F32(eps))).sum())
            tally["misses"] += int(miss.sum())
            if env_map is not None and miss.any():   # the restated miss of environment_composition
                m = live[miss]
                with np.errstate(all="ignore"):
                    c = (col[m] * E.lookup(env_map, d[m])).astype(F32)
                    s[act[m]] += c
                    s2[act[m]] += c * c
                cnt[act[m]] += 1
                tally["contributing"] += len(m)
                depth[m] = mrr
            mat = tri_mat[np.maximum(hit, 0)]
            is_glass = ~miss & (ior_of[mat] != 0)
            g = live[is_glass]
            if len(g):                               # the restated dielectric step; on a path's last segment nothing is computed
                go = depth[g] + 1 < mrr
                gg, gi = g[go], np.nonzero(is_glass)[0][go]
                ev["last_on_glass"] += int((~go).sum())
                if events is not None:
                    ev["material_ties"] += int(scene.closest_hit_ties(o[g], d[g], eps=eps)[3].sum())
                if len(gg):
                    w3 = V.philox(gpix[act[gg]], p, depth[gg], seed)[:, 3]
                    if events is not None:
                        _, gn, reflected, fres = G.scatter(normals[hit[gi]], d[gg], ior_of[mat[gi]], w3)
                        entering = np.all(gn == normals[hit[gi]], axis=1)
                        ev["entering"] += int(entering.sum())
                        ev["leaving"] += int((~entering).sum())
                        total = G.fresnel(*G.incidence(normals[hit[gi]], d[gg], ior_of[mat[gi]])[1:])[2]
                        ev["total_reflections"] += int(total.sum())
                        ev["partial_reflections"] += int((reflected & ~total).sum())
                        ev["transmissions"] += int((~reflected).sum())
                    o[gg], d[gg], col[gg] = step(normals[hit[gi]], o[gg], d[gg], t[gi], col[gg], w3, ior_of[mat[gi]], tint_of[mat[gi]], eps)
                    if events is not None:
                        ev["origins_beyond_vertices"] += int((~reflected & (np.abs(o[gg]).max(1) > vertex_bound)).sum())
                depth[g] += 1
            rest = live[~is_glass & ~(miss & (env_map is not None))]
            if len(rest):
                w = V.philox(gpix[act[rest]], p, depth[rest], seed)[:, :3]
                o2, d2, c2, dep2, contrib, did = scene.segments(o[rest], d[rest], col[rest], depth[rest], w, eps=eps, mrr=mrr, trig=O.TRIG_PORTABLE)
                o[rest], d[rest], col[rest], depth[rest] = o2, d2, c2, dep2
                k = act[rest[did]]
                with np.errstate(all="ignore"):
                    s[k] += contrib[did]
                    s2[k] += contrib[did] * contrib[did]
                cnt[k] += 1
                tally["contributing"] += int(did.sum())
            live = live[(depth[live] < mrr) & np.any(col[live] != 0, axis=1)]
    if stats is not None:
        stats.update(tally)
    if events is not None:
        events.update(ev)
    return (s, s2, cnt, tainted) if want_tainted else (s, s2, cnt)
