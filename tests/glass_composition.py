"""The frame of a scene whose handle carries DIELECTRICS (pt_hip.h: pt_dielectric), composed on the host from the CPU oracle's parts:
tests/environment_composition.compose (every view, an optional environment map) with one more step per segment -- Scene.closest_hits
gives the triangle; rays whose triangle's material is in the list take the restated dielectric step (tests/glass_restatement.py) with
the fourth word of the segment's Philox call; the rest go to Scene.segments as they do there.  Without a map a miss goes to
Scene.segments too, which ends the path (and adds the oracle scene's skybox sample if it has one)."""
import numpy as np

import environment_restatement as E
import glass_restatement as G
import motion_composition as M
import oracle_lib as O
import projection_composition as P
import view_composition as V

F32 = np.float32


def compose(scene, glass, env_map, width, height, pixels, spp, mrr, *, camera=None, projection=(P.PERSPECTIVE, 0.0, 0.0), lens=None, motion_end=None,
            seed=42, eps=1e-4, error=-1.0, pass_begin=0, stats=None):
    """sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)) after passes pass_begin ..
    pass_begin + spp - 1.  `glass`: {material index: (ior, (tr, tg, tb))}.  `env_map`: an (N, N, 3) octahedral map or None.
    `stats`: a dict that receives samples_traced, segments, misses and contributing of these pixels."""
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
            hit, t, _ = scene.closest_hits(o[live], d[live], eps=eps)
            miss = hit < 0
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
                if len(gg):
                    w3 = V.philox(gpix[act[gg]], p, depth[gg], seed)[:, 3]
                    o[gg], d[gg], col[gg] = G.step(normals[hit[gi]], o[gg], d[gg], t[gi], col[gg], w3, ior_of[mat[gi]], tint_of[mat[gi]], eps)
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
    return s, s2, cnt
