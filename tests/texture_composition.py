"""The frame of a scene whose handle carries TEXTURES (pt_hip.h: pt_texture), composed on the host from the CPU oracle's parts:
tests/glass_composition.compose -- every view, an optional environment map, optional dielectrics -- with one more step per segment.
Scene.closest_hits gives the triangle; the lobe choice is restated (texture_restatement.lobe_kind); where the material is textured and
the lobe is the emissive or the diffuse one the throughput is multiplied by the restated texel (texture_restatement); then the ray goes
to Scene.segments as it does there.  (On a path's last segment the product changes nothing for the diffuse lobe: the path ends.)
`errors`: keyword switches of the restatement (swap_b, flip_v, clamp) and `glossy_too`, the single errors of the discrimination test."""
import numpy as np

import environment_restatement as E
import glass_restatement as G
import motion_composition as M
import oracle_lib as O
import projection_composition as P
import texture_restatement as T
import view_composition as V

F32 = np.float32


def compose(scene, textures, uv, glass, env_map, width, height, pixels, spp, mrr, *, camera=None, projection=(P.PERSPECTIVE, 0.0, 0.0), lens=None,
            motion_end=None, seed=42, eps=1e-4, error=-1.0, pass_begin=0, stats=None, errors=None):
    """sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)).  `textures`: {material: (texels (h, w, 3),
    filter)}; `uv`: (n_tri, 3, 2); `glass` and `env_map` as in glass_composition.  `stats` also receives "tainted": the pixels one of
    whose segments the oracle marks nan_seen."""
    errors = dict(errors or {})
    glossy_too = errors.pop("glossy_too", False)
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    n = len(px)
    gpix = (px[:, 1] * width + px[:, 0]).astype(np.uint32)
    s, s2, cnt = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, np.int32)
    tainted = np.zeros(n, bool)
    tri, tri_mat = scene.triangles()
    mats = scene.materials()
    normals = np.ascontiguousarray(tri[:, 0:3], F32)
    ior_of, tint_of = np.zeros(scene.n_mat, F32), np.ones((scene.n_mat, 3), F32)
    for m, (ior, tint) in (glass or {}).items():
        ior_of[m], tint_of[m] = F32(ior), np.asarray(tint, F32)
    textured = np.zeros(scene.n_mat, bool)
    for m in (textures or {}):
        textured[m] = True
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
            hit, t, nan_seen = scene.closest_hits(o[live], d[live], eps=eps)
            tainted[act[live[nan_seen]]] = True
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
            if len(g):                               # the restated dielectric step of glass_composition
                go = depth[g] + 1 < mrr
                gg, gi = g[go], np.nonzero(is_glass)[0][go]
                if len(gg):
                    w3 = V.philox(gpix[act[gg]], p, depth[gg], seed)[:, 3]
                    o[gg], d[gg], col[gg] = G.step(normals[hit[gi]], o[gg], d[gg], t[gi], col[gg], w3, ior_of[mat[gi]], tint_of[mat[gi]], eps)
                depth[g] += 1
            sel = ~is_glass & ~(miss & (env_map is not None))
            rest = live[sel]
            if len(rest):
                w = V.philox(gpix[act[rest]], p, depth[rest], seed)[:, :3]
                # the texel step: the lobe as the material's step will choose it, then col *= texel for the emissive and the diffuse one
                ri = np.nonzero(sel)[0]
                tex_here = ~miss[ri] & textured[mat[ri]]
                if tex_here.any():
                    k = ri[tex_here]
                    kind = T.lobe_kind(mats, mat[k], w[tex_here, 0])
                    takes = (kind == 0) | (kind == 2) | (glossy_too & (kind == 1))
                    k, rk = k[takes], rest[tex_here][takes]
                    if len(k):
                        with np.errstate(all="ignore"):
                            pt_hit = (o[rk] + d[rk] * t[k][:, None]).astype(F32)
                        coords = T.uv_at(tri, uv, hit[k], pt_hit, swap_b=errors.get("swap_b", False))
                        texel = np.zeros((len(k), 3), F32)
                        for m, (texels, filt) in textures.items():
                            q = mat[k] == m
                            if q.any():
                                texel[q] = T.lookup(texels, coords[q], filt, flip_v=errors.get("flip_v", True), clamp=errors.get("clamp", False))
                        col[rk] = (col[rk] * texel).astype(F32)
                o2, d2, c2, dep2, contrib, did = scene.segments(o[rest], d[rest], col[rest], depth[rest], w, eps=eps, mrr=mrr, trig=O.TRIG_PORTABLE)
                o[rest], d[rest], col[rest], depth[rest] = o2, d2, c2, dep2
                kk = act[rest[did]]
                with np.errstate(all="ignore"):
                    s[kk] += contrib[did]
                    s2[kk] += contrib[did] * contrib[did]
                cnt[kk] += 1
                tally["contributing"] += int(did.sum())
            live = live[(depth[live] < mrr) & np.any(col[live] != 0, axis=1)]
    if stats is not None:
        stats.update(tally)
        stats["tainted"] = tainted
    return s, s2, cnt
