"""The frame of a scene whose handle carries a ROUGHNESS LIST (pt_hip.h: rough specular), composed on the host from the CPU oracle's
parts: tests/smooth_composition.compose -- every view, an optional environment map, optional dielectrics, textures and shading normals
-- with the rough step (tests/rough_restatement.py) inserted where the glossy lobe (kind 1) is chosen on a listed material by a ray
that scatters.  Without shading normals the step is made with the stored normal N; with them it is made with Ns and with N from the
same words, and the fallback rule selects, as for every other lobe.  `errors`: the single errors of the discrimination tests (the
smooth ones, and w23, drop_g1, origin_on_h, mirror for the rough step)."""
import numpy as np

import environment_restatement as E
import glass_restatement as G
import motion_composition as M
import oracle_lib as O
import projection_composition as P
import rough_restatement as R
import smooth_restatement as S
import texture_restatement as T
import view_composition as V

F32 = np.float32


def compose(scene, rough, normals9, textures, uv, glass, env_map, width, height, pixels, spp, mrr, *, camera=None, projection=(P.PERSPECTIVE, 0.0, 0.0),
            lens=None, motion_end=None, seed=42, eps=1e-4, error=-1.0, pass_begin=0, stats=None, errors=None):
    """sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)).  `normals9`: (n_tri, 3, 3) or None.
    `rough`: {material: alpha} or None.  `stats` also receives "rough_steps", "rough_zero" (those with G1 = 0) and "tainted" (pixels one of whose segments the oracle marks nan_seen), "events" (entering, leaving and totally
    reflected dielectric steps made with Ns) and "smooth_steps" / "fallbacks"."""
    errors = dict(errors or {})
    px = np.asarray(pixels, np.int64).reshape(-1, 2)
    n = len(px)
    gpix = (px[:, 1] * width + px[:, 0]).astype(np.uint32)
    s, s2, cnt = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, np.int32)
    tainted = np.zeros(n, bool)
    tri, tri_mat = scene.triangles()
    mats = scene.materials()
    normals = np.ascontiguousarray(tri[:, 0:3], F32)
    n9 = None if normals9 is None else np.ascontiguousarray(normals9, F32).reshape(-1, 3, 3)
    ior_of, tint_of = np.zeros(scene.n_mat, F32), np.ones((scene.n_mat, 3), F32)
    for m, (ior, tint) in (glass or {}).items():
        ior_of[m], tint_of[m] = F32(ior), np.asarray(tint, F32)
    alpha_of = np.zeros(scene.n_mat, F32)
    for m, al in (rough or {}).items():
        alpha_of[m] = F32(al)
    if errors.get("mirror"):
        alpha_of[:] = 0
    wa, wb = (2, 3) if errors.get("w23") else (1, 2)
    textured = np.zeros(scene.n_mat, bool)
    for m in (textures or {}):
        textured[m] = True
    tally = dict(samples_traced=0, segments=0, misses=0, contributing=0, smooth_steps=0, fallbacks=0, rough_steps=0, rough_zero=0)
    events = dict(entering=0, leaving=0, total=0)
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
            if env_map is not None and miss.any():
                m = live[miss]
                with np.errstate(all="ignore"):
                    c = (col[m] * E.lookup(env_map, d[m])).astype(F32)
                    s[act[m]] += c
                    s2[act[m]] += c * c
                cnt[act[m]] += 1
                tally["contributing"] += len(m)
                depth[m] = mrr
            mat = tri_mat[np.maximum(hit, 0)]
            all_words = V.philox(gpix[act[live]], p, depth[live], seed)
            kind = T.lobe_kind(mats, mat, all_words[:, 0])
            is_glass = ~miss & (ior_of[mat] != 0)
            kind[is_glass] = 3
            kind[miss] = -1
            with np.errstate(all="ignore"):
                pts = (o[live] + d[live] * t[:, None]).astype(F32)
            # the texel step: the emissive and the diffuse lobe of a textured material (texture_composition)
            tex_here = ~miss & textured[mat] & ((kind == 0) | (kind == 2))
            if tex_here.any():
                k = np.nonzero(tex_here)[0]
                coords = T.uv_at(tri, uv, hit[k], pts[k])
                texel = np.zeros((len(k), 3), F32)
                for m, (texels, filt) in textures.items():
                    q = mat[k] == m
                    if q.any():
                        texel[q] = T.lookup(texels, coords[q], filt)
                col[live[k]] = (col[live[k]] * texel).astype(F32)
            handled = np.zeros(len(live), bool)
            # the smooth step and the rough step: rays that scatter from a triangle with a usable Ns, or from a listed material's glossy lobe
            scat = ~miss & (kind >= 1) & (depth[live] + 1 < mrr)
            is_rough = scat & (kind == 1) & (alpha_of[mat] != 0)
            cand = np.nonzero(scat if n9 is not None else is_rough)[0]
            if n9 is not None and errors.get("emissive_on_ns"):
                cand = np.nonzero(scat | (~miss & (kind == 0)))[0]
            if len(cand):
                N = normals[hit[cand]]
                if n9 is not None:
                    ns, usable = S.normal_at(tri, n9, hit[cand], pts[cand], swap_b=errors.get("swap_b", False), normalise=not errors.get("no_normalise", False))
                else:
                    ns, usable = N.copy(), np.zeros(len(cand), bool)
                sel_ = usable | is_rough[cand]
                cand, ns, usable, N = cand[sel_], ns[sel_], usable[sel_], N[sel_]
            if len(cand):
                rc = live[cand]
                ns = np.where(usable[:, None], ns, N).astype(F32)
                kc = kind[cand]
                w = all_words[cand]
                al = alpha_of[mat[cand]]
                rgh = (kc == 1) & (al != 0)

                def lobes(nn):
                    """The step with normal nn for every candidate: direction, throughput, oe, the origin's base, dielectric events."""
                    r = np.zeros((len(cand), 3), F32)
                    c2 = col[rc].copy()
                    oe = np.full(len(cand), F32(eps), F32)
                    base = N.copy()
                    q = (kc == 1) & ~rgh
                    if q.any():
                        r[q], c2[q], oe[q] = S.glossy(nn[q], d[rc[q]], col[rc[q]], mats[mat[cand[q]], 6:9], eps)
                    q = rgh
                    if q.any():
                        r[q], c2[q], oe[q], H = R.glossy(nn[q], d[rc[q]], col[rc[q]], mats[mat[cand[q]], 6:9], al[q], w[q, wa], w[q, wb], eps, drop_g1=bool(errors.get("drop_g1")))
                        if errors.get("origin_on_h"):
                            base[q] = H
                    q = kc == 2
                    if q.any():
                        r[q], c2[q], oe[q] = S.diffuse(nn[q], col[rc[q]], mats[mat[cand[q]], 0:3], w[q, 1], w[q, 2], eps)
                    q = kc == 3
                    ev = None
                    if q.any():
                        r[q], c2[q], oe[q], ev = S.dielectric(nn[q], d[rc[q]], col[rc[q]], w[q, 3], ior_of[mat[cand[q]]], tint_of[mat[cand[q]]], eps)
                    return r, c2, oe, base, ev

                r, c2, oe, base, ev = lobes(ns)
                keep = S.keeps(r, N, oe) | bool(errors.get("no_fallback", False))
                emis = kc == 0                                   # (only under the single error emissive_on_ns)
                keep &= ~emis
                back = ~keep & ~emis & rgh                       # a rough step that falls back: the rough step with N
                if back.any():
                    r2, c22, oe2, base2, _ = lobes(N)
                    r[back], c2[back], oe[back], base[back] = r2[back], c22[back], oe2[back], base2[back]
                if ev is not None:
                    kq = keep[kc == 3]
                    events["entering"] += int((ev[0] & kq).sum()); events["leaving"] += int((~ev[0] & kq).sum()); events["total"] += int((ev[2] & kq).sum())
                tally["smooth_steps"] += int((keep & usable).sum())
                tally["fallbacks"] += int((~keep & ~emis & usable).sum())
                take = keep | back
                tally["rough_steps"] += int((take & rgh).sum())
                tally["rough_zero"] += int((take & rgh & ~np.any(c2 != 0, axis=1) & np.any(col[rc] != 0, axis=1)).sum())
                kk = rc[take]
                if errors.get("origin_on_ns"):
                    base = np.where((usable & keep & ~rgh)[:, None], ns, base).astype(F32)
                with np.errstate(all="ignore"):
                    o[kk] = (pts[cand[take]] + base[take] * oe[take][:, None]).astype(F32)
                d[kk], col[kk] = r[take], c2[take]
                depth[kk] += 1
                handled[cand[take]] = True
                if emis.any():                                   # the emissive lobe with its facing test on Ns: the error
                    e = cand[emis]
                    re_ = live[e]
                    faces = ~(S.dot(d[re_], ns[emis]) > 0)
                    c = (col[re_[faces]] * mats[mat[e[faces]], 0:3]).astype(F32)
                    with np.errstate(all="ignore"):
                        s[act[re_[faces]]] += c
                        s2[act[re_[faces]]] += c * c
                    cnt[act[re_[faces]]] += 1
                    tally["contributing"] += int(faces.sum())
                    depth[re_] = mrr
                    handled[e] = True
            g = np.nonzero(is_glass & ~handled)[0]
            if len(g):                                               # the dielectric step with the stored normal (glass_composition)
                go = depth[live[g]] + 1 < mrr
                gi, gg = g[go], live[g[go]]
                if len(gg):
                    o[gg], d[gg], col[gg] = G.step(normals[hit[gi]], o[gg], d[gg], t[gi], col[gg], all_words[gi, 3], ior_of[mat[gi]], tint_of[mat[gi]], eps)
                depth[live[g]] += 1
            sel = ~is_glass & ~handled & ~(miss & (env_map is not None))
            rest = live[sel]
            if len(rest):
                o2, d2, c2, dep2, contrib, did = scene.segments(o[rest], d[rest], col[rest], depth[rest], all_words[sel, :3], eps=eps, mrr=mrr, trig=O.TRIG_PORTABLE)
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
        stats["events"] = events
    return s, s2, cnt
