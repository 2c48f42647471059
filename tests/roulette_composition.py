"""The frame of a scene whose handle has RUSSIAN ROULETTE set (pt_hip.h: Russian roulette), composed on the host from the CPU oracle's
parts: the loop of tests/envdirect_composition.compose -- every view, the environment map, dielectrics, textures, shading normals, a
roughness list, per-path accounting, the bit, and with `sampling` the choice between the emitters and the environment -- with the step
of tests/roulette_restatement.py at the end of every scattering step.  sampling=False is direct lighting alone (the loop is then
tests/direct_composition.compose's: tests/test_roulette_host.py holds the two equal where the step never fires).  `roulette`:
(start, floor) or None.  The estimator it must agree with in expectation is the same call with roulette=None.  `errors`: those of
the two compositions, and the single errors of the roulette's discrimination test -- undivided (survivors keep their throughput),
unfloored_divide (survives by the floored p, divided by the unfloored m), killed_uncounted (a path the step ends never reaches the
accumulators), inverted (the survive test the wrong way round)."""
import numpy as np

import direct_restatement as D
import envdirect_restatement as ED
import environment_restatement as E
import glass_restatement as G
import motion_composition as M
import oracle_lib as O
import projection_composition as P
import rough_restatement as R
import roulette_restatement as RR
import smooth_restatement as S
import texture_restatement as T
import view_composition as V

F32 = np.float32
_TABLES = {}


def table_of(env_map):
    """tests/envdirect_restatement.table of a map, computed once per map."""
    key = (env_map.shape, env_map.tobytes())
    if key not in _TABLES:
        _TABLES[key] = ED.table(env_map)
    return _TABLES[key]


def compose(scene, rough, normals9, textures, uv, glass, env_map, width, height, pixels, spp, mrr, *, camera=None, projection=(P.PERSPECTIVE, 0.0, 0.0),
            lens=None, motion_end=None, seed=42, eps=1e-4, error=-1.0, pass_begin=0, stats=None, errors=None, nee=True, share=None, sampling=False,
            roulette=None):
    """`sampling`: ENVIRONMENT SAMPLING on; `share`: None = the default, else the caller's value.  `stats` also receives "sky_rays" (shadow
    rays sent to the environment), "sky_terms" (those that missed), "suppressed_misses", "share", and "roulette_steps", "roulette_kills",
    "roulette_draws" (steps with m < 1: the words drawn) and "paths_counted".
    sum [n, 3], sum2 [n, 3], count [n] of the frame's pixels `pixels` ([n, 2] of (x, y)).  `normals9`: (n_tri, 3, 3) or None.
    `rough`: {material: alpha} or None.  `stats` also receives "shadow_rays", "visible_terms", "suppressed_emitter_hits", "ns_terms" (terms
    whose shading normal is not the stored one), "cleared_by_glossy" / "cleared_by_glass" (the bit cleared by such a step), "rough_steps", "rough_zero" (those with G1 = 0) and "tainted" (pixels one of whose segments the oracle marks nan_seen), "events" (entering, leaving and totally
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
    tally = dict(samples_traced=0, segments=0, misses=0, contributing=0, smooth_steps=0, fallbacks=0, rough_steps=0, rough_zero=0,
                 shadow_rays=0, visible_terms=0, suppressed_emitter_hits=0, ns_terms=0, cleared_by_glossy=0, cleared_by_glass=0,
                 sky_rays=0, sky_terms=0, suppressed_misses=0, roulette_steps=0, roulette_kills=0, roulette_draws=0, paths_counted=0)
    lights, area = D.light_table(tri, tri_mat, mats)
    n_lights = len(lights["area"])
    if sampling:
        rec, _, phi_env, cells = table_of(env_map)
        share = ED.default_share(phi_env, lights) if share is None or n_lights == 0 else F32(share)
    else:
        rec, cells, share = None, 0, F32(0)                          # (no word is below 0: every shadow ray goes to the emitters, undivided)
    roulette_errors = {k: True for k in ("undivided", "unfloored_divide", "inverted") if errors.get(k)}
    tally["share"] = share
    sample_errors = {k: True for k in ("drop_jacobian", "self_pdf", "skip_fold") if errors.get(k)}
    sky_errors = {k: True for k in ("cs_twice", "no_pi", "keep_share") if errors.get(k)}
    term_errors = {k: True for k in ("cosine_once", "cs_squared", "drop_cl", "no_pi", "own_area") if errors.get(k)}
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
        L = np.zeros((len(act), 3), F32)                             # per-path accounting
        lit = np.zeros(len(act), bool)                               # the bit: the last step was a diffuse one under direct lighting
        dropped = np.zeros(len(act), bool)                           # (only under the single error killed_uncounted)
        while len(live):
            tally["segments"] += len(live)
            depth_in = depth[live].copy()
            hit, t, nan_seen = scene.closest_hits(o[live], d[live], eps=eps)
            tainted[act[live[nan_seen]]] = True
            miss = hit < 0
            tally["misses"] += int(miss.sum())
            if env_map is not None and miss.any():
                m = live[miss]
                held = lit[m] & sampling & (not errors.get("escape_counted"))
                tally["suppressed_misses"] += int(held.sum())
                ma = m[~held]
                with np.errstate(all="ignore"):
                    c = (col[ma] * E.lookup(env_map, d[ma])).astype(F32)
                    L[ma] = (L[ma] + c).astype(F32)
                tally["contributing"] += len(ma)
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
            # the direct term: a scattering diffuse hit samples a light, asks the oracle whether the point is visible, and sets the bit
            was_lit = lit[live].copy()
            dif = ~miss & (kind == 2) & (depth[live] + 1 < mrr)
            step_kind = np.where(~miss & (kind >= 1) & (depth[live] + 1 < mrr), kind, 0)
            tally["cleared_by_glossy"] += int((was_lit & (step_kind == 1)).sum())
            tally["cleared_by_glass"] += int((was_lit & (step_kind == 3)).sum())
            if errors.get("bit_never_cleared"):
                lit[live] = was_lit | (dif & nee)
            else:
                lit[live] = dif & nee & (not errors.get("bit_never_set"))
            if nee and dif.any():
                k = np.nonzero(dif)[0]
                rk = live[k]
                Nk = normals[hit[k]]
                nk = Nk
                if n9 is not None:
                    ns, usable = S.normal_at(tri, n9, hit[k], pts[k])
                    nk = np.where(usable[:, None], ns, Nk).astype(F32)
                with np.errstate(all="ignore"):
                    Ok = pts[k] if errors.get("origin_p") else (pts[k] + Nk * F32(eps)).astype(F32)
                lw = D.light_words(gpix[act[rk]], p, depth[rk], seed)
                to_sky = G.unit_float(lw[:, 3]) < share
                e = np.nonzero(~to_sky)[0]                           # the emitters' branch: the direct term over 1 - share
                if len(e):
                    li, _, om, term, has = D.term(lights, area, Ok[e], Nk[e], nk[e], col[rk[e]], mats[mat[k[e]], 0:3], lw[e, 0], lw[e, 1], lw[e, 2])
                    if sampling and not errors.get("emitters_undivided"):
                        with np.errstate(all="ignore"):
                            term = (term / (F32(1) - share)).astype(F32)
                    if has.any():
                        h = np.nonzero(has)[0]
                        shit, _, snan = scene.closest_hits(Ok[e[h]], om[h], eps=eps)
                        tainted[act[rk[e[h[snan]]]]] = True
                        vis = shit == lights["triangle"][li[h]]
                        tally["shadow_rays"] += len(h)
                        tally["visible_terms"] += int(vis.sum())
                        tally["contributing"] += int(vis.sum())
                        v = rk[e[h[vis]]]
                        with np.errstate(all="ignore"):
                            L[v] = (L[v] + term[h[vis]]).astype(F32)
                e = np.nonzero(to_sky)[0]                            # the environment's branch: a drawn direction, counted at a miss
                if len(e):
                    ew = ED.sample_words(gpix[act[rk[e]]], p, depth[rk[e]], seed)
                    _, om, pdf_w = ED.sample(rec, cells, ew[:, 0], ew[:, 1], ew[:, 2], ew[:, 3], **sample_errors)
                    term, has = ED.term(env_map, om, pdf_w, share, Nk[e], nk[e], col[rk[e]], mats[mat[k[e]], 0:3], **sky_errors)
                    if has.any():
                        h = np.nonzero(has)[0]
                        shit, _, snan = scene.closest_hits(Ok[e[h]], om[h], eps=eps)
                        tainted[act[rk[e[h[snan]]]]] = True
                        vis = shit < 0
                        tally["shadow_rays"] += len(h)
                        tally["sky_rays"] += len(h)
                        tally["sky_terms"] += int(vis.sum())
                        tally["visible_terms"] += int(vis.sum())
                        tally["contributing"] += int(vis.sum())
                        v = rk[e[h[vis]]]
                        with np.errstate(all="ignore"):
                            L[v] = (L[v] + term[h[vis]]).astype(F32)
            # the smooth step and the rough step: rays that scatter from a triangle with a usable Ns, or from a listed material's glossy lobe
            scat = ~miss & (kind >= 1) & (depth[live] + 1 < mrr)
            is_rough = scat & (kind == 1) & (alpha_of[mat] != 0)
            cand = np.nonzero(scat if n9 is not None else is_rough)[0]
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
                # an emitter hit adds its term only when the bit is clear; the skybox (a miss) adds whatever the bit
                held = did & ~miss[sel] & was_lit[sel]
                tally["suppressed_emitter_hits"] += int(held.sum())
                add = did & ~held
                with np.errstate(all="ignore"):
                    L[rest[add]] = (L[rest[add]] + contrib[add]).astype(F32)
                tally["contributing"] += int(add.sum())
            # the roulette step: every path that has scattered (its depth went up by one) and whose next ray will be traced
            if roulette is not None:
                start, floor = roulette
                k = np.nonzero(~miss & (depth[live] == depth_in + 1) & (depth[live] < mrr) & (depth_in + 1 >= start))[0]
                if len(k):
                    rk = live[k]
                    w0 = RR.words(gpix[act[rk]], p, depth_in[k], seed)
                    col[rk], alive, drew = RR.step(col[rk], w0, floor, **roulette_errors)
                    tally["roulette_steps"] += len(k)
                    tally["roulette_kills"] += int((~alive).sum())
                    tally["roulette_draws"] += int(drew.sum())
                    if errors.get("killed_uncounted"):
                        dropped[rk[~alive]] = True
            live = live[(depth[live] < mrr) & np.any(col[live] != 0, axis=1)]
        keep = ~dropped
        with np.errstate(all="ignore"):                               # every traced path, once, when it has ended
            s[act[keep]] += L[keep]
            s2[act[keep]] += L[keep] * L[keep]
        cnt[act[keep]] += 1
        tally["paths_counted"] += int(keep.sum())
    if stats is not None:
        stats.update(tally)
        stats["tainted"] = tainted
        stats["events"] = events
    return s, s2, cnt
