"""Direct lighting restated in numpy from the text of include/pt_hip.h ("direct lighting": THE LIGHT TABLE, THE DIRECT TERM), operation
by operation: the table's areas and cdf in float64 from the float32 edges, everything else a float32 operation rounded once in the
order the header writes it, nothing fused; normalize3 is tests/glass_restatement.py's.  The keyword switches of `term` are the single
errors tests/test_direct_host.py plants to show that the agreement in expectation tells them from the stated term."""
import numpy as np

import glass_restatement as G
import grain_restatement as GR
import view_composition as V

F32 = np.float32
f32 = G.f32
PI = F32(3.141593)


def light_table(tri14, tri_mat, mats):
    """(lights, A) of a scene: tri14 [n, 14] = plane[4], v0, v1, v2, square; mats [m, 10] = Kd, Ke, Ks, Ns.  lights is a dict of arrays
    in table order: v0, e1, e2, normal, le [k, 3], triangle [k], cdf [k], area [k] (float64)."""
    tri14, mats = f32(tri14), f32(mats)
    v0, v1, v2 = tri14[:, 4:7], tri14[:, 7:10], tri14[:, 10:13]
    e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
    a, b = e1.astype(np.float64), e2.astype(np.float64)
    cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    emits = np.any(mats[:, 3:6] != 0, axis=1)                     # Ke != 0: the emissive lobe alone (material.h:58-106)
    keep = np.nonzero(emits[np.asarray(tri_mat)] & (area > 0) & np.isfinite(area))[0]
    total = 0.0
    for x in area[keep]:
        total += float(x)
    cum, cdf = 0.0, np.zeros(len(keep), F32)
    for i, x in enumerate(area[keep]):
        cum += float(x)
        cdf[i] = F32(cum / total) if total > 0 else F32(0)
    if len(keep):
        cdf[-1] = F32(1.0)
    lights = dict(v0=v0[keep], e1=e1[keep], e2=e2[keep], normal=tri14[keep, 0:3], le=mats[np.asarray(tri_mat)[keep], 0:3],
                  triangle=keep.astype(np.int32), cdf=cdf, area=area[keep])
    return lights, F32(total)


def light_words(pixel, pass_, depth, seed):
    """(l0, l1, l2, l3) = philox(pixel, pass, depth, 3) under the integrator's key (1 and 2 are the display's dither and grain)."""
    w = GR.philox(np.asarray(pixel, np.uint32), pass_, np.asarray(depth, np.uint32), 3, seed, V.PHILOX_KEY1)
    return np.stack(w, 1).astype(np.uint32)


def pick(lights, l0):
    """The first light with unit_float(l0) < cdf_i."""
    u = G.unit_float(l0)
    return np.searchsorted(lights["cdf"], u, side="right").astype(np.int32)


def point(lights, i, l1, l2):
    u1, u2 = G.unit_float(l1), G.unit_float(l2)
    fold = (u1 + u2).astype(F32) > F32(1)
    u1 = np.where(fold, F32(1) - u1, u1).astype(F32)
    u2 = np.where(fold, F32(1) - u2, u2).astype(F32)
    return ((lights["v0"][i] + lights["e1"][i] * u1[:, None]).astype(F32) + lights["e2"][i] * u2[:, None]).astype(F32)


def dot(a, b):
    with np.errstate(all="ignore"):
        return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F32) + a[:, 2] * b[:, 2]).astype(F32)


def term(lights, A, O, N, n, T, kd, l0, l1, l2, *, cosine_once=False, cs_squared=False, drop_cl=False, no_pi=False, own_area=False):
    """(i, P, omega, term, has) of THE DIRECT TERM without the visibility."""
    O, N, n, T, kd = f32(O).reshape(-1, 3), f32(N).reshape(-1, 3), f32(n).reshape(-1, 3), f32(T).reshape(-1, 3), f32(kd).reshape(-1, 3)
    i = pick(lights, l0)
    P = point(lights, i, l1, l2)
    with np.errstate(all="ignore"):
        w = (P - O).astype(F32)
        r2 = ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]).astype(F32) + w[:, 2] * w[:, 2]).astype(F32)
        om = G.normalize(w)
        cn, cs, cl = dot(N, om), dot(n, om), (-dot(lights["normal"][i], om)).astype(F32)
        has = (r2 > 0) & (cn > 0) & (cs > 0) & (cl > 0)
        area = lights["area"][i].astype(F32) if own_area else np.full(len(O), F32(A), F32)
        num = cs if cosine_once else (cs * cs).astype(F32) if cs_squared else (cs * np.abs(om[:, 2])).astype(F32)
        num = num if drop_cl else (num * cl).astype(F32)
        num = (num * area).astype(F32)
        den = r2 if no_pi else (PI * r2).astype(F32)
        g = (num / den).astype(F32)
        t = (((T * kd).astype(F32) * lights["le"][i]).astype(F32) * g[:, None]).astype(F32)
    return i, P, om, np.where(has[:, None], t, F32(0)).astype(F32), has
