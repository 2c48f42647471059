"""Rough specular reflection restated in numpy float32 from the text of include/pt_hip.h ("rough specular": THE STEP), operation by
operation: every operation is a float32 operation rounded once, in the order the header writes it, nothing fused; normalize3 is built
from numpy's correctly rounded float32 root and IEEE division, as tests/glass_restatement.py builds it; the sine and cosine come from
the oracle's probe (view_composition.sincos), as the diffuse lobe's do.  Not written from pt_rough.hpp.  The keyword switches are the
planted errors tests/test_rough_host.py puts on this side to show that the chi-square test tells them from the stated distribution."""
import numpy as np

import glass_restatement as G
import view_composition as V

F32 = np.float32
ONE, ZERO, TWO, HALF = F32(1.0), F32(0.0), F32(2.0), F32(0.5)
ALPHA_MIN, ALPHA_MAX = F32(2.0 ** -10), F32(1.0)
AXIS_FLOOR = F32(2.0 ** -40)
TWO_PI = F32(2) * F32(3.141593)
f32 = G.f32


def dot(a, b):
    with np.errstate(all="ignore"):
        return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(F32)


def _max0(x):
    return np.where(x > 0, x, ZERO).astype(F32)


def step(n, d, alpha, w1, w2, alpha_squared=False, no_warp=False, no_unstretch=False, want_scene=False):
    """(l [k, 3], G1 [k], h [k, 3]) for normals n [k, 3], unit directions d [k, 3], alpha [k] or one value and the words w1, w2 [k]."""
    n, d = f32(n).reshape(-1, 3).copy(), f32(d).reshape(-1, 3)
    alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, F32), (len(n),)))
    al = (alpha * alpha).astype(F32) if alpha_squared else alpha
    with np.errstate(all="ignore"):
        c = dot(n, d)
        n = np.where((c > 0)[:, None], -n, n).astype(F32)
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        s = np.copysign(ONE, nz).astype(F32)
        a = -(ONE / (s + nz))
        b = (nx * ny) * a
        t1 = np.stack([ONE + ((s * nx) * nx) * a, s * b, -(s * nx)], 1).astype(F32)
        t2 = np.stack([b, s + (ny * ny) * a, -ny], 1).astype(F32)
        vx, vy, vz = -dot(t1, d), -dot(t2, d), np.abs(c)
        e = G.normalize(np.stack([al * vx, al * vy, vz], 1).astype(F32))
        ex, ey, ez = e[:, 0], e[:, 1], e[:, 2]
        q = ex * ex + ey * ey
        big = q >= AXIS_FLOOR
        iq = ONE / np.sqrt(np.where(big, q, ONE).astype(F32))
        T1x = np.where(big, -(ey * iq), ONE).astype(F32)
        T1y = np.where(big, ex * iq, ZERO).astype(F32)
        T2x, T2y, T2z = -(ez * T1y), ez * T1x, ex * T1y - ey * T1x
        u1, u2 = G.unit_float(w1), G.unit_float(w2)
        r = np.sqrt(u1)
        sn, cs = V.sincos((TWO_PI * u2).astype(F32))
        p1, p2 = r * cs, r * sn
        if not no_warp:
            w = HALF * (ONE + ez)
            p2 = (ONE - w) * np.sqrt(_max0(ONE - p1 * p1)) + w * p2
        p3 = np.sqrt(_max0((ONE - p1 * p1) - p2 * p2))
        mx = (p1 * T1x + p2 * T2x) + p3 * ex
        my = (p1 * T1y + p2 * T2y) + p3 * ey
        mz = p2 * T2z + p3 * ez
        if no_unstretch:
            h = G.normalize(np.stack([mx, my, _max0(mz)], 1).astype(F32))
        else:
            h = G.normalize(np.stack([al * mx, al * my, _max0(mz)], 1).astype(F32))
        H = ((h[:, 0:1] * t1 + h[:, 1:2] * t2) + h[:, 2:3] * n).astype(F32)
        dh = dot(H, d)
        l = G.normalize((d - H * dh[:, None] * TWO).astype(F32))
        nl = dot(n, l)
        a2 = al * al
        g = (TWO * nl) / (nl + np.sqrt(a2 + (ONE - a2) * (nl * nl)))
        g1 = np.where(nl > 0, np.where(g < ONE, g, ONE), ZERO).astype(F32)
    return (l, g1, h, H) if want_scene else (l, g1, h)


def glossy(n, d, col, ks, alpha, w1, w2, eps, drop_g1=False, **errors):
    """The rough glossy lobe with normal n: (unit direction, throughput, oe, microfacet normal in the scene's frame)."""
    l, g1, _, H = step(n, d, alpha, w1, w2, want_scene=True, **errors)
    if drop_g1:
        g1 = np.ones_like(g1)
    with np.errstate(all="ignore"):
        col2 = (f32(col) * (f32(ks) * g1[:, None])).astype(F32)
    return l, col2, np.full(len(l), F32(eps), F32), H
