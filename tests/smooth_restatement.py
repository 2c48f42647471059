"""Smooth shading restated in numpy float32 from the text of include/pt_hip.h ("smooth shading": THE SHADING NORMAL, THE SHADING STEP,
FALLBACK), operation by operation: every operation is a float32 operation rounded once, in the order the header writes it, nothing
fused; normalize3 is built from numpy's correctly rounded float32 root and IEEE division, as tests/glass_restatement.py builds it; the
sine and cosine of the diffuse lobe come from the oracle's probe (view_composition.sincos).  The keyword switches are the single errors
tests/test_smooth_host.py puts on the reference side to show that a frame tells them from the stated step."""
import numpy as np

import glass_restatement as G
import texture_restatement as T
import view_composition as V

F32 = np.float32
ONE, ZERO, TWO = F32(1.0), F32(0.0), F32(2.0)
f32 = G.f32


def dot(a, b):
    with np.errstate(all="ignore"):
        return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(F32)


def shading_normal(rec, n9, N, p, swap_b=False, normalise=True):
    """Ns [n, 3] and whether it came from the corners, for points p on triangles with records rec [n, 8], corner normals n9 [n, 3, 3]
    and stored normals N [n, 3]."""
    rec, n9, N, p = f32(rec), f32(n9).reshape(-1, 3, 3), f32(N), f32(p)
    b1, b2 = T.barycentrics(rec, p)
    if swap_b:
        b1, b2 = b2, b1
    with np.errstate(all="ignore"):
        b0 = (ONE - b1) - b2
        m = ((b0[:, None] * n9[:, 0] + b1[:, None] * n9[:, 1]) + b2[:, None] * n9[:, 2]).astype(F32)
        l = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        usable = np.isfinite(l) & (l > 0)
        unit = G.normalize(m) if normalise else m
    ns = np.where(usable[:, None], unit, N).astype(F32)
    flip = dot(ns, N) < 0
    return np.where(flip[:, None], -ns, ns).astype(F32), usable


def normal_at(tri14, n9, hit, p, **errors):
    t = f32(tri14)[hit]
    return shading_normal(T.bary_records(t), f32(n9).reshape(-1, 3, 3)[hit], t[:, 0:3], p, **errors)


def glossy(n, d, col, ks, eps):
    """The glossy lobe with normal n: (unit direction, throughput, oe)."""
    n, d = f32(n), f32(d)
    with np.errstate(all="ignore"):
        dn = dot(n, d)
        r = d - n * dn[:, None] * TWO
        return G.normalize(r), (f32(col) * f32(ks)).astype(F32), np.full(len(d), F32(eps), F32)


def diffuse(n, col, kd, w1, w2, eps):
    """The diffuse lobe with normal n and the words w1, w2."""
    n = f32(n)
    xi1, xi2 = G.unit_float(w1), G.unit_float(w2)
    with np.errstate(all="ignore"):
        sn, cs = V.sincos((F32(2 * F32(3.141593)) * xi2).astype(F32))
        sq = np.sqrt(xi1)
        h = G.normalize(np.stack([sq * cs, sq * sn, np.sqrt(ONE - xi1)], 1).astype(F32))
        h = np.where((dot(n, h) < 0)[:, None], h * F32(-1), h).astype(F32)
        dt = dot(n, h)
        dt = np.where(dt > 0, dt, ZERO).astype(F32)
        return G.normalize(h), (f32(col) * (f32(kd) * dt[:, None])).astype(F32), np.full(len(n), F32(eps), F32)


def dielectric(n, d, col, w3, ior, tint, eps):
    """The dielectric step with normal n: (unit direction, throughput, oe, (entering, reflected, total))."""
    n, d = f32(n), f32(d)
    r, _, reflected, _ = G.scatter(n, d, ior, w3)
    entering = dot(n, d) < 0
    _, ci, eta = G.incidence(n, d, ior)
    total = G.fresnel(ci, eta)[2]
    oe = np.where(reflected == entering, F32(eps), -F32(eps)).astype(F32)
    col2 = np.where(reflected[:, None], f32(col), f32(col) * f32(tint)).astype(F32)
    return G.normalize(r), col2, oe, (entering, reflected, total)


def keeps(r, N, oe):
    """The fallback rule: True where the step made with Ns is kept."""
    with np.errstate(all="ignore"):
        return (dot(f32(r), f32(N)) * f32(oe)) > 0
