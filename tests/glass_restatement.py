"""The shading step of a smooth dielectric, restated in numpy float32 from the text of include/pt_hip.h ("dielectric materials": THE
SHADING STEP), operation by operation: every operation is a float32 operation rounded once, in the order the header writes it, nothing
fused; the root is numpy's correctly rounded float32 root, the divisions are IEEE divisions."""
import numpy as np

F32 = np.float32
ONE, HALF, TWO = F32(1.0), F32(0.5), F32(2.0)


def f32(a):
    return np.ascontiguousarray(a, F32)


def unit_float(w):
    """((w >> 9) << 1 | 1) * 2^-24: the unit float every lobe uses, in (0, 1)."""
    w = np.asarray(w, np.uint32)
    return (((w >> np.uint32(9)) << np.uint32(1)) | np.uint32(1)).astype(F32) * F32(2.0 ** -24)


def inv_ior(ior):
    """1.0f / ior, formed once on the host."""
    return ONE / f32(ior)


def fresnel(ci, eta):
    """F and ct for cos(incidence) `ci` (already clamped to <= 1) and relative index `eta`; ct is 0 where the reflection is total."""
    ci, eta = f32(ci), f32(eta)
    with np.errstate(all="ignore"):
        s2 = (eta * eta) * (ONE - ci * ci)
        total = ~(s2 < ONE)
        ct = np.sqrt(np.where(total, F32(0.0), ONE - s2).astype(F32))
        ec = eta * ci
        et = eta * ct
        rs = (ec - ct) / (ec + ct)
        rp = (ci - et) / (ci + et)
        F = HALF * (rs * rs + rp * rp)
    return np.where(total, ONE, F).astype(F32), np.where(total, F32(0.0), ct).astype(F32), total


def incidence(N, d, ior):
    """c, then (n, ci, eta) by the side the ray comes from; ci clamped to 1."""
    N, d, ior = f32(N), f32(d), f32(ior)
    c = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2]
    entering = c < 0
    n = np.where(entering[:, None], N, -N).astype(F32)
    ci = np.where(entering, -c, c).astype(F32)
    eta = np.where(entering, inv_ior(ior), ior).astype(F32)
    ci = np.where(ci < ONE, ci, ONE).astype(F32)
    return n, ci, eta


def normalize(r):
    """r * (1 / sqrt((r.x * r.x + r.y * r.y) + r.z * r.z)), as every scattered ray is normalised."""
    r = f32(r)
    with np.errstate(all="ignore"):
        inv = ONE / np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        return (r * inv[:, None]).astype(F32)


def scatter(N, d, ior, w3):
    """The unnormalised new direction r, the unit normal n of the side the ray came from, whether the ray was reflected, and F."""
    d = f32(d)
    n, ci, eta = incidence(N, d, ior)
    F, ct, _ = fresnel(ci, eta)
    reflected = unit_float(w3) < F
    with np.errstate(all="ignore"):
        r_reflect = d + n * (TWO * ci)[:, None]
        r_transmit = d * eta[:, None] + n * (eta * ci - ct)[:, None]
    return np.where(reflected[:, None], r_reflect, r_transmit).astype(F32), n, reflected, F


def step(N, o, d, t, col, w3, ior, tint, eps):
    """One dielectric hit: rays (o, d) that hit a triangle of stored normal N at distance t, throughput col, the fourth Philox word w3,
    the material's ior [n] and tint [n, 3].  Returns the next ray's origin, its unit direction and the throughput."""
    o, d, t, col, eps = f32(o), f32(d), f32(t), f32(col), F32(eps)
    p = o + d * t[:, None]
    r, n, reflected, _ = scatter(N, d, ior, w3)
    origin = np.where(reflected[:, None], p + n * eps, p - n * eps).astype(F32)
    col2 = np.where(reflected[:, None], col, col * f32(tint)).astype(F32)
    return origin, normalize(r), col2
