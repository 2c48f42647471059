"""Scenes at other scales and places, and the adversarial rays that go with them -- test infrastructure, no test.

The culling margins (pt_cull_tables.cpp: build_cull_tables, margins) are derived from the scene's extent, and several of
their constants are in absolute units.  transformed() writes an OBJ whose vertices are scaled by a power of two and / or
shifted, camera_for() moves the reference's camera along, adversarial_rays() takes the box the origins are drawn from and the
length unit of its offsets, so that a test can ask at every entry of TRANSFORMS what the suite asks at scale 1."""
import importlib
import os
import shutil

import numpy as np

# (scale, offset): each vertex coordinate x becomes float32(float32(x) * scale + offset)
TRANSFORMS = [
    (2.0 ** -10, (0.0, 0.0, 0.0)),
    (2.0 ** -4, (0.0, 0.0, 0.0)),
    (2.0 ** 4, (0.0, 0.0, 0.0)),
    (2.0 ** 10, (0.0, 0.0, 0.0)),
    (1.0, (512.0, -256.0, 1024.0)),
    (1.0, (4096.0, 4096.0, 4096.0)),
    (2.0 ** -4, (100.0, 0.0, 0.0)),      # a small scene far from the origin: feature size against the coordinates' ulp is worst
]
EXTREME_SCALES = [TRANSFORMS[0], TRANSFORMS[3]]

# the box the plain scenes' ray origins are drawn from (the room of Tor.obj is [-10, 10] x [-10, 10] x [-21, 10]) and the
# reference's eye
PLAIN_LO, PLAIN_HI = (-9.9, -9.9, -20.9), (9.9, 9.9, 9.9)
REFERENCE_EYE, REFERENCE_TARGET = (0.0, 0.0, -20.0), (0.0, 0.0, 0.0)


def transform_id(tr):
    scale, off = tr
    e = int(round(np.log2(scale)))
    s = "x1" if e == 0 else f"x2^{e}"
    return s if not any(off) else s + "+(" + ",".join("%g" % c for c in off) + ")"


def apply(points, scale, offset):
    """float32(float32(x) * scale + offset) for points [..., 3] (the product and the sum in double, rounded once)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    return (p * float(scale) + np.asarray(offset, np.float64)).astype(np.float32)


def transformed(model_dir, name, out_dir, scale, offset):
    """Writes out_dir/name: model_dir/name with every `v` line transformed, printed so that it round-trips; every other line --
    `vn` included: normals do not scale -- and every file an `mtllib` line names are copied unchanged.  Returns out_dir with a
    trailing slash."""
    os.makedirs(out_dir, exist_ok=True)
    out = []
    for line in open(os.path.join(model_dir, name)).read().split("\n"):
        tok = line.split()
        if tok and tok[0] == "v":
            q = apply([float(t) for t in tok[1:4]], scale, offset)
            line = "v " + " ".join(repr(float(c)) for c in q)
        elif tok and tok[0] == "mtllib":
            for m in tok[1:]:
                if os.path.abspath(model_dir) != os.path.abspath(out_dir):
                    shutil.copy(os.path.join(model_dir, m), os.path.join(out_dir, m))
        out.append(line)
    open(os.path.join(out_dir, name), "w").write("\n".join(out))
    return os.path.join(out_dir, "")


def box_for(scale, offset):
    """PLAIN_LO, PLAIN_HI transformed (float64)."""
    off = np.asarray(offset, np.float64)
    return np.asarray(PLAIN_LO) * scale + off, np.asarray(PLAIN_HI) * scale + off


def camera_for(scale, offset, W, H):
    """pt.look_at from the reference's eye to its target, both transformed (W, H: the frame the camera is for; the reference's
    mapping -- the full width and the full height span the same angle -- does not depend on them)."""
    pt = importlib.import_module("path-tracing_amd")
    eye = apply(REFERENCE_EYE, scale, offset)
    target = apply(REFERENCE_TARGET, scale, offset)
    return pt.look_at(tuple(float(c) for c in eye), tuple(float(c) for c in target))


def normalise(d):
    """Ray's constructor (ray.h:23): v * (1 / sqrt((x*x + y*y) + z*z)) in float32."""
    d = np.ascontiguousarray(d, np.float32)
    inv = np.float32(1.0) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
    return (d * inv[:, None]).astype(np.float32)


def adversarial_rays(tri, rng, n, lo=PLAIN_LO, hi=PLAIN_HI, unit=1.0, origin=(0.0, 0.0, 0.0), lattice=9):
    """Five families of n rays each that ordinary path sampling rarely produces.  `lo`, `hi`: the box interior origins are
    drawn from; `unit`: the length the offsets, the lattice step and the tangent walks are multiples of; `origin`: a point
    of the lattice (the image of the world's origin); `lattice`: its half-width in steps, to be kept inside the room (a ray
    that lies exactly in a wall's plane is outside the contract, pt_hip.h).  The defaults are the plain scenes' values."""
    T = len(tri)
    v = tri[:, 4:13].reshape(T, 3, 3).astype(np.float64)
    nrm = tri[:, 0:3].astype(np.float64)
    org0 = np.asarray(origin, np.float64)
    O_, D_ = [], []
    # (1) random interior origins, random directions
    o = rng.uniform(list(lo), list(hi), (n, 3))
    d = rng.normal(size=(n, 3))
    O_.append(o); D_.append(d)
    # (2) from a surface point (+eps*N like the lobes do) towards a point on another triangle's EDGE or VERTEX
    a, b = rng.integers(0, T, n), rng.integers(0, T, n)
    w = rng.dirichlet([1, 1, 1], n)
    src = (v[a] * w[:, :, None]).sum(1) + nrm[a] * (1e-4 * unit)
    e = rng.random((n, 1))
    kind = rng.integers(0, 3, n)
    tgt = np.where((kind == 0)[:, None], v[b, 0], np.where((kind == 1)[:, None], v[b, 0] * e + v[b, 1] * (1 - e),
                                                           v[b, 1] * e + v[b, 2] * (1 - e)))
    O_.append(src); D_.append(tgt - src)
    # (3) grazing: direction in the plane of a triangle, tilted by a tiny angle, from just above that plane
    a = rng.integers(0, T, n)
    tang = v[a, 1] - v[a, 0]
    tang /= np.linalg.norm(tang, axis=1, keepdims=True) + 1e-30
    tilt = rng.choice([0.0, 1e-7, -1e-7, 1e-5, -1e-5, 1e-3, -1e-3], n)[:, None]
    src = ((v[a] * w[:, :, None]).sum(1) + nrm[a] * (rng.choice([0.0, 1e-4, -1e-4, 1e-2], n)[:, None] * unit)
           - tang * (rng.uniform(0, 5, (n, 1)) * unit))
    O_.append(src); D_.append(tang + tilt * nrm[a])
    # (4) axis-aligned directions and origins on lattice points (exact zeros in products)
    o = rng.integers(-lattice, lattice + 1, (n, 3)).astype(np.float64) * unit + org0
    d = np.zeros((n, 3)); d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    O_.append(o); D_.append(d)
    # (5) towards the centroid of a random triangle, from far and from very near
    a = rng.integers(0, T, n)
    cen = v[a].mean(1)
    src = np.where(rng.random((n, 1)) < 0.5, rng.uniform(-9, 9, (n, 3)) * unit + org0, cen + rng.normal(size=(n, 3)) * (1e-3 * unit))
    O_.append(src); D_.append(cen - src + 1e-12 * unit)
    o = np.concatenate(O_).astype(np.float32)
    d = normalise(np.concatenate(D_).astype(np.float32))
    ok = np.isfinite(d).all(1)
    return o[ok], d[ok]


def rays_pointing_away(rng, n, lo, hi, distance):
    """n rays that start `distance` outside one face of the box [lo, hi] and point away from it.  Half a unit puts them
    outside the room (whose walls lie a tenth of a unit beyond the box) and inside the envelope of origins: misses, as long
    as the reference's area test means anything -- it accepts a plane crossing up to about eps / edge beyond a triangle."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o = rng.uniform(lo, hi, (n, 3))
    axis, up = rng.integers(0, 3, n), rng.random(n) < 0.5
    k = np.arange(n)
    o[k, axis] = np.where(up, hi[axis] + distance, lo[axis] - distance)
    d = rng.normal(size=(n, 3))
    d[k, axis] = np.where(up, 1.0, -1.0) * (np.abs(d[k, axis]) + 0.05)
    return o.astype(np.float32), normalise(d.astype(np.float32))
