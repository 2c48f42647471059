"""The soundness checks of the culling hierarchy as functions of the scene -- test infrastructure, no test.

"A triangle the reference ACCEPTS for a ray is never culled for that ray", restated for the three structures the host builds
(pt_cull_tables.cpp: build_cull_tables): the sphere levels of a small cluster, the quad records of the large class and the chain of
box-tree nodes above a hit.  tests/test_cull_tables_host.py runs them on the scenes as they are, tests/test_scene_scales_host.py on
scaled and shifted copies; each takes the box its ray origins are drawn from and the length unit of its offsets."""
import ctypes as C

import numpy as np

import oracle_lib as O


def ray_sphere_keep(c, r2, o, d):
    """float64 model of sphere_keep() in pt_kernels.hip (the float32 rounding slack is part of r2)."""
    m = c - o
    b = np.maximum((m * d).sum(-1), 0.0)
    return ~((m * m).sum(-1) - b * b > r2)


def layout(t):
    """slot -> (cluster, [sphere index of its ancestor at every level, top first ... level 0 last])."""
    out = {}
    for ci in range(len(t["kind"])):
        if t["kind"][ci] != 0:
            continue
        for k in range(t["n_tri"][ci]):
            chain = [t["data_off"][ci] + t["level_off"][ci][lv] + (k >> (3 * lv)) for lv in range(t["n_levels"][ci] - 1, -1, -1)]
            out[t["first_tri"][ci] + k] = (ci, chain)
    return out


def _unit_directions(target, org):
    d = (target - org).astype(np.float32)
    inv = np.float32(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
    return d * inv[:, None]


def _accepts(L, oracle_scene, ti, o, d, eps, best):
    return L.orc_probe_intersect(oracle_scene.h, int(ti), o.ctypes.data_as(C.POINTER(C.c_float)), d.ctypes.data_as(C.POINTER(C.c_float)),
                                 eps, np.float32(np.inf), C.byref(best)) == 4


def sphere_levels(scene, oracle_scene, rng, n, lo, hi, eps=1e-4):
    """n rays from uniform origins in [lo, hi] aimed at random points of the triangles under sphere trees (inside, on edges,
    just outside).  Returns (accepted pairs, the pairs Triangle::Intersect accepts although a sphere of the cluster's chain
    drops the ray: [(ray, triangle, sphere)])."""
    t = scene.cull_tables(eps)
    lay = layout(t)
    tri, _ = scene.triangles()
    st = scene.cull_layout(eps)["slot_triangle"]
    slot_of = np.full(len(tri), -1)
    slot_of[st[st >= 0]] = np.flatnonzero(st >= 0)
    v = tri[:, 4:13].reshape(-1, 3, 3).astype(np.float64)
    small = np.array(sorted(st[k] for k in lay))
    if len(small) == 0:
        return 0, []
    a = small[rng.integers(0, len(small), n)]
    w = rng.dirichlet([0.6, 0.6, 0.6], n) * rng.choice([1.0, 1.0, 1.001, 1.01], n)[:, None]
    target = (v[a] * w[:, :, None]).sum(1)
    org = rng.uniform(list(lo), list(hi), (n, 3))
    d = _unit_directions(target, org)
    o32 = org.astype(np.float32)
    accepted, dropped = 0, []
    best = C.c_float()
    L = O.lib()
    for i in range(n):
        if not _accepts(L, oracle_scene, a[i], o32[i], d[i], eps, best):
            continue
        accepted += 1
        ci, chain = lay[int(slot_of[a[i]])]
        o64, d64 = o32[i].astype(np.float64), d[i].astype(np.float64)
        for sph in [t["cluster_sphere"][ci]] + [t["spheres"][k] for k in chain]:
            if not ray_sphere_keep(sph[:3].astype(np.float64), float(sph[3]), o64, d64):
                dropped.append((i, int(a[i]), sph.tolist()))
    return accepted, dropped


def quad_records(scene, oracle_scene, rng, n_per_triangle, lo, hi, eps=1e-4):
    """Large class: every (ray, triangle of a fused quad) pair the reference accepts must satisfy the quad test with the
    margins the kernel uses (`constants` of the tables for this scene and eps).  Returns (quads, accepted pairs, the pairs
    that fail it: [(triangle, e, t)])."""
    t = scene.cull_tables(eps)
    k1, k2, a_max, m0 = (t["constants"][k] for k in ("k1", "k2", "a_max", "m0"))
    tri, _ = scene.triangles()
    slot_tri = scene.cull_layout(eps)["slot_triangle"]
    v = tri[:, 4:13].reshape(-1, 3, 3).astype(np.float64)
    L = O.lib()
    best = C.c_float()
    quads, checked, failed = 0, 0, []
    for c in np.flatnonzero(t["kind"] == 1):
        first, n, off, mask = t["first_tri"][c], t["n_tri"][c], t["data_off"][c], int(t["level_off"][c][1])
        for k in range(0, min(n, 32), 2):           # (the quad mask of word 0 covers the first 32 records)
            if not (mask >> k) & 1:
                continue
            quads += 1
            rec = t["bary"][off + k].astype(np.float64)
            for half in (0, 1):
                ti = int(slot_tri[first + k + half])      # slot -> original triangle
                m = n_per_triangle
                w = rng.dirichlet([0.5, 0.5, 0.5], m) * rng.choice([1.0, 1.0, 1.0005], m)[:, None]   # incl. edges / just outside
                target = (v[ti] * w[:, :, None]).sum(1)
                org = rng.uniform(list(lo), list(hi), (m, 3))
                d = _unit_directions(target, org)
                o32 = org.astype(np.float32)
                for i in range(m):
                    if not _accepts(L, oracle_scene, ti, o32[i], d[i], eps, best):
                        continue
                    checked += 1
                    o64, d64 = o32[i].astype(np.float64), d[i].astype(np.float64)
                    num, den = rec[0:3] @ o64 + rec[3], rec[0:3] @ d64
                    tt = -num / den
                    P = o64 + tt * d64
                    al, be = rec[4:7] @ P + rec[7], rec[8:11] @ P + rec[11]
                    e = min(be, al - be, 1 - al) if half == 0 else min(al, be - al, 1 - be)
                    et = (k1 * abs(tt) + k2) / abs(den)
                    if not (e >= -(a_max * et + m0) and tt >= -et):
                        failed.append((ti, e, tt))
    return quads, checked, failed


def box_chain(g, o, rng, n, unit=1.0, eps=1e-4):
    """Big scenes: the chain of box-tree nodes above the triangle the reference hits must survive the kernel's slab test (numpy
    restatement in float32, tests/bvh_emulation.py) for the tightest t_best the
    walk can hold: the hit's own t.  n rays from points `1e-4 unit` off random surfaces into random directions.  `g`: the
    library's scene (its box tree), `o`: the oracle's.  Returns (hits on triangles of the tree, levels walked, dropped: [(level,
    form, count)])."""
    import bvh_emulation as B
    lay = g.cull_layout(eps)
    t, fl = B.decode(lay["bvh"]), lay["bvh_inner_nodes"]
    st = lay["slot_triangle"]
    n_tri = o.n_tri
    assert len(lay["bvh"]) > fl > 0 and sorted(st[st >= 0]) == list(range(n_tri))
    n_tree_slots = (len(lay["bvh"]) - fl) * 8
    assert (st[n_tree_slots:] >= 0).all()                          # padding only inside the tree's leaves
    par, pos = B.parents(t, fl)
    assert (par[1:] >= 0).all() and par[0] == -1                   # one root, every other node has a parent
    slot_of = np.full(n_tri, -1)
    slot_of[st[st >= 0]] = np.flatnonzero(st >= 0)
    tri, _ = o.triangles()
    v = tri[:, 4:13].reshape(-1, 3, 3).astype(np.float64)
    a = rng.integers(0, n_tri, n)
    w = rng.dirichlet([1, 1, 1], n)
    src = ((v[a] * w[:, :, None]).sum(1) + tri[a, 0:3] * (1e-4 * unit)).astype(np.float32)
    dd = rng.normal(size=(n, 3)).astype(np.float32)
    dd[::7, 0] = 0                                                  # some axis-parallel components (the 1e-30 substitution)
    inv = np.float32(1) / np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2], dtype=np.float32)
    dd = (dd * inv[:, None]).astype(np.float32)
    hi, ht, nan = o.closest_hits(src, dd, eps)
    ok = (hi >= 0) & ~nan
    ok &= slot_of[np.maximum(hi, 0)] < n_tree_slots                 # hits on triangles of the tree (not the walls)
    ro, rd, tb, sl = src[ok], dd[ok], ht[ok], slot_of[hi[ok]]
    hits = len(sl)
    leaf_of_group = np.full(n_tree_slots // 8, -1)                  # leaf node that holds slots 8 g ... 8 g + 7
    leaf_of_group[t["base"][t["leaf"]]] = np.flatnonzero(t["leaf"])
    assert (leaf_of_group >= 0).all() and t["leaf"].sum() == len(lay["bvh"]) - fl
    node, child = leaf_of_group[sl // 8], sl % 8
    levels, dropped = 0, []
    while len(node):
        kept = B.children_kept(t, node, ro, rd, tb, 5e-7)
        if not kept[np.arange(len(node)), child].all():
            dropped.append((levels, "float", int((~kept[np.arange(len(node)), child]).sum())))
        child, node = pos[node], par[node]
        live = node >= 0
        node, child, ro, rd, tb = node[live], child[live], ro[live], rd[live], tb[live]
        levels += 1
    return hits, levels, dropped
