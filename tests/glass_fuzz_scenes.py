"""Scene generators for the dielectric fuzz tests (tests/test_glass_fuzz_host.py on the CPU, tests/test_gpu_glass_fuzz.py on the GPU),
importable without a GPU: the randomised scenes of tests/test_gpu_fuzz.py and tests/test_gpu_environment.py (moved here unchanged: the
files they write are the bytes they were), the room of tests/test_gpu_glass.py, and three scenes built to put geometry within a few eps
BEHIND a dielectric surface, where no ray started before there were transmitted rays.  Every generator writes its vertices with 6
decimals, so the library and the oracle parse the same records.  CASES lists the frames both tests look at; REQUIRED says which of
glass_composition's event counters a scene is there to raise."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-4


# ---- the generators of tests/test_gpu_fuzz.py and tests/test_gpu_environment.py ---------------------------------------------------------
def _random_scene(d, seed, n_small, n_large, n_dup, few_emitters=False):
    rng = np.random.default_rng(seed)
    mtl = ["newmtl 0\nKe 1 1 1\nKd 0.9 0.7 0.5\n", "newmtl 1\nNs 300\nKs 0.7 0.7 0.7\nKd 0.6 0.6 0.6\n",
           "newmtl 2\nNs 0\nKd 0.8 0.3 0.3\n", "newmtl 3\nNs 1000\nKs 0.9 0.9 0.9\n"]
    open(d + "f.mtl", "w").write("".join(mtl))
    lines = ["mtllib f.mtl"]
    nv = nn = 0

    def tri(p, q, r, m, with_vn):
        nonlocal nv, nn
        lines.extend(["v %.6f %.6f %.6f" % tuple(p), "v %.6f %.6f %.6f" % tuple(q), "v %.6f %.6f %.6f" % tuple(r)])
        lines.append(f"usemtl {m}")
        if with_vn:
            n = np.cross(q - p, r - p)
            n = n / (np.linalg.norm(n) + 1e-30) + rng.normal(size=3) * 0.05      # a slightly "wrong" normal, like Tor.obj's
            lines.append("vn %.4f %.4f %.4f" % tuple(n))
            nn += 1
            lines.append(f"f {nv+1}//{nn} {nv+2}//{nn} {nv+3}//{nn}")
        else:
            lines.append(f"f {nv+1} {nv+2} {nv+3}")
        nv += 3

    L = 9.0
    box = [(-L, -L, -24), (L, -L, -24), (L, L, -24), (-L, L, -24), (-L, -L, 8), (L, -L, 8), (L, L, 8), (-L, L, 8)]
    box = [np.array(b, float) for b in box]
    order = []
    for (a, b, c, e), m in [((0, 1, 2, 3), 2), ((4, 5, 6, 7), 1), ((0, 1, 5, 4), 2), ((3, 2, 6, 7), 0), ((0, 3, 7, 4), 1), ((1, 2, 6, 5), 2)]:
        order.append((box[a], box[b], box[c], m))
        order.append((box[a], box[c], box[e], m))
    smalls = []
    for k in range(n_small):
        p = rng.uniform(-6, 6, 3) + [0, 0, -6]
        size = rng.choice([0.05, 0.3, 1.0])
        q, r = p + rng.normal(size=3) * size, p + rng.normal(size=3) * size
        if k % 17 == 0:
            r = p + (q - p) * rng.uniform(0.2, 0.8) + rng.normal(size=3) * 1e-4       # a sliver
        smalls.append((p, q, r, int(rng.integers(1 if few_emitters else 0, 4))))
    larges = []
    for k in range(n_large):
        p = rng.uniform(-8, 8, 3) + [0, 0, -8]
        larges.append((p, p + rng.normal(size=3) * 6, p + rng.normal(size=3) * 6, 0 if few_emitters and k < 2 else int(rng.integers(1, 3))))
    everything = [(t, rng.random() < 0.5) for t in order + smalls + larges]
    idx = rng.permutation(len(everything))
    everything = [everything[i] for i in idx]                      # classes interleave: many clusters
    for i in range(n_dup):                                        # exact duplicates and coplanar overlaps: ties
        (p, q, r, m), vn = everything[int(rng.integers(0, len(everything)))]
        everything.insert(int(rng.integers(0, len(everything))), ((p, q, r, (m % 3) + 1 if few_emitters else (m + 1) % 4), False))
        everything.append(((p, q, p + (r - p) * 0.7 + (q - p) * 0.1, m), False))
    for (p, q, r, m), vn in everything:
        tri(np.asarray(p, float), np.asarray(q, float), np.asarray(r, float), m, vn)
    open(d + "f.obj", "w").write("\n".join(lines) + "\n")
    return len(everything)


def _sliver_scene(d, n_small, seed):
    """An OPEN scene whose paths can leave the culling envelope: n_small random triangles around (0, 0, -6), every 17th a sliver (the
    recipe of tests/test_gpu_fuzz.py), one triangle whose vertices are exactly collinear, six large ones, an emitter among them."""
    rng = np.random.default_rng(seed)
    open(d + "f.mtl", "w").write("newmtl 0\nKe 1 1 1\nKd 0.9 0.7 0.5\nnewmtl 1\nNs 300\nKs 0.7 0.7 0.7\nKd 0.6 0.6 0.6\nnewmtl 2\nNs 0\nKd 0.8 0.3 0.3\n")
    tris = [((1.0, 1.0, -6.0), (2.0, 1.0, -6.0), (1.5, 1.0, -6.0), 2)]
    for k in range(n_small):
        p = rng.uniform(-6, 6, 3) + [0, 0, -6]
        size = rng.choice([0.05, 0.3, 1.0])
        q, r = p + rng.normal(size=3) * size, p + rng.normal(size=3) * size
        if k % 17 == 0:
            r = p + (q - p) * rng.uniform(0.2, 0.8) + rng.normal(size=3) * 1e-4
        tris.append((p, q, r, int(rng.integers(1, 3))))
    for k in range(6):
        p = rng.uniform(-8, 8, 3) + [0, 0, -4]
        tris.append((p, p + rng.normal(size=3) * 6, p + rng.normal(size=3) * 6, 0 if k == 0 else int(rng.integers(1, 3))))
    lines = ["mtllib f.mtl", "vn 0.0 0.0 -1.0"]
    for i, (p, q, r, m) in enumerate(tris):
        lines += ["v %.6f %.6f %.6f" % tuple(v) for v in (p, q, r)] + ["usemtl %d" % m]
        lines.append("f %d//1 %d//1 %d//1" % (3 * i + 1, 3 * i + 2, 3 * i + 3) if i == 0 else "f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    open(d + "f.obj", "w").write("\n".join(lines) + "\n")
    return len(tris)


# ---- the room of tests/test_gpu_glass.py ---------------------------------------------------------------------------------------------
MTL = ("newmtl 0\nKe 3 3 3\nKd 1 1 1\nnewmtl 1\nNs 0\nKd 0.8 0.8 0.8\nnewmtl 2\nNs 300\nKs 0.7 0.7 0.7\nKd 0.6 0.6 0.9\n"
       "newmtl 3\nNs 0\nKd 0.9 0.3 0.3\n")      # 0 the emitter, 1 the walls, 2 and 3 to be glass (their lobes are not looked at)


def _quad(a, b, c, d, m):
    return [(a, b, c, m), (a, c, d, m)]


def _box(lo, hi, m, split=1, inward=False, faces=range(6)):
    """The six faces of a box (or those of `faces`: z0, z1, y0, y1, x0, x1), each cut into split x split quads.  inward: the stored
    normals point into the box, as a room's must -- a scattered ray starts at p + N eps, whichever way N points."""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = np.array([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], np.float64)
    all_faces = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    tris = []
    for f in [all_faces[k] for k in faces]:
        a, b, c, d = v[list(f)]
        at = lambda i, j: tuple(a + (b - a) * (i / split) + (d - a) * (j / split))      # (a face is a parallelogram)
        for i in range(split):
            for j in range(split):
                tris += _quad(at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1), m)
    centre = (np.asarray(lo, np.float64) + np.asarray(hi, np.float64)) / 2
    out = []
    for p, q, r, mm in tris:      # (the reference's normal is (q - p) x (r - p), normalised)
        n = np.cross(np.subtract(q, p), np.subtract(r, p))
        points_in = np.dot(n, centre - np.asarray(p)) > 0
        out.append((p, q, r, mm) if points_in == inward else (p, r, q, mm))
    return out


def _write_obj(d, name, tris):
    open(d + "g.mtl", "w").write(MTL)
    p, q, r, _ = tris[0]          # (the first face names a normal, as the parser wants one: the one its winding gives)
    n = np.cross(np.subtract(q, p), np.subtract(r, p))
    lines = ["mtllib g.mtl", "vn %.6f %.6f %.6f" % tuple(n / np.linalg.norm(n))]
    for i, (p, q, r, m) in enumerate(tris):
        lines += ["v %.6f %.6f %.6f" % tuple(v) for v in (p, q, r)] + ["usemtl %d" % m]
        lines.append("f %d//1 %d//1 %d//1" % (3 * i + 1, 3 * i + 2, 3 * i + 3) if i == 0 else "f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    open(d + name, "w").write("\n".join(lines) + "\n")


EMITTER = _quad((-3.0, 5.5, -9.0), (3.0, 5.5, -9.0), (3.0, 5.5, -3.0), (-3.0, 5.5, -3.0), 0)      # (its normal points down)


def _room():
    """A closed room of 12 x 12 x 28 units around the reference eye (0, 0, -20), its normals inward, with an emitter of 6 x 6 units
    under its ceiling that shines down."""
    return _box((-6.0, -6.0, -22.0), (6.0, 6.0, 6.0), 1, split=2, inward=True) + EMITTER


# ---- geometry within a few eps behind a dielectric surface --------------------------------------------------------------------------
def _sheet(x0, y0, z, m, normal=(0.0, 0.0, -1.0), reverse=False, size=2.0):
    """A size x size quad whose corner (x0, y0, z) and plane normal `normal` are given, wound so that its stored normal is `normal`
    (towards the reference eye for the default), or the opposite with `reverse`."""
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    u = np.cross(n, (0.0, 1.0, 0.0))
    u /= np.linalg.norm(u)          # (+x for the default normal)
    v = np.cross(u, n)              # (+y for the default normal; v x u = n)
    a = np.array((x0, y0, z), np.float64)
    q = _quad(tuple(a), tuple(a + v * size), tuple(a + u * size + v * size), tuple(a + u * size), m)
    return [(p, r, s, mm) for p, s, r, mm in q] if reverse else q


def _pair(x0, y0, z, gap, normal=(0.0, 0.0, -1.0), reverse_second=False, first=2):
    """Two parallel sheets `gap` apart along the normal, the second one behind the first as the eye sees them; materials first, 5 - first."""
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    back = np.array((x0, y0, z)) - n * gap
    return _sheet(x0, y0, z, first, normal) + _sheet(back[0], back[1], back[2], 5 - first, normal, reverse=reverse_second)


def thin_sheets(d, name="thin.obj"):
    """The closed room with six pairs of parallel glass quads that face the eye, 0.5, 1.5, 10 and 1000 eps apart, one pair with the
    second sheet wound the other way and a diffuse quad 1.5 eps behind it, one pair tilted; materials 2 and 3 alternate.  A ray that
    crosses the first sheet starts eps behind it: beyond the second sheet, before it but nearer than eps, or properly in front of it."""
    tris = _room()
    tris += _pair(-4.0, 1.0, -10.0, 0.5 * EPS, first=2) + _pair(-1.0, 1.0, -10.0, 1.5 * EPS, first=3)
    tris += _pair(2.0, 1.0, -10.0, 10 * EPS, first=2) + _pair(-4.0, -3.0, -10.0, 1000 * EPS, first=3)
    tris += _pair(-1.0, -3.0, -10.0, 1.5 * EPS, reverse_second=True, first=2) + _sheet(-1.0, -3.0, -10.0 + 3.0 * EPS, 1)
    tris += _pair(2.0, -3.0, -10.0, 1.5 * EPS, normal=(0.3, 0.2, -1.0), first=3)
    _write_obj(d, name, tris)
    return len(tris)


def shared_faces(d, name="shared.obj", open_room=False):
    """A glass box (material 2) whose bottom lies in the floor's plane and comes BEFORE the floor in the file, so the tie goes to the
    glass; the room; two glass boxes of materials 2 and 3 that share the face x = -1 exactly (coplanar duplicates with opposite
    normals: the lower index, material 2's, wins).  open_room: the room lacks its far wall z = 6 and a box of material 2 reaches from
    z = 4 through the opening to z = 23, beyond every other vertex: rays that leave it there start outside the vertices' bound.
    The box does NOT pierce a wall that is there: a closed wall would cross the box's inside and stop every ray before the part
    beyond it, so nothing would ever start out there.  The whole far wall is left out and the box passes through the opening."""
    tris = _box((2.0, -6.0, -9.0), (4.0, -4.0, -7.0), 2)
    tris += (_box((-6.0, -6.0, -22.0), (6.0, 6.0, 6.0), 1, split=2, inward=True, faces=(0, 2, 3, 4, 5)) + EMITTER) if open_room else _room()
    tris += _box((-3.0, -2.0, -8.0), (-1.0, 0.0, -6.0), 2) + _box((-1.0, -2.0, -8.0), (1.0, 0.0, -6.0), 3)
    if open_room:
        tris += _box((-2.0, 1.0, 4.0), (2.0, 4.0, 23.0), 2)
    _write_obj(d, name, tris)
    return len(tris)


def glass_slivers(d, n_small, seed, name="f.obj", room=False):
    """_sliver_scene's recipe, its random numbers drawn in the same order, with a fourth material (3, to be glass) that the exactly
    collinear triangle and every 17th small triangle -- the slivers -- get.  A sliver 1e-4 units wide is hit a few times per frame, so
    the three small triangles after each sliver are glass too: paths are refracted and reflected AMONG the slivers.  room: the diffuse
    walls (material 2) and the emitter of _room() around it -- the open scene has one emissive triangle and is nearly black without a
    miss shader; this one is lit, so a frame WITHOUT a map or a skybox has something to compare."""
    rng = np.random.default_rng(seed)
    open(d + "f.mtl", "w").write("newmtl 0\nKe 1 1 1\nKd 0.9 0.7 0.5\nnewmtl 1\nNs 300\nKs 0.7 0.7 0.7\nKd 0.6 0.6 0.6\nnewmtl 2\nNs 0\nKd 0.8 0.3 0.3\n"
                                 "newmtl 3\nNs 0\nKd 0.5 0.5 0.5\n")
    tris = [((1.0, 1.0, -6.0), (2.0, 1.0, -6.0), (1.5, 1.0, -6.0), 3)]
    for k in range(n_small):
        p = rng.uniform(-6, 6, 3) + [0, 0, -6]
        size = rng.choice([0.05, 0.3, 1.0])
        q, r = p + rng.normal(size=3) * size, p + rng.normal(size=3) * size
        if k % 17 == 0:
            r = p + (q - p) * rng.uniform(0.2, 0.8) + rng.normal(size=3) * 1e-4
        m = int(rng.integers(1, 3))
        tris.append((p, q, r, 3 if k % 17 < 4 else m))
    for k in range(6):
        p = rng.uniform(-8, 8, 3) + [0, 0, -4]
        tris.append((p, p + rng.normal(size=3) * 6, p + rng.normal(size=3) * 6, 0 if k == 0 else int(rng.integers(1, 3))))
    if room:
        tris += _box((-6.0, -6.0, -22.0), (6.0, 6.0, 6.0), 2, split=2, inward=True) + EMITTER
    lines = ["mtllib f.mtl", "vn 0.0 0.0 -1.0"]
    for i, (p, q, r, m) in enumerate(tris):
        lines += ["v %.6f %.6f %.6f" % tuple(v) for v in (p, q, r)] + ["usemtl %d" % m]
        lines.append("f %d//1 %d//1 %d//1" % (3 * i + 1, 3 * i + 2, 3 * i + 3) if i == 0 else "f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    open(d + name, "w").write("\n".join(lines) + "\n")
    return len(tris)


def write_sky(d):
    """The generated sky bitmap of tools/make_open_scene.py as d + 'sky.bmp'."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_open_scene as MO
    MO.write_sky_bmp(d + "sky.bmp")
    return d + "sky.bmp"


def env_map(seed):
    return np.random.default_rng(seed).uniform(0.05, 2.0, (8, 8, 3)).astype(np.float32)


# ---- what the two tests look at -------------------------------------------------------------------------------------------------------
FUZZ_CONFIGS = [(1, 300, 6, 20, False), (2, 40, 30, 10, False), (3, 3000, 10, 40, False), (4, 3000, 12, 30, True), (5, 300, 8, 20, True)]
# (configurations 1-5 of tests/test_gpu_fuzz._configs(); tests/test_glass_fuzz_host.py compares)
TINT = (0.8, 0.0, 0.9)                                      # the tint with a zero channel
FUZZ_GLASS = {"m1": {1: (1.5, (1.0, 1.0, 1.0))}, "m3": {3: (0.67, TINT)},
              "m123": {1: (1.5, (1.0, 0.9, 0.8)), 2: (0.67, (0.9, 1.0, 0.9)), 3: (1.5, TINT)}}
SHEET_GLASS = {2: (1.5, (1.0, 0.9, 0.8)), 3: (0.67, TINT)}
SLIVER_GLASS = {3: (1.5, TINT)}
SHAPES = [(40, 28), (17, 9)]
SPP, MRR = 4, 8

# name -> (generator call, file name, glass, open?)
SCENES = {"thin_sheets": (lambda d: thin_sheets(d), "thin.obj", SHEET_GLASS, False),
          "shared_faces": (lambda d: shared_faces(d), "shared.obj", SHEET_GLASS, False),
          "shared_faces_open": (lambda d: shared_faces(d, open_room=True), "shared.obj", SHEET_GLASS, True),
          "glass_slivers_300": (lambda d: glass_slivers(d, 300, seed=300), "f.obj", SLIVER_GLASS, True),
          "glass_slivers_3000": (lambda d: glass_slivers(d, 3000, seed=3000), "f.obj", SLIVER_GLASS, True),
          # (only in ADAPTIVE: the slivers inside the lit closed room)
          "glass_slivers_room_300": (lambda d: glass_slivers(d, 300, seed=300, room=True), "f.obj", SLIVER_GLASS, False),
          "glass_slivers_room_3000": (lambda d: glass_slivers(d, 3000, seed=3000, room=True), "f.obj", SLIVER_GLASS, False)}
for _cfg in FUZZ_CONFIGS:
    SCENES["fuzz%d" % _cfg[0]] = ((lambda d, c=_cfg: _random_scene(d, *c)), "f.obj", None, False)

# The events (glass_composition.EVENTS) each scene is there to produce, summed over its frames of cases(); both tests assert them > 0.
REQUIRED = {
    "thin_sheets": ("entering", "leaving", "total_reflections", "partial_reflections", "transmissions", "near_hits", "last_on_glass"),
    "shared_faces": ("entering", "leaving", "total_reflections", "partial_reflections", "transmissions", "material_ties", "last_on_glass"),
    "shared_faces_open": ("entering", "leaving", "transmissions", "material_ties", "origins_beyond_vertices"),
    "glass_slivers_300": ("entering", "leaving", "partial_reflections", "transmissions", "near_hits"),
    "glass_slivers_3000": ("entering", "leaving", "partial_reflections", "transmissions", "near_hits"),
    "fuzz1": ("entering", "leaving", "total_reflections", "partial_reflections", "transmissions", "material_ties", "near_hits"),
    "fuzz2": ("entering", "leaving", "total_reflections", "partial_reflections", "transmissions", "material_ties", "near_hits"),
    "fuzz3": ("entering", "leaving", "total_reflections", "partial_reflections", "transmissions", "material_ties", "near_hits"),
    "fuzz4": ("entering", "leaving", "total_reflections", "partial_reflections", "transmissions", "material_ties", "near_hits",
              "last_on_glass"),      # (its frames at -MRR 1 and 2: elsewhere few paths are still alive on their eighth segment)
    "fuzz5": ("entering", "leaving", "total_reflections", "partial_reflections", "transmissions", "material_ties", "near_hits"),
}

VIEWS = ("free", "camera", "fisheye")
ROOM_CAMERA = dict(eye=(4.0, 3.0, -19.0), target=(0.0, 0.0, -8.0), up=(0.0, 1.0, 0.0))
SLIVER_CAMERA = dict(eye=(3.0, 2.0, -22.0), target=(0.0, 0.0, -6.0), up=(0.0, 1.0, 0.0))
BIG = ("fuzz3", "fuzz4", "glass_slivers_3000", "glass_slivers_room_3000")      # more than BIG_SCENE_TRIANGLES triangles: the 40 x 28 frame is sampled


def view_of(pt, scene_name, view, w, h):
    """(camera or None, projection or None, the composition's keywords) of `view` for a scene of CASES."""
    if view == "free":
        return None, None, {}
    c = SLIVER_CAMERA if scene_name.startswith("glass_slivers") else ROOM_CAMERA
    cam = pt.look_at(c["eye"], c["target"], c["up"], fov_y=60.0, aspect=w / h)
    if view == "camera":
        return cam, None, dict(camera=cam.as_array())
    prj = pt.projection("fisheye", fov_y=170.0, aspect=w / h)
    return cam, prj, dict(camera=cam.as_array(), projection=(prj.kind, prj.span_x, prj.span_y))


def pixels_of(scene_name, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    px = np.stack([xs.ravel(), ys.ravel()], 1)
    return px[::3] if scene_name in BIG and w * h > 200 else px


def cases():
    """Every frame both tests look at: dicts of id, scene, glass_id, glass, view, miss ('none' / 'environment' / 'skybox'), w, h, mrr."""
    out = []
    for cfg in FUZZ_CONFIGS:
        name = "fuzz%d" % cfg[0]
        for gid, glass in FUZZ_GLASS.items():
            for w, h in SHAPES:
                for mrr in ((1, 2, MRR) if cfg[0] == 4 else (MRR,)):      # the few-emitter box-tree scene: the last-segment filter is on
                    out.append(dict(scene=name, glass_id=gid, glass=glass, view="free", miss="none", w=w, h=h, mrr=mrr))
    for name in ("thin_sheets", "shared_faces", "shared_faces_open", "glass_slivers_300", "glass_slivers_3000"):
        glass, is_open = SCENES[name][2], SCENES[name][3]
        for view in VIEWS:
            for miss in (("environment", "skybox") if is_open else ("none",)):
                for w, h in SHAPES:
                    out.append(dict(scene=name, glass_id="own", glass=glass, view=view, miss=miss, w=w, h=h, mrr=MRR))
    for c in out:
        c["id"] = "%s-%s-%s-%s-%dx%d-mrr%d" % (c["scene"], c["glass_id"], c["view"], c["miss"], c["w"], c["h"], c["mrr"])
    return out


ENV_SEED = 11


def compose_case(pt, case, osc, sky_path, **flaw):
    """glass_composition.compose of one of cases() on the oracle scene `osc`: (sum, sum2, count, tainted), the pixels, the statistics
    and the events.  `flaw`: compose's keywords for a deliberate error (the events are then not counted)."""
    import glass_composition as GC
    px = pixels_of(case["scene"], case["w"], case["h"])
    kw = view_of(pt, case["scene"], case["view"], case["w"], case["h"])[2]
    osc.set_skybox(sky_path if case["miss"] == "skybox" else None)
    stats, events = {}, None if flaw else {}
    try:
        r = GC.compose(osc, case["glass"], env_map(ENV_SEED) if case["miss"] == "environment" else None, case["w"], case["h"], px, SPP,
                       case["mrr"], stats=stats, events=events, want_tainted=True, **kw, **flaw)
    finally:
        osc.set_skybox(None)
    return r, px, stats, events


# Adaptive frames at the size at which Tor.obj runs the batch kernels (tests/test_gpu_glass.py: test_adaptive_batches_over_wide_tiles),
# of scenes that need the envelope test, which the batch kernels are built without.  Only a launch WITHOUT a map or a skybox, without
# statistics, reaches the clause of plan_tiles that decides on may_leave_envelope (a launch with either is planned as a skybox launch,
# which never runs batches): miss 'none'.  The open sliver scene is nearly black there, so the slivers also stand in the lit closed
# room, on the sphere trees and on the box tree; the frame under the map stays as one more adaptive frame of the envelope-test kernels.
_ADAPTIVE = dict(glass=SLIVER_GLASS, w=200, h=144, spp=14, mrr=3, error=0.05, n_pixels=40)
ADAPTIVE = [dict(_ADAPTIVE, id="%s-%s" % (name, miss), scene=name, miss=miss, n_pixels=n) for name, miss, n in
            (("glass_slivers_300", "none", 40), ("glass_slivers_300", "environment", 40), ("glass_slivers_room_300", "none", 200),
             ("glass_slivers_room_3000", "none", 200))]      # (at -MRR 3 a room pixel in three contributes: more of them)


def compose_adaptive(a, osc):
    """(sum, sum2, count, tainted), the pixels and the events of one of ADAPTIVE."""
    import glass_composition as GC
    rng = np.random.default_rng(0)
    px = np.unique(np.stack([rng.integers(0, a["w"], a["n_pixels"]), rng.integers(0, a["h"], a["n_pixels"])], 1), axis=0)
    events = {}
    r = GC.compose(osc, a["glass"], env_map(ENV_SEED) if a["miss"] == "environment" else None, a["w"], a["h"], px, a["spp"], a["mrr"],
                   error=a["error"], events=events, want_tainted=True)
    return r, px, events
