"""The device's closest hits and frames at other scene scales and positions (tests/scene_transforms.py: TRANSFORMS).

Every other scene of the suite lies within about 25 units of the origin, so the scale dependence of the culling margins -- the
absolute constants of pt_cull_tables.cpp (r_org's + 1, the envelope's 0.01, m0's 1e-6, t_guard, the absorption bound, disc_err), the
8-bit quantisation of the box tree's nodes and the kernel's envelope test -- went unchecked on the device.  The reference itself
behaves differently there (at 2^10 with the default eps its area test drowns in float error and it accepts barely half of the
aimed rays), and the library promises its bits for any OBJ.  Three scenes -- Tor.obj (sphere trees, large class), its x9
replica (box tree) and the fuzz scene of seed 1 (slivers, duplicates, vn) -- are scaled by 2^-10 ... 2^10 and shifted by up to
4096:

  * test_closest_hits: 20 000 adversarial rays against the oracle's all-triangles loop, index and distance bits;
  * test_every_segment: a small frame from the transformed reference camera, every segment against the all-triangles loop on
    the device, on both verification builds, and the product's frame = theirs, for both small-scene tile variants;
  * test_frame_equals_the_composition: that frame against the oracle's parts chained on the host (tests/view_composition.py);
  * test_the_checks_bite: the negative control -- a margin family tightened must show as differing rays on transformed scenes.

The measured shares and the control's outcome are recorded in profiles/r06_scene_scales.txt."""
import importlib
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import scene_transforms as S

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENES = ["tor", "x9", "fuzz1"]
FILE = {"tor": "Tor.obj", "x9": "x9.obj", "fuzz1": "f.obj"}
# the box interior origins are drawn from, in the plain scene's units: just inside the room (the fuzz scenes' room is
# [-9, 9] x [-9, 9] x [-24, 8])
PLAIN_BOX = {"tor": (S.PLAIN_LO, S.PLAIN_HI), "x9": (S.PLAIN_LO, S.PLAIN_HI), "fuzz1": ((-8.9, -8.9, -23.9), (8.9, 8.9, 7.9))}
N_PER_FAMILY = 4000
LATTICE = {"tor": 9, "x9": 9, "fuzz1": 8}      # half-width of the lattice family's origins, in steps: inside the room

EPS_CASES = [(tr, scaled) for tr in S.TRANSFORMS for scaled in ((False, True) if tr[0] != 1.0 else (False,))]
EPS_IDS = [S.transform_id(tr) + ("-eps*scale" if scaled else "-eps1e-4") for tr, scaled in EPS_CASES]
TR_IDS = [S.transform_id(tr) for tr in S.TRANSFORMS]


class Workloads:
    """Transformed scene files, their oracle scenes, rays and the oracle's answers, each made once (needs no GPU)."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.plain, self.dirs, self.oracle, self.rays_, self.hits_ = {}, {}, {}, {}, {}

    def plain_dir(self, kind):
        if kind not in self.plain:
            d = os.path.join(self.tmp, "plain_" + kind, "")
            if kind == "tor":
                d = os.path.join(ROOT, "models", "")
            elif kind == "x9":
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import make_replicated_scene as M
                assert M.generate(os.path.join(ROOT, "models"), d, "x9.obj", 9) == 2318
            else:
                import test_gpu_fuzz as F
                os.makedirs(d)
                F._random_scene(d, 1, 300, 6, 20)
            self.plain[kind] = d
        return self.plain[kind]

    def scene_dir(self, kind, tr):
        if (kind, tr) not in self.dirs:
            out = os.path.join(self.tmp, f"{kind}_{S.TRANSFORMS.index(tr)}")
            self.dirs[kind, tr] = S.transformed(self.plain_dir(kind), FILE[kind], out, *tr)
        return self.dirs[kind, tr]

    def oracle_scene(self, kind, tr):
        if (kind, tr) not in self.oracle:
            self.oracle[kind, tr] = O.Scene.load(self.scene_dir(kind, tr), FILE[kind])
        return self.oracle[kind, tr]

    def box(self, kind, tr):
        lo, hi = PLAIN_BOX[kind]
        off = np.asarray(tr[1], np.float64)
        return np.asarray(lo) * tr[0] + off, np.asarray(hi) * tr[0] + off

    def rays(self, kind, tr):
        """The five adversarial families, 4 000 rays each, in the transformed scene's box and unit -- and, where the closed room
        leaves fewer than 100 of them without a hit at either eps, 500 rays that start outside the room and point away (twice,
        from farther out, where the first 500 do not miss either)."""
        if (kind, tr) not in self.rays_:
            o_scene = self.oracle_scene(kind, tr)
            tri, _ = o_scene.triangles()
            lo, hi = self.box(kind, tr)
            rng = np.random.default_rng(31 + SCENES.index(kind))
            o, d = S.adversarial_rays(tri, rng, N_PER_FAMILY, lo, hi, unit=tr[0], origin=tr[1], lattice=LATTICE[kind])
            # Half a unit outside the room; and where that is not enough -- at 2^-10 with the default eps the reference accepts a
            # plane crossing up to eps / edge = 0.1, a hundred of the scene's units, beyond a torus triangle, farther beyond a sliver -- from 10.0
            # in absolute units, half the floor of r_max, which a scene that small still has inside its envelope of origins.
            for distance in (0.5 * tr[0], 10.0):
                misses = min(int(((ri < 0) & ~nan).sum()) for ri, _, nan in (o_scene.closest_hits(o, d, e) for e in {1e-4, 1e-4 * tr[0]}))
                if misses < 100:
                    o2, d2 = S.rays_pointing_away(rng, 500, lo, hi, distance)
                    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
            self.rays_[kind, tr] = (o, d)
        return self.rays_[kind, tr]

    def hits(self, kind, tr, eps):
        if (kind, tr, eps) not in self.hits_:
            self.hits_[kind, tr, eps] = self.oracle_scene(kind, tr).closest_hits(*self.rays(kind, tr), eps)
        return self.hits_[kind, tr, eps]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    assert pt.device_count() >= 1, "no HIP device: the integrator has no CPU fallback"
    return Workloads(str(tmp_path_factory.mktemp("scales")))


def oracle_conditions(hits):
    """The conditions the oracle alone must meet for a case to say anything: (nan_seen share, hits, misses among the compared
    rays)."""
    ri, rt, nan = hits
    return float(nan.mean()), int(((ri >= 0) & ~nan).sum()), int(((ri < 0) & ~nan).sum())


def differing_rays(g, work, kind, tr, eps):
    """test_closest_hits' comparison: the rays whose index or distance bits differ from the oracle's, nan_seen rays excepted."""
    o, d = work.rays(kind, tr)
    ri, rt, nan = work.hits(kind, tr, eps)
    nan_share, n_hits, n_misses = oracle_conditions((ri, rt, nan))
    print(f"{kind} {S.transform_id(tr)} eps {eps:g}: {len(o)} rays, hit share {(ri >= 0).mean():.4f}, nan_seen share {nan_share:.5f}, "
          f"compared {int((~nan).sum())} ({n_hits} hits, {n_misses} misses)")
    assert nan_share < 0.01 and n_hits >= 100 and n_misses >= 100
    gi, gt = g.trace_rays(o, d, eps)
    return np.flatnonzero(((gi != ri) | (gt.view(np.uint32) != rt.view(np.uint32))) & ~nan), (gi, gt, ri, rt)


@pytest.mark.parametrize("tr,scaled", EPS_CASES, ids=EPS_IDS)
@pytest.mark.parametrize("kind", SCENES)
def test_closest_hits(work, kind, tr, scaled):
    eps = 1e-4 * tr[0] if scaled else 1e-4
    g = pt.Scene.load_obj(work.scene_dir(kind, tr), FILE[kind], device=0)
    bad, (gi, gt, ri, rt) = differing_rays(g, work, kind, tr, eps)
    o, d = work.rays(kind, tr)
    assert bad.size == 0, (f"{bad.size} of {len(o)} rays differ; first: ray {bad[0]} o={o[bad[0]]} d={d[bad[0]]} "
                           f"gpu=({gi[bad[0]]},{gt[bad[0]]}) oracle=({ri[bad[0]]},{rt[bad[0]]})")


def _same_bits(a, b):
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            and np.array_equal(a[2], b[2]))


@pytest.mark.parametrize("tr", S.TRANSFORMS, ids=TR_IDS)
@pytest.mark.parametrize("kind", SCENES)
def test_every_segment(work, kind, tr):
    """64 x 48 x 8 spp, MRR 8, eps 1e-4 from the transformed reference camera: every segment against the all-triangles loop on
    the device -- the statistics instantiations (libpt_verify.so) and the ones that ship (libpt_verify_shipped.so) --, the
    product's frame with and without statistics = the verified frames, and the same through the hook builds with the tile
    width pinned, so that both the 16 x 8 (2) and the 8 x 8 (1) small-scene kernels run."""
    W, H, spp, mrr = 64, 48, 8, 8
    d, name = work.scene_dir(kind, tr), FILE[kind]
    cam = S.camera_for(tr[0], tr[1], W, H)
    lib_dir = os.path.dirname(pt.LIB_PATH)
    verify = pt.load_library(pt.VERIFY_LIB_PATH)
    vship = pt.load_library(os.path.join(lib_dir, "libpt_verify_shipped.so"))
    hooks = pt.load_library(pt.TESTHOOKS_LIB_PATH)

    def frame(L, want_stats, tile_width=None):
        if L is not None:
            L.pt_test_set_mutation(b"reset", 0.0)
            if tile_width is not None:
                L.pt_test_set_mutation(b"tile_width", float(tile_width))
        try:
            g = pt.Scene.load_obj(d, name, device=0, library=L)
            g.set_camera(cam)
            return g.render_host(W, H, spp, mrr, eps=1e-4, want_stats=want_stats)
        finally:
            if L is not None:
                L.pt_test_set_mutation(b"reset", 0.0)

    full = frame(verify, True)
    st = full[3]
    print(f"{kind} {S.transform_id(tr)}: segments {st['segments']}, verify_checked {st['verify_checked']}, mismatches {st['verify_mismatches']}")
    assert st["verify_checked"] == st["segments"] >= W * H * spp
    assert st["verify_mismatches"] == 0
    shipped = frame(vship, True)
    assert shipped[3]["verify_checked"] == st["segments"] and shipped[3]["verify_mismatches"] == 0
    assert _same_bits(shipped, full)
    product = frame(None, True)
    assert product[3]["segments"] == st["segments"] and product[3]["verify_checked"] == 0
    assert _same_bits(product, full) and _same_bits(frame(None, False), full)
    for tile_width in (2, 1):
        assert _same_bits(frame(hooks, False, tile_width), full), tile_width
        v = frame(vship, True, tile_width)
        assert _same_bits(v, full) and v[3]["verify_checked"] == st["segments"] and v[3]["verify_mismatches"] == 0, tile_width


@pytest.mark.parametrize("tr", S.TRANSFORMS, ids=TR_IDS)
def test_frame_equals_the_composition(work, tr):
    """Tor.obj, 24 x 16 x 4 spp, MRR 8: every pixel's sum, sum2 and count = the oracle's parts chained on the host for the
    transformed camera.  This ties the device to the oracle and not only to its own all-triangles loop."""
    import view_composition as V
    W, H, spp, mrr = 24, 16, 4, 8
    cam = S.camera_for(tr[0], tr[1], W, H)
    g = pt.Scene.load_obj(work.scene_dir("tor", tr), FILE["tor"], device=0)
    g.set_camera(cam)
    px = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)
    want = V.compose(work.oracle_scene("tor", tr), W, H, px, spp, mrr, camera=cam.as_array())
    for want_stats in (True, False):
        got = g.render_host(W, H, spp, mrr, want_stats=want_stats)
        assert _same_bits(got, want), want_stats
        assert not want_stats or got[3]["segments"] >= W * H * spp
    # (at 2^-10 with the default eps the reference accepts the nearest plane crossing of almost every ray, no path reaches the
    # light and the frame is empty -- in the oracle and on the device alike)
    assert want[2].sum() > 0 or tr == S.TRANSFORMS[0]


# the negative control: (scene, margin family) -> the transforms it is run at.  Tor.obj has no box tree, so the leaf boxes are
# tightened under the x9 replica
CONTROL_TRANSFORMS = [S.TRANSFORMS[3], S.TRANSFORMS[6]]
CONTROL = [("tor", "sphere_r2"), ("x9", "box")]
LADDER = [0.98, 0.9, 0.5]


def first_noticed(work, hooks, kind, family, tr, eps=1e-4):
    """The largest scale of LADDER at which `family`, tightened, shows as differing rays: (scale, differing rays), or (None, 0)."""
    for scale in LADDER:
        hooks.pt_test_set_mutation(b"reset", 0.0)
        hooks.pt_test_set_mutation(family.encode(), scale)
        try:
            g = pt.Scene.load_obj(work.scene_dir(kind, tr), FILE[kind], device=0, library=hooks)
            bad, _ = differing_rays(g, work, kind, tr, eps)
        finally:
            hooks.pt_test_set_mutation(b"reset", 0.0)
        print(f"control {kind} {S.transform_id(tr)} {family} x {scale}: {bad.size} differing rays")
        if bad.size:
            return scale, int(bad.size)
    return None, 0


# What the first run on an MI355X showed (profiles/r06_scene_scales.txt), pinned: the largest scale of the ladder at which the
# family is noticed.  On the small scene far from the origin the spheres' r^2 is mostly disc_err, the allowance for the float error
# of |m|^2 - (m.d)^2 at r_org = 101.6 (0.18, against a triangle's own r^2 of about 0.001): the cull has room there that it does
# not have on the plain scene, 0.98 and 0.9 go unnoticed and 0.5 is the largest scale of {0.9, 0.5} that is.
NOTICED_AT = {("tor", "sphere_r2", S.TRANSFORMS[3]): 0.98, ("tor", "sphere_r2", S.TRANSFORMS[6]): 0.5,
              ("x9", "box", S.TRANSFORMS[3]): 0.98, ("x9", "box", S.TRANSFORMS[6]): 0.98}


@pytest.mark.parametrize("tr", CONTROL_TRANSFORMS, ids=[S.transform_id(tr) for tr in CONTROL_TRANSFORMS])
@pytest.mark.parametrize("kind,family", CONTROL)
def test_the_checks_bite(work, kind, family, tr):
    """After test_gpu_mutation.py: with the bounding spheres' r^2, then the leaf boxes' half-extents, scaled down through the
    test-hook build, test_closest_hits' comparison must find differing rays -- and, as shipped, none."""
    hooks = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    hooks.pt_test_set_mutation(b"reset", 0.0)
    g = pt.Scene.load_obj(work.scene_dir(kind, tr), FILE[kind], device=0, library=hooks)
    assert differing_rays(g, work, kind, tr, 1e-4)[0].size == 0
    scale, n = first_noticed(work, hooks, kind, family, tr)
    assert scale is not None, f"{family} tightened to {LADDER[-1]} went unnoticed"
    assert scale == NOTICED_AT[kind, family, tr], f"{family} is first noticed at {scale} ({n} rays), not at {NOTICED_AT[kind, family, tr]}"
