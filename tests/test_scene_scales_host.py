"""CPU checks of the culling hierarchy at other scene scales and positions (tests/scene_transforms.py: TRANSFORMS).

The margins of pt_cull_tables.cpp (build_cull_tables, margins) are derived from the scene's extent r_org, and several of their
constants are absolute; every other scene of the suite lies within about 25 units of the origin.  Here Tor.obj and its x9
replica are scaled by 2^-10 ... 2^10 and shifted by up to 4096, and the soundness checks of test_cull_tables_host.py
(tests/cull_checks.py) are asked again, each with the reference's default eps and with eps scaled along with the scene: a
triangle the reference accepts for a ray is never culled for that ray.

What the hierarchy looks like there (recorded with the counts in profiles/r06_scene_scales.txt): the classes follow
r_max = max(20, largest |coordinate|), so a room of any size around the origin keeps its walls in the large class (quad
records), a room far from the origin or much smaller than 20 units has them under sphere trees, and at 2^-10 with the default eps
every triangle's area is below the reference's own threshold: nothing can be bounded, everything is a NaN record that is
always kept, and a big scene has no box tree at all."""
import importlib
import os
import sys

import numpy as np
import pytest

import cull_checks as K
import oracle_lib as O
import scene_transforms as S

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(tr, scaled) for tr in S.TRANSFORMS for scaled in ((False, True) if tr[0] != 1.0 else (False,))]
IDS = [S.transform_id(tr) + ("-eps*scale" if scaled else "-eps1e-4") for tr, scaled in CASES]


def _eps(tr, scaled):
    return 1e-4 * tr[0] if scaled else 1e-4


@pytest.fixture(scope="module")
def scenes(tmp_path_factory, models_dir):
    """(library scene, oracle scene) of the transformed Tor.obj, loaded once per transform."""
    cache = {}

    def get(tr):
        if tr not in cache:
            d = S.transformed(models_dir, "Tor.obj", str(tmp_path_factory.mktemp("tor")), *tr)
            cache[tr] = (pt.Scene.load_obj(d, "Tor.obj", device=-1), O.Scene.load(d, "Tor.obj"))
        return cache[tr]
    return get


@pytest.fixture(scope="module")
def x9_dir(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_replicated_scene as M
    d = str(tmp_path_factory.mktemp("x9")) + "/"
    assert M.generate(os.path.join(ROOT, "models"), d, "x9.obj", 9) == 2318 > pt.BIG_SCENE_TRIANGLES
    return d


def test_transformed_files_round_trip(scenes, oracle_scene):
    """The helper itself: every vertex the loaders read back is float32(float32(x) * scale + offset), normals are untouched."""
    tri, _ = oracle_scene.triangles()
    for tr in S.TRANSFORMS:
        g, o = scenes(tr)
        got, _ = o.triangles()
        assert np.array_equal(got[:, 4:13].reshape(-1, 3).view(np.uint32), S.apply(tri[:, 4:13].reshape(-1, 3), *tr).view(np.uint32))
        assert np.array_equal(g.triangles()[0].view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("tr,scaled", CASES, ids=IDS)
def test_sphere_levels(scenes, tr, scaled):
    """test_accepted_triangles_are_never_culled on the transformed Tor.obj: origins uniform in the transformed box, every accepted
    (ray, triangle) pair passes the cluster sphere and its chain.  16 000 rays: at 2^10 with the default eps the reference
    accepts one aimed ray in six (its area test drowns in float error), and 2 000 accepted pairs are asked of every case."""
    g, o = scenes(tr)
    lo, hi = S.box_for(*tr)
    accepted, dropped = K.sphere_levels(g, o, np.random.default_rng(17), 16000, lo, hi, _eps(tr, scaled))
    print(f"accepted pairs {accepted}, dropped {len(dropped)}")
    assert not dropped, dropped[:3]
    assert accepted >= 2000


@pytest.mark.parametrize("tr,scaled", CASES, ids=IDS)
def test_quad_records(scenes, tr, scaled):
    """The quad check of test_quads_of_the_room_are_fused_and_never_cull_an_accepted_hit with the margins the tables report for
    THIS scene.  The walls are in the large class -- seven fused quads -- where the room is at least as large as the 20-unit
    floor of r_max and centred on the origin; elsewhere their own spheres are below 0.12 r_max and they sit under sphere
    trees, where test_sphere_levels reaches them."""
    g, o = scenes(tr)
    lo, hi = S.box_for(*tr)
    quads, checked, failed = K.quad_records(g, o, np.random.default_rng(23), 600, lo, hi, _eps(tr, scaled))
    print(f"quads {quads}, accepted pairs {checked}, failed {len(failed)}")
    assert not failed, failed[:3]
    if tr[0] >= 1.0 and not any(tr[1]):
        assert quads == 7 and checked >= 2000
    else:
        assert quads == 0


BOX_CASES = [(tr, scaled, mode) for mode in (0, 1) for tr, scaled in CASES if mode == 0 or tr in S.EXTREME_SCALES]
BOX_IDS = [S.transform_id(tr) + ("-eps*scale" if scaled else "-eps1e-4") + ("-sah-collapsed" if mode else "-uniform-depth")
           for tr, scaled, mode in BOX_CASES]


@pytest.mark.parametrize("tr,scaled,bvh_mode", BOX_CASES, ids=BOX_IDS)
def test_box_chain(tmp_path, x9_dir, tr, scaled, bvh_mode, request):
    """test_box_tree_never_drops_the_chain_above_a_hit on the transformed x9 replica; the SAH builder at the two extreme
    scales only."""
    d = S.transformed(x9_dir, "x9.obj", str(tmp_path), *tr)
    hooks = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    hooks.pt_test_set_mutation(b"reset", 0.0)
    hooks.pt_test_set_mutation(b"bvh_mode", float(bvh_mode))
    request.addfinalizer(lambda: hooks.pt_test_set_mutation(b"reset", 0.0))
    g = pt.Scene.load_obj(d, "x9.obj", device=-1, library=hooks)
    o = O.Scene.load(d, "x9.obj")
    eps = _eps(tr, scaled)
    lay = g.cull_layout(eps)
    if tr[0] == 2.0 ** -10 and not scaled:
        # the triangles' areas are below what this eps lets a box or a sphere bound: the builder leaves one empty root and no
        # inner node, and there is no chain that could drop anything
        assert lay["bvh_inner_nodes"] == 0 and len(lay["bvh"]) == 1
        return
    hits, levels, dropped = K.box_chain(g, o, np.random.default_rng(8), 20000, unit=tr[0], eps=eps)
    print(f"hits under the tree {hits}, levels {levels}, dropped {dropped}")
    assert not dropped, f"a node above a hit was dropped (level, form, rays): {dropped}"
    assert hits >= 2000 and levels >= 2


def test_the_scaled_reference_camera_is_accepted(scenes):
    """pt_scene_set_camera: PT_CAMERA_MAX_ORIGIN (4096) is absolute, but an origin within the scene's own vertex extent does not
    enlarge the envelope the margins are derived for.  The 2^10 room reaches |z| = 21 504 and its reference eye is (0, 0, -20480):
    accepted, with the tables the scene has anyway; one beyond the extent is refused as before."""
    for tr in S.TRANSFORMS:
        g, _ = scenes(tr)
        before = g.cull_tables()["constants"]
        g.set_camera(S.camera_for(tr[0], tr[1], 64, 48))
        assert g.cull_tables()["constants"] == before
        g.set_camera(None)
    g, _ = scenes(S.TRANSFORMS[3])
    with pytest.raises(pt.PtError) as e:
        g.set_camera(((0, 0, -21505.0), (1, 0, 0), (0, 1, 0), (0, 0, 1)))
    assert e.value.status == pt.PT_ERR_UNSUPPORTED and g.camera() is None
