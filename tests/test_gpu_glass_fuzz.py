"""The dielectric kernels on the scenes that were built to break the search, bit for bit against tests/glass_composition.py: the
randomised scenes of tests/test_gpu_fuzz.py (slivers, exact duplicates and coplanar overlaps of DIFFERENT materials, where the
lowest-index tie decides whether a hit is glass at all; vertex normals that disagree with the winding; the few-emitter box-tree
scene with the last-segment filter on) with materials {1}, {3} and {1, 2, 3} as glass, and three scenes that put geometry within a
few eps behind a dielectric surface (tests/glass_fuzz_scenes.py: thin_sheets, shared_faces, glass_slivers).  Every frame of
glass_fuzz_scenes.cases() is compared (sum, sum2, count) over the pixels the composition does not mark `tainted` (a segment lay
exactly in a stored plane: the library's documented deviation); tests/test_glass_fuzz_host.py checks on the CPU that these are at most
2 % of any frame and that the frames tell a flawed reference from the true one; both tests assert that each scene produces the events
it is there for (glass_fuzz_scenes.REQUIRED).
Each frame with statistics (the counters too, where nothing is tainted) and without; the random scenes also through the test-hook build
with 16 x 8 tiles and through both verification builds (every segment against the all-triangles loop: no mismatch)."""
import importlib
import os

import numpy as np
import pytest

import glass_fuzz_scenes as S
import oracle_lib as O

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = S.cases()
LIB_DIR = os.path.dirname(pt.LIB_PATH)
LIBS = {"shipped": None, "hooks": pt.TESTHOOKS_LIB_PATH, "verify_shipped": os.path.join(LIB_DIR, "libpt_verify_shipped.so"), "verify": pt.VERIFY_LIB_PATH}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    assert pt.device_count() >= 1, "no HIP device: the integrator has no CPU fallback"


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """(name, library key) -> (directory, oracle scene, handle loaded through that library), made when first asked for."""
    files, handles = {}, {}

    def get(name, lib="shipped"):
        if name not in files:
            d = str(tmp_path_factory.mktemp(name)) + "/"
            n = S.SCENES[name][0](d)
            S.write_sky(d)
            files[name] = (d, O.Scene.load(d, S.SCENES[name][1]), n)
        d, osc, n = files[name]
        if (name, lib) not in handles:
            L = pt.load_library(LIBS[lib]) if LIBS[lib] else None
            handles[name, lib] = pt.Scene.load_obj(d, S.SCENES[name][1], device=0, library=L)
            assert handles[name, lib].counts()[0] == n == osc.n_tri
        return d, osc, handles[name, lib]
    yield get
    for h in handles.values():
        h.close()


@pytest.fixture(scope="module")
def composed(scenes):
    done = {}

    def get(case):
        if case["id"] not in done:
            d, osc, _ = scenes(case["scene"])
            done[case["id"]] = S.compose_case(pt, case, osc, d + "sky.bmp")
        return done[case["id"]]
    return get


def _entries(glass):
    return [pt.dielectric(m, ior, tint) for m, (ior, tint) in glass.items()]


def _reset(scene):
    scene.set_projection(None); scene.set_camera(None); scene.set_environment(None); scene.set_skybox(None); scene.set_dielectrics(None)


def _dress(scene, d, case):
    """The case's view, miss shader and dielectric list on the handle."""
    _reset(scene)
    cam, prj, _ = S.view_of(pt, case["scene"], case["view"], case["w"], case["h"])
    if cam is not None:
        scene.set_camera(cam)
    if prj is not None:
        scene.set_projection(prj)
    if case["miss"] == "environment":
        scene.set_environment_map(S.env_map(S.ENV_SEED))
    elif case["miss"] == "skybox":
        scene.set_skybox(d + "sky.bmp")
    scene.set_dielectrics(_entries(case["glass"]))


def _equal(got, ref, px, w, what):
    """The frame `got` equals the composition `ref` at the untainted pixels of `px`."""
    s, s2, c, tainted = ref
    i, keep = px[:, 1] * w + px[:, 0], ~tainted
    n_bad = int(((got[2][i] != c) & keep).sum() + ((_bits(got[0].reshape(-1, 3)[i]) != _bits(s)).any(1) & keep).sum() +
                ((_bits(got[1].reshape(-1, 3)[i]) != _bits(s2)).any(1) & keep).sum())
    assert n_bad == 0, "%s: %d of %d untainted pixels differ" % (what, n_bad, int(keep.sum()))


def _with_tile_width(L, width, render):
    L.pt_test_set_mutation(b"reset", 0.0)
    L.pt_test_set_mutation(b"tile_width", float(width))
    try:
        return render()
    finally:
        L.pt_test_set_mutation(b"reset", 0.0)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_frames_equal_the_composition(gpu, scenes, composed, case):
    d, osc, scene = scenes(case["scene"])
    ref, px, tally, events = composed(case)
    w, h, mrr = case["w"], case["h"], case["mrr"]
    assert ref[3].mean() <= 0.02
    whole_and_clean = len(px) == w * h and not ref[3].any()
    _dress(scene, d, case)
    try:
        s, s2, c, st = scene.render_host(w, h, S.SPP, mrr, want_stats=True)
        _equal((s, s2, c), ref, px, w, "statistics kernel")
        if whole_and_clean:
            assert (st["samples_traced"], st["segments"], st["misses"], st["contributing"]) == \
                   (tally["samples_traced"], tally["segments"], tally["misses"], tally["contributing"]), (st, tally)
        _equal(scene.render_host(w, h, S.SPP, mrr, want_stats=False), ref, px, w, "statistics-free kernel")
    finally:
        _reset(scene)
    if not case["scene"].startswith("fuzz"):
        return
    # the 16 x 8-tile form of the same kernels (two pixels per lane) through the test-hook build, and every segment against the
    # all-triangles loop in the build that checks the shipped instantiations (16 x 8 tiles too) and in the one that checks its own
    for lib in ("hooks", "verify_shipped", "verify"):
        _, _, sc = scenes(case["scene"], lib)
        L = pt.load_library(LIBS[lib])
        _dress(sc, d, case)
        try:
            render = lambda: sc.render_host(w, h, S.SPP, mrr, want_stats=(lib != "hooks"))
            r = render() if lib == "verify" else _with_tile_width(L, 2, render)
        finally:
            _reset(sc)
        _equal(r, ref, px, w, lib)
        if lib != "hooks":
            assert r[3]["verify_mismatches"] == 0 and r[3]["verify_checked"] > 0, (lib, r[3])
            if whole_and_clean:
                assert r[3]["verify_checked"] == tally["segments"], (lib, r[3], tally)


def test_the_setter_refuses_the_emissive_material_and_the_few_emitter_scene_keeps_its_filter(gpu, scenes):
    _, osc, scene = scenes("fuzz1")
    with pytest.raises(pt.PtError):
        scene.set_dielectrics([pt.dielectric(0, 1.5)])              # material 0 is emissive
    assert scene.dielectrics() == []
    _, osc, g = scenes("fuzz4")                                      # the box-tree kernel's last-segment test is on: every emitter sits in the large class
    tri, tri_mat = osc.triangles()
    assert osc.n_tri > pt.BIG_SCENE_TRIANGLES
    emitters = set(np.flatnonzero((osc.materials()[tri_mat, 3:6] != 0).any(1)).tolist())
    lay = g.cull_layout()
    large = set(int(t) for t in lay["slot_triangle"][(len(lay["bvh"]) - lay["bvh_inner_nodes"]) * 8:] if t >= 0)
    assert 0 < len(emitters) <= 8 and emitters <= large


@pytest.mark.parametrize("name", sorted(S.REQUIRED))
def test_each_scene_produced_the_events_it_is_there_for(gpu, composed, name):
    """The frames compared above met what they were built to meet (the `dup_hits > 0` of tests/test_gpu_fuzz.py): the counters of the
    compositions they were compared with, summed over the scene's frames."""
    total = dict.fromkeys(S.REQUIRED[name], 0)
    for case in CASES:
        if case["scene"] == name:
            for k in total:
                total[k] += composed(case)[3][k]
    assert all(v > 0 for v in total.values()), total


@pytest.mark.parametrize("a", S.ADAPTIVE, ids=[a["id"] for a in S.ADAPTIVE])
def test_adaptive_frames_of_batch_size_on_scenes_that_need_the_envelope_test(gpu, scenes, a):
    """200 x 144 under adaptive sampling is the size at which Tor.obj runs the batch kernels, which are built without the envelope test.
    These scenes have a degenerate triangle.  CullTables::may_leave_envelope itself is not exported; what is observed is the NaN
    barycentric record of that triangle in the handle's cull tables, and a degenerate triangle sets the flag (pt_cull_tables.cpp:
    tri_geometry, cull_record, may_leave_envelope).  Without a map, a skybox or statistics (miss 'none') the launch reaches the
    clause of plan_tiles that must keep such a scene off the batch kernels; the test-hook build's tile widths then choose between the
    8 x 8 and the 16 x 8 form with the envelope test (the box tree has one form).  Under the map the launch is planned as a skybox
    launch, whose kernels never run batches: one more adaptive frame of the envelope-test kernels.  Each frame is the composition."""
    d, osc, scene = scenes(a["scene"])
    assert np.isnan(scene.cull_tables()["bary"][:, 4:]).all(1).any()
    ref, px, events = S.compose_adaptive(a, osc)
    assert ref[3].mean() <= 0.02 and events["transmissions"] > 0 and ref[2].max() <= a["spp"]
    if a["id"] != "glass_slivers_300-none":                           # (the open scene without a miss shader is nearly black)
        assert (ref[2] > 0).sum() >= 10
    render = lambda sc: sc.render_host(a["w"], a["h"], a["spp"], a["mrr"], error=a["error"], want_stats=False)

    def dress(sc):
        _reset(sc)
        if a["miss"] == "environment":
            sc.set_environment_map(S.env_map(S.ENV_SEED))
        sc.set_dielectrics(_entries(a["glass"]))
    dress(scene)
    try:
        _equal(render(scene), ref, px, a["w"], "the plan's own choice")
    finally:
        _reset(scene)
    _, _, sc = scenes(a["scene"], "hooks")
    L = pt.load_library(LIBS["hooks"])
    dress(sc)
    try:
        for width in (1, 2, 3):
            _equal(_with_tile_width(L, width, lambda: render(sc)), ref, px, a["w"], "tile_width %d" % width)
    finally:
        _reset(sc)


@pytest.mark.parametrize("name", ["thin_sheets", "shared_faces", "shared_faces_open", "glass_slivers_300", "glass_slivers_3000"])
def test_a_list_set_and_cleared_leaves_the_bytes_it_found(gpu, scenes, name):
    d, _, scene = scenes(name)
    w, h = S.SHAPES[0]
    _reset(scene)
    if S.SCENES[name][3]:
        scene.set_environment_map(S.env_map(S.ENV_SEED))
    try:
        before = scene.render_host(w, h, S.SPP, S.MRR, want_stats=False)
        scene.set_dielectrics(_entries(S.SCENES[name][2]))
        with_list = scene.render_host(w, h, S.SPP, S.MRR, want_stats=False)
        scene.set_dielectrics(None)
        after = scene.render_host(w, h, S.SPP, S.MRR, want_stats=False)
    finally:
        _reset(scene)
    same = lambda a, b: np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])
    assert same(after, before) and not same(with_list, before)
