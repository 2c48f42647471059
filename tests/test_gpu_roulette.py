"""Russian roulette on the GPU (pt_hip.h: Russian roulette; pt_kernels.hip: integrate_kernel_roulette), bit for bit on sum, sum2 and
count against tests/roulette_composition.py: the direct and the environment-sampling composition with the restated step of
tests/roulette_restatement.py at the end of every scattering step.  40 x 28 x 4 spp (partial edge tiles, several passes per lane, so
that the closed-room kernels regenerate paths) and 5 x 3 (fewer pixels than a wave); through the wide form, the 8 x 8 form and both
batch forms under adaptive sampling (the planner's tile_width override of the test-hook library); the box tree; skybox, environment and
environment sampling; a camera, a lens, a moving camera and a projection; statistics; -MRR 8 and 24, start 1 and 3, floor 1/16 and
1/2.  A start at the cap equals the frame without roulette; the frame is the same under the regen_min_dead hook at 1, 4 and 64; row
bands, a clone and a rehearsed multi-device frame equal the whole frame; both verification builds report no differing search; count is
the number of paths traced; the diagnostic build refuses.  tests/test_roulette_host.py holds the composition itself."""
import importlib
import os

import numpy as np
import pytest

import direct_scenes as DS
import envdirect_scenes as ES
import roulette_composition as RC
import texture_scenes as S

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(got, ref):
    return np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(_bits(got[1]), _bits(ref[1])) and np.array_equal(got[2], ref[2])


@pytest.fixture(scope="module")
def gpu():
    assert pt.device_count() >= 1, "no HIP device: the integrator has no CPU fallback"


def _check(scene, osc, n9, uv, w, h, spp, mrr, roulette, *, rough=None, smooth=False, textures=None, glass=None, env=None, sampling=False, px=None,
           error=-1.0, stats=False, seed=42, **view):
    scene.set_roulette(None)
    scene.set_direct_lighting(False)
    scene.set_roughness(None)
    scene.set_textures([pt.texture(m, t, f) for m, (t, f) in (textures or {}).items()])
    scene.set_dielectrics([pt.dielectric(m, ior, tint) for m, (ior, tint) in (glass or {}).items()])
    scene.set_shading_normals(n9 if smooth else None)
    scene.set_roughness([pt.rough(m, a) for m, a in (rough or {}).items()])
    if sampling:
        scene.set_environment_sampling()
    else:
        scene.set_direct_lighting(True)
    scene.set_roulette(*roulette)
    assert scene.roulette() == (roulette[0], F32(roulette[1]))
    px = S.all_pixels(w, h) if px is None else px
    s, s2, c, st = scene.render_host(w, h, spp, mrr, error=error, seed=seed, want_stats=stats)
    i = px[:, 1] * w + px[:, 0]
    tally = {}
    ws, ws2, wc = RC.compose(osc, rough, n9 if smooth else None, textures, uv, glass, env, w, h, px, spp, mrr, seed=seed, error=error, stats=tally,
                             sampling=sampling, roulette=roulette, **view)
    assert not tally["tainted"].any() and tally["visible_terms"] > 0
    assert np.array_equal(c[i], wc), int((c[i] != wc).sum())
    if error < 0:
        assert (wc == spp).all()                                                    # count = the paths traced
    bad = int((_bits(s.reshape(-1, 3)[i]) != _bits(ws)).any(1).sum())
    assert bad == 0 and np.array_equal(_bits(s2.reshape(-1, 3)[i]), _bits(ws2)), bad
    if stats and len(px) == w * h:
        assert (st["samples_traced"], st["segments"], st["misses"], st["contributing"]) == \
               (tally["samples_traced"], tally["segments"], tally["misses"], tally["contributing"]), (st, tally)
    return tally


@pytest.fixture(scope="module")
def tor(models_dir):
    osc, uv = S.tor(models_dir)
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    n9 = pt.smooth_normals(osc.triangles()[0])
    scene.set_texcoords(uv)
    yield scene, osc, uv, n9
    scene.close()


def _reset(scene):
    scene.set_roulette(None)
    scene.set_environment_sampling(False) if scene.environment() is not None else None
    scene.set_direct_lighting(False)
    scene.set_projection(None); scene.set_camera_motion(None); scene.set_lens(None); scene.set_camera(None)


@pytest.mark.parametrize("mrr,start,floor", [(8, 1, 0.5), (8, 3, 1.0 / 16.0), (24, 1, 1.0 / 16.0), (24, 3, 0.5)])
@pytest.mark.parametrize("shape,stats", [((40, 28), False), ((5, 3), False), ((40, 28), True)])
def test_tor_frames_equal_the_composition(gpu, tor, shape, stats, mrr, start, floor):
    scene, osc, uv, n9 = tor
    _reset(scene)
    tally = _check(scene, osc, n9, uv, shape[0], shape[1], 4, mrr, (start, floor), stats=stats)
    assert tally["roulette_kills"] > 0 and tally["roulette_steps"] >= tally["roulette_draws"]
    _reset(scene)


def test_glass_roughness_shading_normals_and_a_texture(gpu, tor):
    scene, osc, uv, n9 = tor
    _reset(scene)
    tally = _check(scene, osc, n9, uv, 40, 28, 4, 8, (1, 0.5), rough=DS.ROUGH_FLOOR, glass=DS.GLASS_TORUS, smooth=True, textures=DS.TEX_WALL, stats=True)
    assert tally["roulette_kills"] > 0 and tally["rough_steps"] > 0 and tally["cleared_by_glass"] > 0
    scene.set_textures(None); scene.set_dielectrics(None); scene.set_shading_normals(None); scene.set_roughness(None)
    _reset(scene)


@pytest.mark.parametrize("view", DS.VIEWS)
def test_a_camera_a_lens_a_moving_camera_and_a_projection(gpu, tor, view):
    scene, osc, uv, n9 = tor
    _reset(scene)
    tally = _check(scene, osc, n9, uv, 40, 28, 4, 8, (3, 1.0 / 16.0), **S.set_view(pt, scene, view, 40, 28))
    assert tally["roulette_kills"] > 0
    _reset(scene)


@pytest.mark.parametrize("miss", ["skybox", "environment", "environment_sampling"])
def test_under_every_miss_shader_and_environment_sampling(gpu, tmp_path, miss):
    d = str(tmp_path) + "/"
    osc, uv = S.open_tor(d)
    scene = pt.Scene.load_obj(d, "Open.obj", device=0)
    osc.set_skybox(None)
    env = None
    if miss == "skybox":
        scene.set_skybox(d + "sky.bmp")
        osc.set_skybox(d + "sky.bmp")
    else:
        env = ES.MAPS["sun32"]()
        scene.set_environment_map(env)
    try:
        tally = _check(scene, osc, None, uv, 40, 28, 4, 8, (1, 0.5), env=env, sampling=miss == "environment_sampling", stats=True,
                       **S.set_view(pt, scene, "camera", 40, 28))
        assert tally["misses"] > 0 and tally["roulette_kills"] > 0 and (tally["sky_terms"] > 0) == (miss == "environment_sampling")
    finally:
        osc.set_skybox(None)
        scene.close()


# ---- every kernel form (tests/test_gpu_direct.py: the planner's tile_width override of the test-hook library)
@pytest.fixture()
def hooks(gpu):
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    L.pt_test_set_mutation(b"reset", 0.0)
    yield L
    L.pt_test_set_mutation(b"reset", 0.0)


# (shape, spp, mrr, tile_width, error, roulette): the 8 x 8 form, two pixels per lane over 16 x 8 tiles, the batch forms over 16 x 8 and 32 x 8
FORMS = {
    "narrow_8x8": ((40, 28), 4, 8, 1, -1.0, (1, 0.5)),
    "narrow_8x8_5x3": ((5, 3), 4, 24, 1, -1.0, (3, 1.0 / 16.0)),
    "wide_16x8": ((40, 28), 4, 8, 2, -1.0, (1, 0.5)),
    "wide_16x8_deep": ((40, 28), 4, 24, 2, -1.0, (3, 1.0 / 16.0)),
    "wide_16x8_5x3": ((5, 3), 4, 8, 2, -1.0, (1, 1.0 / 16.0)),
    "batch_16x8": ((40, 28), 16, 8, 2, 0.02, (1, 0.5)),
    "batch_32x8": ((40, 28), 16, 8, 3, 0.02, (3, 1.0 / 16.0)),
}


@pytest.mark.parametrize("name", list(FORMS))
def test_tor_frames_through_every_kernel_form_equal_the_composition(hooks, models_dir, tor, name):
    _, osc, uv, n9 = tor
    (w, h), spp, mrr, tile_width, error, roulette = FORMS[name]
    hooks.pt_test_set_mutation(b"tile_width", float(tile_width))
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=hooks)
    scene.set_texcoords(uv)
    tally = _check(scene, osc, n9, uv, w, h, spp, mrr, roulette, error=error)
    assert tally["roulette_kills"] > 0
    scene.close()


@pytest.mark.parametrize("view,tile_width", [("lens", 2), ("shutter", 2), ("camera", 1)])
def test_the_views_of_the_regenerating_closed_room_forms(hooks, models_dir, tor, view, tile_width):
    _, osc, uv, n9 = tor
    hooks.pt_test_set_mutation(b"tile_width", float(tile_width))
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=hooks)
    scene.set_texcoords(uv)
    _check(scene, osc, n9, uv, 40, 28, 4, 8, (1, 0.5), **S.set_view(pt, scene, view, 40, 28))
    scene.close()


def test_box_tree_frames_equal_the_composition(gpu, tmp_path):
    d = str(tmp_path) + "/"
    osc, uv, _ = S.box_tree(d)
    scene = pt.Scene.load_obj(d, "TorX4.obj", device=0)
    assert scene.counts()[0] > pt.BIG_SCENE_TRIANGLES
    px = S.all_pixels(40, 28)[::5]
    tally = _check(scene, osc, None, uv, 40, 28, 4, 8, (1, 0.5), px=px, stats=True)
    assert tally["roulette_kills"] > 0
    scene.close()


def test_a_start_at_the_cap_is_the_frame_without_roulette_and_the_regeneration_threshold_changes_nothing(hooks, models_dir):
    W, H, SPP, MRR = 40, 28, 4, 8
    for tile_width in (1, 2):
        hooks.pt_test_set_mutation(b"reset", 0.0)
        hooks.pt_test_set_mutation(b"tile_width", float(tile_width))
        scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=hooks)
        scene.set_direct_lighting(True)
        direct = scene.render_host(W, H, SPP, MRR, want_stats=False)
        for start in (MRR, MRR + 5):
            scene.set_roulette(start, 0.5)
            assert _same(scene.render_host(W, H, SPP, MRR, want_stats=False), direct), (tile_width, start)
        scene.set_roulette(1, 0.5)
        frames = []
        for dead in (1, 4, 64):
            hooks.pt_test_set_mutation(b"regen_min_dead", float(dead))
            frames.append(scene.render_host(W, H, SPP, MRR, want_stats=False))
        assert not _same(frames[0], direct) and _same(frames[1], frames[0]) and _same(frames[2], frames[0]), tile_width
        assert (frames[0][2] == SPP).all()                                         # count = the paths traced
        scene.close()


def test_bands_a_clone_a_frame_and_the_verification_builds(gpu, models_dir):
    W, H, SPP, MRR = 40, 28, 4, 8
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    scene.set_direct_lighting(True)
    direct = scene.render_host(W, H, SPP, MRR, want_stats=False)
    scene.set_roulette(1, 0.5)
    one = scene.render_host(W, H, SPP, MRR, want_stats=False)
    assert not _same(one, direct) and (one[2] == SPP).all()
    parts = [scene.render_host(W, H, SPP, MRR, rows=r, want_stats=False) for r in ((0, 8), (8, H))]
    assert _same([np.concatenate([p[k] for p in parts]) for k in range(3)], one)
    clone = scene.clone_to_device(0)
    assert clone.roulette() == (1, F32(0.5)) and clone.direct_lighting()
    assert _same(clone.render_host(W, H, SPP, MRR, want_stats=False), one)
    clone.close()
    g = pt.Frame(scene, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)                  # an interleaved frame made from the scene: inherits the setting
    assert g.roulette() == (1, F32(0.5))
    g.render(0, SPP, MRR, error=-1.0)
    assert _same(g.read(), one)
    g.clear()
    with pytest.raises(pt.PtError):
        g.set_direct_lighting(False)
    g.set_roulette(None)
    g.render(0, SPP, MRR, error=-1.0)
    assert _same(g.read(), direct)
    g.clear()
    g.set_roulette(1, 0.5)
    g.render(0, SPP, MRR, error=-1.0)
    assert _same(g.read(), one)
    g.close()
    scene.set_roulette(None)
    assert _same(scene.render_host(W, H, SPP, MRR, want_stats=False), direct)
    scene.close()
    for path in (pt.VERIFY_LIB_PATH, os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_verify_shipped.so")):
        L = pt.load_library(path)
        for tile_width in (1, 2):
            L.pt_test_set_mutation(b"reset", 0.0)
            L.pt_test_set_mutation(b"tile_width", float(tile_width))
            sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=L)
            sc.set_direct_lighting(True)
            sc.set_roulette(1, 0.5)
            r = sc.render_host(W, H, SPP, MRR, want_stats=True)
            sc.close()
            assert r[3]["verify_checked"] > W * H * SPP * 2 and r[3]["verify_mismatches"] == 0, (path, tile_width, r[3])
            assert _same(r, one), (path, tile_width)
        L.pt_test_set_mutation(b"reset", 0.0)


def test_the_phase_timer_build_refuses_a_handle_with_roulette(gpu, models_dir):
    L = pt.load_library(os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_phase.so"))
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=L)
    sc.set_direct_lighting(True)
    sc.set_roulette(3)
    with pytest.raises(pt.PtError) as e:
        sc.render_host(24, 20, 2, 4, want_stats=False)
    assert e.value.status == 7                                                     # PT_ERR_UNSUPPORTED
    sc.close()
