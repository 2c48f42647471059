"""Environment sampling on the GPU (pt_hip.h: environment sampling; pt_kernels.hip: integrate_kernel_envdirect), bit for bit on sum, sum2
and count against tests/envdirect_composition.py: the direct composition with the choice between the emitters and the environment, the
restated sample and term, the verdict at a miss and the suppression of a miss after a diffuse step.  The open Tor scene under the sun
map at sizes that are and are not multiples of a tile, with statistics, with adaptive sampling, combined with glass, roughness, shading
normals and a texture; a camera, a lens, a moving camera and a projection; the box tree; the room with a lamp at the default and at a
given share, the room without an emitter; a map whose size is no power of two and one larger than the table; the switch set and
cleared; an environment replaced while the switch is on; bands, a clone and a rehearsed three-band frame; both verification builds; the
diagnostic build's refusal; the untouched feature pass.  tests/test_envdirect_host.py composes frames of these scenes on the CPU and
asserts that none is tainted."""
import importlib
import os

import numpy as np
import pytest

import envdirect_composition as EC
import envdirect_scenes as ES
import texture_scenes as S

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    assert pt.device_count() >= 1, "no HIP device: the integrator has no CPU fallback"


def _reset(scene):
    scene.set_environment_sampling(False)
    scene.set_direct_lighting(False)
    scene.set_projection(None); scene.set_camera_motion(None); scene.set_lens(None); scene.set_camera(None)
    scene.set_textures(None); scene.set_roughness(None); scene.set_dielectrics(None); scene.set_shading_normals(None)


def _check(scene, osc, n9, uv, env, w, h, spp, mrr, *, share=None, rough=None, smooth=False, textures=None, glass=None, px=None, error=-1.0, stats=False, seed=42, **view):
    scene.set_environment_sampling(False)
    scene.set_roughness(None)
    scene.set_textures([pt.texture(m, t, f) for m, (t, f) in (textures or {}).items()])
    scene.set_dielectrics([pt.dielectric(m, ior, tint) for m, (ior, tint) in (glass or {}).items()])
    scene.set_shading_normals(n9 if smooth else None)
    scene.set_roughness([pt.rough(m, a) for m, a in (rough or {}).items()])
    scene.set_environment_map(env)
    scene.set_environment_sampling(share)
    px = S.all_pixels(w, h) if px is None else px
    s, s2, c, st = scene.render_host(w, h, spp, mrr, error=error, seed=seed, want_stats=stats)
    i = px[:, 1] * w + px[:, 0]
    tally = {}
    ws, ws2, wc = EC.compose(osc, rough, n9 if smooth else None, textures, uv, glass, env, w, h, px, spp, mrr, seed=seed, error=error, stats=tally, share=share, **view)
    assert not tally["tainted"].any() and tally["sky_terms"] > 0
    assert _bits(scene.environment_sampling()) == _bits(tally["share"])
    assert np.array_equal(c[i], wc), int((c[i] != wc).sum())
    bad = int((_bits(s.reshape(-1, 3)[i]) != _bits(ws)).any(1).sum())
    assert bad == 0 and np.array_equal(_bits(s2.reshape(-1, 3)[i]), _bits(ws2)), bad
    if stats and len(px) == w * h:
        assert (st["samples_traced"], st["segments"], st["misses"], st["contributing"]) == \
               (tally["samples_traced"], tally["segments"], tally["misses"], tally["contributing"]), (st, tally)
    return tally


@pytest.fixture(scope="module")
def tor(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("open")) + "/"
    osc, uv = ES.open_tor(d)
    osc.set_skybox(None)
    scene = pt.Scene.load_obj(d, "Open.obj", device=0)
    n9 = pt.smooth_normals(osc.triangles()[0])
    scene.set_texcoords(uv)
    return scene, osc, uv, n9, d


@pytest.mark.parametrize("name", list(ES.TOR_FRAMES))
def test_open_tor_frames_under_the_sun_equal_the_composition(gpu, tor, name):
    scene, osc, uv, n9, _ = tor
    _reset(scene)
    (w, h), spp, mrr, kw = ES.TOR_FRAMES[name]
    tally = _check(scene, osc, n9, uv, ES.MAPS["sun32"](), w, h, spp, mrr, **dict(kw))
    assert tally["sky_rays"] > tally["sky_terms"] and tally["suppressed_misses"] > 0           # the torus and the walls shadow the floor
    if name == "two_pixel_40x28":
        assert tally["visible_terms"] > tally["sky_terms"] and 0 < tally["share"] < 1         # both branches ran: the scene has its lamp
    if "glass" in kw:
        assert tally["cleared_by_glass"] > 0 and tally["rough_steps"] > 0
    _reset(scene)


@pytest.mark.parametrize("view", ES.VIEWS)
def test_a_camera_a_lens_a_moving_camera_and_a_projection(gpu, tor, view):
    scene, osc, uv, n9, _ = tor
    _reset(scene)
    _check(scene, osc, n9, uv, ES.MAPS["sun32"](), 40, 28, 3, 4, **S.set_view(pt, scene, view, 40, 28))
    _reset(scene)


@pytest.mark.parametrize("name", ["n12", "n512", "sun32_black"])
def test_a_map_that_is_no_power_of_two_one_larger_than_the_table_and_a_black_sky(gpu, tor, name):
    scene, osc, uv, n9, _ = tor
    _reset(scene)
    _check(scene, osc, n9, uv, ES.MAPS[name](), 40, 28, 3, 4)
    _reset(scene)


def test_the_box_tree_on_every_fifth_pixel(gpu, tmp_path):
    d = str(tmp_path) + "/"
    osc, uv, _ = S.box_tree(d)
    scene = pt.Scene.load_obj(d, "TorX4.obj", device=0)
    assert scene.counts()[0] > pt.BIG_SCENE_TRIANGLES
    px = S.all_pixels(48, 24)[::5]
    env = ES.MAPS["n8"]()                                                      # (a closed scene: the sky is reached by no ray; the unit still runs)
    scene.set_environment_map(env)
    scene.set_environment_sampling()
    s, s2, c, st = scene.render_host(48, 24, 3, 4, want_stats=True)
    i = px[:, 1] * 48 + px[:, 0]
    tally = {}
    ws, ws2, wc = EC.compose(osc, None, None, None, uv, None, env, 48, 24, px, 3, 4, stats=tally)
    assert not tally["tainted"].any() and tally["shadow_rays"] > 0
    assert np.array_equal(c[i], wc) and np.array_equal(_bits(s.reshape(-1, 3)[i]), _bits(ws)) and np.array_equal(_bits(s2.reshape(-1, 3)[i]), _bits(ws2))
    scene.close()


@pytest.mark.parametrize("lamp,share", [(True, None), (True, 0.7), (False, None)])
def test_the_open_room_with_a_lamp_at_two_shares_and_without_an_emitter(gpu, tmp_path, lamp, share):
    d = str(tmp_path) + "/"
    osc = ES.open_room(d, lamp=lamp)
    scene = pt.Scene.load_obj(d, "lamp_room.obj" if lamp else "dark_room.obj", device=0)
    (w, h), spp, mrr = ES.ROOM_FRAME
    tally = _check(scene, osc, None, None, ES.MAPS["n8" if lamp else "sun32_black"](), w, h, spp, mrr, share=share, stats=True)
    if lamp:
        assert tally["visible_terms"] > tally["sky_terms"] > 0 and tally["suppressed_emitter_hits"] > 0
        assert (tally["share"] == F32(0.7)) == (share is not None)
    else:
        assert tally["share"] == 1 and tally["visible_terms"] == tally["sky_terms"] and len(scene.lights()[0]) == 0
    scene.close()


def _same(got, ref):
    return np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(_bits(got[1]), _bits(ref[1])) and np.array_equal(got[2], ref[2])


def test_the_switch_set_and_cleared_an_environment_replaced_bands_a_clone_a_frame_and_the_verification_builds(gpu, tor):
    W, H, SPP = 40, 28, 4
    _, _, _, _, d = tor
    scene = pt.Scene.load_obj(d, "Open.obj", device=0)
    sun, other = ES.MAPS["sun32"](), ES.MAPS["n12"]()
    scene.set_environment_map(sun)
    plain = scene.render_host(W, H, SPP, 4, want_stats=False)                     # no flag: the environment kernels
    scene.set_direct_lighting(True)
    direct = scene.render_host(W, H, SPP, 4, want_stats=False)                    # -DIRECT 1 -ENV: the direct kernels
    scene.set_environment_sampling()
    one = scene.render_host(W, H, SPP, 4, want_stats=False)                       # with both on, this one picks the unit
    assert not _same(one, plain) and not _same(one, direct) and (one[2] == SPP).all()
    scene.set_environment_sampling(False)
    assert _same(scene.render_host(W, H, SPP, 4, want_stats=False), direct)        # cleared: the -DIRECT 1 frame again ...
    scene.set_direct_lighting(False)
    assert _same(scene.render_host(W, H, SPP, 4, want_stats=False), plain)         # ... and the frame of a handle that never had either
    scene.set_environment_sampling()
    assert _same(scene.render_host(W, H, SPP, 4, want_stats=False), one)           # (independent of direct lighting's switch)
    scene.set_environment_map(other)                                              # replaced while the switch is on: the table follows
    fresh = pt.Scene.load_obj(d, "Open.obj", device=0)
    fresh.set_environment_map(other)
    fresh.set_environment_sampling()
    replaced = scene.render_host(W, H, SPP, 4, want_stats=False)
    assert _same(replaced, fresh.render_host(W, H, SPP, 4, want_stats=False)) and not _same(replaced, one)
    fresh.close()
    scene.set_environment_map(sun)
    parts = [scene.render_host(W, H, SPP, 4, rows=r, want_stats=False) for r in ((0, 8), (8, H))]
    assert _same([np.concatenate([p[k] for p in parts]) for k in range(3)], one)
    clone = scene.clone_to_device(0)
    assert clone.environment_sampling() == scene.environment_sampling() and clone.environment_sampling_table()[0].shape == (32, 32)
    assert _same(clone.render_host(W, H, SPP, 4, want_stats=False), one)
    clone.close()
    g = pt.Frame(scene, [0, 0, 0], W, H, flags=pt.FRAME_REHEARSE)                  # a rehearsed three-band frame made from the scene: inherits the switch
    assert g.environment_sampling() == scene.environment_sampling()
    g.render(0, SPP, 4, error=-1.0)
    assert _same(g.read(), one)
    g.clear()
    g.set_environment_sampling(False)
    g.render(0, SPP, 4, error=-1.0)
    assert _same(g.read(), plain)
    g.clear()
    g.set_environment_sampling()
    g.set_environment_map(other)                                                  # the frame's setter rebuilds every copy's table
    g.render(0, SPP, 4, error=-1.0)
    assert _same(g.read(), replaced)
    g.close()
    scene.close()
    for path in (pt.VERIFY_LIB_PATH, os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_verify_shipped.so")):
        L = pt.load_library(path)
        sc = pt.Scene.load_obj(d, "Open.obj", device=0, library=L)
        sc.set_environment_map(sun)
        sc.set_environment_sampling()
        r = sc.render_host(W, H, SPP, 4, want_stats=True)
        assert r[3]["verify_checked"] > W * H * SPP and r[3]["verify_mismatches"] == 0, r[3]      # (the shadow searches are checked too)
        assert _same(r, one)
        sc.close()


def test_the_phase_timer_build_refuses_a_handle_with_environment_sampling(gpu, tor):
    _, _, _, _, d = tor
    L = pt.load_library(os.path.join(os.path.dirname(pt.VERIFY_LIB_PATH), "libpt_phase.so"))
    sc = pt.Scene.load_obj(d, "Open.obj", device=0, library=L)
    sc.set_environment_map(ES.MAPS["n8"]())
    sc.set_environment_sampling()
    with pytest.raises(pt.PtError) as e:
        sc.render_host(24, 20, 2, 4, want_stats=False)
    assert e.value.status == 7                                                     # PT_ERR_UNSUPPORTED
    sc.close()


def test_the_feature_pass_is_unchanged(gpu, tor):
    scene, osc, uv, n9, _ = tor
    _reset(scene)
    scene.set_environment_map(ES.MAPS["n8"]())
    base = scene.render_features(40, 28)
    scene.set_environment_sampling()
    got = scene.render_features(40, 28)
    for k in base:
        a, b = np.asarray(got[k]), np.asarray(base[k])
        assert np.array_equal(a.view(np.uint32) if a.dtype == F32 else a, b.view(np.uint32) if b.dtype == F32 else b), k
    _reset(scene)
