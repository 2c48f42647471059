"""First-hit feature buffers and the denoiser without a GPU: argument checks and error codes, struct layout, pt_tonemap against
pt_resolve_float, and what the filter is worth -- the numpy restatement of include/pt_hip.h's text (tests/denoise_restatement.py)
against the reference's own -GAUSS and -MEDIAN on oracle frames."""
import ctypes as C
import importlib

import numpy as np
import pytest

import denoise_restatement as R
import oracle_lib as O

pt = importlib.import_module("path-tracing_amd")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frame(W, H, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 5, W * H).astype(np.int32)
    s = (rng.random((W * H, 3), dtype=np.float32) * c[:, None]).astype(np.float32)
    return s, (s * s).astype(np.float32), c


def _flat_features(W, H, albedo=(0.5, 0.25, 1.0)):
    """A wall facing the reference camera at z = 5."""
    o, d = R.centre_rays(W, H)
    t = (np.float32(25.0) / d[:, 2]).astype(np.float32)
    return {"hit_index": np.zeros(W * H, np.int32), "hit_t": t, "position": (o + d * t[:, None]).astype(np.float32),
            "normal": np.tile(np.array([0, 0, -1], np.float32), (W * H, 1)), "albedo": np.tile(np.array(albedo, np.float32), (W * H, 1))}


def test_struct_layout():
    assert C.sizeof(pt.DenoiseParams) == 20
    assert [n for n, _ in pt.DenoiseParams._fields_] == ["levels", "sigma_luminance", "sigma_plane", "normal_power_log2", "demodulate_albedo"]
    assert pt.DENOISE_MAX_LEVELS == R.LEVELS_MAX == 8


def test_denoise_argument_checks():
    W, H = 8, 6
    s, s2, c = _frame(W, H)
    f = _flat_features(W, H)
    for kw in ({"levels": -1}, {"levels": 9}, {"sigma_luminance": float("nan")}, {"sigma_luminance": float("inf")},
               {"sigma_plane": float("nan")}, {"sigma_plane": -1.0}, {"sigma_luminance": -0.5}, {"normal_power_log2": -1},
               {"normal_power_log2": 17}):
        with pytest.raises(pt.PtError) as e:
            pt.denoise(W, H, s, s2, c, f, **{"levels": 2, **kw})
        assert e.value.status == 1, kw
    with pytest.raises(pt.PtError) as e:      # levels > 0 needs the feature buffers
        pt.denoise(W, H, s, s2, c, None, levels=1)
    assert e.value.status == 1
    L, fp, ip = pt.lib(), pt._fp, pt._ip
    prm, out = pt.DenoiseParams(0, 0, 0, 0, 0), np.zeros((W * H, 3), np.float32)
    assert L.pt_denoise_host(0, 0, H, fp(s), fp(s2), ip(c), None, None, None, None, C.byref(prm), fp(out), None, None) == 1   # empty image
    assert L.pt_denoise_host(0, W, H, None, fp(s2), ip(c), None, None, None, None, C.byref(prm), fp(out), None, None) == 1
    assert L.pt_denoise_host(0, W, H, fp(s), fp(s2), ip(c), None, None, None, None, None, fp(out), None, None) == 1
    assert L.pt_denoise_host(0, W, H, fp(s), fp(s2), ip(c), None, None, None, None, C.byref(prm), None, None, None) == 1
    assert L.pt_tonemap(W, H, None, ip(c), 0.5, fp(out)) == 1 and L.pt_tonemap(W, 0, fp(out), ip(c), 0.5, fp(out)) == 1
    # an unusable device is an error, not a fallback (as pt_post_filter_host)
    with pytest.raises(pt.PtError) as e:
        pt.denoise(W, H, s, s2, c, f, levels=1, device=10_000)
    assert e.value.status == 4
    if pt.device_count() == 0:
        with pytest.raises(pt.PtError) as e:
            pt.denoise(W, H, s, s2, c, f, levels=1)
        assert e.value.status == 4


def test_features_argument_checks(models_dir):
    sc = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    for kw, status in (({"row_stride": 2}, 7), ({"row_stride": -1}, 1), ({"rows": (4, 2)}, 1), ({"rows": (0, 9)}, 1), ({}, 4)):
        with pytest.raises(pt.PtError) as e:
            sc.render_features(8, 8, **kw)
        assert e.value.status == status, kw
    for w, h in ((0, 8), (8, 0)):
        with pytest.raises(pt.PtError) as e:
            sc.render_features(w, h)
        assert e.value.status == 1
    p = pt.RenderParams(8, 8, 0, 8, 0, 0, 0, 1e-4, -1.0, 0, 0, 0)
    assert pt.lib().pt_render_features_host(None, C.byref(p), None, None, None, None, None) == 1
    assert pt.lib().pt_render_features_host(sc._h, None, None, None, None, None, None) == 1


def test_levels_zero_and_tonemap_equal_resolve_float(oracle_scene):
    """levels = 0 is sum / n on the host (no device); pt_tonemap of it is pt_resolve_float's image bit for bit."""
    W, H = 37, 21
    s, s2, c, _ = O.render(oracle_scene, W, H, 24, 6, error=0.001)
    assert (c > 0).sum() > 20 and (c == 0).sum() > 0
    mean, cout = pt.denoise(W, H, s, s2, c, None, levels=0)
    n = np.where(c > 0, c, 1).astype(np.float32)[:, None]
    expect = np.where((c > 0)[:, None], s / n, s).astype(np.float32)
    assert np.array_equal(_bits(mean), _bits(expect)) and np.array_equal(cout, c)
    rmean, rcount = R.denoise(W, H, s, s2, c, None, levels=0)
    assert np.array_equal(_bits(rmean), _bits(expect)) and np.array_equal(rcount, c)
    rgb, _ = pt.resolve_float(W, H, s, s2, c)
    assert np.array_equal(_bits(pt.tonemap(W, H, mean, c)), _bits(rgb))
    assert np.array_equal(_bits(pt.tonemap(W, H, expect, c)), _bits(rgb))


@pytest.mark.parametrize("demodulate", [0, -1])
def test_restatement_fixed_point(demodulate):
    """A constant image with constant features comes back bit-identical (whatever the albedo: step 5 adds the filter's CHANGE)."""
    W, H = 23, 17
    c = np.full(W * H, 3, np.int32)
    m = np.array([0.1, 0.7, 0.3], np.float32)
    s = np.tile(m * np.float32(3), (W * H, 1)).astype(np.float32)
    s2 = (s * s / np.float32(2)).astype(np.float32)
    f = _flat_features(W, H, albedo=(0.3, 0.7, 0.9))
    mean, cout = R.denoise(W, H, s, s2, c, f, levels=5, demodulate_albedo=demodulate)
    assert np.array_equal(_bits(mean), _bits(s / np.float32(3))) and np.array_equal(cout, c)


def test_restatement_fills_only_from_its_class():
    """Pixels without samples take their value from sampled pixels of their class; a class without any sample stays as it is."""
    W, H = 16, 8
    f = _flat_features(W, H, albedo=(1, 1, 1))
    f["hit_index"][: W] = -1                      # the top row saw the sky ...
    for k in ("position", "normal", "albedo"):
        f[k][: W] = 0
    c = np.ones(W * H, np.int32)
    c[: W] = 0                                    # ... and has no sample, nor has one pixel of the wall
    c[3 * W + 5] = 0
    s = np.tile(np.array([0.25, 0.5, 0.75], np.float32), (W * H, 1)) * c[:, None].astype(np.float32)
    mean, cout = R.denoise(W, H, s, s * s, c, f, levels=2)
    assert np.array_equal(cout[: W], np.zeros(W, np.int32)) and not mean[: W].any()
    assert cout[3 * W + 5] == 1 and np.array_equal(_bits(mean[3 * W + 5]), _bits(np.array([0.25, 0.5, 0.75], np.float32)))


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.fixture(scope="module")
def truth(oracle_scene):
    gs, gs2, gc, _ = O.render(oracle_scene, 128, 128, 1024, 8, error=-1.0, seed=1234)
    return O.resolve_float(128, 128, gs, gs2, gc)[0]


@pytest.mark.parametrize("spp,seed", [(16, 42), (64, 7)])
def test_restatement_beats_the_blind_filters(oracle_scene, truth, spp, seed):
    """Oracle frames of Tor.obj, 128 x 128, -ERR -1; ground truth: 1024 spp of the same view.  On the tone-mapped float image the
    denoised frame (defaults, 5 levels) must be closer to the truth than the frame itself and than the best of -GAUSS 1, 2, 3 and
    -MEDIAN 3, 5 of that frame.  Measured (RMSE, 0 .. 255 scale): see DESIGN.md section 10."""
    W = H = 128
    s, s2, c, _ = O.render(oracle_scene, W, H, spp, 8, error=-1.0, seed=seed)
    noisy, _ = O.resolve_float(W, H, s, s2, c)
    f = R.features(oracle_scene, W, H)
    assert not f["nan_seen"].any()
    mean, cout = R.denoise(W, H, s, s2, c, f, levels=5)
    ours = pt.tonemap(W, H, mean, cout)
    blind = {f"gauss {r}": _rmse(O.gauss_blur(noisy, r), truth) for r in (1, 2, 3)}
    blind.update({f"median {w}": _rmse(O.median_filter(noisy, w), truth) for w in (3, 5)})
    e_noisy, e_ours, e_blind = _rmse(noisy, truth), _rmse(ours, truth), min(blind.values())
    print(f"spp {spp}: undenoised {e_noisy:.2f}, denoised {e_ours:.2f}, best blind filter {e_blind:.2f} ({blind})")
    assert e_ours < e_noisy
    assert e_ours < e_blind
