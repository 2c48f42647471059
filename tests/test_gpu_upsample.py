"""The feature-guided upsampler on the GPU: pt_upsample_host must equal the numpy restatement of include/pt_hip.h's text
(tests/upsample_restatement.py) bit for bit -- on synthetic inputs that cross the 32 x 8 workgroup in both directions with
remainders, and on a rendered, denoised frame."""
import importlib

import numpy as np
import pytest

import denoise_restatement as R
import image_kernel_cases as K
import upsample_restatement as U

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu

LOW_SIZES = [(1, 1), (3, 2), (17, 5), (33, 9)]      # x 2, 3, 4: up to 132 x 36; 1 x 1 leaves three of four taps outside
# (generator arguments of the full-resolution features, of the low accumulators, upsampler parameters)
CONTENT = [
    (dict(), dict(), dict()),                                                                             # mixed classes, counts of 0, albedo around the floor
    (dict(normal="unit", position="random"), dict(count="sampled"), dict(demodulate_albedo=-1)),
    (dict(hit="blocks", normal="orthogonal"), dict(), dict(sigma_plane=0.5, normal_power_log2=3)),
    (dict(hit="checker", normal="some_zero", position="scales"), dict(), dict(sigma_plane=2.0, normal_power_log2=16)),
    (dict(hit="none", albedo="materials"), dict(count="sampled"), dict()),
    (dict(hit="all", normal="opposite"), dict(count="zero"), dict(demodulate_albedo=-1)),
]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(W, H, mean_lo, count_lo, feat, scale, **kw):
    mean, cout, ms = pt.upsample(0, W, H, mean_lo, count_lo, feat, scale, want_ms=True, **kw)
    rmean, rcount = U.upsample(W, H, mean_lo, count_lo, feat, scale=scale, **kw)
    assert np.array_equal(cout, rcount), (scale, kw, int((cout != rcount).sum()))
    bad = _bits(mean) != _bits(rmean)
    assert not bad.any(), (scale, kw, int(bad.sum()), np.argwhere(bad)[:4].tolist(), mean[bad][:4].tolist(), rmean[bad][:4].tolist())
    assert ms > 0
    return mean, cout


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"


@pytest.mark.parametrize("scale", U.SCALES)
@pytest.mark.parametrize("w,h", LOW_SIZES)
def test_synthetic_inputs_bit_exact(w, h, scale):
    W, H = scale * w, scale * h
    seen_empty = seen_value = False
    for i, (feat_kw, low_kw, prm) in enumerate(CONTENT):
        feat = K.denoise_inputs(W, H, seed=10 + i, **feat_kw)[3]
        s, s2, c, low_feat = K.denoise_inputs(w, h, seed=20 + i, **low_kw)
        mean_lo, count_lo = R.denoise(w, h, s, s2, c, low_feat, levels=0)          # the plain mean: sum / n, sum where n = 0
        mean, cout = _check(W, H, mean_lo, count_lo, feat, scale, **prm)
        seen_empty |= bool((cout == 0).any())
        seen_value |= bool((cout == 1).any())
    assert seen_empty and seen_value


def test_rendered_denoised_frame(models_dir):
    """Tor.obj traced at 24 x 16, denoised, upsampled to 48 x 32 and 72 x 48 with the device's own full-resolution features."""
    w, h, spp, mrr = 24, 16, 8, 3
    tor = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    s, s2, c, _ = tor.render_host(w, h, spp, mrr, error=-1.0, seed=42)
    mean_lo, count_lo = pt.denoise(w, h, s, s2, c, tor.render_features(w, h), levels=3)
    # (8 spp, 3 segments: some pixels have no sample, and three levels do not fill every one of them -- the upsampler sees both)
    assert (count_lo > 0).mean() > 0.8 and (c == 0).any()
    for scale in (2, 3):
        W, H = scale * w, scale * h
        feat = tor.render_features(W, H)
        for kw in (dict(), dict(demodulate_albedo=-1)):
            mean, cout = _check(W, H, mean_lo, count_lo, feat, scale, **kw)
            assert np.isfinite(mean).all() and (cout == 1).mean() >= (count_lo > 0).mean()
            assert not mean[cout == 0].any()
            # it is an interpolation: inside the low image's range per channel, and not the nearest low pixel everywhere
            y, x = np.mgrid[0:H, 0:W]
            nearest = mean_lo.reshape(h, w, 3)[y // scale, x // scale].reshape(-1, 3)
            assert (mean != nearest).any()
        plain, _ = pt.upsample(0, W, H, mean_lo, count_lo, feat, scale, demodulate_albedo=-1)
        assert plain.max() <= mean_lo.max() * (1 + 1e-5) and plain.min() >= 0
