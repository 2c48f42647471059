"""The image-space kernels -- the Gaussian blur (LDS-tiled and global), the two median kernels, the a-trous denoiser with its
prepare / variance / finish passes -- against their references bit for bit, beyond one shape and beyond rendered input.

References, unchanged: oracle_lib.gauss_blur / median_filter (the reference's loops) and denoise_restatement.denoise (numpy,
from the text of include/pt_hip.h).  Every comparison is on uint32 views of float32; there is no tolerance anywhere.

  shapes    image_kernel_cases.GRID: 1 x 1, one row, one column, 15 / 16 / 17 and 31 / 32 / 33 in each direction, tall-narrow and
            wide-low, smaller than the halo, 6 x 6 workgroups; and 1920 x 1080 (120 x 68 workgroups, the last row 8 pixels high),
            compared through crops: both operations are local, so the reference on a crop padded by the reach (ceil(2.57 r) for the
            Gaussian, the window size for the median, 3 + 2 (1 + 2 + 4 + 8 + 16) = 65 for five denoiser levels) is exact for the crop's
            interior -- tests/test_image_crops_host.py asserts that on the CPU
  content   dense, mostly black with isolated bright pixels, few integer levels (ties), mixed sign, ~1e30, ~1e-30, constant, and
            lines of infinities where the result is defined (one sign for the Gaussian, both for the median)
  denoiser  synthetic features and accumulators (image_kernel_cases.denoise_inputs): classes interleaved pixel by pixel, opposite,
            orthogonal and zero normals, albedo at, just below and just above the floor, counts around the spatial-variance threshold
            and around 2^24, cancelling second moments, every level count, the extremes of every parameter

-0.0 and NaN are kept out of the compared inputs: the reference reads its order statistic from a sorted window, so which of two
equal zeros lands at the chosen rank is unspecified and any ordering of a NaN is undefined.  For the same reason a median follows
a Gaussian only on non-negative content here (a negative mean can round to -0.0).
"""
import importlib

import numpy as np
import pytest

import denoise_restatement as R
import image_kernel_cases as K
import oracle_lib as O

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
FULL_W, FULL_H = 1920, 1080


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, f"{len(bad)} values differ, first (y, x, channel) {bad[:4].tolist()}")


def _reference_filter(img, gauss, median):
    if gauss:
        img = O.gauss_blur(img, gauss)
    if median:
        img = O.median_filter(img, median)
    return img


def _check_filter(kind, W, H, gauss, median, seed=0, telling=False):
    """telling: the reference's output must not be constant (or the cell could not tell a wrong tap from a right one)."""
    img = K.image(kind, W, H, seed)
    want = _reference_filter(img, gauss, median)
    if telling and W * H > 1:
        assert len(np.unique(want)) > 1, (kind, W, H, gauss, median, "the reference output is constant")
    _assert_same(pt.post_filter(img, gauss=gauss, median=median), want, (kind, W, H, gauss, median))


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"


# ---- post filters ----------------------------------------------------------------------------------------------------

RADII = [(g, 0) for g in K.GAUSS_RADII] + [(0, m) for m in K.MEDIAN_SIZES]


GRID_CONTENT = ("dense", "signed")      # content that can tell on every shape: no cell of the grid is left to a degenerate image


@pytest.mark.parametrize("gauss,median", RADII)
def test_filters_shape_grid(gauss, median):
    """Every shape of the grid at this radius, on dense content of one sign or of both (alternating over shapes and radii); every
    cell's reference output is checked not to be constant.  The other kinds of content are test_filters_content's."""
    for i, (W, H) in enumerate(K.GRID):
        _check_filter(GRID_CONTENT[(i + RADII.index((gauss, median))) % 2], W, H, gauss, median, telling=True)


@pytest.mark.parametrize("kind", list(K.CONTENT))
def test_filters_content(kind):
    """Every kind of content at every radius on an image with ragged tiles, and once per kernel on a tall narrow one."""
    for gauss, median in RADII:
        _check_filter(kind, 33, 31, gauss, median, seed=1)
    for gauss, median in ((9, 0), (10, 0), (0, 3), (0, 4)):
        _check_filter(kind, 7, 90, gauss, median, seed=1)


def test_filters_infinities():
    """An order statistic of values that compare is defined whatever their magnitude: lines of +Inf and -Inf through the median.  The
    Gaussian's weights are all positive, so a window that holds +Inf (and no -Inf) sums to +Inf, and round(+Inf) = +Inf."""
    for W, H in ((33, 31), (17, 33)):
        for median in K.MEDIAN_SIZES:
            _check_filter("inf_lines", W, H, 0, median)
        for gauss in K.GAUSS_RADII:
            _check_filter("pos_inf_lines", W, H, gauss, 0)


@pytest.mark.parametrize("W,H", [(33, 31), (90, 7)])
def test_filters_composition(W, H):
    """Both filters in one call: the Gaussian runs first (main.cpp:187-192)."""
    for kind in K.NON_NEGATIVE:
        for gauss, median in ((1, 1), (9, 3), (10, 4), (2, 11)):
            img = K.image(kind, W, H, seed=2)
            want = O.median_filter(O.gauss_blur(img, gauss), median)
            _assert_same(pt.post_filter(img, gauss=gauss, median=median), want, (kind, W, H, gauss, median))
            if kind == "dense":   # the order matters on this input, so the assertion above can tell the two orders apart
                assert not np.array_equal(want, O.gauss_blur(O.median_filter(img, median), gauss))


@pytest.fixture(scope="module")
def full_image():
    """1920 x 1080: dense content on the left, a band of few levels across the middle rows, and mostly black with isolated bright
    pixels on the right (the right-hand windows lie in it), so that the windows see all three."""
    img = K.image("dense", FULL_W, FULL_H, seed=3)
    img[300:800] = K.image("levels", FULL_W, 500, seed=3)
    img[:, 1200:] = K.image("sparse", FULL_W - 1200, FULL_H, seed=3)
    assert (img[:, 1200:] == 0).mean() > 0.9 and (img[:300, :1200] > 0).all()
    return img


@pytest.mark.parametrize("gauss,median", RADII)
def test_filters_full_size_windows(full_image, gauss, median):
    """One launch of 120 x 68 workgroups; ten windows of it against the reference on crops."""
    got = pt.post_filter(full_image, gauss=gauss, median=median)
    reach = K.gauss_reach(gauss) if gauss else median
    side = 24 if reach > 8 else 48                    # the reference's work per window grows with (side + 2 reach)^2 reach^2
    for name, box in K.windows(FULL_W, FULL_H, side, side).items():
        want = K.crop_reference([full_image], box, reach, lambda crops, w, h: _reference_filter(crops[0], gauss, median))
        x0, y0, x1, y1 = box
        _assert_same(np.ascontiguousarray(got[y0:y1, x0:x1]), np.ascontiguousarray(want), (name, box, gauss, median))


# ---- denoiser --------------------------------------------------------------------------------------------------------

def _check_denoise(W, H, inputs, **kw):
    s, s2, c, f = inputs
    mean, cout = pt.denoise(W, H, s, s2, c, f, **kw)
    with np.errstate(all="ignore"):                    # lanes that np.where discards may divide by zero
        rmean, rcount = R.denoise(W, H, s, s2, c, f, **kw)
    assert np.isfinite(rmean).all(), (W, H, kw)
    assert np.array_equal(cout, rcount), (W, H, kw)
    _assert_same(mean, rmean, (W, H, kw))
    return mean, cout


@pytest.mark.parametrize("demodulate", [0, -1])
def test_denoise_shape_grid(demodulate):
    """Every shape of the grid -- most are smaller than the last level's tap reach of 32, five are smaller than one 32 x 8 workgroup
    in some direction -- with the classes, normals and counts rotating."""
    for i, (W, H) in enumerate(K.GRID):
        inputs = K.denoise_inputs(W, H, seed=i, hit=K.HIT_KINDS[i % 3], normal=K.NORMAL_KINDS[(i + demodulate) % len(K.NORMAL_KINDS)],
                                  position=K.POSITION_KINDS[i % 2], count=K.COUNT_KINDS[0 if i % 2 else 3])
        _check_denoise(W, H, inputs, levels=5, demodulate_albedo=demodulate)


@pytest.mark.parametrize("hit", K.HIT_KINDS)
@pytest.mark.parametrize("normal", K.NORMAL_KINDS)
def test_denoise_classes_and_normals(hit, normal):
    """Every class pattern with every kind of normal; the positions and the demodulation switch rotate."""
    W, H = 45, 19
    i = K.HIT_KINDS.index(hit) + K.NORMAL_KINDS.index(normal)
    _check_denoise(W, H, K.denoise_inputs(W, H, seed=i, hit=hit, normal=normal, position=K.POSITION_KINDS[i % 3]), levels=3,
                   demodulate_albedo=-(i % 2))


@pytest.mark.parametrize("count", K.COUNT_KINDS)
@pytest.mark.parametrize("albedo", K.ALBEDO_KINDS)
def test_denoise_counts_and_albedo(count, albedo):
    """Both demodulate_albedo settings for every kind of count and albedo."""
    for (W, H), demodulate in (((33, 17), 0), ((16, 40), -1)):
        _check_denoise(W, H, K.denoise_inputs(W, H, hit="random", albedo=albedo, count=count), levels=4, demodulate_albedo=demodulate)


def test_denoise_inputs_reach_the_edges_they_name():
    """The generators do produce what the cases above are named for (a generator that silently stopped would leave them vacuous)."""
    W, H = 33, 17
    s, s2, c, f = K.denoise_inputs(W, H, hit="random", albedo="floor", count="threshold")
    hit3 = np.repeat(f["hit_index"] >= 0, 3).reshape(-1, 3)
    for v in (0.0, np.nextafter(K.ALBEDO_FLOOR, np.float32(0)), K.ALBEDO_FLOOR, np.nextafter(K.ALBEDO_FLOOR, np.float32(1)), 2.5):
        assert ((f["albedo"] == np.float32(v)) & hit3).any(), v
    assert set(np.unique(c)) == {K.SPATIAL_BELOW - 1, K.SPATIAL_BELOW, K.SPATIAL_BELOW + 1} and K.SPATIAL_BELOW == R.SPATIAL_BELOW
    assert K.ALBEDO_FLOOR == R.ALBEDO_FLOOR
    s, s2, c, f = K.denoise_inputs(W, H, count="two_pow_24")
    assert (c == 2 ** 24).any() and (c == 2 ** 24 + 1).any()
    s, s2, c, f = K.denoise_inputs(W, H, count="cancel")
    n = c[:, None].astype(np.float32)
    d = s2 / n - (s / n) * (s / n)
    assert (d < 0).any() and (d >= 0).any()
    s, s2, c, f = K.denoise_inputs(W, H, hit="all", normal="some_zero")
    assert (~f["normal"].any(axis=1)).any()
    N = K.denoise_inputs(W, H, normal="opposite")[3]["normal"].reshape(H, W, 3)
    assert ((N[:, 1:] * N[:, :-1]).sum(-1) == -1).all()
    N = K.denoise_inputs(W, H, normal="orthogonal")[3]["normal"].reshape(H, W, 3)
    assert ((N[:, 1:] * N[:, :-1]).sum(-1) == 0).all()


@pytest.mark.parametrize("levels", range(0, pt.DENOISE_MAX_LEVELS + 1))
def test_denoise_every_level_count(levels):
    assert R.LEVELS_MAX == pt.DENOISE_MAX_LEVELS
    for W, H in ((40, 23), (150, 9)):                  # the second is wider than the last level's spacing of 128
        _check_denoise(W, H, K.denoise_inputs(W, H, seed=levels, hit="blocks"), levels=levels)


@pytest.mark.parametrize("kw", [dict(normal_power_log2=1), dict(normal_power_log2=16), dict(sigma_luminance=1e-20), dict(sigma_luminance=1e20),
                                dict(sigma_plane=1e-20), dict(sigma_plane=1e20),
                                dict(sigma_luminance=1e-20, sigma_plane=1e20, normal_power_log2=16)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_denoise_parameter_extremes(kw):
    W, H = 37, 21
    for normal, position in (("unit", "scales"), ("discrete", "coplanar")):
        _check_denoise(W, H, K.denoise_inputs(W, H, hit="random", normal=normal, position=position), levels=5, **kw)


def test_denoise_full_size_windows():
    """1920 x 1080 at five levels, once on the device; ten windows against the restatement on crops padded by the reach of 65."""
    W, H, levels = FULL_W, FULL_H, 5
    inputs = K.denoise_inputs(W, H, hit="blocks", normal="discrete", position="coplanar", albedo="materials", count="mixed")
    s, s2, c, f = inputs
    mean, cout = pt.denoise(W, H, s, s2, c, f, levels=levels)
    mean, cout = mean.reshape(H, W, 3), cout.reshape(H, W)
    reach = K.denoise_reach(levels)
    assert reach == 65
    fn = K.denoise_from_planes(R.denoise, levels=levels)
    for name, box in K.windows(W, H, 16, 16, tile_w=32, tile_h=8).items():
        with np.errstate(all="ignore"):
            rmean, rcount = K.crop_reference(K.denoise_planes(W, H, *inputs), box, reach, fn)
        x0, y0, x1, y1 = box
        assert np.array_equal(cout[y0:y1, x0:x1], rcount), name
        _assert_same(np.ascontiguousarray(mean[y0:y1, x0:x1]), np.ascontiguousarray(rmean), (name, box))
        assert (cout[y0:y1, x0:x1] > c.reshape(H, W)[y0:y1, x0:x1]).any(), name      # the filter filled pixels in this window
