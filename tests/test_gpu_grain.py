"""The grain display kernel alone (include/pt_hip.h: pt_display_bytes_grain_host) against the numpy restatement of the header
(tests/grain_restatement.py) as bytes, every one of them: over the shapes at which four pixels per lane, a row end inside a lane's
pixels, the flat tail and more than one wave could go wrong, the contents that meet every branch of the header (tests/grain_cases.py),
every lattice pitch, the frames 0, 1 and 2^32 - 1, grain and dither each alone and together, the four curves, and with and without a
small LUT.  The value the stage acts on, g, is the library's own host colour step (pt_colour_host, pinned bit for bit against its
restatement by tests/test_colour_host.py).  The entry point takes means; the kernel's instantiations for sums run in
tests/test_gpu_grain_display.py, whose sessions hand it sums."""
import importlib

import numpy as np
import pytest

import colour_cases as CK
import grain_cases as K
import grain_restatement as R

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu

F = np.float32
GAMMA = K.GAMMA
CURVES = ["reference", "clamp", "reinhard", "aces"]
MODES = {"grain": dict(strength=0.6), "dither": dict(dither=1.0), "both": dict(strength=0.35, dither=1.0)}


@pytest.fixture(scope="module")
def cache():
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"
    return {}


@pytest.fixture(scope="module")
def small_lut():
    return pt.Lut.create(CK.lut("random", 5))


def _deferred(v, count, gamma):
    with np.errstate(invalid="ignore"):
        return int(((~R.covered(v, gamma)).any(axis=2) & (count != 0)).sum())


def _check(cache, m, c, grade, colour, grain, where):
    """One call: the bytes are the restatement's of the host's g, and the deferred list is as long as the header says."""
    h, w, _ = m.shape
    e = F(grade.get("exposure", 0.0) or 1.0)
    g = pt.colour(m, c, e, grade.get("curve", 0), colour)
    want = K.reference(cache, g, c, GAMMA, **grain)
    got, info = pt.display_bytes_grain(m, c, grade, colour, grain, GAMMA)
    K.same(got, want, where)
    v = R.grained(g, grain.get("strength", 0.0), grain.get("size", 0.0), grain.get("seed", 0), grain.get("frame", 0))
    assert info["deferred_pixels"] == _deferred(v, c, GAMMA), where
    return got, info


@pytest.mark.parametrize("shape", K.SHAPES, ids=["%dx%d" % s for s in K.SHAPES])
@pytest.mark.parametrize("name", list(K.CASES))
def test_shapes_contents_pitches_frames_and_modes(cache, small_lut, name, shape):
    w, h = shape
    m, c = K.CASES[name](w, h)
    plain, _ = pt.display_bytes_colour(m, c, {}, None, GAMMA)
    i = K.SHAPES.index(shape) + 3 * list(K.CASES).index(name)
    changed = False
    for size in K.SIZES:
        for mode, prm in MODES.items():
            curve, lut = CURVES[i % 4], (small_lut if i % 3 == 0 else None)
            grain = dict(prm, size=size, seed=17 + i, frame=K.FRAMES[i % 3])
            got, _ = _check(cache, m, c, dict(curve=curve, exposure=1.0), dict(lut=lut) if lut else None, grain, (name, shape, size, mode, curve, bool(lut)))
            changed |= curve == "reference" and lut is None and bool((got != plain).any())
            i += 1
    # the stage off: the colour kernel's bytes (curve reference, exposure 1: g is the mean)
    K.same(pt.display_bytes_grain(m, c, {}, None, None, GAMMA)[0], plain, (name, shape, "zeroed"))
    K.same(pt.display_bytes_grain(m, c, {}, None, dict(size=2.0, seed=3, frame=4), GAMMA)[0], plain, (name, shape, "zeroed but for size, seed, frame"))
    if name in ("grey", "ramp", "holes") and w * h > 1:
        assert changed, "the stage changed no byte: the test would pass without it"


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("with_lut", [False, True], ids=["no LUT", "LUT"])
def test_every_curve_with_and_without_a_lut_at_every_pitch(cache, small_lut, curve, with_lut):
    w, h = 97, 31
    m, c = CK.image("random", w, h)                      # 0 .. 1.2 with a tenth of the pixels without samples
    colour = dict(wb=(1.1, 1.0, 0.9), saturation=0.8, lut=small_lut) if with_lut else dict(wb=(1.1, 1.0, 0.9), saturation=0.8)
    seen, distinct = set(), set()
    for k, size in enumerate(K.SIZES):
        for mode, prm in MODES.items():
            got, info = _check(cache, m, c, dict(curve=curve, exposure=1.5), colour, dict(prm, size=size, seed=5, frame=K.FRAMES[k % 3]),
                               (curve, with_lut, size, mode))
            seen.add(got.tobytes())
            distinct.add((mode, size if "strength" in prm else None, K.FRAMES[k % 3]))      # (the dither alone does not see the pitch)
    assert len(seen) == len(distinct) == 13
    # without the matrix and the LUT: the kernel in the graded one's place
    _check(cache, m, c, dict(curve=curve, exposure=0.75), None, dict(strength=0.5, size=2.0, dither=1.0, seed=1), (curve, "no colour stage"))


def test_the_deferred_list_among_dithered_pixels(cache):
    """NaN, negative, infinite and over-table pixels among dithered ones: the host finishes them with the header's steps, from the
    pixel's index, the seed and the frame -- the grain of a deferred pixel's valid channels and their dither included."""
    w, h = 97, 31
    rng = np.random.default_rng(12)
    m = rng.uniform(0.0, 1.0, (h, w, 3)).astype(F)
    c = np.full((h, w), 2, np.int32)
    T, _ = R.table(GAMMA)
    poison = np.array([np.nan, -1.0, 1e30, np.inf, T[-1], 2 * T[-1]], F)
    flat = m.reshape(-1, 3)
    where = np.arange(0, w * h, 5)
    flat[where, where % 3] = poison[(where // 5) % len(poison)]
    for grain in (dict(strength=0.6, size=2.5, dither=1.0, seed=9, frame=2 ** 32 - 1), dict(dither=1.0, seed=9), dict(strength=1.0, seed=9, frame=1)):
        for curve in ("reference", "aces"):
            got, info = _check(cache, m, c, dict(curve=curve), None, grain, (grain, curve))
            assert info["deferred_pixels"] >= len(where) // 3
    # every pixel deferred: the list filled to its capacity
    flat[:, 0] = np.nan
    got, info = _check(cache, m, c, {}, None, dict(strength=0.6, size=1.5, dither=1.0, seed=2), "all deferred")
    assert info["deferred_pixels"] == w * h
