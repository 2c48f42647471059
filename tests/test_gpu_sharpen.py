"""pt_sharpen_host against the numpy restatement of the header's text (tests/sharpen_restatement.py), bit for bit, at the smallest
shapes at which the kernels can go wrong: 1 x 1, one column and one row, 2 x 2 (the ring's four borders and its substitution), a
32 x 8 tile exactly, 33 x 9 (one more both ways) and 97 x 31 (several tiles, partial ones at both rims).  Strength 1 and 0.25, the
default limit and 0.05, exposures 2^-8, 1 and 2^8, with out_rgb the input and apart from it.  The images are
tests/sharpen_cases.py's.  The kernels' sums form (their divide) goes through a display whose chain ends in sums."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sharpen_cases as K
import sharpen_restatement as R

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
F = np.float32
GAMMA = F(1) / F(2.2)


@pytest.fixture(scope="module")
def references():
    return {}


@pytest.mark.parametrize("shape", K.SHAPES, ids=["%dx%d" % s for s in K.SHAPES])
def test_sharpening_equals_the_restatement_bit_for_bit(references, shape):
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"
    w, h = shape
    for name, (make, changes) in K.CASES.items():
        m, c = make(w, h)
        changed = False
        for strength, limit in K.PARAMS:
            for e in K.EXPOSURES:
                want = K.reference(references, name, w, h, strength, limit, e)
                got = pt.sharpen(0, m, c, exposure=e, strength=strength, limit=limit)
                K.compare(got, want, (name, shape, float(strength), float(limit), float(e), "apart"))
                buf, prm = m.copy(), pt.SharpenParams(strength, limit)                     # out_rgb == mean_rgb
                assert pt.lib().pt_sharpen_host(0, w, h, pt._fp(buf), pt._ip(c), C.c_float(e), C.byref(prm), pt._fp(buf), None) == pt.PT_OK
                K.compare(buf, want, (name, shape, float(strength), float(limit), float(e), "in place"))
                changed |= bool((want.view(np.uint32) != m.view(np.uint32)).any())
        assert changed == changes(w, h), (name, shape)


def test_the_defaults_strength_zero_and_the_time():
    m, c = K.hdr(97, 31)
    want = R.sharpen(m, c, 1.0, 1.0, 0.1875)
    got, ms = pt.sharpen(0, m, c, want_ms=True)                                           # strength 1, limit 0 = 0.1875
    K.compare(got, want, "defaults")
    assert ms > 0
    same, ms = pt.sharpen(0, m, c, strength=0.0, limit=0.1, want_ms=True)
    assert (same.view(np.uint32) == m.view(np.uint32)).all() and ms == 0                  # a copy, NaN payloads included


def test_host_entry_point_holds_no_device_object_afterwards():
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    before = L.pt_test_live_device_objects()
    m, c = K.hostile(33, 9)
    K.compare(pt.sharpen(0, m, c, strength=0.5, library=L), R.sharpen(m, c, 1.0, 0.5), "test build")
    assert L.pt_test_live_device_objects() == before


@pytest.mark.parametrize("grade", [dict(), dict(curve="aces", exposure=3.0)], ids=["no grade", "aces at e = 3"])
def test_the_sums_form_through_a_display(models_dir, grade):
    """A present without a filter hands the stage the session's sums: the kernels divide, as the display chain does, and write a
    plane of the display's; the accumulators stay as they were."""
    w, h = 65, 47                            # partial tiles at both rims
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    g.set_camera(pt.look_at((-2.0, -5.0, -8.0), (0.0, 9.0, 0.0), aspect=w / h))
    ses = pt.Session(g, w, h)
    ses.render(0, 64, 4, error=-1.0, seed=42)   # (at a few samples the frame is lit pixels on black: no headroom, no change)
    s, s2, c = [np.array(a) for a in ses.read()]
    disp = pt.Display(ses)
    mean, count = pt.denoise(w, h, s, s2, c, None, levels=0)
    mean, count = np.asarray(mean, F).reshape(h, w, 3), np.asarray(count, np.int32).reshape(h, w)
    e = F(grade.get("exposure", 0.0) or 1.0)
    finish = lambda img: pt.quantize(pt.tonemap(w, h, pt.grade(img, count, e, grade.get("curve", 0)), count.reshape(-1), GAMMA), count)
    for prm in (dict(strength=1.0), dict(strength=0.25, limit=0.05)):
        got, info = disp.present(gamma=GAMMA, grade=grade or None, sharpen=prm)
        want = finish(R.sharpen(mean, count, e, **prm))
        assert (got == want).all(), (prm, int((got != want).sum()))
        assert (want != finish(mean)).any(), "the stage changed no byte"
        assert info["kernel_ms"] > 0
    again = ses.read()
    for a, b in zip((s, s2, c), again):
        assert (np.asarray(a).view(np.uint32) == np.asarray(b).view(np.uint32)).all()    # sharpened into the display's plane, not in place
