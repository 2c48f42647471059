"""pt_local_host against the numpy restatement of the header's text (tests/local_restatement.py), bit for bit, at the smallest
shapes at which the kernels can go wrong: 1 x 1, one row and one column; 31, 32 and 33 by 7, 8 and 9 (a 32 x 8 tile less one,
exactly, and one more, both ways); 65 x 17 and 257 x 129 (several tiles, partial ones at both rims).  Bases of 1, 2, 3, 5 and 8
levels: both spacings that are staged through LDS, the first that reads global memory, the default, and with 8 a reach of 510
pixels, beyond every image, so that most taps fall outside it.  Exposures 2^-3, 1 and 2^4; sigma 1e-20 (only equal values count),
the default and 1e20 (no edge stop).  The images are tests/local_cases.py's.  Both forms of the kernels' divide go through the
display path: tests/test_gpu_local_display.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import local_cases as K
import local_restatement as R

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def references():
    return {}


@pytest.mark.parametrize("levels", K.LEVELS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=["%dx%d" % s for s in K.SHAPES])
def test_local_exposure_equals_the_restatement_bit_for_bit(references, shape, levels):
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"
    w, h = shape
    for name, (make, changes) in K.CASES.items():
        m, c = make(w, h)
        for sigma in K.SIGMAS:
            for e in K.EXPOSURES:
                got = pt.local_exposure(0, m, c, exposure=e, strength=K.STRENGTH, pivot=K.PIVOT, levels=levels, sigma=sigma)
                want = K.reference(references, name, w, h, levels, sigma, e)
                K.compare(got, want, (name, shape, levels, float(sigma), float(e)))
                assert bool((want.view(np.uint32) != m.view(np.uint32)).any()) == changes, (name, shape, levels)


def test_in_place_the_defaults_strength_zero_and_the_time():
    m, c = K.field(65, 17)
    want = R.local_exposure(m, c, 1.0, 1.0, 0.18, 5, 0.5)
    got, ms = pt.local_exposure(0, m, c, want_ms=True)                            # strength 1, pivot 0.18, 5 levels, sigma 0.5
    K.compare(got, want, "defaults")
    assert ms > 0
    zeroed = pt.LocalParams(1.0, 0.0, 0, 0.0)                                     # pivot 0 = 0.18, levels 0 = 5, sigma 0 = 0.5
    buf = m.copy()
    assert pt.lib().pt_local_host(0, 65, 17, pt._fp(buf), pt._ip(c), C.c_float(1.0), C.byref(zeroed), pt._fp(buf), None) == pt.PT_OK
    K.compare(buf, want, "in place, zeroed defaults")
    same, ms = pt.local_exposure(0, m, c, strength=0.0, want_ms=True)
    assert (same.view(np.uint32) == m.view(np.uint32)).all() and ms == 0          # a copy, NaN payloads included


def test_host_entry_point_holds_no_device_object_afterwards():
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    before = L.pt_test_live_device_objects()
    m, c = K.impulses(33, 9)
    K.compare(pt.local_exposure(0, m, c, strength=K.STRENGTH, levels=3, library=L), R.local_exposure(m, c, 1.0, K.STRENGTH, 0.18, 3, 0.5), "test build")
    assert L.pt_test_live_device_objects() == before
