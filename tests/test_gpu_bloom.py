"""pt_bloom_host against the numpy restatement of the header's text (tests/bloom_restatement.py), bit for bit, at the smallest
shapes at which the kernels can go wrong: 1 x 1 and 3 x 2 (every level 1 x 1 or nearly), 33 x 9 (one pixel past a 32 x 8 tile),
66 x 18 and 67 x 19 (the region a down tile reads, and one more), 130 x 70 and 257 x 129 (several tiles, odd sizes at every
level); pyramids of 1, 2, 5 and 8 levels; exposures 2^-3, 1 and 2^4.  The images are tests/bloom_cases.py's: impulses at the corners,
edges and tile seams; a random field with holes and a few negative, NaN and infinite channels.  Both forms of the kernels' divide
go through the display path: tests/test_gpu_bloom_display.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bloom_cases as K
import bloom_restatement as B

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def references():
    return {}


@pytest.mark.parametrize("levels", K.LEVELS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=["%dx%d" % s for s in K.SHAPES])
def test_bloom_equals_the_restatement_bit_for_bit(references, shape, levels):
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"
    w, h = shape
    for name, make in K.CASES.items():
        m, c = make(w, h)
        for e, T in K.SETTINGS:
            got = pt.bloom(0, m, c, exposure=e, threshold=T, strength=K.STRENGTH, levels=levels)
            want = K.reference(references, name, w, h, levels, e, T)
            assert K.compare(got, want, (name, shape, levels, float(e))) >= 0.9


def test_in_place_the_defaults_strength_zero_and_the_time():
    m, c = K.field(67, 19)
    want = B.bloom(m, c, 1.0, 1.0, 0.5, 5)
    got, ms = pt.bloom(0, m, c, want_ms=True)                                     # threshold 1, strength 0.5, 5 levels
    K.compare(got, want, "defaults")
    assert ms > 0
    zeroed = pt.BloomParams(0.0, 0.5, 0)                                          # threshold 0 = 1, levels 0 = 5
    buf = m.copy()
    assert pt.lib().pt_bloom_host(0, 67, 19, pt._fp(buf), pt._ip(c), C.c_float(1.0), C.byref(zeroed), pt._fp(buf), None) == pt.PT_OK
    K.compare(buf, want, "in place, zeroed defaults")
    same, ms = pt.bloom(0, m, c, strength=0.0, want_ms=True)
    assert (same.view(np.uint32) == m.view(np.uint32)).all() and ms == 0          # a copy, NaN payloads included


def test_host_entry_point_holds_no_device_object_afterwards():
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    before = L.pt_test_live_device_objects()
    m, c = K.impulses(33, 9)
    K.compare(pt.bloom(0, m, c, strength=K.STRENGTH, levels=2, library=L), B.bloom(m, c, 1.0, 1.0, K.STRENGTH, 2), "test build")
    assert L.pt_test_live_device_objects() == before
