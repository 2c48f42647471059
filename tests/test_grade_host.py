"""Display grading on the host (include/pt_hip.h: pt_grade_host, pt_exposure_from_histogram) against the numpy restatement of the
header's text, bit for bit; the parameter checks; the struct layouts; and that the saturating curves do not wrap.  No device."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import grade_restatement as R

pt = importlib.import_module("path-tracing_amd")
F = np.float32
EXPOSURES = [F(2.0 ** -8), F(0.3), F(1.0), F(2.0 ** 8)]


def _below(x):
    return np.nextafter(F(x), F(-np.inf))


def _above(x):
    return np.nextafter(F(x), F(np.inf))


def _values():
    v = [0.0, 1e-45, 1e-40, 1.1754942e-38, 1.0, _below(1), _above(1), 0.999, 1.001, 2.0, 1e6, np.inf, -0.0, -1e-3, -1.0, -np.inf, np.nan,
         0.18, 0.5, 3.4e38, 1.0 / 256, 255.0, 256.0, 1.0 / 0.3]
    rng = np.random.default_rng(7)
    v += list(np.exp2(rng.uniform(-20, 20, 231)))
    return np.array(v, F)


def _image():
    v = _values()
    m = np.stack([v, np.roll(v, 1), np.roll(v, 5)], axis=1).reshape(1, -1, 3)
    c = np.ones(m.shape[1], np.int32)
    c[::7] = 0
    c[3] = -2                                     # any count but 0 is "has samples"
    return np.ascontiguousarray(m), c


def _same_bits(a, b, where):
    a, b = np.asarray(a, F), np.asarray(b, F)
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), (where, np.argwhere(bad)[:4].tolist(), a[bad][:4], b[bad][:4])


@pytest.mark.parametrize("curve", R.CURVES)
def test_grade_equals_the_restatement_bit_for_bit(curve):
    m, c = _image()
    for e in EXPOSURES:
        got = pt.grade(m, c, e, curve)
        _same_bits(got, R.grade(m, c.reshape(1, -1), e, curve), (curve, e))
        skipped = c == 0
        _same_bits(got[0, skipped], m[0, skipped], "pixels without samples pass through")


def test_grade_by_name_and_in_place():
    m, c = _image()
    _same_bits(pt.grade(m, c, 0.3, "aces"), pt.grade(m, c, 0.3, pt.CURVE_ACES), "name")
    buf = m.copy()
    assert pt.lib().pt_grade_host(m.shape[1], 1, pt._fp(buf), pt._ip(c), C.c_float(0.3), pt.CURVE_REINHARD, pt._fp(buf)) == pt.PT_OK
    _same_bits(buf, pt.grade(m, c, 0.3, pt.CURVE_REINHARD), "in place")


def test_reference_with_unit_exposure_changes_no_byte():
    m, c = _image()
    keep = np.isfinite(m).all(axis=2)[0] & (m >= 0).all(axis=2)[0]
    m, c = np.ascontiguousarray(m[:, keep]), c[keep]
    g = pt.grade(m, c, 1.0, pt.CURVE_REFERENCE)
    _same_bits(g, m, "x = m * 1")
    w = m.shape[1]
    assert np.array_equal(pt.quantize(pt.tonemap(w, 1, g, c), c.reshape(1, w)), pt.quantize(pt.tonemap(w, 1, m, c), c.reshape(1, w)))


def test_grade_refuses_bad_arguments():
    L = pt.lib()
    m, c = _image()
    w = m.shape[1]
    out = np.full_like(m, 7.0)
    for e, curve in [(0.0, 0), (-1.0, 0), (float("nan"), 1), (float("inf"), 2), (1.0, 4), (1.0, -1)]:
        assert L.pt_grade_host(w, 1, pt._fp(m), pt._ip(c), C.c_float(e), curve, pt._fp(out)) == pt.PT_ERR_INVALID_ARGUMENT, (e, curve)
    assert L.pt_grade_host(w, 1, None, pt._ip(c), C.c_float(1), 0, pt._fp(out)) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_grade_host(w, 1, pt._fp(m), None, C.c_float(1), 0, pt._fp(out)) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_grade_host(w, 1, pt._fp(m), pt._ip(c), C.c_float(1), 0, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_grade_host(0, 1, pt._fp(m), pt._ip(c), C.c_float(1), 0, pt._fp(out)) == pt.PT_ERR_INVALID_ARGUMENT
    assert (out == 7.0).all()


@pytest.mark.parametrize("curve", [R.CLAMP, R.REINHARD, R.ACES])
def test_saturating_curves_do_not_wrap(curve):
    """Finite, non-negative means at the default gamma: the level (int)(pow(g, gamma) * 255) stays at or below 255 whatever the
    exposure, so the byte is the level and brighter never turns darker through the wrap.  Means up to 2^40: with e <= 2^8 every
    intermediate of the curves stays finite (the largest, 2.51 x^2 of ACES, is below 2^98).  Beyond x = 2^63 or so the header's
    arithmetic itself gives inf / inf = NaN (no special case, as it says), which is not a wrap but is not white either."""
    rng = np.random.default_rng(11)
    v = np.concatenate([np.exp2(rng.uniform(-30, 40, 30000)).astype(F), np.array([0, 1e-45, 1, 2, _above(1), 2.0 ** 40, 1e6], F)])
    v = v[: len(v) // 3 * 3]
    m = v.reshape(1, -1, 3)
    w = m.shape[1]
    c = np.ones(w, np.int32)
    for e in EXPOSURES:
        g = pt.grade(m, c, e, curve)
        assert np.isfinite(g).all() and (g >= 0).all() and (g <= 1).all(), (curve, e)
        tone = pt.tonemap(w, 1, g, c)
        assert (tone >= 0).all() and (tone < 256).all(), (curve, e, float(tone.max()))
        assert np.array_equal(pt.quantize(tone, c.reshape(1, w)).reshape(-1, 3)[:, ::-1], tone.astype(np.int64).reshape(-1, 3))


def test_the_emitter_is_white_under_clamp_and_wraps_under_reference():
    m = np.full((1, 1, 3), 2.0, F)                                   # Tor.obj's emitter: Ke = 2
    c = np.ones(1, np.int32)
    byte = lambda curve: pt.quantize(pt.tonemap(1, 1, pt.grade(m, c, 1.0, curve), c), c.reshape(1, 1))[0, 0].tolist()
    assert byte(pt.CURVE_REFERENCE) == [93, 93, 93]                  # level 349 & 255
    assert byte(pt.CURVE_CLAMP) == [255, 255, 255]
    assert 93 < byte(pt.CURVE_REINHARD)[0] < byte(pt.CURVE_ACES)[0] < 255      # 2 / 3 and 10.1 / 11.04: bright, not yet white


# ---- the exposure rule --------------------------------------------------------------------------------------------------

def _hist(entries):
    h = np.zeros(R.ENTRIES, np.uint32)
    for b, n in entries.items():
        h[b] = n
    return h


HISTOGRAMS = {
    "empty": _hist({}),
    "only dark": _hist({128: 1000}),
    "bin 0": _hist({0: 5}),
    "bin 64": _hist({64: 1}),
    "bin 127": _hist({127: 4000000000}),
    "two bins, a tie at the median": _hist({40: 50, 80: 50}),
    "tie at 1 percent": _hist({3: 1, 70: 99}),
    "just short of the tie": _hist({40: 49, 80: 51}),
    "spread": _hist({b: (b * 37) % 11 + 1 for b in range(0, 128, 3)}),
    "large counts": _hist({40: 4294967295, 41: 4294967295, 100: 4294967295, 128: 7}),
}
RULES = [dict(), dict(percentile=1), dict(percentile=50), dict(percentile=100), dict(rate=0.25), dict(rate=1.0), dict(rate=0.0),
         dict(rate=3.0), dict(key=0.5, percentile=90), dict(e_min=0.5, e_max=2.0), dict(e_min=1.0, e_max=1.0), dict(e_min=300.0, e_max=0.0 + 1000.0),
         dict(key=1e-6), dict(key=1e6, rate=0.5)]


@pytest.mark.parametrize("name", list(HISTOGRAMS))
def test_exposure_equals_the_restatement(name):
    h = HISTOGRAMS[name]
    for prm, e_prev in itertools.product(RULES, [None, F(1.0), F(0.0123), F(200.0)]):
        got = pt.exposure_from_histogram(h, dict(prm), e_prev)
        want = R.exposure(h, R.rule(**prm), e_prev)
        assert got[0].view(np.uint32) == want[0].view(np.uint32) and got[1].view(np.uint32) == want[1].view(np.uint32), (name, prm, e_prev, got, want)


def test_exposure_known_answers():
    E = pt.exposure_from_histogram
    assert E(HISTOGRAMS["empty"]) == (1.0, 1.0) and E(HISTOGRAMS["empty"], e_prev=F(3.5)) == (3.5, 3.5)
    assert E(HISTOGRAMS["only dark"], dict(rate=0.25), e_prev=F(0.75)) == (0.75, 0.75)
    assert R.edge(0) == F(2.0 ** -16) and R.edge(64) == F(1.0) and R.edge(65) == F(1.25) and R.edge(127) == F(1.75 * 2.0 ** 15)
    assert E(HISTOGRAMS["bin 64"]) == (F(0.18), F(0.18))                           # key / 1
    assert E(HISTOGRAMS["bin 0"]) == (256.0, 256.0) and E(HISTOGRAMS["bin 127"]) == (F(2.0 ** -8), F(2.0 ** -8))     # clamped at both ends
    tie = HISTOGRAMS["two bins, a tie at the median"]
    assert R.edge(40) == F(2.0 ** -6) and R.edge(80) == F(16.0)
    assert E(tie)[1] == F(F(0.18) / F(2.0 ** -6)) and E(HISTOGRAMS["just short of the tie"])[1] == F(F(0.18) / F(16.0))
    assert E(tie, dict(percentile=51))[1] == F(F(0.18) / F(16.0))                  # one percent more reaches into the upper bin
    first = E(HISTOGRAMS["bin 64"], dict(rate=0.25))                               # a first frame jumps to the target
    assert first == (F(0.18), F(0.18))
    nxt = E(HISTOGRAMS["bin 0"], dict(rate=0.25), e_prev=first[0])
    assert nxt[1] == 256.0 and nxt[0] == F(F(0.18) + F(F(F(256.0) - F(0.18)) * F(0.25)))
    assert E(HISTOGRAMS["bin 0"], dict(rate=0.0), e_prev=first[0])[0] == 256.0     # rate 0 is the default, 1


BAD_PARAMS = [dict(curve=4), dict(curve=-1), dict(exposure=-1.0), dict(exposure=float("nan")), dict(exposure=float("inf")),
              dict(percentile=-1), dict(percentile=101), dict(key=-0.1), dict(key=float("nan")), dict(key=float("inf")),
              dict(e_min=-1.0), dict(e_min=float("inf")), dict(e_max=-1.0), dict(e_max=float("nan")), dict(rate=-0.5), dict(rate=float("nan")),
              dict(rate=float("inf")), dict(e_min=2.0, e_max=1.0), dict(e_min=300.0), dict(e_max=0.001)]


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=[str(b) for b in BAD_PARAMS])
def test_invalid_parameters_are_refused_and_nothing_is_written(bad):
    L = pt.lib()
    h = HISTOGRAMS["spread"]
    gp = pt._grade_params(dict(bad))
    e, t = C.c_float(-7.0), C.c_float(-7.0)
    rc = L.pt_exposure_from_histogram(h.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(gp), 1, C.c_float(1.0), C.byref(e), C.byref(t))
    assert rc == pt.PT_ERR_INVALID_ARGUMENT and e.value == -7.0 and t.value == -7.0
    # the device entry points check the same parameters before they look at a device: device -1 would be PT_ERR_NO_DEVICE
    m, c, out = np.zeros(3, F), np.ones(1, np.int32), np.full(3, 9, np.uint8)
    rc = L.pt_display_bytes_graded_host(-1, 1, 1, pt._fp(m), pt._ip(c), C.c_float(0.45), C.byref(gp), 0, C.c_float(0), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        None, None)
    assert rc == pt.PT_ERR_INVALID_ARGUMENT and (out == 9).all()


def test_null_pointers_and_no_device():
    L = pt.lib()
    h = HISTOGRAMS["spread"]
    hp = h.ctypes.data_as(C.POINTER(C.c_uint32))
    gp = pt.GradeParams()
    e, t = C.c_float(-7.0), C.c_float(-7.0)
    assert L.pt_exposure_from_histogram(None, C.byref(gp), 0, C.c_float(0), C.byref(e), C.byref(t)) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_exposure_from_histogram(hp, None, 0, C.c_float(0), C.byref(e), C.byref(t)) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_exposure_from_histogram(hp, C.byref(gp), 0, C.c_float(0), None, C.byref(t)) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_exposure_from_histogram(hp, C.byref(gp), 0, C.c_float(0), C.byref(e), None) == pt.PT_ERR_INVALID_ARGUMENT
    assert e.value == -7.0 and t.value == -7.0
    m, c = np.zeros(3, F), np.ones(1, np.int32)
    assert L.pt_meter_host(-1, 1, 1, None, pt._ip(c), hp, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_meter_host(-1, 1, 1, pt._fp(m), None, hp, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_meter_host(-1, 1, 1, pt._fp(m), pt._ip(c), None, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_meter_host(-1, 0, 1, pt._fp(m), pt._ip(c), hp, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_meter_host(-1, 1, 1, pt._fp(m), pt._ip(c), hp, None) == 4                   # PT_ERR_NO_DEVICE: there is no CPU fallback
    out = np.zeros(3, np.uint8)
    assert L.pt_display_present_graded(None, None, None, C.byref(gp), out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_display_bytes_graded_host(-1, 1, 1, pt._fp(m), pt._ip(c), C.c_float(0.45), None, 0, C.c_float(0), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          None, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_display_bytes_graded_host(-1, 1, 1, pt._fp(m), pt._ip(c), C.c_float(0.45), C.byref(gp), 0, C.c_float(0),
                                          out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None) == 4


def test_struct_layouts_match_the_header():
    G, I = pt.GradeParams, pt.GradeInfo
    assert C.sizeof(G) == 32 and C.sizeof(I) == 16
    assert [getattr(G, k).offset for k, _ in G._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [getattr(I, k).offset for k, _ in I._fields_] == [0, 4, 8, 12]
    assert [k for k, _ in G._fields_] == ["curve", "exposure", "auto_exposure", "percentile", "key", "e_min", "e_max", "rate"]
    # ... and against what the compiler makes of include/pt_hip.h
    import os
    import shutil
    import subprocess
    import tempfile
    if shutil.which("g++") is None:
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.cpp")
        open(src, "w").write('#include <cstddef>\n#include <cstdio>\n#include "pt_hip.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                             "sizeof(pt_grade_params), offsetof(pt_grade_params, exposure), offsetof(pt_grade_params, auto_exposure), "
                             "offsetof(pt_grade_params, percentile), offsetof(pt_grade_params, key), offsetof(pt_grade_params, rate), "
                             "sizeof(pt_grade_info), offsetof(pt_grade_info, target), offsetof(pt_grade_info, dark)); }\n")
        exe = os.path.join(d, "layout")
        subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(root, "include"), src, "-o", exe])
        assert subprocess.check_output([exe], text=True).split() == ["32", "4", "8", "12", "16", "28", "16", "4", "12"]
