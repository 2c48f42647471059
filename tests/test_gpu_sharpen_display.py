"""pt_display_present_sharpen against the host chain it is defined by (include/pt_hip.h): the row of the display's table up to the
linear mean and count at the output size, then pt_optics_host, then pt_meter_host -> pt_exposure_from_histogram if the exposure is
automatic, then pt_bloom_host -> pt_local_host -> sharpening -> pt_colour_host -> pt_tonemap -> pt_quantize -- every byte.  The
sharpening of the host chain is the numpy restatement (tests/sharpen_restatement.py), not the library's.  Tor.obj sessions of
64 x 48 whose camera looks up at the emitter, at 64 samples per pixel: at a few, an unfiltered frame is single lit pixels on black,
and between a black ring and a lit pixel there is no headroom -- every lobe is 0, and the stage rightly changes no byte."""
import importlib

import numpy as np
import pytest

import sharpen_restatement as R

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu

F = np.float32
GAMMA = F(1) / F(2.2)
W, H, SPP, MRR = 64, 48, 64, 4
MANUAL = dict(curve="aces", exposure=3.0)
AUTO = dict(curve="aces", auto_exposure=True, percentile=20, key=1.0, rate=0.5)
BLOOM = dict(strength=0.8, levels=4)
LOCAL = dict(strength=1.5, levels=4)
COLOUR = dict(wb=(1.1, 1.0, 0.9), saturation=0.8)
OPTICS = dict(k1=-0.3, k2=0.05, ca=0.02, vignette=1.5)
SHARPEN = dict(strength=0.75)


def _cam(i, w=W, h=H):
    return pt.look_at((-2.0 + 2.0 * i, -5.0, -8.0 - i), (0.0, 9.0, 0.0), aspect=w / h)


@pytest.fixture()
def tor(models_dir):
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    return g, g.clone_to_device(0)          # the handle that renders, and the host chain's own (its Temporal lives on it)


class HostChain:
    """The host chain from the linear mean on, with the previous exposure a display would keep."""

    def __init__(self):
        self.e_prev = None

    def bytes(self, mean, count, w, h, grade, bloom=None, local=None, colour=None, optics=None, sharpen=None):
        """(the bytes, e)."""
        m = np.ascontiguousarray(mean, F).reshape(h, w, 3)
        count = np.ascontiguousarray(count, np.int32).reshape(h, w)
        if optics:
            m, count = pt.optics(0, m, count, **optics)
        if grade.get("auto_exposure"):
            e, _ = pt.exposure_from_histogram(pt.meter(m, count), grade, self.e_prev)     # metered before bloom, local exposure and the stage
            self.e_prev = e
        else:
            e = F(grade.get("exposure", 0.0) or 1.0)
        if bloom:
            m = pt.bloom(0, m, count, e, **dict(dict(threshold=1.0, levels=5), **bloom))
        if local:
            m = pt.local_exposure(0, m, count, e, **dict(dict(pivot=0.18, levels=5, sigma=0.5), **local))
        if sharpen:
            m = R.sharpen(m, count, e, **sharpen)
        curve = grade.get("curve", 0)
        img = pt.colour(m, count, e, curve, colour) if colour else pt.grade(m, count, e, curve)
        return pt.quantize(pt.tonemap(w, h, img, count, GAMMA), count), e


def _same(got, want, where):
    bad = got != want
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _bits(x):
    return F(x).view(np.uint32)


def _frame(g, view, ses, i, w=W, h=H):
    cam = _cam(i, w, h)
    g.set_camera(cam)
    view.set_camera(cam)
    ses.clear()
    ses.render(i * SPP, SPP, MRR, error=-1.0, seed=42)


def _mean(ses, w=W, h=H):
    s, s2, c = ses.read()
    return pt.denoise(w, h, s, s2, c, None, levels=0)


STAGES = {"alone": dict(grade={}), "manual": dict(grade=MANUAL), "auto-exposure": dict(grade=AUTO),
          "bloom+local+colour+optics": dict(grade=AUTO, bloom=BLOOM, local=LOCAL, colour=COLOUR, optics=OPTICS)}


@pytest.mark.parametrize("stages", list(STAGES))
def test_the_bytes_are_the_host_chains(tor, stages):
    g, view = tor
    st = dict(STAGES[stages])
    grade = st.pop("grade")
    ses = pt.Session(g, W, H)
    disp, off, host, plain = pt.Display(ses), pt.Display(ses), HostChain(), HostChain()
    for i in range(2):                       # two presents in a row: the second metered one starts from the first one's exposure
        _frame(g, view, ses, i)
        got, info = disp.present(gamma=GAMMA, grade=grade, sharpen=SHARPEN, **st)
        mean, count = _mean(ses)
        want, e = host.bytes(mean, count, W, H, grade, sharpen=SHARPEN, **st)
        _same(got, want, (stages, i))
        assert _bits(info["exposure"]) == _bits(e) and info["kernel_ms"] > 0
        without, e_off = plain.bytes(mean, count, W, H, grade, **st)
        assert (want != without).any(), "the stage changed no byte: the test would pass without it"
        assert info["deferred_pixels"] <= 0.01 * W * H, info
        # the stage off: the same call without the keyword, the same bytes as before it existed, and the same metered exposure
        got_off, info_off = off.present(gamma=GAMMA, grade=grade, **st)
        _same(got_off, without, (stages, i, "off"))
        assert _bits(info_off["exposure"]) == _bits(info["exposure"]) == _bits(e_off)


def test_a_scaled_present(tor):
    g, view = tor
    w, h = W // 2, H // 2                     # traced at 32 x 24, shown at 64 x 48: the stage runs at 64 x 48
    ses = pt.Session(g, w, h)
    disp, host = pt.Display(ses), HostChain()
    for i in range(2):
        _frame(g, view, ses, i, w, h)
        got, info = disp.present(gamma=GAMMA, upsample={"scale": 2}, grade=AUTO, sharpen=SHARPEN)
        mean_lo, count_lo = _mean(ses, w, h)
        mean, count = pt.upsample(0, W, H, mean_lo, count_lo, view.render_features(W, H), scale=2)
        want, e = host.bytes(mean, count, W, H, AUTO, sharpen=SHARPEN)
        assert got.shape == (H, W, 3)
        _same(got, want, ("scaled", i))
        assert _bits(info["exposure"]) == _bits(e)
        assert (want != HostChain().bytes(mean, count, W, H, dict(AUTO, auto_exposure=False, exposure=float(e)))[0]).any()


def test_three_temporal_frames(tor):
    g, view = tor
    ses = pt.Session(g, W, H)
    disp, host, history = pt.Display(ses), HostChain(), pt.Temporal(view, W, H)
    for i in range(3):
        _frame(g, view, ses, i)
        got, info = disp.present(gamma=GAMMA, temporal=True, grade=AUTO, sharpen=SHARPEN)
        s, s2, c = ses.read()
        out = history.push(s, s2, c, denoise=None)
        mean, count = pt.denoise(W, H, out["sum"], out["sum2"], out["count"], None, levels=0)
        want, e = host.bytes(mean, count, W, H, AUTO, sharpen=SHARPEN)
        _same(got, want, ("temporal", i))
        assert _bits(info["exposure"]) == _bits(e)


def test_a_zeroed_block_is_the_call_without_it(tor):
    g, view = tor
    ses = pt.Session(g, W, H)
    _frame(g, view, ses, 0)
    disp = pt.Display(ses)
    for kw in (dict(grade=MANUAL), dict(grade=AUTO, bloom=BLOOM, local=LOCAL), dict(grade=AUTO, colour=COLOUR, optics=OPTICS), dict(grade={})):
        before, binfo = disp.present(gamma=GAMMA, **kw)
        for zero in (dict(), dict(strength=0.0, limit=0.1), pt.SharpenParams()):
            disp.reset()
            got, info = disp.present(gamma=GAMMA, sharpen=zero, **kw)
            _same(got, before, (kw, zero))
            assert _bits(info["exposure"]) == _bits(binfo["exposure"])
        disp.reset()
    # another strength and another limit against the host chain, and they differ
    mean, count = _mean(ses)
    seen = set()
    for prm in (dict(strength=1.0), dict(strength=0.25), dict(strength=1.0, limit=0.05)):
        got, _ = disp.present(gamma=GAMMA, grade=MANUAL, sharpen=prm)
        _same(got, HostChain().bytes(mean, count, W, H, MANUAL, sharpen=prm)[0], prm)
        seen.add(got.tobytes())
    assert len(seen) == 3


def test_a_refused_block_leaves_history_and_exposure_alone(tor):
    g, view = tor
    ses = pt.Session(g, W, H)
    disp, host, history = pt.Display(ses), HostChain(), pt.Temporal(view, W, H)

    def good(i):
        _frame(g, view, ses, i)
        got, info = disp.present(gamma=GAMMA, temporal=True, grade=AUTO, bloom=BLOOM, sharpen=SHARPEN)
        s, s2, c = ses.read()
        out = history.push(s, s2, c, denoise=None)
        mean, count = pt.denoise(W, H, out["sum"], out["sum2"], out["count"], None, levels=0)
        want, e = host.bytes(mean, count, W, H, AUTO, bloom=BLOOM, sharpen=SHARPEN)
        _same(got, want, i)
        assert _bits(info["exposure"]) == _bits(e)

    good(0)
    good(1)
    _frame(g, view, ses, 2)
    for bad in (dict(strength=-1.0), dict(strength=float("nan")), dict(strength=1.5), dict(strength=1.0, limit=0.25),
                dict(strength=1.0, limit=float("inf")), dict(limit=-0.1)):
        with pytest.raises(pt.PtError) as err:
            disp.present(gamma=GAMMA, temporal=True, grade=AUTO, bloom=BLOOM, sharpen=bad)
        assert err.value.status == pt.PT_ERR_INVALID_ARGUMENT
    with pytest.raises(pt.PtError):
        disp.present(gamma=GAMMA, temporal=True, grade=dict(curve=9), bloom=BLOOM, sharpen=SHARPEN)
    good(2)                                    # what it would have been without the refused calls


def test_device_objects_return_to_where_they_were(models_dir):
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    L.pt_test_set_mutation(b"reset", 0.0)
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=L)
    ses = pt.Session(g, W // 2, H // 2)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    disp = pt.Display(ses)
    disp.present(gamma=GAMMA, grade=MANUAL, bloom=BLOOM)
    held = L.pt_test_live_device_objects()     # a display that never uses the stage holds what it held before
    disp.present(gamma=GAMMA, grade=MANUAL, bloom=BLOOM, sharpen=dict())
    assert L.pt_test_live_device_objects() == held
    disp.present(gamma=GAMMA, grade=MANUAL, bloom=BLOOM, sharpen=SHARPEN)      # behind bloom: the luminance plane alone, in bloom's plane
    assert L.pt_test_live_device_objects() == held + 1
    disp.present(gamma=GAMMA, grade=MANUAL, sharpen=SHARPEN)                   # on the session's sums: the plane of means too, one object still
    assert L.pt_test_live_device_objects() == held + 1
    disp.present(gamma=GAMMA, grade=MANUAL, bloom=BLOOM, sharpen=SHARPEN)
    assert L.pt_test_live_device_objects() == held + 1
    disp.close()
    before = L.pt_test_live_device_objects()
    disp = pt.Display(ses)
    for scale in (2, 3, 2):                    # the scaled display's planes follow its size
        disp.present(gamma=GAMMA, upsample={"scale": scale}, grade=AUTO, sharpen=SHARPEN)
        disp.present(gamma=GAMMA, grade=MANUAL, sharpen=dict(strength=0.5, limit=0.1))
    assert L.pt_test_live_device_objects() > before
    disp.close()
    assert L.pt_test_live_device_objects() == before
