"""pt_display_present_grain against the host chain it is defined by (include/pt_hip.h): the row of the display's table up to the linear
mean and count at the output size, then pt_optics_host, then pt_meter_host -> pt_exposure_from_histogram if the exposure is
automatic, then pt_bloom_host -> pt_local_host -> pt_sharpen_host -> pt_colour_host -> grain and dithered quantization -- every byte.
The last step of the host chain is the numpy restatement (tests/grain_restatement.py), not the library's.  Tor.obj sessions of
64 x 48 whose camera looks up at the emitter, at 64 samples per pixel, as the sharpening tests render: a session hands the kernel
sums, so these are its dividing instantiations."""
import importlib

import numpy as np
import pytest

import grain_restatement as R

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
GRAIN = dict(strength=0.4, size=1.5, dither=1.0, seed=11)


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

    def bytes(self, mean, count, w, h, grade, bloom=None, local=None, colour=None, optics=None, sharpen=None, grain=None):
        """(the bytes, e)."""
        m = np.ascontiguousarray(mean, F).reshape(h, w, 3)
        count = np.ascontiguousarray(count, np.int32).reshape(h, w)
        if optics:
            m, count = pt.optics(0, m, count, **optics)
        if grade.get("auto_exposure"):
            e, _ = pt.exposure_from_histogram(pt.meter(m, count), grade, self.e_prev)     # metered before every later stage
            self.e_prev = e
        else:
            e = F(grade.get("exposure", 0.0) or 1.0)
        if bloom:
            m = pt.bloom(0, m, count, e, **dict(dict(threshold=1.0, levels=5), **bloom))
        if local:
            m = pt.local_exposure(0, m, count, e, **dict(dict(pivot=0.18, levels=5, sigma=0.5), **local))
        if sharpen:
            m = pt.sharpen(0, m, count, e, **sharpen)
        curve = grade.get("curve", 0)
        img = pt.colour(m, count, e, curve, colour) if colour else pt.grade(m, count, e, curve)
        if grain:
            return R.quantize(img, count, GAMMA, **grain), e
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
          "every other stage": dict(grade=AUTO, bloom=BLOOM, local=LOCAL, colour=COLOUR, optics=OPTICS, sharpen=SHARPEN)}


@pytest.mark.parametrize("stages", list(STAGES))
def test_the_bytes_are_the_host_chains(tor, stages):
    g, view = tor
    st = dict(STAGES[stages])
    grade = st.pop("grade")
    ses = pt.Session(g, W, H)
    disp, off, host, plain = pt.Display(ses), pt.Display(ses), HostChain(), HostChain()
    for i in range(2):                       # two presents in a row: the second metered one starts from the first one's exposure
        _frame(g, view, ses, i)
        grain = dict(GRAIN, frame=i)
        got, info = disp.present(gamma=GAMMA, grade=grade, grain=grain, **st)
        mean, count = _mean(ses)
        want, e = host.bytes(mean, count, W, H, grade, grain=grain, **st)
        _same(got, want, (stages, i))
        assert _bits(info["exposure"]) == _bits(e) and info["kernel_ms"] > 0
        without, e_off = plain.bytes(mean, count, W, H, grade, **st)
        assert (want != without).mean() > 0.02, "the stage changed few bytes: the test would pass without it"
        # the stage off: the same call without the keyword, the same bytes as before it existed, and the same metered exposure
        got_off, info_off = off.present(gamma=GAMMA, grade=grade, **st)
        _same(got_off, without, (stages, i, "off"))
        assert _bits(info_off["exposure"]) == _bits(info["exposure"]) == _bits(e_off)
    # grain alone and dither alone, and a pitch of 1
    mean, count = _mean(ses)
    alone = (dict(strength=0.5, seed=3), dict(dither=0.5, seed=3), dict(strength=0.2, size=8.0, dither=1.0, frame=2 ** 32 - 1))
    for prm in (() if grade.get("auto_exposure") else alone):      # (a metered present more would move the display's exposure on)
        got, _ = disp.present(gamma=GAMMA, grade=grade, grain=prm, **st)
        _same(got, HostChain().bytes(mean, count, W, H, grade, grain=prm, **st)[0], (stages, prm))


def test_a_scaled_present(tor):
    g, view = tor
    w, h = W // 2, H // 2                     # traced at 32 x 24, shown at 64 x 48: the stage runs at 64 x 48
    ses = pt.Session(g, w, h)
    disp, host = pt.Display(ses), HostChain()
    for i in range(2):
        _frame(g, view, ses, i, w, h)
        grain = dict(GRAIN, frame=i)
        got, info = disp.present(gamma=GAMMA, upsample={"scale": 2}, grade=AUTO, grain=grain)
        mean_lo, count_lo = _mean(ses, w, h)
        mean, count = pt.upsample(0, W, H, mean_lo, count_lo, view.render_features(W, H), scale=2)
        want, e = host.bytes(mean, count, W, H, AUTO, grain=grain)
        assert got.shape == (H, W, 3)
        _same(got, want, ("scaled", i))
        assert _bits(info["exposure"]) == _bits(e)


def test_three_temporal_frames_with_the_frame_advancing(tor):
    g, view = tor
    ses = pt.Session(g, W, H)
    disp, host, history = pt.Display(ses), HostChain(), pt.Temporal(view, W, H)
    for i in range(3):
        _frame(g, view, ses, i)
        grain = dict(GRAIN, frame=i)
        got, info = disp.present(gamma=GAMMA, temporal=True, grade=AUTO, grain=grain)
        s, s2, c = ses.read()
        out = history.push(s, s2, c, denoise=None)
        mean, count = pt.denoise(W, H, out["sum"], out["sum2"], out["count"], None, levels=0)
        want, e = host.bytes(mean, count, W, H, AUTO, grain=grain)
        _same(got, want, ("temporal", i))
        assert _bits(info["exposure"]) == _bits(e)
        # the same image under the next frame's noise is another one
        assert (want != HostChain().bytes(mean, count, W, H, dict(AUTO, auto_exposure=False, exposure=float(e)), grain=dict(GRAIN, frame=i + 1))[0]).mean() > 0.02


def test_a_zeroed_block_is_present_sharpen(tor):
    g, view = tor
    ses = pt.Session(g, W, H)
    _frame(g, view, ses, 0)
    disp = pt.Display(ses)
    for kw in (dict(grade=MANUAL, sharpen=SHARPEN), dict(grade=AUTO, bloom=BLOOM, local=LOCAL), dict(grade=AUTO, colour=COLOUR, optics=OPTICS, sharpen=SHARPEN),
               dict(grade={})):
        before, binfo = disp.present(gamma=GAMMA, **kw)
        for zero in (dict(), dict(size=3.0, seed=5, frame=9), pt.GrainParams()):
            disp.reset()
            got, info = disp.present(gamma=GAMMA, grain=zero, **kw)
            _same(got, before, (kw, zero))
            assert _bits(info["exposure"]) == _bits(binfo["exposure"])
        disp.reset()


def test_a_refused_block_leaves_history_and_exposure_alone(tor):
    g, view = tor
    ses = pt.Session(g, W, H)
    disp, host, history = pt.Display(ses), HostChain(), pt.Temporal(view, W, H)

    def good(i):
        _frame(g, view, ses, i)
        grain = dict(GRAIN, frame=i)
        got, info = disp.present(gamma=GAMMA, temporal=True, grade=AUTO, bloom=BLOOM, grain=grain)
        s, s2, c = ses.read()
        out = history.push(s, s2, c, denoise=None)
        mean, count = pt.denoise(W, H, out["sum"], out["sum2"], out["count"], None, levels=0)
        want, e = host.bytes(mean, count, W, H, AUTO, bloom=BLOOM, grain=grain)
        _same(got, want, i)
        assert _bits(info["exposure"]) == _bits(e)

    good(0)
    good(1)
    _frame(g, view, ses, 2)
    for bad in (dict(strength=-1.0), dict(strength=float("nan")), dict(strength=1.5), dict(strength=0.5, size=0.5), dict(size=9.0),
                dict(dither=float("inf")), dict(dither=-0.1), dict(strength=0.5, dither=2.0)):
        with pytest.raises(pt.PtError) as err:
            disp.present(gamma=GAMMA, temporal=True, grade=AUTO, bloom=BLOOM, grain=bad)
        assert err.value.status == pt.PT_ERR_INVALID_ARGUMENT
    with pytest.raises(pt.PtError):
        disp.present(gamma=GAMMA, temporal=True, grade=dict(curve=9), bloom=BLOOM, grain=GRAIN)
    good(2)                                    # what it would have been without the refused calls


def test_the_stage_holds_no_device_object_of_its_own(models_dir):
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    L.pt_test_set_mutation(b"reset", 0.0)
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=L)
    ses = pt.Session(g, W // 2, H // 2)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    disp = pt.Display(ses)
    disp.present(gamma=GAMMA, grade=MANUAL, bloom=BLOOM)
    held = L.pt_test_live_device_objects()
    disp.present(gamma=GAMMA, grade=MANUAL, bloom=BLOOM, grain=GRAIN)          # inside the display kernel: no plane is added
    assert L.pt_test_live_device_objects() == held
    disp.close()
