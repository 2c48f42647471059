"""pt_display_present_bloom against the host chain it is defined by (include/pt_hip.h): the row of the display's table up to the
linear mean and count, then pt_meter_host -> pt_exposure_from_histogram on the mean before bloom if the exposure is automatic,
then bloom -> pt_grade_host -> pt_tonemap -> pt_quantize -- every byte.  The bloom of the host chain is the numpy restatement
(tests/bloom_restatement.py), not the library's.  A Tor.obj session of 64 x 48 whose camera looks up at the emitter; a low
percentile brought to a high key opens the exposure until the light is far above the threshold.  The rows without a filter hand the bloom kernels sums
(their divide), the filtered and the scaled ones means."""
import importlib

import numpy as np
import pytest

import bloom_restatement as B

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu

F = np.float32
GAMMA = F(1) / F(2.2)
W, H, SPP, MRR = 64, 48, 4, 4
ROWS = [(False, None), (False, {"levels": 3}), (True, None), (True, {"levels": 3})]
ROW_IDS = ["resolve", "denoise", "temporal", "temporal+denoise"]
MANUAL = dict(curve="aces", exposure=3.0)
AUTO = dict(curve="aces", auto_exposure=True, percentile=20, key=1.0, rate=0.5)      # the 20th percentile at 1: the light (a mean of 1) far above it
BLOOM = dict(strength=0.8, levels=4)


def _cam(i, w=W, h=H):
    return pt.look_at((-2.0 + 2.0 * i, -5.0, -8.0 - i), (0.0, 9.0, 0.0), aspect=w / h)      # the emitter: a quad at y = 9 around x = z = 0


@pytest.fixture()
def tor(models_dir):
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0)
    return g, g.clone_to_device(0)          # the handle that renders, and the host chain's own (its Temporal lives on it)


def _linear_mean(view, acc, history, denoise, w=W, h=H):
    """The row of the display's table up to the linear mean and its count."""
    s, s2, c = acc
    if history is not None:
        out = history.push(s, s2, c, denoise=denoise)
        if denoise:
            return out["mean_rgb"], out["mean_count"]
        s, s2, c = out["sum"], out["sum2"], out["count"]
    elif denoise:
        return pt.denoise(w, h, s, s2, c, view.render_features(w, h), **denoise)
    return pt.denoise(w, h, s, s2, c, None, levels=0)


class HostChain:
    """The host chain from the linear mean on, with the previous exposure a display would keep."""

    def __init__(self):
        self.e_prev = None

    def bytes(self, mean, count, w, h, grade, bloom):
        m = np.ascontiguousarray(mean, F).reshape(h, w, 3)
        count = np.ascontiguousarray(count, np.int32)
        if grade.get("auto_exposure"):
            e, _ = pt.exposure_from_histogram(pt.meter(m, count), grade, self.e_prev)       # metered before bloom
            self.e_prev = e
        else:
            e = F(grade.get("exposure", 0.0) or 1.0)
        finish = lambda img: pt.quantize(pt.tonemap(w, h, pt.grade(img, count, e, grade.get("curve", 0)), count, GAMMA), count.reshape(h, w))
        bloomed = finish(B.bloom(m, count.reshape(h, w), e, **bloom)) if bloom else None
        return bloomed, finish(m), e


def _same(got, want, where):
    bad = got != want
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _same_float(a, b, where):
    assert F(a).view(np.uint32) == F(b).view(np.uint32), (where, a, b)


def _frame(g, view, ses, i):
    cam = _cam(i)
    g.set_camera(cam)
    view.set_camera(cam)
    ses.clear()
    ses.render(i * SPP, SPP, MRR, error=-1.0, seed=42)


@pytest.mark.parametrize("grade", [MANUAL, AUTO], ids=["manual", "automatic"])
@pytest.mark.parametrize("temporal,denoise", ROWS, ids=ROW_IDS)
def test_rows_of_the_table(tor, temporal, denoise, grade):
    g, view = tor
    ses = pt.Session(g, W, H)
    disp, host = pt.Display(ses), HostChain()
    history = pt.Temporal(view, W, H) if temporal else None
    for i in range(2):                       # two presents in a row: the second metered one starts from the first one's exposure
        _frame(g, view, ses, i)
        got, info = disp.present(gamma=GAMMA, temporal=True if temporal else None, denoise=denoise, grade=grade, bloom=BLOOM)
        mean, count = _linear_mean(view, ses.read(), history, denoise)
        want, graded_only, e = host.bytes(mean, count, W, H, grade, BLOOM)
        _same(got, want, (i,))
        _same_float(info["exposure"], e, i)
        assert info["kernel_ms"] > 0
        assert (want != graded_only).any(), "the bloom changed no byte: the test would pass without it"
        lum = B.luminance(np.asarray(mean, F).reshape(-1, 3)[np.asarray(count).reshape(-1) != 0])
        assert (lum * e > 2).any()            # the light is well above the threshold after exposure
    if grade is AUTO:
        assert host.e_prev is not None and info["metered"] + info["dark"] == int((np.asarray(count) != 0).sum())


@pytest.mark.parametrize("grade", [MANUAL, AUTO], ids=["manual", "automatic"])
def test_a_scaled_present(tor, grade):
    g, view = tor
    w, h = W // 2, H // 2                     # traced at 32 x 24, shown at 64 x 48
    ses = pt.Session(g, w, h)
    disp, host, history = pt.Display(ses), HostChain(), pt.Temporal(view, w, h)
    for i in range(2):
        cam = _cam(i, w, h)
        g.set_camera(cam)
        view.set_camera(cam)
        ses.clear()
        ses.render(i * SPP, SPP, MRR, error=-1.0, seed=42)
        got, info = disp.present(gamma=GAMMA, temporal=True, denoise={"levels": 2}, upsample={"scale": 2}, grade=grade, bloom=BLOOM)
        mean_lo, count_lo = _linear_mean(view, ses.read(), history, {"levels": 2}, w, h)
        mean, count = pt.upsample(0, W, H, mean_lo, count_lo, view.render_features(W, H), scale=2)
        want, graded_only, e = host.bytes(mean, count, W, H, grade, BLOOM)
        assert got.shape == (H, W, 3)
        _same(got, want, ("scaled", i))
        _same_float(info["exposure"], e, ("scaled", i))
        assert (want != graded_only).any()
    # ... and without a filter the upsampler is handed the unfiltered mean; bloom still reads the upsampled means
    disp2, host2 = pt.Display(ses), HostChain()
    got, _ = disp2.present(gamma=GAMMA, upsample={"scale": 2}, grade=grade, bloom=BLOOM)
    mean_lo, count_lo = _linear_mean(view, ses.read(), None, None, w, h)
    mean, count = pt.upsample(0, W, H, mean_lo, count_lo, view.render_features(W, H), scale=2)
    _same(got, host2.bytes(mean, count, W, H, grade, BLOOM)[0], "scaled, no filter")


def test_strength_zero_is_the_graded_present_and_other_levels_differ(tor):
    g, view = tor
    ses = pt.Session(g, W, H)
    _frame(g, view, ses, 0)
    disp = pt.Display(ses)
    for grade in (MANUAL, AUTO, dict()):
        graded, ginfo = disp.present(gamma=GAMMA, denoise={"levels": 3}, grade=grade)
        for bloom in (dict(), dict(strength=0.0, levels=3, threshold=0.5), pt.BloomParams()):
            disp.reset()
            got, info = disp.present(gamma=GAMMA, denoise={"levels": 3}, grade=grade, bloom=bloom)
            _same(got, graded, (grade, bloom))
            _same_float(info["exposure"], ginfo["exposure"], "strength 0")
        disp.reset()
    # bloom without a grade at all: the zeroed grade (no curve, e = 1) -- and every depth of the pyramid against the host chain
    mean, count = _linear_mean(view, ses.read(), None, None)
    seen = set()
    for levels in (1, 2, 5, 8):
        bloom = dict(strength=1.0, levels=levels, threshold=0.5)
        got, _ = disp.present(gamma=GAMMA, bloom=bloom)
        want, _, _ = HostChain().bytes(mean, count, W, H, dict(), bloom)
        _same(got, want, ("no grade", levels))
        seen.add(got.tobytes())
    assert len(seen) == 4


def test_a_refused_present_leaves_history_and_exposure_alone(tor):
    g, view = tor
    ses = pt.Session(g, W, H)
    disp, host, history = pt.Display(ses), HostChain(), pt.Temporal(view, W, H)

    def good(i):
        _frame(g, view, ses, i)
        got, info = disp.present(gamma=GAMMA, temporal=True, grade=AUTO, bloom=BLOOM)
        mean, count = _linear_mean(view, ses.read(), history, None)
        want, _, e = host.bytes(mean, count, W, H, AUTO, BLOOM)
        _same(got, want, i)
        _same_float(info["exposure"], e, i)

    good(0)
    good(1)
    _frame(g, view, ses, 2)
    for bad in (dict(strength=-1.0), dict(strength=float("nan")), dict(strength=0.5, threshold=float("inf")), dict(strength=0.5, levels=9),
                dict(strength=0.5, levels=-2), dict(threshold=-0.5)):
        with pytest.raises(pt.PtError) as err:
            disp.present(gamma=GAMMA, temporal=True, grade=AUTO, bloom=bad)
        assert err.value.status == pt.PT_ERR_INVALID_ARGUMENT
    with pytest.raises(pt.PtError):
        disp.present(gamma=GAMMA, temporal=True, grade=dict(curve=9), bloom=BLOOM)
    good(2)                                    # what it would have been without the refused calls


def test_device_objects_return_to_where_they_were(models_dir):
    L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
    L.pt_test_set_mutation(b"reset", 0.0)
    g = pt.Scene.load_obj(models_dir, "Tor.obj", device=0, library=L)
    ses = pt.Session(g, W // 2, H // 2)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    before = L.pt_test_live_device_objects()
    disp = pt.Display(ses)
    for scale in (2, 3, 2):                    # the scaled display's bloom planes follow its size
        disp.present(gamma=GAMMA, upsample={"scale": scale}, grade=AUTO, bloom=BLOOM)
        disp.present(gamma=GAMMA, grade=MANUAL, bloom=dict(strength=0.5, levels=8))
    assert L.pt_test_live_device_objects() > before
    disp.close()
    assert L.pt_test_live_device_objects() == before
