"""What the lens optics stage costs at 1920 x 1080 (profiles/display_optics.txt): pt_optics_host's kernel alone, HIP events around
it, for each part of the stage and all of them, with the bytes the kernel must move over that time; and kernel_ms of a present
without the stage -- the path as it was, which a zeroed struct takes -- and with it, alternating in the same run, plain, metered,
and with bloom, local exposure and colour behind it.
    python tools/optics_study.py [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("path-tracing_amd")
W, H, SPP, MRR, REPEATS = 1920, 1080, 4, 4, 9
EYE, LOOKAT = (-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)
# every plane read once and written once: the means and the count in (16 B a pixel), the means and the count out (16); what the
# lanes ask the caches for on top of that is 12 taps of 4 bytes and up to 12 counts a pixel
NEEDED = 32
SETS = [("distortion -0.3, 0.05", dict(k1=-0.3, k2=0.05)), ("chromatic aberration 0.02", dict(ca=0.02)), ("vignette 1.5", dict(vignette=1.5)),
        ("all three", dict(k1=-0.3, k2=0.05, ca=0.02, vignette=1.5)), ("the extreme 4, 4, 0.25, 64 (every source on the clamp)", dict(k1=4.0, k2=4.0, ca=0.25, vignette=64.0))]


def _stats(t):
    return "min %.4f  median %.4f  max %.4f ms" % (min(t), statistics.median(t), max(t))


def timing():
    if pt.device_count() < 1:
        raise SystemExit("optics_study: no HIP device; a time comes from the device or not at all")
    g = pt.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
    g.set_camera(pt.look_at(EYE, LOOKAT, aspect=W / H))
    ses = pt.Session(g, W, H)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    disp = pt.Display(ses)
    lines = ["%d x %d, Tor.obj looking up at the emitter, %d spp; %d repeats after one warm-up; HIP events around the kernels" % (W, H, SPP, REPEATS)]
    s, s2, c = ses.read()
    mean, cnt = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean = mean.reshape(H, W, 3)
    lines.append("pt_optics_host, the kernel alone (means in); needed = every plane read once and written once, %d B/pixel" % NEEDED)
    for tag, prm in SETS:
        alone = lambda: pt.optics(0, mean, cnt, want_ms=True, **prm)[2]
        alone()
        t = [alone() for _ in range(REPEATS)]
        lines.append("  %-56s %s   %.0f GB/s of needed bytes" % (tag, _stats(t), NEEDED * W * H / statistics.median(t) / 1e6))
    optics = SETS[3][1]
    manual, auto = dict(curve="aces", exposure=2.0), dict(curve="aces", auto_exposure=True, rate=0.25)
    rest = dict(bloom=dict(strength=0.5, levels=5), local=dict(strength=1.0), colour=dict(wb=(1.1, 1.0, 0.9), saturation=0.8))
    lines.append("present, kernel_ms of the whole chain, without the stage (a zeroed struct: the path as it was) and with all three, alternating:")
    for tag, kw in (("aces, manual exposure (sums in: DIVIDE)", dict(grade=manual)), ("aces, auto exposure", dict(grade=auto)),
                    ("aces, auto exposure, bloom, local exposure, colour", dict(grade=auto, **rest))):
        without = lambda: disp.present(optics={}, **kw)[1]["kernel_ms"]
        with_it = lambda: disp.present(optics=optics, **kw)[1]["kernel_ms"]
        without(), with_it()
        a, b = [], []
        for _ in range(REPEATS):
            a.append(without())
            b.append(with_it())
        lines.append("  %-52s without: %s" % (tag, _stats(a)))
        lines.append("  %-52s with:    %s   (%+.4f ms median)" % ("", _stats(b), statistics.median(b) - statistics.median(a)))
    lines.append("not measured: tiles other than 32 x 8; an LDS tile of the source; the three channels' counts read once where the positions coincide")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = "\n".join(timing()) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
