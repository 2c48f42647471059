"""What film grain and dithered quantization cost at 1920 x 1080 (profiles/display_grain.txt): kernel_ms of a present with the stage
and without it, alternating in one run -- ACES with a manual exposure against dither alone, grain at pitch 1, grain at pitch 2.5 and
both together, and the chain with every stage on with and without it.
    python tools/grain_study.py [--out FILE] [--parent DIR]
--parent names the package directory of another commit's built checkout (the parent commit's path-tracing_amd/, for the yardstick row:
its present of the same frame without the stage, alternating with this build's in the same process); without it the yardstick is
this build's present with a zeroed block, which enqueues what the parent's did."""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("path-tracing_amd")
W, H, SPP, MRR, REPEATS = 1920, 1080, 64, 4, 9
EYE, LOOKAT = (-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)
EXPECTED = ("expected, from instruction counts alone: the display kernel streams 19 B a pixel (12 of means, 4 of count, 3 of bytes); the stage "
            "adds two to five Philox calls a pixel, a few hundred vector instructions, no memory traffic: the kernel moves from memory-bound "
            "towards ALU-bound, and a present costs some tens of microseconds more")


def _fmt(t):
    return "min %.4f  median %.4f ms" % (min(t), statistics.median(t))


def _alternate(on, off):
    """REPEATS of each after one warm-up of each, alternating, so that neither has the clock or the cache to itself."""
    on(), off()
    a, b = [], []
    for _ in range(REPEATS):
        a.append(on())
        b.append(off())
    return a, b


def timing(parent=None):
    g = pt.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
    g.set_camera(pt.look_at(EYE, LOOKAT, aspect=W / H))
    ses = pt.Session(g, W, H)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    disp = pt.Display(ses)
    lines = ["%d x %d, Tor.obj looking up at the emitter, %d spp; %d repeats after one warm-up, the stage on and off alternating; "
             "kernel_ms = HIP events around the chain" % (W, H, SPP, REPEATS), EXPECTED]
    manual = dict(grade=dict(curve="aces", exposure=2.0))
    full = dict(grade=dict(curve="aces", auto_exposure=True, rate=0.25), bloom=dict(strength=0.5, levels=5), local=dict(strength=1.0),
                colour=dict(wb=(1.1, 1.0, 0.9), saturation=0.8), optics=dict(k1=-0.1, ca=0.01, vignette=1.0), sharpen=dict(strength=0.5),
                denoise=dict(levels=5))
    rows = [("aces, manual exposure: dither alone", manual, dict(dither=1.0)),
            ("aces, manual exposure: grain, pitch 1", manual, dict(strength=0.3)),
            ("aces, manual exposure: grain, pitch 2.5", manual, dict(strength=0.3, size=2.5)),
            ("aces, manual exposure: grain 2.5 + dither", manual, dict(strength=0.3, size=2.5, dither=1.0)),
            ("everything on: grain 2.5 + dither", full, dict(strength=0.3, size=2.5, dither=1.0))]
    for name, kw, stage in rows:
        on, off = _alternate(lambda: disp.present(grain=stage, **kw)[1]["kernel_ms"], lambda: disp.present(**kw)[1]["kernel_ms"])
        lines.append("present, %-42s with the stage %s   without %s   difference of the medians %.4f ms"
                     % (name, _fmt(on), _fmt(off), statistics.median(on) - statistics.median(off)))
    zero, none = _alternate(lambda: disp.present(grain=dict(), **manual)[1]["kernel_ms"], lambda: disp.present(**manual)[1]["kernel_ms"])
    lines.append("present, aces, manual exposure: a zeroed block %s   no block %s" % (_fmt(zero), _fmt(none)))
    if parent:
        spec = importlib.util.spec_from_file_location("pt_parent", os.path.join(parent, "__init__.py"))
        old = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(old)                     # (its own binding and its own library)
        g2 = old.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
        g2.set_camera(old.look_at(EYE, LOOKAT, aspect=W / H))
        ses2 = old.Session(g2, W, H)
        ses2.render(0, SPP, MRR, error=-1.0, seed=42)
        disp2 = old.Display(ses2)
        theirs, ours = _alternate(lambda: disp2.present(**manual)[1]["kernel_ms"], lambda: disp.present(**manual)[1]["kernel_ms"])
        lines.append("yardstick: the parent commit's build, the same present without the stage %s   this build's, same run %s"
                     % (_fmt(theirs), _fmt(ours)))
    else:
        lines.append("yardstick: this build's present with a zeroed block (the row above) stands in for the parent commit's binary, which was not run")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    lines = timing(a.parent)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
