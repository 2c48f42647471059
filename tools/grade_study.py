"""What display grading costs at 1920 x 1080 (profiles/display_grading.txt): kernel_ms of a present without grading, with a manual
exposure and with the metered one; pt_meter_host on a flat image (every pixel in one bin: the worst case for same-address LDS
atomics) against a rendered one; and one a-trous level from the same run as the yardstick.
    python tools/grade_study.py [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("path-tracing_amd")
W, H, SPP, MRR, REPEATS = 1920, 1080, 4, 4, 7


def _ms(fn):
    fn()                                             # warm-up: code object load, allocations
    t = [fn() for _ in range(REPEATS)]
    return "min %.4f  median %.4f ms" % (min(t), statistics.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = pt.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
    g.set_camera(pt.look_at((-2.0, -5.0, -8.0), (0.0, 9.0, 0.0), aspect=W / H))
    ses = pt.Session(g, W, H)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    disp = pt.Display(ses)
    lines = ["%d x %d, Tor.obj looking up at the emitter, %d spp; %d repeats after one warm-up; kernel_ms = HIP events around the chain" % (W, H, SPP, REPEATS)]
    present = lambda **kw: (lambda: disp.present(**kw)[1]["kernel_ms"])
    lines.append("present, no grading (display_kernel<true>)              %s" % _ms(present()))
    lines.append("present, REFERENCE curve, e = 1 (graded kernel)          %s" % _ms(present(grade={})))
    for curve in ("clamp", "reinhard", "aces"):
        lines.append("present, %-8s manual exposure 0.6                   %s" % (curve, _ms(present(grade=dict(curve=curve, exposure=0.6)))))
    lines.append("present, aces, auto exposure (memset + meter + exposure) %s" % _ms(present(grade=dict(curve="aces", auto_exposure=True, rate=0.25))))
    s, s2, c = ses.read()
    f = g.render_features(W, H)
    one = lambda levels: (lambda: pt.denoise(W, H, s, s2, c, f, levels=levels, want_ms=True)[2])
    lines.append("pt_denoise_host levels = 1                               %s" % _ms(one(1)))
    lines.append("pt_denoise_host levels = 2 (the difference: one a-trous level) %s" % _ms(one(2)))
    mean, cnt = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean = mean.reshape(H, W, 3)
    meter = lambda m: (lambda: pt.meter(m, cnt, want_ms=True)[1])
    hist = pt.meter(mean, cnt)
    lines.append("pt_meter_host, rendered image (%d bins in use)          %s" % (int(np.count_nonzero(hist)), _ms(meter(mean))))
    lines.append("pt_meter_host, flat image (one bin)                      %s" % _ms(meter(np.full((H, W, 3), 0.5, np.float32))))
    rng = np.random.default_rng(3)
    lines.append("pt_meter_host, random image (every bin, no flat wave)    %s" % _ms(meter(np.exp2(rng.uniform(-16, 16, (H, W, 3))).astype(np.float32))))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
