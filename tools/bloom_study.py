"""What bloom costs at 1920 x 1080 (profiles/display_bloom.txt): kernel_ms of a graded present without bloom -- the path as it was
-- and with bloom at 1, 3, 5 and 8 levels, in the same run; pt_bloom_host's kernels alone; the bytes the stage moves, counted
from the kernels as written, over that time; and one a-trous level from the same run as the yardstick.
    python tools/bloom_study.py [--out FILE]"""
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
LEVELS = (1, 3, 5, 8)


def _times(fn):
    fn()                                             # warm-up: code object load, allocations
    t = [fn() for _ in range(REPEATS)]
    return min(t), statistics.median(t)


def _ms(fn):
    return "min %.4f  median %.4f ms" % _times(fn)


def stage_bytes(w, h, levels):
    """(needed, requested) bytes of the 2 L kernels.  Needed: every plane read once and written once -- means and counts (16 bytes a
    pixel) by the first down and the last up kernel, 16-byte records of the levels, 12 bytes a pixel of output.  Requested: what
    the lanes ask the cache for -- a down kernel's lane loads 4 taps for each of the 18 rows under its tile's 8 (9/4 rows of taps a
    record written), an up kernel's lane 2 taps for each of the 6 coarse rows under its tile's 8 (3/4 a record), plus its own."""
    n = [w * h]
    for _ in range(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        n.append(w * h)
    needed = requested = 0
    for k in range(1, levels + 1):                   # down: level k - 1 in, level k out
        needed += 16 * n[k - 1] + 16 * n[k]
        requested += 16 * 4 * 9 / 4 * n[k] + 16 * n[k]
    for k in range(levels - 1, -1, -1):              # up: level k + 1 and level k (or the image) in, level k (or the means) out
        needed += 16 * n[k + 1] + 16 * n[k] + (16 if k else 12) * n[k]
        requested += 16 * 2 * 3 / 4 * n[k] + 16 * n[k] + (16 if k else 12) * n[k]
    return needed, requested


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = pt.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
    g.set_camera(pt.look_at((-2.0, -5.0, -8.0), (0.0, 9.0, 0.0), aspect=W / H))
    ses = pt.Session(g, W, H)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    disp = pt.Display(ses)
    grade = dict(curve="aces", exposure=2.0)
    lines = ["%d x %d, Tor.obj looking up at the emitter, %d spp; %d repeats after one warm-up; kernel_ms = HIP events around the chain" % (W, H, SPP, REPEATS)]
    present = lambda **kw: (lambda: disp.present(grade=grade, **kw)[1]["kernel_ms"])
    lines.append("present, aces, manual exposure, no bloom (the path as it was)   %s" % _ms(present()))
    for L in LEVELS:
        lines.append("present, the same with bloom, %d level%s (sums in: DIVIDE)        %s" % (L, " " if L == 1 else "s", _ms(present(bloom=dict(strength=0.5, levels=L)))))
    lines.append("present, aces, manual exposure, no bloom, again                 %s" % _ms(present()))
    auto = dict(curve="aces", auto_exposure=True, rate=0.25)
    lines.append("present, aces, auto exposure, no bloom                          %s" % _ms(lambda: disp.present(grade=auto)[1]["kernel_ms"]))
    lines.append("present, aces, auto exposure, bloom 5 levels                    %s" % _ms(lambda: disp.present(grade=auto, bloom=dict(strength=0.5, levels=5))[1]["kernel_ms"]))
    s, s2, c = ses.read()
    mean, cnt = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean = mean.reshape(H, W, 3)
    lit = float(np.mean(0.2126 * mean[..., 0] + 0.7152 * mean[..., 1] + 0.0722 * mean[..., 2] > 0.5))
    lines.append("pt_bloom_host, the 2 L kernels alone (means in), exposure 2, threshold 1: %.1f %% of the pixels above it" % (100 * lit))
    for L in LEVELS:
        lo, med = _times(lambda: pt.bloom(0, mean, cnt, exposure=2.0, strength=0.5, levels=L, want_ms=True)[1])
        needed, requested = stage_bytes(W, H, L)
        lines.append("  %d level%s  %2d launches  min %.4f  median %.4f ms   needed %.1f B/pixel = %.0f GB/s   requested %.1f B/pixel = %.0f GB/s"
                     % (L, " " if L == 1 else "s", 2 * L, lo, med, needed / (W * H), needed / med / 1e6, requested / (W * H), requested / med / 1e6))
    f = g.render_features(W, H)
    one = lambda levels: (lambda: pt.denoise(W, H, s, s2, c, f, levels=levels, want_ms=True)[2])
    lines.append("pt_denoise_host levels = 1                                      %s" % _ms(one(1)))
    lines.append("pt_denoise_host levels = 2 (the difference: one a-trous level)  %s" % _ms(one(2)))
    lines.append("not measured: an unfused bright pass; tiles other than 32 x 8; the taps staged through LDS instead of the cache")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
