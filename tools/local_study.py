"""What local exposure costs at 1920 x 1080 (profiles/display_local.txt): kernel_ms of a graded and bloomed present without the
stage -- the path as it was -- and with it at 1, 3, 5 and 8 levels, in the same run; pt_local_host's kernels alone; the bytes each
kernel must move, counted from the kernels as written, over that time; the first two levels with their taps staged through LDS
and read from global memory (make -C path-tracing_amd/csrc local-variant builds the second library); and one a-trous level of the
denoiser from the same run as the yardstick.
    python tools/local_study.py [--out FILE]
What the stage does to a picture, on the CPU alone (the numpy restatement of the header on a frame composed from the CPU oracle):
    python tools/local_study.py --quality [--out FILE]"""
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
GLOBAL_LIB = os.path.join(ROOT, "path-tracing_amd", "lib", "libpt_local_global.so")
EYE, LOOKAT = (-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)


def _times(fn):
    fn()                                             # warm-up: code object load, allocations
    t = [fn() for _ in range(REPEATS)]
    return min(t), statistics.median(t)


def _ms(fn):
    return "min %.4f  median %.4f ms" % _times(fn)


def stage_bytes(levels):
    """Bytes a pixel the L + 2 kernels must move, every plane read once and written once: the luminance kernel reads the means and
    the count (16) and writes b_0 (4); a level reads one plane and writes one (8); the gain reads the means, the count and b_L (20)
    and writes the means (12).  What a level's lanes ask the cache or LDS for on top of that -- 25 taps of 4 bytes a pixel -- is
    the same at every spacing."""
    return 20 + 8 * levels + 32


def timing():
    g = pt.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
    g.set_camera(pt.look_at(EYE, LOOKAT, aspect=W / H))
    ses = pt.Session(g, W, H)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    disp = pt.Display(ses)
    grade, bloom = dict(curve="aces", exposure=2.0), dict(strength=0.5, levels=5)
    lines = ["%d x %d, Tor.obj looking up at the emitter, %d spp; %d repeats after one warm-up; kernel_ms = HIP events around the chain" % (W, H, SPP, REPEATS)]
    present = lambda **kw: (lambda: disp.present(grade=grade, bloom=bloom, **kw)[1]["kernel_ms"])
    lines.append("present, aces, manual exposure, bloom 5 levels (the path as it was)  %s" % _ms(present()))
    for L in LEVELS:
        lines.append("present, the same with local exposure, %d level%s                     %s" % (L, " " if L == 1 else "s", _ms(present(local=dict(strength=1.0, levels=L)))))
    lines.append("present, aces, manual exposure, bloom 5 levels, again                %s" % _ms(present()))
    lines.append("present, aces, no bloom, local exposure 5 levels (sums in: DIVIDE)   %s" % _ms(lambda: disp.present(grade=grade, local=dict(strength=1.0))[1]["kernel_ms"]))
    auto = dict(curve="aces", auto_exposure=True, rate=0.25)
    lines.append("present, aces, auto exposure, bloom 5 levels                         %s" % _ms(lambda: disp.present(grade=auto, bloom=bloom)[1]["kernel_ms"]))
    lines.append("present, aces, auto exposure, bloom and local exposure 5 levels      %s" % _ms(lambda: disp.present(grade=auto, bloom=bloom, local=dict(strength=1.0))[1]["kernel_ms"]))
    s, s2, c = ses.read()
    mean, cnt = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean = mean.reshape(H, W, 3)
    alone = lambda L, lib=None: (lambda: pt.local_exposure(0, mean, cnt, exposure=2.0, strength=1.0, levels=L, want_ms=True, library=lib)[1])
    lines.append("pt_local_host, the L + 2 kernels alone (means in), exposure 2; needed = every plane read once and written once")
    at = {}
    for L in (1, 2) + LEVELS[1:]:
        lo, med = _times(alone(L))
        at[L] = med
        b = stage_bytes(L)
        lines.append("  %d level%s  %2d launches  min %.4f  median %.4f ms   needed %d B/pixel = %.0f GB/s"
                     % (L, " " if L == 1 else "s", L + 2, lo, med, b, b * W * H / med / 1e6))
    lines.append("  per level, from the medians: spacing 1 with luminance and gain %.4f ms; spacing 2 %.4f; spacings 4 .. 16 %.4f each; 32 .. 128 %.4f each"
                 % (at[1], at[2] - at[1], (at[5] - at[2]) / 3, (at[8] - at[5]) / 3))
    if os.path.exists(GLOBAL_LIB):
        other = pt.load_library(GLOBAL_LIB)
        lines.append("the first two levels staged through LDS (36 x 12 and 40 x 16 floats a tile) against the same levels from global memory, alternating:")
        for L in (1, 2):
            staged, plain = [], []
            alone(L)(), alone(L, other)()
            for _ in range(REPEATS):
                staged.append(alone(L)())
                plain.append(alone(L, other)())
            lines.append("  %d level%s  LDS: min %.4f  median %.4f ms     global: min %.4f  median %.4f ms"
                         % (L, " " if L == 1 else "s", min(staged), statistics.median(staged), min(plain), statistics.median(plain)))
    else:
        lines.append("not measured: the first two levels without LDS staging (libpt_local_global.so is not built: make local-variant)")
    f = g.render_features(W, H)
    one = lambda levels: (lambda: pt.denoise(W, H, s, s2, c, f, levels=levels, want_ms=True)[2])
    lines.append("pt_denoise_host levels = 1                                           %s" % _ms(one(1)))
    lines.append("pt_denoise_host levels = 2 (the difference: one a-trous level)       %s" % _ms(one(2)))
    lines.append("not measured: tiles other than 32 x 8; the apply kernel writing in place; one division per tap (s^2 / (s^2 + d^2)) instead of two")
    return lines


def quality():
    """The restatement on a 96 x 72 frame of Tor.obj looking up at the emitter, composed from the CPU oracle's parts."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import local_restatement as R
    import oracle_lib as O
    import view_composition as V
    w, h, spp, mrr, e = 96, 72, 64, 4, np.float32(4.0)
    scene = O.Scene.load(os.path.join(ROOT, "models") + "/", "Tor.obj")
    cam = pt.look_at(EYE, LOOKAT, aspect=w / h).as_array()
    px = np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).reshape(-1, 2)
    s, _, c = V.compose(scene, w, h, px, spp, mrr, camera=cam)
    with np.errstate(all="ignore"):
        mean = np.where((c != 0)[:, None], s / c.astype(np.float32)[:, None], s).astype(np.float32).reshape(h, w, 3)
    c = c.reshape(h, w)
    lum = lambda m: R.luminance(m).astype(np.float64) * float(e)
    base_l = lum(mean)
    dark = (c != 0) & (base_l < np.median(base_l[c != 0]))           # the dark half: below the median exposed luminance

    def describe(tag, m):
        l = lum(m)
        shown = (c != 0) & (l >= 1 / 255) & (l <= 1.0)
        # RMS local contrast: the luminance over the mean of its 3 x 3 neighbourhood, less one, over the dark half's inner pixels
        pad = np.pad(l, 1, mode="edge")
        local_mean = sum(pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9
        inner = dark & (local_mean > 0)
        contrast = np.sqrt(np.mean((l[inner] / local_mean[inner] - 1) ** 2))
        return "%-34s %5.1f %% of the pixels with an exposed luminance in 1/255 .. 1;  dark half: median %.4f, RMS local contrast %.4f" % (
            tag, 100 * shown.sum() / (c != 0).sum(), np.median(l[dark]), contrast)

    lines = ["%d x %d, Tor.obj looking up at the emitter, %d spp, MRR %d, exposure %g; the numpy restatement, no device" % (w, h, spp, mrr, e),
             describe("without the stage", mean)]
    for strength, sigma, levels in ((1.0, 0.5, 5), (2.0, 0.5, 5), (1.0, 0.5, 3), (1.0, 2.0, 5), (1.0, 1e20, 5)):
        out_m = R.local_exposure(mean, c, e, strength, 0.18, levels, sigma)
        b, valid = R.base(mean, c, levels, np.float32(sigma))
        # a halo shows as a base that overshoots its pixel near an edge: the largest base / luminance among valid pixels next to a
        # pixel 10 times as bright
        l0 = R.luminance(mean).astype(np.float64)
        pad = np.pad(l0, 1, mode="edge")
        brightest = np.max([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)
        at_edge = valid & (l0 > 0) & (brightest > 10 * l0)
        over = float(np.max(b[at_edge] / l0[at_edge])) if at_edge.any() else float("nan")
        lines.append(describe("strength %g, sigma %g, %d levels" % (strength, sigma, levels), out_m) +
                     ";  base / luminance next to a 10 x edge: at most %.3f (%d pixels)" % (over, int(at_edge.sum())))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    lines = quality() if a.quality else timing()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
