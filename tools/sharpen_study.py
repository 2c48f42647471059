"""What sharpening costs at 1920 x 1080 (profiles/display_sharpen.txt): pt_sharpen_host's two kernels alone and the bytes they must
move over that time, beside pt_local_host at one level (its luminance, one level and apply kernels: the nearest thing to the apply
kernel alone that an entry point times) from the same run; and kernel_ms of a present with the stage and without it, alternating in
one run, for three chains -- ACES with a manual exposure, with the automatic one, and with every stage on.
    python tools/sharpen_study.py [--out FILE]
The equal-cost quality row (RMSE against 4096 spp of -RENDER_SCALE 2 -DENOISE 5 at 64 spp with -SHARPEN 0, 0.5 and 1) is not made
here: it is three pt_render runs and a reference, compared on the written files."""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("path-tracing_amd")
W, H, SPP, MRR, REPEATS = 1920, 1080, 64, 4, 9
EYE, LOOKAT = (-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)
# bytes a pixel in the means form: the plane kernel reads the means and the count and writes y; the apply kernel reads the means,
# the count and y (its ring's four further reads of y are its neighbours' own, from the cache) and writes the means
PLANE_BYTES, APPLY_BYTES = (12 + 4) + 4, (12 + 4 + 4) + 12


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


def timing():
    g = pt.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
    g.set_camera(pt.look_at(EYE, LOOKAT, aspect=W / H))
    ses = pt.Session(g, W, H)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    disp = pt.Display(ses)
    lines = ["%d x %d, Tor.obj looking up at the emitter, %d spp; %d repeats after one warm-up, the stage on and off alternating; "
             "kernel_ms = HIP events around the chain" % (W, H, SPP, REPEATS)]
    s, s2, c = ses.read()
    mean, cnt = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean = mean.reshape(H, W, 3)
    sharp, local = _alternate(lambda: pt.sharpen(0, mean, cnt, exposure=2.0, strength=1.0, want_ms=True)[1],
                              lambda: pt.local_exposure(0, mean, cnt, exposure=2.0, strength=1.0, levels=1, want_ms=True)[1])
    need = PLANE_BYTES + APPLY_BYTES
    lines.append("pt_sharpen_host, the two kernels (means in)            %s   needed %d + %d B/pixel = %.0f GB/s at the median"
                 % (_fmt(sharp), PLANE_BYTES, APPLY_BYTES, need * W * H / statistics.median(sharp) / 1e6))
    lines.append("pt_local_host at 1 level, its three kernels (yardstick) %s   needed 60 B/pixel = %.0f GB/s at the median"
                 % (_fmt(local), 60 * W * H / statistics.median(local) / 1e6))
    stage = dict(strength=0.5)
    chains = [("aces, manual exposure", dict(grade=dict(curve="aces", exposure=2.0))),
              ("aces, automatic exposure", dict(grade=dict(curve="aces", auto_exposure=True, rate=0.25))),
              ("everything on", dict(grade=dict(curve="aces", auto_exposure=True, rate=0.25), bloom=dict(strength=0.5, levels=5), local=dict(strength=1.0),
                                     colour=dict(wb=(1.1, 1.0, 0.9), saturation=0.8), optics=dict(k1=-0.1, ca=0.01, vignette=1.0), denoise=dict(levels=5)))]
    for name, kw in chains:
        on, off = _alternate(lambda: disp.present(sharpen=stage, **kw)[1]["kernel_ms"], lambda: disp.present(**kw)[1]["kernel_ms"])
        lines.append("present, %-26s with the stage %s   without %s   difference of the medians %.4f ms"
                     % (name, _fmt(on), _fmt(off), statistics.median(on) - statistics.median(off)))
    lines.append("the figures without the stage are this build's; the parent commit's binary on the same machine is the comparison that shows "
                 "whether the path as it was moved")
    lines.append("not measured: an LDS tile for the ring; tiles other than 32 x 8; the two kernels fused into one that recomputes y five times")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = timing()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
