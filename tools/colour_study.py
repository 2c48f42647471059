"""What colour grading costs at 1920 x 1080 (profiles/r10_colour.txt): the ungraded display kernel, the graded one -- the same
instructions as before this stage existed: its source is compiled from the same tokens -- and the colour kernel with the matrix
only and with a LUT only at N = 17, 33 and 65, each alone on a host image (pt_display_bytes_host and its graded and colour twins).
The runs are interleaved in one process: a warm-up round, then seven rounds of every variant in turn; kernel_ms = HIP events
around the chain on the device (the clears of the deferred list's length and of the exposure block, the manual exposure's write,
the kernel).  Medians with min - max, and each median over the graded kernel's.
    python tools/colour_study.py [--out FILE]"""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("path-tracing_amd")
W, H, ROUNDS = 1920, 1080, 7
SIZES = (17, 33, 65)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    mean = rng.uniform(0.0, 1.5, (H, W, 3)).astype(np.float32)        # every pixel another cell of the LUT: the gathers at their worst
    smooth = np.empty_like(mean)                                      # a picture's neighbours share cells: a ramp across the frame
    y, x = np.mgrid[0:H, 0:W]
    smooth[..., 0], smooth[..., 1], smooth[..., 2] = x / (W - 1.0), y / (H - 1.0), (x + y) / (W + H - 2.0)
    count = np.ones((H, W), np.int32)
    grade = dict(curve="aces", exposure=1.5)
    luts = {n: pt.Lut.create(rng.uniform(0.0, 1.0, (n, n, n, 3)).astype(np.float32)) for n in SIZES}
    variants = [("ungraded display kernel", lambda m: pt.display_bytes(m, count)[1]),
                ("graded kernel, aces", lambda m: pt.display_bytes_graded(m, count, grade)[1]),
                ("colour kernel, matrix only", lambda m: pt.display_bytes_colour(m, count, grade, dict(wb=(1.1, 1.0, 0.9), saturation=0.8))[1])]
    for n in SIZES:
        variants.append(("colour kernel, LUT only, N = %d (%.1f MB)" % (n, 16 * n ** 3 / 1e6), lambda m, n=n: pt.display_bytes_colour(m, count, grade, dict(lut=luts[n]))[1]))
    variants.append(("colour kernel, matrix and LUT, N = 33", lambda m: pt.display_bytes_colour(m, count, grade, dict(wb=(1.1, 1.0, 0.9), saturation=0.8, lut=luts[33]))[1]))
    lines = ["%d x %d, %d rounds after one warm-up round, every variant in turn in each round; kernel_ms = HIP events around the chain" % (W, H, ROUNDS),
             "the kernel reads 16 B and writes 3 B a pixel: %.1f MB a frame" % (19 * W * H / 1e6)]
    for title, image in (("random colours (every pixel another cell of the LUT)", mean), ("a smooth ramp (neighbours share cells)", smooth)):
        times = {name: [] for name, _ in variants}
        deferred = {}
        for r in range(ROUNDS + 1):
            for name, fn in variants:
                info = fn(image)
                deferred[name] = info["deferred_pixels"]
                if r:
                    times[name].append(info["kernel_ms"])
        base = statistics.median(times["graded kernel, aces"])
        lines.append(title)
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            lines.append("  %-44s median %.4f ms  (%.4f - %.4f)   x %.3f of graded   %4.0f GB/s of the 19 B   deferred %d"
                         % (name, med, min(t), max(t), med / base, 19 * W * H / med / 1e6, deferred[name]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
