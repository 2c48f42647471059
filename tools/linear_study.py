"""What scene-linear output costs at 1920 x 1080 (profiles/display_linear.txt): the encode kernel alone in both
formats beside the display kernel on the same image -- HIP-event time, median of several launches, and the bytes each moves over that
time --, a present with the stage and without it, alternating, and pt_render -LINEAR_OUT end to end on the host path and with
-DEVICE_RESOLVE 1, from its -TIMING phases.
    python tools/linear_study.py [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("path-tracing_amd")
W, H, SPP, MRR, REPEATS = 1920, 1080, 16, 4, 9
EYE, LOOKAT = (-2.0, -5.0, -8.0), (0.0, 9.0, 0.0)
EXE = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
EXPECTED = ("expected, from the bytes alone: per pixel the display kernel moves 16 B in and 3 out, the RGBE encode 16 in and 4 out, the PFM "
            "encode 16 in and 12 out; all three stream, so the encode should take the display kernel's time (RGBE) to one and a half times it (PFM)")


def _fmt(t):
    return "min %.4f  median %.4f ms" % (min(t), statistics.median(t))


def _repeat(f):
    f()
    return [f() for _ in range(REPEATS)]


def kernels():
    g = pt.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
    g.set_camera(pt.look_at(EYE, LOOKAT, aspect=W / H))
    ses = pt.Session(g, W, H)
    ses.render(0, SPP, MRR, error=-1.0, seed=42)
    s, s2, c = ses.read()
    mean, count = pt.denoise(W, H, s, s2, c, None, levels=0)
    mean, count = mean.reshape(H, W, 3), count.reshape(H, W)
    lines = ["%d x %d, Tor.obj looking up at the emitter, %d spp; median of %d launches after one warm-up; kernel_ms = HIP events round the kernel"
             % (W, H, SPP, REPEATS), EXPECTED]
    px = W * H
    rows = [("display kernel (launch_display), the yardstick", 19, lambda: pt.display_bytes(mean, count)[1]["kernel_ms"]),
            ("encode, RGBE", 20, lambda: pt.linear_encode_device(0, mean, count, 1.0, "hdr", want_info=True)[1]["kernel_ms"]),
            ("encode, RGBE, exposed", 20, lambda: pt.linear_encode_device(0, mean, count, 1.5, "hdr", True, want_info=True)[1]["kernel_ms"]),
            ("encode, PFM (width % 4 == 0: aligned loads)", 28, lambda: pt.linear_encode_device(0, mean, count, 1.0, "pfm", want_info=True)[1]["kernel_ms"]),
            ("encode, PFM, 1919 wide (loads float by float)", 28,
             lambda: pt.linear_encode_device(0, mean[:, :1919], count[:, :1919], 1.0, "pfm", want_info=True)[1]["kernel_ms"])]
    for name, bytes_px, f in rows:
        t = _repeat(f)
        lines.append("kernel alone, %-48s %s   %d B a pixel: %.0f GB/s at the median" % (name, _fmt(t), bytes_px, bytes_px * px / statistics.median(t) / 1e6))
    disp = pt.Display(ses)
    full = dict(grade=dict(curve="aces", exposure=2.0), bloom=dict(strength=0.5, levels=5), sharpen=dict(strength=0.5))
    for name, kw in (("bare chain (sums: the dividing kernels)", {}), ("aces + bloom + sharpen", full)):
        for fmt in ("hdr", "pfm"):
            on, off = [], []
            disp.present(linear=dict(format=fmt), **kw), disp.present(**kw)
            for _ in range(REPEATS):
                on.append(disp.present(linear=dict(format=fmt), **kw)[1]["kernel_ms"])
                off.append(disp.present(**kw)[1]["kernel_ms"])
            lines.append("present, %-40s with %s %s   without %s   difference of the medians %.4f ms"
                         % (name, fmt, _fmt(on), _fmt(off), statistics.median(on) - statistics.median(off)))
    return lines


def end_to_end():
    lines = []
    with tempfile.TemporaryDirectory() as work:
        base = [EXE, "--W", W, "--H", H, "-RPP", SPP, "-MRR", MRR, "-UPDATE", 0, "-QUIET", 1, "-SEED", 42, "-MODEL_PATH", os.path.join(ROOT, "models") + "/",
                "-EYE", "-2,-5,-8", "-LOOKAT", "0,9,0", "-OUT", "one.bmp", "-TIMING", 1]
        for name, extra in (("no linear file, host path", []), ("no linear file, -DEVICE_RESOLVE 1", ["-DEVICE_RESOLVE", 1]),
                            ("-LINEAR_OUT x.hdr, host path", ["-LINEAR_OUT", "x.hdr"]), ("-LINEAR_OUT x.hdr, -DEVICE_RESOLVE 1", ["-LINEAR_OUT", "x.hdr", "-DEVICE_RESOLVE", 1]),
                            ("-LINEAR_OUT x.pfm, host path", ["-LINEAR_OUT", "x.pfm"]), ("-LINEAR_OUT x.pfm, -DEVICE_RESOLVE 1", ["-LINEAR_OUT", "x.pfm", "-DEVICE_RESOLVE", 1])):
            best = None
            for _ in range(3):
                r = subprocess.run([str(a) for a in base + extra], cwd=work, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(r.stderr)
                t = json.loads([ln for ln in r.stderr.splitlines() if ln.startswith("{")][-1])
                if best is None or t["main_s"] < best["main_s"]:
                    best = t
            lines.append("pt_render, %-36s read_back %.4f s  resolve (the image chain) %.4f s  file writes %.4f s  main %.4f s   (best of 3 by main_s)"
                         % (name, best["read_back_s"], best["resolve_s"], best["bmp_write_s"], best["main_s"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = "\n".join(kernels() + end_to_end()) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
