#!/usr/bin/env python3
"""Kernel time of the camera twin, the lens kernel and their motion twins on the bench.py default frame:
Tor.obj 1920 x 1080 x 256 spp, -MRR 8, no adaptive sampling.  The five configurations are interleaved in one process (free, camera,
motion, lens, motion + lens; one warm-up round, then --rounds rounds), HIP events around each launch, as bench.py times its steps.
Prints one JSON object: medians, every sample, and the two ratios.  profiles/r09_motion_twins.txt is its output on one MI355X.

    python tools/motion_study.py [--rounds 7]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pt = importlib.import_module("path-tracing_amd")
W, H, SPP, MRR = 1920, 1080, 256, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sc = pt.Scene.load_obj(os.path.join(ROOT, "models") + "/", "Tor.obj", device=0)
    npx = W * H
    buf = torch.zeros(28 * npx, dtype=torch.uint8, device=dev)      # sum, sum2 (12 bytes per pixel each), count (4)
    stream = torch.cuda.current_stream(dev)
    params = pt.RenderParams(W, H, 0, H, 0, SPP, MRR, 1e-4, -1.0, 42, 0, 0)
    start = pt.look_at((1.0, 0.5, -20.0), (0.0, 0.0, 0.0), fov_y=pt.REFERENCE_FOV_Y)
    end = pt.look_at((1.3, 0.6, -19.8), (0.1, 0.0, 0.0), fov_y=pt.REFERENCE_FOV_Y)
    lens = (0.5, 20.0)
    configs = {"free": (None, None, None), "camera": (start, None, None), "motion": (start, None, end),
               "lens": (start, lens, None), "motion_lens": (start, lens, end)}

    def one(name):
        cam, ln, mot = configs[name]
        sc.set_camera_motion(None)      # (a camera is checked against the motion its handle has: clear it first)
        sc.set_lens(None)
        sc.set_camera(cam)
        if ln:
            sc.set_lens(*ln)
        sc.set_camera_motion(mot)
        buf.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        sc.render_device(params, buf.data_ptr(), buf.data_ptr() + 12 * npx, buf.data_ptr() + 24 * npx, stream=stream.cuda_stream, want_stats=False)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    for k in configs:       # warm-up: code object, cull tables
        one(k)
    times = {k: [] for k in configs}
    for _ in range(args.rounds):
        for k in configs:
            times[k].append(round(one(k), 4))
    med = {k: round(float(np.median(v)), 4) for k, v in times.items()}
    print(json.dumps({"frame": f"Tor.obj {W}x{H}x{SPP} spp, MRR {MRR}", "ms_median": med,
                      "motion_over_camera": round(med["motion"] / med["camera"], 4),
                      "motion_lens_over_lens": round(med["motion_lens"] / med["lens"], 4), "ms_all": times}, indent=1))


if __name__ == "__main__":
    main()
