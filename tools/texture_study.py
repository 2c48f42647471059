#!/usr/bin/env python3
"""Frame time of models/Tor.obj with textured walls: 1920 x 1080 x 256 spp, -MRR 8, no adaptive sampling.
Every configuration is one `pt_render -BENCH_STEPS 3` process (one warm-up frame, then three timed ones), run twice; the
configurations are interleaved, so that the two runs of each lie apart in time.  The model is Tor.obj with planar `vt` coordinates
(tools/make_textured_scene.py: the repository's own model has none); `none` renders it without a list -- the kernels and the bytes of
Tor.obj itself --, `bilinear` with a 1024 x 1024 checkerboard on the three wall materials (1, 2, 3), `nearest` the same with nearest
filtering.  --parent-exe names a pt_render built from the parent commit: its `none` run is the yardstick, interleaved with the
others.  Prints one JSON object: both runs of every configuration, their mean, and the ratios.

    python tools/texture_study.py [--exe path/to/pt_render] [--parent-exe path/to/parent/pt_render] > profiles/texture_study.txt"""
import argparse
import json
import os
import tempfile

import environment_study as ES
import make_textured_scene as MT
from glass_study import one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render"))
    ap.add_argument("--parent-exe", default=None, help="pt_render of the parent commit: the yardstick for the run without -TEXTURE")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        d = tmp + "/"
        MT.generate(os.path.join(ROOT, "models"), d)
        pic = d + "checker.bmp"
        configs = {"none": (args.exe, []), "bilinear": (args.exe, ["-TEXTURE", ",".join(f"{m}:{pic}:bilinear" for m in MT.WALLS)]),
                   "nearest": (args.exe, ["-TEXTURE", ",".join(f"{m}:{pic}:nearest" for m in MT.WALLS)])}
        if args.parent_exe:
            configs["parent_none"] = (args.parent_exe, [])
        runs = {k: [] for k in configs}
        for _ in range(2):
            for k, (exe, flags) in configs.items():
                runs[k].append(round(one(exe, d, "TorUV.obj", flags), 4))
    mean = {k: round(sum(v) / len(v), 4) for k, v in runs.items()}
    out = {"frame": f"Tor.obj with planar vt, {ES.W}x{ES.H}x{ES.SPP} spp, MRR {ES.MRR}, pt_render -BENCH_STEPS 3; a 1024 x 1024 checkerboard on materials 1, 2, 3",
           "ms_per_frame_runs": runs, "ms_per_frame_mean": mean,
           "run_to_run_spread_percent": {k: round(100.0 * abs(v[0] - v[1]) / min(v), 3) for k, v in runs.items()},
           "bilinear_over_none": round(mean["bilinear"] / mean["none"], 4), "nearest_over_none": round(mean["nearest"] / mean["none"], 4)}
    if args.parent_exe:
        out["none_over_parent_none"] = round(mean["none"] / mean["parent_none"], 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
