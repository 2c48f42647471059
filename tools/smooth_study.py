#!/usr/bin/env python3
"""Frame time of models/Tor.obj with shading normals: 1920 x 1080 x 256 spp, -MRR 8, no adaptive sampling.
Every configuration is one `pt_render -BENCH_STEPS 3` process (one warm-up frame, then three timed ones), run twice; the
configurations are interleaved, so that the two runs of each lie apart in time.  `none` is the closed room without the flag -- the
parent's kernels on the parent's bytes --, `smooth` the same with -SMOOTH auto (the torus rounded, every wall corner its face normal),
`glass` the torus as glass of ior 1.5 without shading normals (the yardstick of section 26), `smooth_glass` -SMOOTH auto with that
glass torus.  --parent-exe names a pt_render built from the parent commit: its `none` run is the yardstick, interleaved with the
others.  Prints one JSON object: both runs of every configuration, their mean, and the ratios.

    python tools/smooth_study.py [--exe path/to/pt_render] [--parent-exe path/to/parent/pt_render] > profiles/smooth_study.txt"""
import argparse
import json
import os

import environment_study as ES
from glass_study import GLASS, one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH = ["-SMOOTH", "auto"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render"))
    ap.add_argument("--parent-exe", default=None, help="pt_render of the parent commit: the yardstick for the run without -SMOOTH")
    args = ap.parse_args()
    models = os.path.join(ROOT, "models") + "/"
    configs = {"none": (args.exe, []), "smooth": (args.exe, SMOOTH), "glass": (args.exe, GLASS), "smooth_glass": (args.exe, SMOOTH + GLASS)}
    if args.parent_exe:
        configs["parent_none"] = (args.parent_exe, [])
    runs = {k: [] for k in configs}
    for _ in range(2):
        for k, (exe, flags) in configs.items():
            runs[k].append(round(one(exe, models, "Tor.obj", flags), 4))
    mean = {k: round(sum(v) / len(v), 4) for k, v in runs.items()}
    out = {"frame": f"Tor.obj, {ES.W}x{ES.H}x{ES.SPP} spp, MRR {ES.MRR}, pt_render -BENCH_STEPS 3; smooth: -SMOOTH auto (crease 60); glass: -GLASS 4:1.5 (the torus)",
           "ms_per_frame_runs": runs, "ms_per_frame_mean": mean,
           "run_to_run_spread_percent": {k: round(100.0 * abs(v[0] - v[1]) / min(v), 3) for k, v in runs.items()},
           "smooth_over_none": round(mean["smooth"] / mean["none"], 4), "smooth_glass_over_glass": round(mean["smooth_glass"] / mean["glass"], 4)}
    if args.parent_exe:
        out["none_over_parent_none"] = round(mean["none"] / mean["parent_none"], 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
