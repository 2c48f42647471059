#!/usr/bin/env python3
"""Frame time of models/Tor.obj with a roughness list: 1920 x 1080 x 256 spp, -MRR 8, no adaptive sampling.
Every configuration is one `pt_render -BENCH_STEPS 3` process (one warm-up frame, then three timed ones), run twice; the
configurations are interleaved, so that the two runs of each lie apart in time.  `none` is the closed room without the flag -- the
parent's kernels on the parent's bytes --, `torus` the same with -ROUGH 4:0.3, `all` with -ROUGH on all four materials that do not
emit.  --parent-exe names a pt_render built from the parent commit: its `none` run is the yardstick, interleaved with the others.
Prints one JSON object: both runs of every configuration, their mean, and the ratios.

    python tools/rough_study.py [--exe path/to/pt_render] [--parent-exe path/to/parent/pt_render] > profiles/rough_study.txt"""
import argparse
import json
import os

import environment_study as ES
from glass_study import one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORUS = ["-ROUGH", "4:0.3"]
ALL = ["-ROUGH", "1:0.3,2:0.3,3:0.3,4:0.3"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render"))
    ap.add_argument("--parent-exe", default=None, help="pt_render of the parent commit: the yardstick for the run without -ROUGH")
    args = ap.parse_args()
    models = os.path.join(ROOT, "models") + "/"
    configs = {"none": (args.exe, []), "torus": (args.exe, TORUS), "all": (args.exe, ALL)}
    if args.parent_exe:
        configs["parent_none"] = (args.parent_exe, [])
    runs = {k: [] for k in configs}
    for _ in range(2):
        for k, (exe, flags) in configs.items():
            runs[k].append(round(one(exe, models, "Tor.obj", flags), 4))
    mean = {k: round(sum(v) / len(v), 4) for k, v in runs.items()}
    out = {"frame": f"Tor.obj, {ES.W}x{ES.H}x{ES.SPP} spp, MRR {ES.MRR}, pt_render -BENCH_STEPS 3; torus: -ROUGH 4:0.3; all: -ROUGH 1:0.3,2:0.3,3:0.3,4:0.3",
           "ms_per_frame_runs": runs, "ms_per_frame_mean": mean,
           "run_to_run_spread_percent": {k: round(100.0 * abs(v[0] - v[1]) / min(v), 3) for k, v in runs.items()},
           "torus_over_none": round(mean["torus"] / mean["none"], 4), "all_over_none": round(mean["all"] / mean["none"], 4)}
    if args.parent_exe:
        out["none_over_parent_none"] = round(mean["none"] / mean["parent_none"], 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
