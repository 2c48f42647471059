#!/usr/bin/env python3
"""Frame time of models/Tor.obj with direct lighting: 1920 x 1080 x 256 spp, -MRR 8, no adaptive sampling.
Every configuration is one `pt_render -BENCH_STEPS 3` process (one warm-up frame, then three timed ones), run twice; the
configurations are interleaved, so that the two runs of each lie apart in time.  `none` is the closed room without the flag -- the
parent's kernels on the parent's bytes --, `direct` the same with -DIRECT 1, `direct_smooth` with -DIRECT 1 -SMOOTH auto.
--parent-exe names a pt_render built from the parent commit: its `none` run is the yardstick, interleaved with the others.
Then the payoff, at equal time: the -DIRECT 1 sample count is the no-flag frame's 256 scaled by the two measured frame times (and that
frame is timed too), both frames are rendered through the library at the full size, and each one's per-pixel RMSE (all pixels, three
channels, linear) is taken against a -DIRECT 1 frame of REF_SPP samples under another seed.  The no-flag estimator is taken per path:
its frame's sum divided by the paths traced, 256 for every pixel of this closed room without adaptive sampling -- the full frame on
the device, not the host composition at a reduced size.  The reference's own noise (from its sum2 plane) is printed beside them.
Prints one JSON object: both runs of every configuration, their mean, the ratios and the payoff.

    python tools/direct_study.py [--exe path/to/pt_render] [--parent-exe path/to/parent/pt_render] > profiles/direct_study.txt"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

import environment_study as ES
from glass_study import one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = ["-DIRECT", "1"]
DIRECT_SMOOTH = ["-DIRECT", "1", "-SMOOTH", "auto"]
REF_SPP, REF_CHUNK, REF_SEED = 8192, 1024, 4242


def timed(exe, models, spp, flags):
    cmd = [exe, "--W", str(ES.W), "--H", str(ES.H), "-RPP", str(spp), "-MRR", str(ES.MRR), "-ERR", "-1", "-SEED", "42", "-QUIET", "1",
           "-MODEL_PATH", models, "-MODEL_NAME", "Tor.obj", "-BENCH_STEPS", "3", "-BENCH_WARMUP", "1"] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: status {r.returncode}: {r.stderr.strip()}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def payoff(exe, models, none_ms, direct_ms):
    sys.path.insert(0, ROOT)
    pt = importlib.import_module("path-tracing_amd")
    W, H, SPP, MRR = ES.W, ES.H, ES.SPP, ES.MRR
    spp_eq = max(1, int(round(SPP * none_ms / direct_ms)))
    eq_ms = [round(timed(exe, models, spp_eq, DIRECT), 4) for _ in range(2)]
    scene = pt.Scene.load_obj(models, "Tor.obj", device=0)
    s, _, c, st = scene.render_host(W, H, SPP, MRR, seed=42, want_stats=True)
    assert st["samples_traced"] == W * H * SPP, st                        # no adaptive sampling, a closed room: no pixel sat a pass out
    per_path = s.astype(np.float64) / SPP                                 # every pixel traced SPP paths: count holds the contributing ones only
    contributing = float(c.mean())
    scene.set_direct_lighting(True)
    s, _, c, _ = scene.render_host(W, H, spp_eq, MRR, seed=42, want_stats=False)
    assert (c == spp_eq).all()
    direct = s.astype(np.float64) / c[:, None]
    acc = None
    for begin in range(0, REF_SPP, REF_CHUNK):
        r = scene.render_host(W, H, REF_CHUNK, MRR, seed=REF_SEED, pass_begin=begin, accum=acc, want_stats=False)
        acc = r[:3]
    assert (acc[2] == REF_SPP).all()
    ref = acc[0].astype(np.float64) / REF_SPP
    ref_var = np.maximum(acc[1].astype(np.float64) / REF_SPP - ref * ref, 0.0) / REF_SPP
    scene.close()
    rmse = lambda est: float(np.sqrt(np.mean((est - ref) ** 2)))
    e_none, e_direct = rmse(per_path), rmse(direct)
    return {"reference": f"-DIRECT 1, {REF_SPP} spp, seed {REF_SEED}, full frame", "reference_mean": round(float(ref.mean()), 6),
            "reference_own_rmse": round(float(np.sqrt(ref_var.mean())), 6),
            "none_spp": SPP, "none_ms": none_ms, "none_contributing_paths_per_pixel": round(contributing, 3),
            "none_per_path_mean": round(float(per_path.mean()), 6), "none_per_path_rmse": round(e_none, 6),
            "direct_spp_at_equal_time": spp_eq, "direct_ms_at_that_spp_runs": eq_ms, "direct_mean": round(float(direct.mean()), 6),
            "direct_rmse": round(e_direct, 6),
            "rmse_none_over_direct": round(e_none / e_direct, 3), "variance_none_over_direct": round((e_none / e_direct) ** 2, 2),
            "no_flag_estimator": "the device's no-flag frame at the full size, sum / paths traced (not the host composition)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render"))
    ap.add_argument("--parent-exe", default=None, help="pt_render of the parent commit: the yardstick for the run without -DIRECT")
    args = ap.parse_args()
    models = os.path.join(ROOT, "models") + "/"
    configs = {"none": (args.exe, []), "direct": (args.exe, DIRECT), "direct_smooth": (args.exe, DIRECT_SMOOTH)}
    if args.parent_exe:
        configs["parent_none"] = (args.parent_exe, [])
    runs = {k: [] for k in configs}
    for _ in range(2):
        for k, (exe, flags) in configs.items():
            runs[k].append(round(one(exe, models, "Tor.obj", flags), 4))
    mean = {k: round(sum(v) / len(v), 4) for k, v in runs.items()}
    out = {"frame": f"Tor.obj, {ES.W}x{ES.H}x{ES.SPP} spp, MRR {ES.MRR}, pt_render -BENCH_STEPS 3; direct: -DIRECT 1; direct_smooth: -DIRECT 1 -SMOOTH auto",
           "ms_per_frame_runs": runs, "ms_per_frame_mean": mean,
           "run_to_run_spread_percent": {k: round(100.0 * abs(v[0] - v[1]) / min(v), 3) for k, v in runs.items()},
           "direct_over_none": round(mean["direct"] / mean["none"], 4), "direct_smooth_over_none": round(mean["direct_smooth"] / mean["none"], 4)}
    if args.parent_exe:
        out["none_over_parent_none"] = round(mean["none"] / mean["parent_none"], 4)
    out["equal_time_payoff"] = payoff(args.exe, models, mean["none"], mean["direct"])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
