#!/usr/bin/env python3
"""Frame time of models/Tor.obj with its torus as glass: 1920 x 1080 x 256 spp, -MRR 8, no adaptive sampling.
Every configuration is one `pt_render -BENCH_STEPS 3` process (one warm-up frame, then three timed ones), run twice; the
configurations are interleaved, so that the two runs of each lie apart in time.  `none` is the closed room without -GLASS, `glass`
the same with the torus's material (4) as glass of ior 1.5, `open_env` / `open_env_glass` the room without its back wall
(tools/make_open_scene.py) under an environment (the open scene's own sky picture as a PFM), without and with the glass torus.
--parent-exe names a pt_render built from the parent commit: its `none` and `open_env` runs are the yardstick, interleaved with the
others.  Prints one JSON object: both runs of every configuration, their mean, and the ratios.

    python tools/glass_study.py [--exe path/to/pt_render] [--parent-exe path/to/parent/pt_render] > profiles/glass_study.txt"""
import argparse
import json
import os
import subprocess
import tempfile

import environment_study as ES
import make_open_scene as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLASS = ["-GLASS", "4:1.5"]


def one(exe, scene_dir, name, flags):
    cmd = [exe, "--W", str(ES.W), "--H", str(ES.H), "-RPP", str(ES.SPP), "-MRR", str(ES.MRR), "-ERR", "-1", "-SEED", "42", "-QUIET", "1",
           "-MODEL_PATH", scene_dir, "-MODEL_NAME", name, "-BENCH_STEPS", "3", "-BENCH_WARMUP", "1"] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: status {r.returncode}: {r.stderr.strip()}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render"))
    ap.add_argument("--parent-exe", default=None, help="pt_render of the parent commit: the yardstick for the runs without -GLASS")
    args = ap.parse_args()
    models = os.path.join(ROOT, "models") + "/"
    with tempfile.TemporaryDirectory() as tmp:
        d = tmp + "/"
        MO.generate(models, d)
        ES.bmp_to_pfm(d + "sky.bmp", d + "sky.pfm")
        env = ["-ENV", d + "sky.pfm", "-ENV_SIZE", "1024"]
        configs = {"none": (args.exe, models, "Tor.obj", []), "glass": (args.exe, models, "Tor.obj", GLASS),
                   "open_env": (args.exe, d, "TorOpen.obj", env), "open_env_glass": (args.exe, d, "TorOpen.obj", env + GLASS)}
        if args.parent_exe:
            configs["parent_none"] = (args.parent_exe, models, "Tor.obj", [])
            configs["parent_open_env"] = (args.parent_exe, d, "TorOpen.obj", env)
        runs = {k: [] for k in configs}
        for _ in range(2):
            for k, (exe, scene_dir, name, flags) in configs.items():
                runs[k].append(round(one(exe, scene_dir, name, flags), 4))
    mean = {k: round(sum(v) / len(v), 4) for k, v in runs.items()}
    out = {"frame": f"Tor.obj, {ES.W}x{ES.H}x{ES.SPP} spp, MRR {ES.MRR}, pt_render -BENCH_STEPS 3; glass: -GLASS 4:1.5 (the torus)",
           "ms_per_frame_runs": runs, "ms_per_frame_mean": mean,
           "run_to_run_spread_percent": {k: round(100.0 * abs(v[0] - v[1]) / min(v), 3) for k, v in runs.items()},
           "glass_over_none": round(mean["glass"] / mean["none"], 4), "open_env_glass_over_open_env": round(mean["open_env_glass"] / mean["open_env"], 4)}
    if args.parent_exe:
        out["none_over_parent_none"] = round(mean["none"] / mean["parent_none"], 4)
        out["open_env_over_parent_open_env"] = round(mean["open_env"] / mean["parent_open_env"], 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
