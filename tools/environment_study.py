#!/usr/bin/env python3
"""Frame time of the open Tor scene under the BMP skybox and under an environment of the same content:
models/Tor.obj without its back wall (tools/make_open_scene.py), 1920 x 1080 x 256 spp, -MRR 8, no adaptive sampling.  The
environment is the skybox's own picture as a PFM (every byte / 256: the value the skybox lookup gives a texel), resampled into an
octahedral map of N = 1024.  Every configuration is one `pt_render -BENCH_STEPS 3` process (one warm-up frame, then three timed
ones), run twice; the configurations are interleaved, so that the two runs of each lie apart in time.  `none` is the same scene with
neither (misses contribute nothing, the skybox-free kernel).  Prints one JSON object: both runs of every configuration, their mean,
and the environment's ratio to the skybox.

    python tools/environment_study.py [--exe path/to/pt_render] [--size 1024] > profiles/environment_study.txt"""
import argparse
import json
import os
import struct
import subprocess
import tempfile

import make_open_scene as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, MRR = 1920, 1080, 256, 8


def bmp_to_pfm(bmp, pfm):
    """The skybox's 24-bit BMP as the PFM with the same content: r, g, b = byte / 256, rows bottom-up in both files."""
    data = open(bmp, "rb").read()
    w, h = struct.unpack_from("<ii", data, 18)
    stride = (3 * w + 3) // 4 * 4
    with open(pfm, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        for y in range(h):
            row = data[54 + y * stride:54 + y * stride + 3 * w]
            f.write(struct.pack("<%df" % (3 * w), *[row[3 * x + 2 - c] / 256.0 for x in range(w) for c in range(3)]))


def one(exe, scene_dir, flags):
    cmd = [exe, "--W", str(W), "--H", str(H), "-RPP", str(SPP), "-MRR", str(MRR), "-ERR", "-1", "-SEED", "42", "-QUIET", "1",
           "-MODEL_PATH", scene_dir, "-MODEL_NAME", "TorOpen.obj", "-BENCH_STEPS", "3", "-BENCH_WARMUP", "1"] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: status {r.returncode}: {r.stderr.strip()}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render"))
    ap.add_argument("--size", type=int, default=1024, help="N of the octahedral map (-ENV_SIZE)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        d = tmp + "/"
        MO.generate(os.path.join(ROOT, "models"), d)
        bmp_to_pfm(d + "sky.bmp", d + "sky.pfm")
        configs = {"none": [], "skybox": ["-SKYBOX", d + "sky.bmp"], "environment": ["-ENV", d + "sky.pfm", "-ENV_SIZE", str(args.size)]}
        runs = {k: [] for k in configs}
        for _ in range(2):
            for k, flags in configs.items():
                runs[k].append(round(one(args.exe, d, flags), 4))
    mean = {k: round(sum(v) / len(v), 4) for k, v in runs.items()}
    print(json.dumps({"frame": f"Tor.obj without its back wall, {W}x{H}x{SPP} spp, MRR {MRR}, pt_render -BENCH_STEPS 3",
                      "sky": "tools/make_open_scene.py sky.bmp 256x128; the environment: the same picture / 256 as a PFM, -ENV_SIZE %d" % args.size,
                      "exe": os.path.relpath(args.exe, ROOT), "ms_per_frame_runs": runs, "ms_per_frame_mean": mean,
                      "environment_over_skybox": round(mean["environment"] / mean["skybox"], 4)}, indent=1))


if __name__ == "__main__":
    main()
