#!/usr/bin/env python3
"""Frame time and payoff of environment sampling on the open Tor scene (models/Tor.obj without its back wall) under
a sun panorama -- a disc of SUN_RADIANCE, SUN_DEGREES across, on a sky of 0.2 --: 1920 x 1080 x 256 spp, -MRR 8, no adaptive sampling.
Every configuration is one `pt_render -BENCH_STEPS 3` process (one warm-up frame, then three timed ones), run twice; the configurations
are interleaved.  `none` is -ENV alone -- the parent's environment kernels --, `direct` adds -DIRECT 1 -- the parent's direct kernels,
which sample the lamp only --, `direct_env` adds -DIRECT_ENV 1.  --parent-exe names a pt_render built from the parent commit: its
`none` and `direct` runs are the yardsticks, interleaved with the others.
Then the payoff, at equal time: the -DIRECT_ENV 1 sample count is the no-flag frame's 256 scaled by the two measured frame times, both
frames are rendered through the library at the full size, and each one's per-pixel RMSE (all pixels, three channels, linear) is taken
against a frame of the PARENT'S estimator -- the no-flag environment kernels, counted per path: sum / samples traced -- of REF_SPP
samples under another seed, whose own error (from its sum2 plane) is printed beside them; the frames' means against the reference's
mean are the device-side check of unbiasedness, taken a second time with a -DIRECT_ENV 1 frame of HIGH_SPP samples, whose own error is
below the reference's.  A pixel's three channels come from the same paths, so a frame mean's standard error counts pixels, not values.
Prints one JSON object.

    python tools/envdirect_study.py [--exe path/to/pt_render] [--parent-exe path/to/parent/pt_render] > profiles/envdirect_study.txt"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import environment_study as ES
import make_open_scene as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SPP, REF_CHUNK, REF_SEED = 32768, 2048, 4242
HIGH_SPP, HIGH_SEED = 8192, 777
SUN_RADIANCE, SUN_DEGREES, SKY = 400.0, 6.0, 0.2


def sun_panorama(path, w=512, h=256):
    """An equirectangular PFM: the sun 35 degrees above the horizon, behind the scene and to its right."""
    theta = (np.arange(h) + 0.5) / h * np.pi
    phi = (np.arange(w) + 0.5) / w * 2 * np.pi
    d = np.stack([np.sin(theta)[:, None] * np.cos(phi)[None, :], np.broadcast_to(np.cos(theta)[:, None], (h, w)), np.sin(theta)[:, None] * np.sin(phi)[None, :]], -1)
    row, col = int(h * (90 - 35) / 180), int(w * 0.36)
    pic = np.full((h, w, 3), SKY, np.float32)
    pic[d @ d[row, col] > np.cos(np.radians(SUN_DEGREES / 2))] = SUN_RADIANCE
    body = pic[::-1].astype("<f4").tobytes()
    open(path, "wb").write(b"PF\n%d %d\n-1.0\n" % (w, h) + body)
    return float((pic[..., 0] > SKY).mean())


def timed(exe, models, spp, flags):
    cmd = [exe, "--W", str(ES.W), "--H", str(ES.H), "-RPP", str(spp), "-MRR", str(ES.MRR), "-ERR", "-1", "-SEED", "42", "-QUIET", "1",
           "-MODEL_PATH", models, "-MODEL_NAME", "TorOpen.obj", "-BENCH_STEPS", "3", "-BENCH_WARMUP", "1"] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: status {r.returncode}: {r.stderr.strip()}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def payoff(exe, models, env, none_ms, sampled_ms):
    sys.path.insert(0, ROOT)
    pt = importlib.import_module("path-tracing_amd")
    W, H, SPP, MRR = ES.W, ES.H, ES.SPP, ES.MRR
    spp_eq = max(1, int(round(SPP * none_ms / sampled_ms)))
    eq_ms = [round(timed(exe, models, spp_eq, ["-ENV", env, "-DIRECT_ENV", "1"]), 4) for _ in range(2)]
    scene = pt.Scene.load_obj(models, "TorOpen.obj", device=0)
    scene.set_environment(env)
    s, _, c, st = scene.render_host(W, H, SPP, MRR, seed=42, want_stats=True)
    assert st["samples_traced"] == W * H * SPP, st                        # no adaptive sampling: no pixel sat a pass out
    per_path = s.astype(np.float64) / SPP                                 # count holds the contributing paths only
    acc = None
    for begin in range(0, REF_SPP, REF_CHUNK):                            # the parent's estimator at REF_SPP, another seed
        r = scene.render_host(W, H, REF_CHUNK, MRR, seed=REF_SEED, pass_begin=begin, accum=acc, want_stats=False)
        acc = r[:3]
    ref = acc[0].astype(np.float64) / REF_SPP
    ref_var = np.maximum(acc[1].astype(np.float64) / REF_SPP - ref * ref, 0.0) / REF_SPP
    scene.set_environment_sampling()
    share = float(scene.environment_sampling())
    s, _, c, _ = scene.render_host(W, H, spp_eq, MRR, seed=42, want_stats=False)
    assert (c == spp_eq).all()
    sampled = s.astype(np.float64) / c[:, None]
    acc = None
    for begin in range(0, HIGH_SPP, REF_CHUNK):                           # the unbiasedness check: the sampled estimator at HIGH_SPP, a third seed
        r = scene.render_host(W, H, REF_CHUNK, MRR, seed=HIGH_SEED, pass_begin=begin, accum=acc, want_stats=False)
        acc = r[:3]
    assert (acc[2] == HIGH_SPP).all()
    high = acc[0].astype(np.float64) / HIGH_SPP
    high_var = np.maximum(acc[1].astype(np.float64) / HIGH_SPP - high * high, 0.0) / HIGH_SPP
    scene.close()
    rmse = lambda est: float(np.sqrt(np.mean((est - ref) ** 2)))
    e_none, e_sampled, e_ref = rmse(per_path), rmse(sampled), float(np.sqrt(ref_var.mean()))
    e_high = float(np.sqrt(high_var.mean()))
    n = ref.shape[0]                                                      # (a pixel's three channels come from the same paths: pixels are the independent draws)
    return {"reference": f"no flag (-ENV alone), sum / samples traced, {REF_SPP} spp, seed {REF_SEED}, full frame", "reference_mean": round(float(ref.mean()), 6),
            "reference_own_rmse": round(e_ref, 6), "reference_mean_standard_error": round(e_ref / np.sqrt(n), 8),
            "share": round(share, 6), "none_spp": SPP, "none_ms": none_ms, "none_per_path_mean": round(float(per_path.mean()), 6),
            "none_per_path_rmse": round(e_none, 6), "sampled_spp_at_equal_time": spp_eq, "sampled_ms_at_that_spp_runs": eq_ms,
            "sampled_mean": round(float(sampled.mean()), 6), "sampled_rmse": round(e_sampled, 6),
            "sampled_mean_minus_reference_mean": round(float(sampled.mean() - ref.mean()), 8),
            "sampled_frame_mean_standard_error": round(e_sampled / np.sqrt(n), 8),
            "mean_difference_over_its_standard_error": round(float(sampled.mean() - ref.mean()) / float(np.hypot(e_sampled, e_ref) / np.sqrt(n)), 3),
            "sampled_high_spp": HIGH_SPP, "sampled_high_mean": round(float(high.mean()), 6), "sampled_high_own_rmse": round(e_high, 6),
            "sampled_high_mean_minus_reference_mean": round(float(high.mean() - ref.mean()), 8),
            "sampled_high_difference_over_its_standard_error": round(float(high.mean() - ref.mean()) / float(np.hypot(e_high, e_ref) / np.sqrt(n)), 3),
            "sampled_high_rmse_against_reference": round(rmse(high), 6),
            "rmse_none_over_sampled": round(e_none / e_sampled, 3), "variance_none_over_sampled": round((e_none / e_sampled) ** 2, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render"))
    ap.add_argument("--parent-exe", default=None, help="pt_render of the parent commit: the yardstick for the runs without -DIRECT_ENV")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        models = tmp + "/"
        MO.generate(os.path.join(ROOT, "models"), models)
        env = models + "sun.pfm"
        sun_share = sun_panorama(env)
        e = ["-ENV", env]
        configs = {"none": (args.exe, e), "direct": (args.exe, e + ["-DIRECT", "1"]), "direct_env": (args.exe, e + ["-DIRECT_ENV", "1"])}
        if args.parent_exe:
            configs["parent_none"] = (args.parent_exe, e)
            configs["parent_direct"] = (args.parent_exe, e + ["-DIRECT", "1"])
        runs = {k: [] for k in configs}
        for _ in range(2):
            for k, (exe, flags) in configs.items():
                runs[k].append(round(timed(exe, models, ES.SPP, flags), 4))
        mean = {k: round(sum(v) / len(v), 4) for k, v in runs.items()}
        out = {"frame": f"open Tor scene, {ES.W}x{ES.H}x{ES.SPP} spp, MRR {ES.MRR}, pt_render -BENCH_STEPS 3, -ENV sun.pfm (a disc of {SUN_RADIANCE} over "
                        f"{SUN_DEGREES} degrees, {sun_share:.2e} of the picture, on a sky of {SKY})",
               "ms_per_frame_runs": runs, "ms_per_frame_mean": mean,
               "run_to_run_spread_percent": {k: round(100.0 * abs(v[0] - v[1]) / min(v), 3) for k, v in runs.items()},
               "direct_env_over_none": round(mean["direct_env"] / mean["none"], 4), "direct_env_over_direct": round(mean["direct_env"] / mean["direct"], 4)}
        if args.parent_exe:
            out["none_over_parent_none"] = round(mean["none"] / mean["parent_none"], 4)
            out["direct_over_parent_direct"] = round(mean["direct"] / mean["parent_direct"], 4)
        out["equal_time_payoff"] = payoff(args.exe, models, env, mean["none"], mean["direct_env"])
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
