#!/usr/bin/env python3
"""Frame time and payoff of Russian roulette on models/Tor.obj under -DIRECT 1: 1920 x 1080 x 256 spp, no adaptive
sampling.  Every timed configuration is one `pt_render -BENCH_STEPS 3` process (one warm-up frame, then three timed ones), run twice,
the configurations interleaved: -MRR 8 and -MRR 32, each without the flag and with -RR 3.  Mean segments per path come from the
statistics kernels at 480 x 270 x 16 spp.  The sweeps -- the floor over 1/4, 1/16, 1/64 through pt_render, the regeneration threshold
over 1, 4, 16, 64 through the test-hook library's kernel time (the planner's regen_min_dead override) -- run at -MRR 32, -RR 3.
Then the payoff at equal time, per -MRR: the -RR sample count is 256 scaled by the two measured frame times; both frames are rendered
through the library and each one's per-pixel RMSE (all pixels, three channels, linear) is taken against a -DIRECT 1 frame without
roulette of REF_SPP samples under another seed at the same -MRR, whose own error (from its sum2 plane) is printed beside them, with
the three means.  --env: the same frame times and payoff on the open scene under the sun panorama of tools/envdirect_study.py with
-DIRECT_ENV 1.  Prints one JSON object.

    python tools/roulette_study.py [--exe path/to/pt_render] [--env] > profiles/roulette_study.txt"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 1920, 1080, 256
REF_SPP, REF_CHUNK, REF_SEED = 8192, 1024, 4242
START = 3


def timed(exe, models, name, spp, mrr, flags):
    cmd = [exe, "--W", str(W), "--H", str(H), "-RPP", str(spp), "-MRR", str(mrr), "-ERR", "-1", "-SEED", "42", "-QUIET", "1",
           "-MODEL_PATH", models, "-MODEL_NAME", name, "-BENCH_STEPS", "3", "-BENCH_WARMUP", "1"] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: status {r.returncode}: {r.stderr.strip()}")
    return round(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"], 4)


def interleaved(configs):
    runs = {k: [] for k in configs}
    for _ in range(2):
        for k, run in configs.items():
            runs[k].append(run())
    return runs, {k: round(sum(v) / len(v), 4) for k, v in runs.items()}


def switch_on(scene, env):
    if env:
        scene.set_environment(env)
        scene.set_environment_sampling()
    else:
        scene.set_direct_lighting(True)


def payoff(pt, models, name, env, mrr, plain_ms, rr_ms, floor):
    spp_eq = max(1, int(round(SPP * plain_ms / rr_ms)))
    scene = pt.Scene.load_obj(models, name, device=0)
    switch_on(scene, env)
    s, _, c, _ = scene.render_host(W, H, SPP, mrr, seed=42, want_stats=False)
    plain = s.astype(np.float64) / c[:, None]
    acc = None
    for begin in range(0, REF_SPP, REF_CHUNK):
        acc = scene.render_host(W, H, REF_CHUNK, mrr, seed=REF_SEED, pass_begin=begin, accum=acc, want_stats=False)[:3]
    ref = acc[0].astype(np.float64) / REF_SPP
    ref_var = np.maximum(acc[1].astype(np.float64) / REF_SPP - ref * ref, 0.0) / REF_SPP
    scene.set_roulette(START, floor)
    s, _, c, _ = scene.render_host(W, H, spp_eq, mrr, seed=42, want_stats=False)
    assert (c == spp_eq).all()
    rr = s.astype(np.float64) / c[:, None]
    scene.close()
    rmse = lambda est: float(np.sqrt(np.mean((est - ref) ** 2)))
    e_plain, e_rr, e_ref = rmse(plain), rmse(rr), float(np.sqrt(ref_var.mean()))
    n = ref.shape[0]
    return {"mrr": mrr, "reference": f"no roulette, {REF_SPP} spp, seed {REF_SEED}", "reference_mean": round(float(ref.mean()), 6),
            "reference_own_rmse": round(e_ref, 6), "plain_spp": SPP, "plain_ms": plain_ms, "plain_mean": round(float(plain.mean()), 6),
            "plain_rmse": round(e_plain, 6), "rr_spp_at_equal_time": spp_eq, "rr_ms_at_256_spp": rr_ms, "rr_mean": round(float(rr.mean()), 6),
            "rr_rmse": round(e_rr, 6), "rr_mean_minus_reference_over_its_standard_error":
                round(float(rr.mean() - ref.mean()) / float(np.hypot(e_rr, e_ref) / np.sqrt(n)), 3),
            "rmse_plain_over_rr": round(e_plain / e_rr, 3)}


def segments_per_path(pt, models, name, env, mrr, roulette):
    scene = pt.Scene.load_obj(models, name, device=0)
    switch_on(scene, env)
    if roulette:
        scene.set_roulette(*roulette)
    st = scene.render_host(480, 270, 16, mrr, seed=42, want_stats=True)[3]
    scene.close()
    return round(st["segments"] / st["samples_traced"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render"))
    ap.add_argument("--env", action="store_true", help="the open scene under the sun panorama with -DIRECT_ENV 1")
    ap.add_argument("--no-sweeps", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    pt = importlib.import_module("path-tracing_amd")
    with tempfile.TemporaryDirectory() as tmp:
        models, name, env, on = os.path.join(ROOT, "models") + "/", "Tor.obj", None, ["-DIRECT", "1"]
        if args.env:
            import envdirect_study as EDS
            import make_open_scene as MO
            models, name, env = tmp + "/", "TorOpen.obj", tmp + "/sun.pfm"
            MO.generate(os.path.join(ROOT, "models"), models)
            EDS.sun_panorama(env)
            on = ["-ENV", env, "-DIRECT_ENV", "1"]
        floor = pt.ROULETTE_DEFAULT_FLOOR
        configs = {}
        for mrr in (8, 32):
            configs[f"mrr{mrr}"] = lambda mrr=mrr: timed(args.exe, models, name, SPP, mrr, on)
            configs[f"mrr{mrr}_rr{START}"] = lambda mrr=mrr: timed(args.exe, models, name, SPP, mrr, on + ["-RR", str(START)])
        runs, mean = interleaved(configs)
        out = {"frame": f"{name}, {W}x{H}x{SPP} spp, {' '.join(on[-2:])}, pt_render -BENCH_STEPS 3, -RR {START} (floor {floor})",
               "ms_per_frame_runs": runs, "ms_per_frame_mean": mean,
               "rr_over_plain": {f"mrr{m}": round(mean[f"mrr{m}_rr{START}"] / mean[f"mrr{m}"], 4) for m in (8, 32)},
               "segments_per_path": {f"mrr{m}{'_rr' if r else ''}": segments_per_path(pt, models, name, env, m, (START, floor) if r else None)
                                     for m in (8, 32) for r in (False, True)}}
        if not args.no_sweeps:
            sweep = {f"floor_1/{d}": (lambda d=d: timed(args.exe, models, name, SPP, 32, on + ["-RR", f"{START}:{1.0 / d}"])) for d in (4, 16, 64)}
            out["floor_sweep_mrr32_ms_runs"] = interleaved(sweep)[0]
            L = pt.load_library(pt.TESTHOOKS_LIB_PATH)
            scene = pt.Scene.load_obj(models, name, device=0, library=L)
            switch_on(scene, env)
            scene.set_roulette(START, floor)

            def kernel_ms(dead):
                L.pt_test_set_mutation(b"regen_min_dead", float(dead))
                return round(scene.render_host(W, H, 64, 32, seed=42, want_stats=True)[3]["kernel_ms"], 4)
            kernel_ms(4)                                                          # (warm-up)
            out["regen_min_dead_sweep_mrr32_64spp_kernel_ms_runs"] = interleaved({str(d): (lambda d=d: kernel_ms(d)) for d in (1, 4, 16, 64)})[0]
            L.pt_test_set_mutation(b"reset", 0.0)
            scene.close()
        out["equal_time_payoff"] = [payoff(pt, models, name, env, m, mean[f"mrr{m}"], mean[f"mrr{m}_rr{START}"], floor) for m in (8, 32)]
        print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
