#!/usr/bin/env python3
"""Do the image-space kernels' tests bite?  Each row of MUTATIONS is one small, value-only error planted in a copy of the sources;
the library built from that copy must fail the named test of tests/test_gpu_image_kernels.py.  For every row the suite as it
was BEFORE that file existed (PARENT_TESTS: every earlier GPU test that runs these kernels) is run too: a row it passes is a gap
the new tests closed.  The recorded run is profiles/r05_image_kernel_mutations.jsonl.

    python tools/mutate_image_kernels.py build --libs DIR             # needs hipcc, no device: DIR/<name>/libpt_hip.so per row
    python tools/mutate_image_kernels.py run --libs DIR --record F    # needs a device: one JSON line per row
    python tools/mutate_image_kernels.py all --record F               # both, in a temporary directory

Rules for a row: it changes VALUES only -- every index stays inside its buffer (a clamp that is moved is clamped again), no barrier
is skipped, nothing can fault or hang.  No mutated source is ever written into the tree: the sources are copied (with the tree's
object files, so that only the mutated file is recompiled) and built there by the Makefile itself, i.e. with its own flags.  Every
build and every pytest run is its own `timeout -k 10` child; an exit status that is not a plain pass or test failure (a time
limit, an abort, a segmentation fault) ends the sweep at once -- that row is to be removed from the table, not retried.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "tests/test_gpu_image_kernels.py"
FILTERS, CAPI, DENOISE = (f"path-tracing_amd/csrc/{f}" for f in ("pt_filters.hip", "pt_capi.cpp", "pt_denoise.hip"))
# the GPU tests that ran these kernels before tests/test_gpu_image_kernels.py was added
PARENT_TESTS = {FILTERS: ["tests/test_post_filters.py", "tests/test_gpu_cli.py"], CAPI: ["tests/test_post_filters.py", "tests/test_gpu_cli.py"],
                DENOISE: ["tests/test_gpu_denoise.py", "tests/test_gpu_temporal.py"]}
STOP = (124, 134, 137, 139)      # time limit, abort, kill, segmentation fault: not a test failure
CLAMP = "const int y = min(height - 1, max(0, y0 + ty)), x = min(width - 1, max(0, x0 + tx));"
CLASS_IN_VARIANCE = "if (!(aq.w >= 0.0f) || bq.w != bp.w) continue;\n                if (dy >= -1"

# name, file, [(exact text, replacement)], occurrences of each text in the file, the test expected to fail, note
MUTATIONS = [
    ("gauss_lds_clamp_right", FILTERS, [(CLAMP, CLAMP.replace("x = min(width - 1, max(0, x0 + tx))", "x = max(0, min(width - 2, max(0, x0 + tx)))"))], 1,
     "test_filters_shape_grid[1-0]", "halo clamp on the far side in x: width - 1 -> width - 2 (clamped again at 0 for a width of 1)"),
    ("gauss_lds_clamp_bottom", FILTERS, [(CLAMP, CLAMP.replace("y = min(height - 1, max(0, y0 + ty))", "y = max(0, min(height - 2, max(0, y0 + ty)))"))], 1,
     "test_filters_shape_grid[9-0]", "the same in y"),
    ("gauss_lds_taps_transposed", FILTERS, [("const float *row = tile + (ly + dy) * tw + lx;", "const float *row = tile + ly * tw + lx + dy;"),
                                            ("v0 += row[dx] * w;", "v0 += row[dx * tw] * w;"), ("v1 += row[plane + dx] * w;", "v1 += row[plane + dx * tw] * w;"),
                                            ("v2 += row[2 * plane + dx] * w;", "v2 += row[2 * plane + dx * tw] * w;")], 1,
     "test_filters_content[huge]", "rows and columns of the tap loop exchanged: the weights are symmetric, so only the ORDER of the sum "
     "changes -- visible where round() does not hide the last bits"),
    ("gauss_lds_staging_row", FILTERS, [("const int ty = idx / tw, tx = idx - ty * tw;", "const int ty = idx / (16 + rs), tx = idx - ty * tw;")], 1,
     "test_filters_shape_grid[1-0]", "staging row computed with 16 + rs instead of 16 + 2 rs (coordinates are clamped to the image after it)"),
    ("median_small_rank", FILTERS, [("constexpr int K = WS * WS / 2;", "constexpr int K = WS * WS / 2 - (WS >= 2 ? 1 : 0);")], 1,
     "test_filters_shape_grid[0-3]", "rank K -> K - 1 for WS >= 2 (the register array is sized by K)"),
    ("median_clamps_exchanged", FILTERS, [("const int i = max(min(wx + x, width - 1), 0);", "const int i = min(max(min(wx + x, height - 1), 0), width - 1);"),
                                          ("const int j = max(min(wy + y, height - 1), 0);", "const int j = min(max(min(wy + y, width - 1), 0), height - 1);")], 2,
     "test_filters_shape_grid[0-4]", "width and height exchanged in the clamps of both median kernels (clamped again to stay inside)"),
    ("filter_order", CAPI, [("    if (gauss) {   // main.cpp:187-189",
                             "    if (median) { PT_HIP_TRY(pt::launch_median(d_a, d_b, width, height, median, nullptr)); std::swap(d_a, d_b); }\n"
                             "    if (gauss) {   // main.cpp:187-189"),
                            ("    if (median) {   // main.cpp:190-192", "    if (false) {   // main.cpp:190-192")], 1,
     "test_filters_composition[33-31]", "median before Gaussian"),
    ("albedo_floor_ge", DENOISE, [("al > kDenoiseAlbedoFloor ? al : kDenoiseAlbedoFloor", "al >= kDenoiseAlbedoFloor ? al : kDenoiseAlbedoFloor")], 1,
     None, "EQUIVALENT, expected to pass everything: at al == 0.01 both branches give 0.01, and no other input tells > from >=.  Kept as the control "
     "of the sweep; the next row is the floor error that changes a value"),
    ("albedo_floor_only_at_zero", DENOISE, [("al > kDenoiseAlbedoFloor ? al : kDenoiseAlbedoFloor", "al > 0.0f ? al : kDenoiseAlbedoFloor")], 1,
     "test_denoise_counts_and_albedo[floor-mixed]", "the floor applied to an albedo of 0 only: values just below 0.01 pass through"),
    ("variance_class_test_dropped", DENOISE, [(CLASS_IN_VARIANCE, CLASS_IN_VARIANCE.replace(" || bq.w != bp.w", ""))], 1,
     "test_denoise_classes_and_normals[discrete-checker]", "the variance window also takes taps of the other class"),
    ("spatial_below_off_by_one", DENOISE, [("a.count[p] >= kDenoiseSpatialBelow ?", "a.count[p] >= kDenoiseSpatialBelow + 1 ?")], 1,
     "test_denoise_counts_and_albedo[floor-threshold]", "a pixel with exactly 4 samples still takes the spatial variance"),
    ("last_level_step_halved", DENOISE, [("other, a.width, a.height, 1 << level,", "other, a.width, a.height, (level > 0 && level == a.levels - 1) ? (1 << level) / 2 : 1 << level,")], 1,
     "test_denoise_shape_grid[0]", "the last a-trous level runs at half its spacing"),
]


def _step(cmd, limit, env=None, log=None):
    """One child under its own time limit; returns its exit status (124 / 137: the limit)."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if log:
        with open(log, "a") as f:
            f.write(f"$ {' '.join(cmd)}\n{r.stdout}\n[exit {r.returncode}]\n")
    return r.returncode if r.returncode >= 0 else 128 - r.returncode


def mutated_source(text, edits, occurrences, name):
    for old, new in edits:
        assert text.count(old) == occurrences, f"{name}: {old!r} occurs {text.count(old)} times, expected {occurrences}"
        text = text.replace(old, new)
    return text


def build_one(row, out_dir, log):
    name, rel, edits, occurrences = row[:4]
    with tempfile.TemporaryDirectory(prefix=f"mut_{name}_") as tmp:
        for d in ("include", "path-tracing_amd/csrc", "path-tracing_amd/lib/obj"):       # copy2 keeps mtimes: make rebuilds one file
            if os.path.isdir(os.path.join(ROOT, d)):
                shutil.copytree(os.path.join(ROOT, d), os.path.join(tmp, d), copy_function=shutil.copy2)
        path = os.path.join(tmp, rel)
        text = mutated_source(open(path).read(), edits, occurrences, name)
        with open(path, "w") as f:
            f.write(text)
        rc = _step(["make", "-C", os.path.join(tmp, "path-tracing_amd", "csrc"), "-s", "-j8", "../lib/libpt_hip.so"], 1500, log=log)
        if rc == 0:
            os.makedirs(os.path.join(out_dir, name), exist_ok=True)
            shutil.copy(os.path.join(tmp, "path-tracing_amd", "lib", "libpt_hip.so"), os.path.join(out_dir, name, "libpt_hip.so"))
        return rc


def _run_tests(lib, targets, limit, log):
    env = dict(os.environ, PT_HIP_LIB=lib)
    return _step([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu"] + targets, limit, env=env, log=log)


VERDICT = {0: "pass", 1: "fail"}


def run_one(row, libs, log):
    name, rel, _, _, test, note = row
    lib = os.path.join(libs, name, "libpt_hip.so")
    new_rc = _run_tests(lib, [f"{NEW}::{test}" if test else NEW], 900, log)
    rec = {"mutation": name, "file": rel, "expected_to_fail": f"{NEW}::{test}" if test else None, "note": note,
           "new_tests": VERDICT.get(new_rc, f"exit {new_rc}")}
    if new_rc in STOP:
        return rec, new_rc
    parent_rc = _run_tests(lib, PARENT_TESTS[rel], 900, log)
    rec["parent_suite"] = VERDICT.get(parent_rc, f"exit {parent_rc}")
    rec["parent_tests_run"] = PARENT_TESTS[rel]
    rec["gap_closed"] = bool(test) and new_rc == 1 and parent_rc == 0
    return rec, parent_rc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=["build", "run", "all", "check"])
    ap.add_argument("--libs", help="directory of the mutated libraries")
    ap.add_argument("--record", help="JSON lines, one per row")
    ap.add_argument("--log", help="every child's output")
    ap.add_argument("--only", nargs="*", help="row names")
    a = ap.parse_args()
    rows = [r for r in MUTATIONS if not a.only or r[0] in a.only]
    if a.mode == "check":                                   # every text is where the table says, and nothing else
        for name, rel, edits, occurrences, _, _ in rows:
            mutated_source(open(os.path.join(ROOT, rel)).read(), edits, occurrences, name)
        print(f"{len(rows)} rows apply")
        return 0
    tmp = None
    if not a.libs:
        tmp = tempfile.TemporaryDirectory(prefix="mut_libs_")
        a.libs = tmp.name
    out = open(a.record, "w") if a.record and a.mode != "build" else None
    for row in rows:
        if a.mode in ("build", "all"):
            rc = build_one(row, a.libs, a.log)
            print(f"build {row[0]}: exit {rc}", flush=True)
            if rc != 0:
                return rc
        if a.mode in ("run", "all"):
            rec, rc = run_one(row, a.libs, a.log)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            if rc in STOP:
                print(f"{row[0]}: exit {rc} is not a test failure: the sweep ends here; remove the row, do not retry it", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
