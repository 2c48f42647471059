"""The launch plan (path-tracing_amd/csrc/pt_launch_plan.hpp: kernel variant, tiles, pass chunks) on the CPU: pure host
arithmetic, built with g++ and compared case for case with tests/golden/launch_plans.npz.  The fixture was recorded from the
commit BEFORE the planner became a module of its own -- that commit's compiled library (its integrator_plan_tiles, the
kernel its dispatch ladder handed to the occupancy query, the chunk block of its enqueue_render) -- so it pins the plan that
every tuning log in DESIGN.md section 4 was measured with."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _driver(tmp_path, *defs):
    exe = str(tmp_path / ("launch_plan" + "".join(defs).replace("-D", "_").replace("=", "")))
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *defs, "-I", CSRC,
                            os.path.join(ROOT, "tests", "native", "launch_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0 and not build.stderr, build.stderr[-3000:]
    return exe


def _run(exe, text=None, *args):
    run = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    return np.array([[int(x) for x in line.split()] for line in run.stdout.splitlines()], dtype=np.int64)


def test_plans_are_the_recorded_ones(tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "launch_plans.npz"))
    inp = dict(zip(g["input_columns"].tolist(), g["inputs"].T.tolist()))
    exp = dict(zip(g["expected_columns"].tolist(), g["expected"].T))
    n = len(g["error"])
    assert n >= 3000
    # the grid the fixture must hold
    shapes = set(zip(inp["width"], inp["height"], inp["row_begin"], inp["row_end"], inp["row_stride"]))
    assert {(1920, 1080, 0, 1080, 1), (3840, 2160, 0, 2160, 1), (1366, 768, 0, 768, 1), (1280, 720, 0, 720, 1), (960, 540, 0, 540, 1),
            (256, 256, 0, 256, 1)} <= shapes
    assert {(3840, 2160, 270 * k, 270 * (k + 1), 1) for k in range(8)} <= shapes      # the eight bands of the 3840 x 2160 frame: 8 160 wide tiles each
    assert all(0 <= s[2] < s[3] <= s[1] for s in shapes)
    assert {s[4] for s in shapes if s[:2] == (1920, 1080)} >= {1, 2, 4, 8}
    for error in (-1.0, 0.001):
        sel = g["error"] == np.float32(error)
        assert len({tuple(r) for r in g["inputs"][sel][:, 5:9].tolist()}) == 16      # sky / big / statistics / envelope in every combination
    assert set(inp["pass_count"]) >= {1, 12, 16, 64, 256, 1024} and max(b + c for b, c in zip(inp["pass_begin"], inp["pass_count"])) > 32766
    assert 256 in inp["cu_count"] and min(inp["cu_count"]) < 256 and set(inp["waves_per_cu"]) >= {16, 18, 20, 24}
    assert set(inp["view"]) == {0, 1, 2} and set(inp["tile_width"]) == {0, 1, 2, 3}
    assert set(inp["items_per_slot"]) >= {-1, 0, 16} and set(inp["chunk_min"]) >= {0, 8}
    text = "".join(
        f"{inp['width'][i]} {exp['band_rows'][i]} {inp['sky'][i]} {inp['big'][i]} {inp['stats'][i]} {inp['env'][i]} {float(g['error'][i])!r} "
        f"{inp['pass_begin'][i]} {inp['pass_count'][i]} {inp['cu_count'][i]} {inp['waves_per_cu'][i]} {inp['view'][i]} {inp['tile_width'][i]} "
        f"{inp['items_per_slot'][i]} {inp['chunk_min'][i]}\n" for i in range(n))
    got = _run(_driver(tmp_path), text)
    assert got.shape == (n, 14)
    want = g["expected"][:, 1:]      # (band_rows is an input here)
    bad = np.flatnonzero((got[:, 1:] != want).any(axis=1))
    assert bad.size == 0, [(g["inputs"][i].tolist(), float(g["error"][i]), got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    # every kernel of the product is reached, and a kernel has one id
    kernels = {tuple(r) for r in got[:, 1:8].tolist()}
    assert len(kernels) == 66
    assert len({(r[0],) + tuple(r[1:8]) for r in got.tolist()}) == 66


def test_drivers_plan_with_the_kernels_build_constants():
    """The planner's build constants are -D defaults of the kernels' translation unit; the native drivers, which cannot include
    it, spell them out: they must be the defaults the sources hold."""
    import re
    hip = open(os.path.join(CSRC, "pt_kernels.hip")).read()
    scene = open(os.path.join(CSRC, "pt_scene.hpp")).read()
    define = lambda src, name: int(re.search(r"#ifndef %s\n#define %s (\d+)" % (name, name), src).group(1))
    tile_w = define(scene, "PT_TILE_W")
    small, big, waves = (define(hip, n) for n in ("PT_RAYS_PER_LANE", "PT_BIG_RAYS_PER_LANE", "PT_WAVES_PER_SIMD"))
    max_pass = int(re.search(r"constexpr int kMaxBatchPass = (\d+);", hip).group(1))
    native = os.path.join(ROOT, "tests", "native")
    main = open(os.path.join(native, "launch_plan_main.cpp")).read()
    assert "#define PT_BIG_RAYS_PER_LANE %d\n" % big in main
    assert "kBuild = {%d, %d, %d, PT_BIG_RAYS_PER_LANE, %d, %d, Stats::kAsAsked, false}" % (tile_w, 64 // tile_w, small, waves, max_pass) in main
    for name in ("capi_asan_main.cpp", "resolve_tsan_main.cpp"):
        assert "b = {%d, %d, %d, %d, %d, %d, plan::Stats::kAsAsked, false}" % (tile_w, 64 // tile_w, small, big, waves, max_pass) in open(os.path.join(native, name)).read()


def _variants(tmp_path, *defs):
    v = _run(_driver(tmp_path, *defs), None, "variants")
    assert v.shape == (72, 10) and v[:, 0].tolist() == list(range(72))      # dense: the occupancy cache is indexed by id
    assert v[:, 2].all()                                                     # variant_of and variant_id are inverses
    assert len({tuple(r) for r in v[v[:, 1] == 1][:, 3:].tolist()}) == int(v[:, 1].sum())      # one kernel per id
    return v


def test_ids_round_trip_and_the_product_has_66_kernels(tmp_path):
    v = _variants(tmp_path)
    assert int(v[:, 1].sum()) == 66
    exists = v[v[:, 1] == 1]
    # columns 3..9: SKY BIG STATS ENV NARROW ADAPT lens
    assert not ((exists[:, 7] == 1) & (exists[:, 4] == 1)).any()                 # no 8 x 8 box-tree kernel with one ray slot per lane
    assert not ((exists[:, 8] >= 2) & (exists[:, 6] == 1)).any()                 # no batch kernel with the envelope test
    assert ((exists[:, 8] & 1) == 1).sum() == 44 and (exists[:, 9] == 1).sum() == 22      # 22 camera-free, 22 twins, 22 lens kernels


def test_two_pixels_per_lane_box_tree_build_has_its_narrow_variants(tmp_path):
    v = _variants(tmp_path, "-DPT_BIG_RAYS_PER_LANE=2")
    assert int(v[:, 1].sum()) == 72
    exe = _driver(tmp_path, "-DPT_BIG_RAYS_PER_LANE=2")
    # a 256 x 256 box-tree launch has too few 16 x 8 tiles for 256 CUs: the 8 x 8 kernel; 1080p: the wide one
    for env in (0, 1):
        for view in (0, 1, 2):
            small, full = _run(exe, f"256 256 0 1 0 {env} -1.0 0 16 256 20 {view} 0 0 0\n1920 1080 0 1 0 {env} -1.0 0 16 256 20 {view} 0 0 0\n").tolist()
            assert small[1:8] == [0, 1, 0, env, 1, int(view != 0), int(view == 2)] and small[8:12] == [1, 0, 32, 1024]
            assert full[1:8] == [0, 1, 0, env, 0, int(view != 0), int(view == 2)] and full[8:12] == [0, 0, 120, 16200]
