"""The compiler's report on the roulette kernels (pt_roulette_kernels.hip: integrate_kernel_roulette; CPU: hipcc cross-compiles gfx950
without a GPU), read as tests/test_direct_resources.py reads the direct kernels': which kernels the unit holds -- the direct unit's set
of 102 and the environment-sampling unit's 24, the latter with ENVD --, no scratch memory, no spilled vector register, and every
kernel's vector register count, LDS and waves per SIMD, pinned as found and held against the budget of those waves: 512 vector
registers per SIMD lane in granules of 8, 160 KiB of LDS per compute unit in granules of 1 280 bytes, one wave per workgroup.  Every
kernel is compiled for its twin's 4 waves per SIMD but three (pt_kernels.hip: roulette_fewer_waves)."""
import os
import subprocess

import pytest

from test_glass_resources import _kernels, _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
ROULETTE = "_ZN2pt25integrate_kernel_rouletteILi%dELb%dELb%dELi%dELi%dELb%dEEEvNS_10RenderArgsE"      # MISS, BIG, STATS, FORM, VIEW, ENVD
KERNELS = [k + (0,) for k in _kernels()] + [(2, b, s, 0, v, 1) for b in (0, 1) for s in (0, 1) for v in range(6)]
THREE_WAVES = {(0, 0, 0, 0, v, 0) for v in (2, 3, 4)}      # the two-pixel small-scene kernel under the lens, the moving camera and the moving lens

# (MISS, BIG, STATS, FORM, ENVD) -> (VGPRs of VIEW 0 .. 5, LDS bytes per block), from the compiler's report of `make asm-roulette`
PINS = {
    (0, 0, 0, 0, 0): ([128, 128, 129, 129, 129, 128], 6864),
    (0, 0, 1, 0, 0): ([100, 101, 101, 101, 101, 101], 5840),
    (0, 1, 0, 0, 0): ([104, 104, 104, 104, 104, 104], 6216),
    (0, 1, 1, 0, 0): ([106, 106, 106, 106, 106, 106], 6216),
    (1, 0, 0, 0, 0): ([126, 127, 127, 127, 127, 127], 5840),
    (1, 0, 1, 0, 0): ([126, 123, 123, 123, 123, 123], 5840),
    (1, 1, 0, 0, 0): ([124, 126, 126, 126, 126, 126], 6216),
    (1, 1, 1, 0, 0): ([126, 128, 128, 128, 128, 128], 6216),
    (2, 0, 0, 0, 0): ([100, 101, 101, 101, 101, 101], 5840),
    (2, 0, 1, 0, 0): ([100, 101, 101, 101, 102, 101], 5840),
    (2, 1, 0, 0, 0): ([104, 104, 104, 104, 104, 104], 6216),
    (2, 1, 1, 0, 0): ([106, 106, 106, 106, 107, 107], 6216),
    (0, 0, 0, 1, 0): ([100, 101, 101, 101, 101, 101], 5840),
    (0, 0, 0, 2, 0): ([128, 128, 128, 128, 128, 128], 7120),
    (0, 0, 0, 3, 0): ([124, 125, 125, 125, 125, 125], 7376),
    (0, 1, 0, 2, 0): ([100, 100, 100, 100, 100, 100], 6400),
    (0, 1, 0, 3, 0): ([100, 100, 100, 100, 100, 100], 6400),
    (2, 0, 0, 0, 1): ([100, 101, 101, 101, 101, 101], 5840),
    (2, 0, 1, 0, 1): ([100, 101, 101, 102, 102, 102], 5840),
    (2, 1, 0, 0, 1): ([104, 104, 104, 104, 104, 104], 6216),
    (2, 1, 1, 0, 1): ([106, 106, 106, 107, 107, 107], 6216),
}


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_roulette_kernels.hip", "pt_integrator_body.inc", "pt_sphere_tree_walk.inc", "pt_environment.hpp",
                                            "pt_texture.hpp", "pt_smooth.hpp", "pt_rough.hpp", "pt_direct.hpp", "pt_envdirect.hpp", "pt_roulette.hpp", "pt_grade.hpp",
                                            "pt_projection.hpp", "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    newest = max(os.path.getmtime(f) for f in srcs)
    report = os.path.join(ASM, "roulette_resource_usage.txt")
    if not os.path.exists(report) or os.path.getmtime(report) < newest:
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-roulette"])
    return _report(report)


def test_the_unit_holds_the_direct_units_102_kernels_and_the_24_environment_sampling_kernels(usage):
    want = sorted(ROULETTE % k for k in KERNELS)
    assert sorted(k for k in usage if "integrate_kernel" in k) == want and len(want) == 126 == len(set(want))


def test_no_kernel_has_scratch_or_a_spilled_vector_register(usage):
    for key in KERNELS:
        r = usage[ROULETTE % key]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (key, r)


def test_every_kernels_registers_lds_and_waves_are_pinned_and_within_the_budget_of_its_waves(usage):
    for key in KERNELS:
        r = usage[ROULETTE % key]
        waves = 3 if key in THREE_WAVES else 4
        vgprs, lds = PINS[key[:4] + key[5:]]
        assert (r["VGPRs"], r["LDS Size"], r["Occupancy"]) == (vgprs[key[4]], lds, waves), (key, r)
        assert (r["VGPRs"] + 7) // 8 * 8 <= 512 // waves // 8 * 8, (key, r)
        assert (r["LDS Size"] + 1279) // 1280 * 1280 * 4 * waves <= 160 * 1024, (key, r)
