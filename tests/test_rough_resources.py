"""The compiler's report on the rough kernels (pt_rough_kernels.hip: integrate_kernel_rough; CPU: hipcc cross-compiles gfx950 without a
GPU), read as tests/test_smooth_resources.py reads the smooth kernels': which kernels the unit holds -- the smooth unit's set of 102 --
no scratch memory, no spilled vector register, the twin's LDS, and every kernel's vector register count and waves per SIMD against its
twin, the smooth kernel of the same arguments, with the list of those that hold a wave per SIMD fewer.  The
smooth unit's report is checked to be what it was before the rough unit existed."""
import os
import subprocess

import pytest

from test_glass_resources import _kernels, _report
from test_smooth_resources import PINS as SMOOTH_PINS, SMOOTH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
ROUGH = "_ZN2pt22integrate_kernel_roughILi%dELb%dELb%dELi%dELi%dEEEvNS_10RenderArgsE"      # MISS, BIG, STATS, FORM, VIEW

# (MISS, BIG, STATS, FORM) -> (VGPRs, waves per SIMD) of VIEW 0 .. 5, from the compiler's report of `make asm-rough`
PINS = {
    (0, 0, 0, 0): [(103, 4), (103, 4), (103, 4), (103, 4), (103, 4), (103, 4)],
    (0, 0, 1, 0): [(84, 5), (84, 5), (84, 5), (84, 5), (85, 5), (84, 5)],
    (0, 1, 0, 0): [(88, 5), (88, 5), (88, 5), (88, 5), (88, 5), (88, 5)],
    (0, 1, 1, 0): [(89, 5), (88, 5), (89, 5), (89, 5), (89, 5), (89, 5)],
    (1, 0, 0, 0): [(107, 4), (107, 4), (107, 4), (107, 4), (107, 4), (107, 4)],
    (1, 0, 1, 0): [(107, 4), (107, 4), (107, 4), (107, 4), (108, 4), (107, 4)],
    (1, 1, 0, 0): [(112, 4), (112, 4), (112, 4), (112, 4), (112, 4), (112, 4)],
    (1, 1, 1, 0): [(114, 4), (114, 4), (114, 4), (114, 4), (115, 4), (115, 4)],
    (2, 0, 0, 0): [(86, 5), (86, 5), (92, 5), (86, 5), (92, 5), (86, 5)],
    (2, 0, 1, 0): [(86, 5), (86, 5), (92, 5), (86, 5), (92, 5), (86, 5)],
    (2, 1, 0, 0): [(91, 5), (91, 5), (90, 5), (91, 5), (90, 5), (91, 5)],
    (2, 1, 1, 0): [(92, 5), (92, 5), (92, 5), (92, 5), (93, 5), (92, 5)],
    (0, 0, 0, 1): [(80, 6), (80, 6), (80, 6), (80, 6), (80, 6), (80, 6)],
    (0, 0, 0, 2): [(104, 4), (96, 5), (96, 5), (96, 5), (105, 4), (105, 4)],
    (0, 0, 0, 3): [(96, 5), (96, 5), (96, 5), (96, 5), (96, 5), (96, 5)],
    (0, 1, 0, 2): [(86, 5), (86, 5), (86, 5), (86, 5), (86, 5), (86, 5)],
    (0, 1, 0, 3): [(86, 5), (86, 5), (86, 5), (86, 5), (86, 5), (86, 5)],
}

# The kernels that hold one wave per SIMD fewer than their smooth twin: at the twin's 5 waves and 96 VGPRs they spilled 27 vector
# registers, so they are compiled for 4 (pt_kernels.hip: rough_fewer_waves) -- the small-scene batch kernel over 16 x 8 tiles with a fixed
# eye, with the moving lens and under a projection.
FEWER_WAVES = {(0, 0, 0, 2, 0), (0, 0, 0, 2, 4), (0, 0, 0, 2, 5)}


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_smooth_kernels.hip", "pt_rough_kernels.hip", "pt_integrator_body.inc", "pt_environment.hpp",
                                            "pt_texture.hpp", "pt_smooth.hpp", "pt_rough.hpp", "pt_grade.hpp", "pt_projection.hpp", "pt_kernels.hpp",
                                            "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    newest = max(os.path.getmtime(f) for f in srcs)
    for report, target in (("rough_resource_usage.txt", "asm-rough"), ("smooth_resource_usage.txt", "asm-smooth")):
        if not os.path.exists(os.path.join(ASM, report)) or os.path.getmtime(os.path.join(ASM, report)) < newest:
            subprocess.check_call(["make", "-C", CSRC, "-s", target])
    return tuple(_report(os.path.join(ASM, r)) for r in ("rough_resource_usage.txt", "smooth_resource_usage.txt"))


def test_the_unit_holds_the_smooth_units_set_of_kernels(usage):
    rough, smooth = usage
    want = sorted(ROUGH % k for k in _kernels())
    assert sorted(k for k in rough if "integrate_kernel" in k) == want and len(want) == 102
    assert not [k for k in smooth if "rough" in k]


def test_rough_kernels_do_not_spill_and_keep_their_twins_lds(usage):
    rough, smooth = usage
    for key in _kernels():
        r, twin = rough[ROUGH % key], smooth[SMOOTH % key]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (key, r)
        assert r["LDS Size"] == twin["LDS Size"], (key, r, twin)


def test_every_kernels_registers_and_waves_are_pinned_and_the_named_ones_hold_a_wave_fewer(usage):
    rough, smooth = usage
    fewer = set()
    for key in _kernels():
        r, twin = rough[ROUGH % key], smooth[SMOOTH % key]
        assert (twin["VGPRs"], twin["Occupancy"]) == SMOOTH_PINS[key[:4]][key[4]], (key, twin)      # the smooth unit's report is the parent's
        assert r["Occupancy"] in (twin["Occupancy"], twin["Occupancy"] - 1), (key, r, twin)
        assert (r["VGPRs"], r["Occupancy"]) == PINS[key[:4]][key[4]], (key, r)
        if r["Occupancy"] < twin["Occupancy"]:
            fewer.add(key)
    assert fewer == FEWER_WAVES
