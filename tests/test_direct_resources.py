"""The compiler's report on the direct kernels (pt_direct_kernels.hip: integrate_kernel_direct; CPU: hipcc cross-compiles gfx950 without
a GPU), read as tests/test_rough_resources.py reads the rough kernels': which kernels the unit holds -- the rough unit's set of 102 --
no scratch memory, no spilled vector register, the twin's LDS, and every kernel's vector register count and waves per SIMD, pinned as
found: every direct kernel is compiled for 4 waves per SIMD (pt_kernels.hip: direct_fewer_waves).  The rough unit's
report is checked to be what it was before the direct unit existed."""
import os
import subprocess

import pytest

from test_glass_resources import _kernels, _report
from test_rough_resources import PINS as ROUGH_PINS, ROUGH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
DIRECT = "_ZN2pt23integrate_kernel_directILi%dELb%dELb%dELi%dELi%dEEEvNS_10RenderArgsE"      # MISS, BIG, STATS, FORM, VIEW

# (MISS, BIG, STATS, FORM) -> VGPRs of VIEW 0 .. 5, from the compiler's report of `make asm-direct`; waves per SIMD: 4 everywhere
PINS = {
    (0, 0, 0, 0): [128, 128, 128, 128, 128, 128],
    (0, 0, 1, 0): [98, 98, 99, 99, 99, 99],
    (0, 1, 0, 0): [102, 102, 102, 102, 103, 102],
    (0, 1, 1, 0): [105, 105, 105, 105, 105, 105],
    (1, 0, 0, 0): [122, 122, 122, 122, 122, 122],
    (1, 0, 1, 0): [122, 122, 122, 122, 123, 123],
    (1, 1, 0, 0): [124, 124, 124, 124, 124, 124],
    (1, 1, 1, 0): [126, 126, 127, 127, 127, 127],
    (2, 0, 0, 0): [100, 102, 102, 102, 102, 102],
    (2, 0, 1, 0): [100, 102, 102, 102, 102, 102],
    (2, 1, 0, 0): [104, 104, 104, 104, 104, 104],
    (2, 1, 1, 0): [106, 106, 106, 106, 107, 107],
    (0, 0, 0, 1): [98, 99, 99, 99, 99, 99],
    (0, 0, 0, 2): [128, 128, 128, 128, 128, 128],
    (0, 0, 0, 3): [127, 127, 127, 127, 127, 127],
    (0, 1, 0, 2): [100, 100, 100, 100, 100, 100],
    (0, 1, 0, 3): [100, 100, 100, 100, 100, 100],
}


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_rough_kernels.hip", "pt_direct_kernels.hip", "pt_integrator_body.inc", "pt_environment.hpp",
                                            "pt_texture.hpp", "pt_smooth.hpp", "pt_rough.hpp", "pt_direct.hpp", "pt_grade.hpp", "pt_projection.hpp",
                                            "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    newest = max(os.path.getmtime(f) for f in srcs)
    for report, target in (("direct_resource_usage.txt", "asm-direct"), ("rough_resource_usage.txt", "asm-rough")):
        if not os.path.exists(os.path.join(ASM, report)) or os.path.getmtime(os.path.join(ASM, report)) < newest:
            subprocess.check_call(["make", "-C", CSRC, "-s", target])
    return tuple(_report(os.path.join(ASM, r)) for r in ("direct_resource_usage.txt", "rough_resource_usage.txt"))


def test_the_unit_holds_the_rough_units_set_of_kernels(usage):
    direct, rough = usage
    want = sorted(DIRECT % k for k in _kernels())
    assert sorted(k for k in direct if "integrate_kernel" in k) == want and len(want) == 102
    assert not [k for k in rough if "direct" in k]


def test_direct_kernels_do_not_spill_and_keep_their_twins_lds(usage):
    direct, rough = usage
    for key in _kernels():
        r, twin = direct[DIRECT % key], rough[ROUGH % key]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (key, r)
        assert r["LDS Size"] == twin["LDS Size"], (key, r, twin)


def test_every_kernels_registers_are_pinned_at_four_waves_and_the_rough_units_report_is_unchanged(usage):
    direct, rough = usage
    for key in _kernels():
        r, twin = direct[DIRECT % key], rough[ROUGH % key]
        assert (twin["VGPRs"], twin["Occupancy"]) == ROUGH_PINS[key[:4]][key[4]], (key, twin)      # the rough unit's report is the parent's
        assert (r["VGPRs"], r["Occupancy"]) == (PINS[key[:4]][key[4]], 4), (key, r)
