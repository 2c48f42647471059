"""The compiler's report on the environment-sampling kernels (pt_envdirect_kernels.hip: integrate_kernel_envdirect; CPU: hipcc
cross-compiles gfx950 without a GPU), read as tests/test_direct_resources.py reads the direct kernels': which kernels the unit holds --
the 24 environment instantiations of the wide form: 6 views x box tree x statistics --, no scratch memory, no spilled vector register,
the direct twin's LDS, and every kernel's vector register count and waves per SIMD, pinned as found: every kernel holds the direct
twin's 4 waves per SIMD (pt_kernels.hip: envdirect_fewer_waves is 0 everywhere).  The direct unit's report is
checked to be what it was before this unit existed."""
import os
import subprocess

import pytest

from test_direct_resources import DIRECT, PINS as DIRECT_PINS
from test_glass_resources import _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
ENVDIRECT = "_ZN2pt26integrate_kernel_envdirectILi%dELb%dELb%dELi%dELi%dEEEvNS_10RenderArgsE"      # MISS, BIG, STATS, FORM, VIEW
KERNELS = [(2, b, s, 0, v) for b in (0, 1) for s in (0, 1) for v in range(6)]

# (MISS, BIG, STATS, FORM) -> VGPRs of VIEW 0 .. 5, from the compiler's report of `make asm-envdirect`; waves per SIMD: 4 everywhere
PINS = {
    (2, 0, 0, 0): [100, 102, 102, 102, 102, 102],
    (2, 0, 1, 0): [100, 102, 102, 102, 103, 103],
    (2, 1, 0, 0): [104, 104, 104, 104, 104, 104],
    (2, 1, 1, 0): [106, 106, 106, 106, 107, 107],
}
LDS = {0: 5840, 1: 6216}      # bytes per block, by BIG


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_direct_kernels.hip", "pt_envdirect_kernels.hip", "pt_integrator_body.inc", "pt_environment.hpp",
                                            "pt_texture.hpp", "pt_smooth.hpp", "pt_rough.hpp", "pt_direct.hpp", "pt_envdirect.hpp", "pt_grade.hpp",
                                            "pt_projection.hpp", "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    newest = max(os.path.getmtime(f) for f in srcs)
    for report, target in (("envdirect_resource_usage.txt", "asm-envdirect"), ("direct_resource_usage.txt", "asm-direct")):
        if not os.path.exists(os.path.join(ASM, report)) or os.path.getmtime(os.path.join(ASM, report)) < newest:
            subprocess.check_call(["make", "-C", CSRC, "-s", target])
    return tuple(_report(os.path.join(ASM, r)) for r in ("envdirect_resource_usage.txt", "direct_resource_usage.txt"))


def test_the_unit_holds_exactly_the_24_environment_kernels(usage):
    mine, direct = usage
    want = sorted(ENVDIRECT % k for k in KERNELS)
    assert sorted(k for k in mine if "integrate_kernel" in k) == want and len(want) == 24
    assert not [k for k in direct if "envdirect" in k]


def test_no_kernel_has_scratch_or_a_spilled_vector_register_and_each_keeps_its_twins_lds(usage):
    mine, direct = usage
    for key in KERNELS:
        r, twin = mine[ENVDIRECT % key], direct[DIRECT % key]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (key, r)
        assert r["LDS Size"] == twin["LDS Size"] == LDS[key[1]], (key, r, twin)


def test_every_kernels_registers_are_pinned_at_four_waves_and_the_direct_units_report_is_unchanged(usage):
    mine, direct = usage
    for key in KERNELS:
        r, twin = mine[ENVDIRECT % key], direct[DIRECT % key]
        assert (twin["VGPRs"], twin["Occupancy"]) == (DIRECT_PINS[key[:4]][key[4]], 4), (key, twin)      # the direct unit's report is the parent's
        assert (r["VGPRs"], r["Occupancy"]) == (PINS[key[:4]][key[4]], 4), (key, r)
