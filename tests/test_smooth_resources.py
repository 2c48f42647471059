"""The compiler's report on the smooth kernels (pt_smooth_kernels.hip: integrate_kernel_smooth; CPU: hipcc cross-compiles gfx950
without a GPU), read as tests/test_texture_resources.py reads the texture kernels': which kernels the unit holds -- the texture unit's
set -- no scratch memory, no spilled vector register, the twin's LDS, and every kernel's vector register count and waves per SIMD
against its twin, the texture kernel of the same arguments, with the list of those that hold a wave per SIMD fewer (DESIGN.md section
28).  The texture unit's and pt_denoise.hip's reports are checked to be what they were before the smooth unit existed."""
import os
import subprocess

import pytest

from test_glass_resources import _kernels, _report
from test_texture_resources import PINS as TEXTURE_PINS, TEXTURE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
SMOOTH = "_ZN2pt23integrate_kernel_smoothILi%dELb%dELb%dELi%dELi%dEEEvNS_10RenderArgsE"      # MISS, BIG, STATS, FORM, VIEW

# (MISS, BIG, STATS, FORM) -> (VGPRs, waves per SIMD) of VIEW 0 .. 5, from the compiler's report of `make asm-smooth`
PINS = {
    (0, 0, 0, 0): [(101, 4), (101, 4), (101, 4), (101, 4), (101, 4), (101, 4)],
    (0, 0, 1, 0): [(82, 5), (82, 5), (82, 5), (82, 5), (82, 5), (82, 5)],
    (0, 1, 0, 0): [(85, 5), (85, 5), (85, 5), (85, 5), (85, 5), (85, 5)],
    (0, 1, 1, 0): [(85, 5), (85, 5), (85, 5), (85, 5), (85, 5), (85, 5)],
    (1, 0, 0, 0): [(104, 4), (104, 4), (104, 4), (104, 4), (104, 4), (104, 4)],
    (1, 0, 1, 0): [(104, 4), (104, 4), (104, 4), (104, 4), (104, 4), (104, 4)],
    (1, 1, 0, 0): [(107, 4), (107, 4), (107, 4), (107, 4), (107, 4), (107, 4)],
    (1, 1, 1, 0): [(110, 4), (110, 4), (110, 4), (110, 4), (110, 4), (110, 4)],
    (2, 0, 0, 0): [(83, 5), (83, 5), (92, 5), (83, 5), (92, 5), (83, 5)],
    (2, 0, 1, 0): [(83, 5), (83, 5), (92, 5), (83, 5), (92, 5), (83, 5)],
    (2, 1, 0, 0): [(87, 5), (87, 5), (87, 5), (87, 5), (87, 5), (87, 5)],
    (2, 1, 1, 0): [(90, 5), (90, 5), (90, 5), (90, 5), (90, 5), (90, 5)],
    (0, 0, 0, 1): [(80, 6), (80, 6), (80, 6), (80, 6), (80, 6), (80, 6)],
    (0, 0, 0, 2): [(96, 5), (96, 5), (96, 5), (96, 5), (96, 5), (96, 5)],
    (0, 0, 0, 3): [(96, 5), (96, 5), (96, 5), (96, 5), (96, 5), (96, 5)],
    (0, 1, 0, 2): [(83, 5), (83, 5), (83, 5), (83, 5), (83, 5), (83, 5)],
    (0, 1, 0, 3): [(83, 5), (83, 5), (83, 5), (83, 5), (83, 5), (83, 5)],
}

# The kernels that hold one wave per SIMD fewer than their texture twin.  None is compiled for fewer (pt_kernels.hip:
# smooth_fewer_waves is 0 everywhere) and none spills: they need 82 or 83 registers where the twins need 80, one granule past the 80
# that six waves allow -- the wide small-scene kernel with statistics and the box-tree batch kernels, every view.
FEWER_WAVES = {(0, 0, 1, 0, v) for v in range(6)} | {(0, 1, 0, f, v) for f in (2, 3) for v in range(6)}

# pt_denoise.hip's report as it was before the smooth feature pass got a unit of its own: kernel -> (VGPRs, LDS bytes, waves per SIMD)
DENOISE_PINS = {"feature_rays_kernel": (16, 0, 8), "feature_gather_kernel": (20, 0, 8), "denoise_prepare_kernel": (40, 0, 8),
                "denoise_variance_kernel": (35, 0, 8), "denoise_atrous_kernel": (41, 0, 8), "denoise_finish_kernel": (27, 0, 8)}


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_texture_kernels.hip", "pt_smooth_kernels.hip", "pt_integrator_body.inc", "pt_environment.hpp",
                                            "pt_texture.hpp", "pt_smooth.hpp", "pt_projection.hpp", "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp",
                                            "pt_scene.hpp", "pt_denoise.hip", "Makefile")]
    newest = max(os.path.getmtime(f) for f in srcs)
    for report, target in (("smooth_resource_usage.txt", "asm-smooth"), ("texture_resource_usage.txt", "asm-texture"), ("denoise_resource_usage.txt", "asm-of-pt_denoise")):
        if not os.path.exists(os.path.join(ASM, report)) or os.path.getmtime(os.path.join(ASM, report)) < newest:
            subprocess.check_call(["make", "-C", CSRC, "-s", target])
    return tuple(_report(os.path.join(ASM, r)) for r in ("smooth_resource_usage.txt", "texture_resource_usage.txt", "denoise_resource_usage.txt"))


def test_the_unit_holds_the_texture_units_set_of_kernels(usage):
    smooth, texture, _ = usage
    want = sorted(SMOOTH % k for k in _kernels())
    assert sorted(k for k in smooth if "integrate_kernel" in k) == want and len(want) == 102
    assert not [k for k in texture if "smooth" in k]


def test_smooth_kernels_do_not_spill_and_keep_their_twins_lds(usage):
    smooth, texture, _ = usage
    for key in _kernels():
        r, twin = smooth[SMOOTH % key], texture[TEXTURE % key]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (key, r)
        assert r["LDS Size"] == twin["LDS Size"], (key, r, twin)


def test_every_kernels_registers_and_waves_are_pinned_and_the_named_ones_hold_a_wave_fewer(usage):
    smooth, texture, _ = usage
    fewer = set()
    for key in _kernels():
        r, twin = smooth[SMOOTH % key], texture[TEXTURE % key]
        assert (twin["VGPRs"], twin["Occupancy"]) == TEXTURE_PINS[key[:4]][key[4]], (key, twin)      # the texture unit's report is the parent's
        assert r["Occupancy"] in (twin["Occupancy"], twin["Occupancy"] - 1), (key, r, twin)
        assert (r["VGPRs"], r["Occupancy"]) == PINS[key[:4]][key[4]], (key, r)
        if r["Occupancy"] < twin["Occupancy"]:
            fewer.add(key)
    assert fewer == FEWER_WAVES


def test_the_denoise_units_kernels_are_untouched(usage):
    denoise = usage[2]
    for name, pin in DENOISE_PINS.items():
        ks = [k for k in denoise if name in k]
        assert len(ks) == 1 and denoise[ks[0]]["ScratchSize"] == 0 and denoise[ks[0]]["VGPRs Spill"] == 0, (name, ks)
        assert (denoise[ks[0]]["VGPRs"], denoise[ks[0]]["LDS Size"], denoise[ks[0]]["Occupancy"]) == pin, (name, denoise[ks[0]])
    assert len(denoise) == len(DENOISE_PINS) and not [k for k in denoise if "smooth" in k]
