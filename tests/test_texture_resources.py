"""The compiler's report on the texture kernels (pt_texture_kernels.hip: integrate_kernel_texture; CPU: hipcc cross-compiles gfx950
without a GPU), read as tests/test_glass_resources.py reads the dielectric kernels': which kernels the unit holds -- the dielectric
unit's set -- no scratch memory, no spilled vector register, the twin's LDS (texels, coordinates and the per-material table are read
from memory), and every kernel's vector register count and waves per SIMD against its twin, the dielectric kernel of the same
arguments, with the list of those that hold a wave per SIMD fewer."""
import os
import subprocess

import pytest

from test_glass_resources import GLASS, _kernels, _pin, _report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
TEXTURE = "_ZN2pt24integrate_kernel_textureILi%dELb%dELb%dELi%dELi%dEEEvNS_10RenderArgsE"      # MISS, BIG, STATS, FORM, VIEW

# (MISS, BIG, STATS, FORM) -> (VGPRs, waves per SIMD) of VIEW 0 .. 5, from the compiler's report of `make asm-texture`
PINS = {
    (0, 0, 0, 0): [(99, 4), (100, 4), (100, 4), (100, 4), (100, 4), (100, 4)],
    (0, 0, 1, 0): [(80, 6), (80, 6), (80, 6), (80, 6), (80, 6), (80, 6)],
    (0, 1, 0, 0): [(82, 5), (82, 5), (82, 5), (82, 5), (82, 5), (82, 5)],
    (0, 1, 1, 0): [(82, 5), (82, 5), (82, 5), (82, 5), (82, 5), (82, 5)],
    (1, 0, 0, 0): [(103, 4), (103, 4), (103, 4), (103, 4), (103, 4), (103, 4)],
    (1, 0, 1, 0): [(103, 4), (103, 4), (103, 4), (103, 4), (103, 4), (103, 4)],
    (1, 1, 0, 0): [(104, 4), (104, 4), (104, 4), (104, 4), (104, 4), (104, 4)],
    (1, 1, 1, 0): [(109, 4), (109, 4), (109, 4), (109, 4), (109, 4), (109, 4)],
    (2, 0, 0, 0): [(91, 5), (82, 5), (91, 5), (82, 5), (91, 5), (82, 5)],
    (2, 0, 1, 0): [(82, 5), (82, 5), (91, 5), (82, 5), (91, 5), (82, 5)],
    (2, 1, 0, 0): [(83, 5), (85, 5), (83, 5), (85, 5), (83, 5), (85, 5)],
    (2, 1, 1, 0): [(88, 5), (88, 5), (88, 5), (88, 5), (88, 5), (88, 5)],
    (0, 0, 0, 1): [(80, 6), (80, 6), (80, 6), (80, 6), (80, 6), (80, 6)],
    (0, 0, 0, 2): [(96, 5), (96, 5), (96, 5), (96, 5), (96, 5), (96, 5)],
    (0, 0, 0, 3): [(96, 5), (96, 5), (96, 5), (96, 5), (96, 5), (96, 5)],
    (0, 1, 0, 2): [(80, 6), (80, 6), (80, 6), (80, 6), (80, 6), (80, 6)],
    (0, 1, 0, 3): [(80, 6), (80, 6), (80, 6), (80, 6), (80, 6), (80, 6)],
}

# The kernels that hold one wave per SIMD fewer than their twin.  Two are compiled for it (pt_kernels.hip: texture_fewer_waves): at the
# twin's 5 waves and 96 registers the two-pixel small-scene kernel without a miss shader, fixed eye and camera twin, spilled 1 and 2
# vector registers; they have 99 and 100 registers at 4 waves.  The 12 wide box-tree kernels without a miss shader (with and without
# statistics, every view) are compiled for their twins' bound and do not spill, but need 82 registers where the twins need 80 -- one
# granule past the 80 that six waves allow -- so a SIMD holds five of them.
FEWER_WAVES = {(0, 0, 0, 0, 0), (0, 0, 0, 0, 1)} | {(0, 1, s, 0, v) for s in (0, 1) for v in range(6)}


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_glass_kernels.hip", "pt_texture_kernels.hip", "pt_integrator_body.inc", "pt_environment.hpp",
                                            "pt_texture.hpp", "pt_projection.hpp", "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    newest = max(os.path.getmtime(f) for f in srcs)
    for report, target in (("texture_resource_usage.txt", "asm-texture"), ("glass_resource_usage.txt", "asm-glass")):
        if not os.path.exists(os.path.join(ASM, report)) or os.path.getmtime(os.path.join(ASM, report)) < newest:
            subprocess.check_call(["make", "-C", CSRC, "-s", target])
    return tuple(_report(os.path.join(ASM, r)) for r in ("texture_resource_usage.txt", "glass_resource_usage.txt"))


def test_the_unit_holds_the_dielectric_units_set_of_kernels(usage):
    texture, glass = usage
    want = sorted(TEXTURE % k for k in _kernels())
    assert sorted(k for k in texture if "integrate_kernel" in k) == want and len(want) == 102
    assert not [k for k in glass if "texture" in k]


def test_texture_kernels_do_not_spill_and_keep_their_twins_lds(usage):
    texture, glass = usage
    for key in _kernels():
        r, twin = texture[TEXTURE % key], glass[GLASS % key]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (key, r)
        assert r["LDS Size"] == twin["LDS Size"], (key, r, twin)


def test_every_kernels_registers_and_waves_are_pinned_and_the_named_ones_hold_a_wave_fewer(usage):
    texture, glass = usage
    fewer = set()
    for key in _kernels():
        r, twin = texture[TEXTURE % key], glass[GLASS % key]
        assert twin["Occupancy"] == _pin(*key)[1]           # (the twin is the kernel tests/test_glass_resources.py pins)
        assert r["Occupancy"] in (twin["Occupancy"], twin["Occupancy"] - 1), (key, r, twin)
        assert (r["VGPRs"], r["Occupancy"]) == PINS[key[:4]][key[4]], (key, r)
        if r["Occupancy"] < twin["Occupancy"]:
            fewer.add(key)
    assert fewer == FEWER_WAVES
