"""The compiler's report on the dielectric kernels (pt_glass_kernels.hip: integrate_kernel_glass; CPU: hipcc cross-compiles gfx950
without a GPU), read as tests/test_environment_resources.py reads the environment kernels': which kernels the unit holds, no scratch
memory, no spilled vector register, the twin's LDS (the per-material table is read from memory), and every kernel's exact vector
register count and occupancy -- with the list of those that hold a wave per SIMD fewer than their twin."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
GLASS = "_ZN2pt22integrate_kernel_glassILi%dELb%dELb%dELi%dELi%dEEEvNS_10RenderArgsE"        # MISS, BIG, STATS, FORM, VIEW
ENVIRONMENT = "_ZN2pt28integrate_kernel_environmentILb%dELb%dELb1ELi%dEEEvNS_10RenderArgsE"    # BIG, STATS, (the envelope test), VIEW
# the twin of view 0 .. 5 without a miss shader or under a skybox: the kernel's mangled name and its camera bit
TWINS = {0: ("16integrate_kernel", 0), 1: ("16integrate_kernel", 1), 2: ("21integrate_kernel_lens", 1), 3: ("23integrate_kernel_motion", 1),
         4: ("28integrate_kernel_motion_lens", 1), 5: ("27integrate_kernel_projection", 1)}
VIEWS = range(6)


def _kernels():
    """(MISS, BIG, STATS, FORM, VIEW) of every kernel of the unit: the wide form of every miss shader, box-tree switch and statistics
    switch; without a miss shader and statistics also the 8 x 8 form of the small-scene kernel and the batch kernels over 16 x 8 and
    32 x 8 tiles of both."""
    wide = [(m, b, s, 0) for m in range(3) for b in (0, 1) for s in (0, 1)]
    forms = [(0, 0, 0, 1)] + [(0, b, 0, f) for b in (0, 1) for f in (2, 3)]
    return [k + (v,) for k in wide + forms for v in VIEWS]


def _pin(miss, big, stats, form, view):
    """(VGPRs, occupancy) of that kernel."""
    if miss == 1:                                      # skybox: the lookup's doubles meet the dielectric's operands
        return (109, 4) if big and stats else (103, 4)
    if miss == 2:                                      # environment
        if big:
            return (88, 5) if stats else (82, 5)
        return (91, 5) if view in ((2, 4) if stats else (0, 1, 2, 4)) else (82, 5)
    if big:
        return (77, 6) if form >= 2 else (80, 6)
    if stats or form == 1:
        return (80, 6)
    if form >= 2:
        return (96, 5)
    return (96, 5) if view in (0, 1) else (100, 4)     # the two-pixel small-scene kernel


# The kernels compiled for one wave per SIMD fewer than their twin (pt_kernels.hip: glass_fewer_waves), which at the twin's 5 waves and
# 96 registers spilled 1 (the two-pixel kernel's lens, motion and projection forms) or 6 (the skybox kernels) vector registers.
FEWER_WAVES = {(0, 0, 0, 0, v) for v in (2, 3, 5)} | {(1, b, s, 0, v) for (b, s) in ((0, 0), (0, 1), (1, 0)) for v in (0, 1, 3, 5)}


def _report(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_glass_kernels.hip", "pt_environment_kernels.hip", "pt_integrator_body.inc", "pt_environment.hpp",
                                            "pt_projection.hpp", "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    newest = max(os.path.getmtime(f) for f in srcs)
    for report, target in (("glass_resource_usage.txt", "asm-glass"), ("environment_resource_usage.txt", "asm-environment"), ("resource_usage.txt", "asm-of-pt_kernels")):
        if not os.path.exists(os.path.join(ASM, report)) or os.path.getmtime(os.path.join(ASM, report)) < newest:
            subprocess.check_call(["make", "-C", CSRC, "-s", target])
    return tuple(_report(os.path.join(ASM, r)) for r in ("glass_resource_usage.txt", "resource_usage.txt", "environment_resource_usage.txt"))


def _twin(key, twins, env):
    miss, big, stats, form, view = key
    if miss == 2:
        return env[ENVIRONMENT % (big, stats, view)]
    name, cam = TWINS[view]
    pool = {2: 2, 3: 4}.get(form, 0)
    return twins["_ZN2pt%sILb%dELb%dELb%dELb%dELb%dELi%dEEEvNS_10RenderArgsE" % (name, miss, big, stats, form < 2, form == 1, pool | cam)]


def test_the_unit_holds_the_dielectric_kernels_and_no_other_unit_does(usage):
    glass, twins, env = usage
    want = sorted(GLASS % k for k in _kernels())
    assert sorted(k for k in glass if "integrate_kernel" in k) == want and len(want) == 102
    assert not [k for k in list(twins) + list(env) if "glass" in k]


def test_dielectric_kernels_do_not_spill_and_keep_their_twins_lds(usage):
    glass, twins, env = usage
    for key in _kernels():
        r, base = glass[GLASS % key], _twin(key, twins, env)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (key, r)
        assert r["LDS Size"] == base["LDS Size"], (key, r, base)


def test_every_kernels_registers_and_occupancy_are_pinned(usage):
    glass, twins, env = usage
    fewer = set()
    for key in _kernels():
        r, base = glass[GLASS % key], _twin(key, twins, env)
        assert (r["VGPRs"], r["Occupancy"]) == _pin(*key), (key, r)
        assert r["Occupancy"] in (base["Occupancy"], base["Occupancy"] - 1), (key, r, base)
        if r["Occupancy"] < base["Occupancy"]:
            fewer.add(key)
    assert fewer == FEWER_WAVES
