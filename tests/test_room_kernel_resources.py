"""Compiler-reported resources of the room instantiations of the plain small-scene kernel (CPU: hipcc cross-compiles gfx950).

The room kernels (pt_room_kernels.hip; pt_kernels.hip: closest_hit<..., ROOM>; integrate_kernel<false, false, false, false, NARROW, 8>)
are a translation unit of their own with a report of their own (lib/asm/room_resource_usage.txt: make asm-room).  They exist for one
reason: the generic search loops they leave out hold scalar registers that the generic kernels spill.  So each must be no worse than
its generic sibling in every resource the speed depends on -- vector registers, LDS, spilled scalar registers, scratch -- must spill
FEWER scalar registers than it, and must keep its occupancy: 5 waves per SIMD for the two-pixel form (6 LDS granules of 1 280 bytes),
6 for the 8 x 8 form (5 granules).  Figures when the kernels were added (generic -> room): 16 x 8: 96 -> 90 VGPRs, 45 -> 41 spilled
SGPRs, 6 864 B LDS both; 8 x 8: 79 -> 73 VGPRs, 36 -> 18 spilled SGPRs, 5 840 B LDS both.  The unit holds these two kernels and
nothing else."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "resource_usage.txt")            # the generic siblings (pt_kernels.hip)
ROOM_USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "room_resource_usage.txt")
LDS_GRANULE = 1280

KERNEL = "_ZN2pt16integrate_kernelILb0ELb0ELb0ELb0ELb%dELi%dEEEvNS_10RenderArgsE"
# narrow -> (what, waves per SIMD at least, LDS granules at most, spilled SGPRs at most)
FORMS = {0: ("two pixels per lane (16 x 8 tiles: the headline frame)", 5, 6, 41), 1: ("one pixel per lane (8 x 8 tiles: small launches)", 6, 5, 18)}


def _report(path, target):
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_room_kernels.hip", "pt_integrator_body.inc", "pt_sphere_tree_walk.inc", "pt_kernels.hpp",
                                            "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    if not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-C", CSRC, "-s", target])
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
    return _report(USAGE, "asm-of-pt_kernels")


@pytest.fixture(scope="module")
def room_usage():
    return _report(ROOM_USAGE, "asm-room")


def test_the_room_unit_holds_the_two_room_kernels_and_nothing_else(room_usage):
    assert sorted(room_usage) == sorted(KERNEL % (narrow, 8) for narrow in FORMS), sorted(room_usage)


@pytest.mark.parametrize("narrow", sorted(FORMS))
def test_room_kernels_are_no_worse_than_their_generic_siblings(usage, room_usage, narrow):
    what, waves, granules, spills = FORMS[narrow]
    room, generic = room_usage[KERNEL % (narrow, 8)], usage[KERNEL % (narrow, 0)]
    assert room["ScratchSize"] == 0 and room["VGPRs Spill"] == 0, (what, room)
    assert room["VGPRs"] <= generic["VGPRs"], (what, room, generic)
    assert room["LDS Size"] <= generic["LDS Size"], (what, room, generic)
    assert room["SGPRs Spill"] < generic["SGPRs Spill"], (what, room, generic)      # the point of the kernels
    assert room["SGPRs Spill"] <= spills, (what, room)
    assert room["Occupancy"] >= waves, (what, room)
    assert -(-room["LDS Size"] // LDS_GRANULE) <= granules, (what, room)             # 160 KB of LDS per CU = 128 granules: 4 x waves x granules <= 128
    assert 4 * waves * granules <= 128
