"""Compiler-reported resources of the hot kernels (CPU: hipcc cross-compiles gfx950 without a GPU).

Both integrator kernels sit at the edge of their register budgets; a harmless-looking source change can push one over it
(round 3: wrapping the kernel body in a device function took the Tor.obj kernel from 41 to 163 spilled scalar registers
and one spilled vector register -- 16 % of its speed -- with every test still green).  This pins what the speed depends on:
no scratch memory, no spilled vector registers, and the occupancy each kernel is tuned for."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "resource_usage.txt")


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_integrator_body.inc", "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    if not os.path.exists(USAGE) or os.path.getmtime(USAGE) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    out, name = {}, None
    for line in open(USAGE):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


# mangled name -> (what, waves per SIMD at least, LDS bytes at most).  gfx950 hands out its 160 KB of LDS in granules of 1 280 bytes
# (the 32 x 8 adaptive kernel at 7 888 B lost its fifth wave per SIMD to that -- a sixth granule is 7 680 B -- although 20 x 7 888 <
# 160 K: +13 % frame time, profiles/r04_ab_logs.txt adapt2): 20 waves per CU leave 6 granules each, 24 waves 5.
HOT = {
    "_ZN2pt16integrate_kernelILb0ELb0ELb0ELb0ELb0ELi0EEEvNS_10RenderArgsE": ("small scenes, two pixels per lane (the headline kernel)", 5, 7680),
    "_ZN2pt16integrate_kernelILb0ELb0ELb0ELb0ELb0ELi2EEEvNS_10RenderArgsE": ("the same with adaptive sampling on (batches over 16 x 8 tiles)", 5, 7680),
    "_ZN2pt16integrate_kernelILb0ELb0ELb0ELb0ELb0ELi4EEEvNS_10RenderArgsE": ("the same over 32 x 8 tiles", 5, 7680),
    "_ZN2pt16integrate_kernelILb0ELb0ELb0ELb0ELb1ELi0EEEvNS_10RenderArgsE": ("small scenes, one pixel per lane (small launches)", 6, 6400),
    "_ZN2pt16integrate_kernelILb0ELb1ELb0ELb0ELb0ELi0EEEvNS_10RenderArgsE": ("big scenes (box tree)", 6, 6400),
    "_ZN2pt16integrate_kernelILb0ELb1ELb0ELb0ELb0ELi2EEEvNS_10RenderArgsE": ("the same with adaptive sampling on (batches over 16 x 8 tiles)", 6, 6400),
    "_ZN2pt16integrate_kernelILb0ELb1ELb0ELb0ELb0ELi4EEEvNS_10RenderArgsE": ("the same over 32 x 8 tiles", 6, 6400),
    "_ZN2pt16integrate_kernelILb1ELb0ELb0ELb0ELb0ELi0EEEvNS_10RenderArgsE": ("small scenes under a skybox (path regeneration)", 5, 7680),
    "_ZN2pt16integrate_kernelILb1ELb1ELb0ELb0ELb0ELi0EEEvNS_10RenderArgsE": ("big scenes under a skybox", 5, 7680),
}


@pytest.mark.parametrize("kernel", sorted(HOT))
def test_hot_kernels_keep_their_register_and_lds_budgets(usage, kernel):
    what, waves, lds = HOT[kernel]
    r = usage[kernel]
    assert r["ScratchSize"] == 0, (what, r)
    assert r["VGPRs Spill"] == 0, (what, r)
    assert r["Occupancy"] >= waves, (what, r)
    assert r["LDS Size"] <= lds, (what, r)
    assert r["SGPRs Spill"] <= 64, (what, r)      # 31-42 today; 163 is what the regression looked like


def test_no_integrator_instantiation_uses_scratch(usage):
    bad = {k: v for k, v in usage.items() if "integrate_kernel" in k and v.get("ScratchSize", 0) != 0}
    assert not bad, bad
