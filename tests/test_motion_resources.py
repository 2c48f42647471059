"""The compiler's report on the motion kernels (pt_kernels.hip: integrate_kernel_motion, integrate_kernel_motion_lens; CPU: hipcc
cross-compiles gfx950 without a GPU), read as tests/test_kernel_resources.py reads it: no scratch memory, no spilled vector
register, and the waves per SIMD DESIGN.md section 18 records -- those of the kernel each one is the motion twin of, except one."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "resource_usage.txt")
MOTION, MOTION_LENS = "_ZN2pt23integrate_kernel_motion", "_ZN2pt28integrate_kernel_motion_lens"
TWIN, LENS = "_ZN2pt16integrate_kernel", "_ZN2pt21integrate_kernel_lens"
# The motion kernels compiled for one wave per SIMD fewer than the kernel they are the twin of (pt_kernels.hip: motion_waves): the
# lens twin of the two-pixel small-scene kernel with the envelope test spilled one VGPR at 5.  Template arguments SKY BIG STATS ENV NARROW.
FEWER_WAVES = {MOTION_LENS + "ILb0ELb0ELb0ELb1ELb0ELi1EEEvNS_10RenderArgsE": 4}


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_integrator_body.inc", "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp",
                                            "pt_scene.hpp", "Makefile")]
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


def _parent(name):
    return name.replace(MOTION_LENS, LENS) if name.startswith(MOTION_LENS) else name.replace(MOTION, TWIN)


def test_every_camera_twin_and_lens_kernel_has_exactly_one_motion_twin(usage):
    twins = sorted(k for k in usage if k.startswith(TWIN + "I") and int(re.search(r"ELi(\d+)EEEv", k).group(1)) % 2 == 1)
    lens = sorted(k for k in usage if k.startswith(LENS + "I"))
    motion = sorted(k for k in usage if k.startswith(MOTION + "I"))
    motion_lens = sorted(k for k in usage if k.startswith(MOTION_LENS + "I"))
    assert len(twins) == len(lens) == 22
    assert sorted(_parent(k) for k in motion) == twins and sorted(_parent(k) for k in motion_lens) == lens


def test_motion_kernels_do_not_spill_and_keep_their_recorded_waves(usage):
    seen = set()
    for k, r in usage.items():
        if "integrate_kernel_motion" not in k:
            continue
        base = usage[_parent(k)]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] == base["LDS Size"], (k, r, base)
        if k in FEWER_WAVES:
            seen.add(k)
            assert r["Occupancy"] == base["Occupancy"] - 1 == FEWER_WAVES[k], (k, r, base)
        else:
            assert r["Occupancy"] == base["Occupancy"], (k, r, base)
    assert seen == set(FEWER_WAVES)
