"""The compiler's report on the projection kernels (pt_kernels.hip: integrate_kernel_projection; CPU: hipcc cross-compiles gfx950
without a GPU), read as tests/test_motion_resources.py reads it: one projection kernel per camera twin, no scratch memory, no
spilled vector register, the twin's LDS and the twin's waves per SIMD."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "resource_usage.txt")
PROJECTION, TWIN = "_ZN2pt27integrate_kernel_projection", "_ZN2pt16integrate_kernel"
# The projection kernels compiled for one wave per SIMD fewer than the camera twin they belong to (pt_kernels.hip: projection_waves),
# by mangled name: none -- the one kernel with the three kinds keeps every twin's budget.
FEWER_WAVES = {}


@pytest.fixture(scope="module")
def usage():
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_integrator_body.inc", "pt_projection.hpp", "pt_kernels.hpp", "pt_launch_plan.hpp",
                                            "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
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


def test_every_camera_twin_has_exactly_one_projection_kernel(usage):
    twins = sorted(k for k in usage if k.startswith(TWIN + "I") and int(re.search(r"ELi(\d+)EEEv", k).group(1)) % 2 == 1)
    projection = sorted(k for k in usage if k.startswith(PROJECTION + "I"))
    assert len(twins) == 22
    assert sorted(k.replace(PROJECTION, TWIN) for k in projection) == twins


def test_projection_kernels_do_not_spill_and_keep_the_budgets_of_their_twins(usage):
    seen, n = set(), 0
    for k, r in usage.items():
        if not k.startswith(PROJECTION + "I"):
            continue
        n += 1
        base = usage[k.replace(PROJECTION, TWIN)]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] == base["LDS Size"], (k, r, base)
        if k in FEWER_WAVES:
            seen.add(k)
            assert r["Occupancy"] == base["Occupancy"] - 1 == FEWER_WAVES[k], (k, r, base)
        else:
            assert r["Occupancy"] == base["Occupancy"], (k, r, base)
    assert n == 22 and seen == set(FEWER_WAVES)


def test_the_feature_pass_kernel_of_a_projection_is_small(usage):
    rays = [r for k, r in usage.items() if "projection_rays_kernel" in k]
    assert len(rays) == 1 and rays[0]["ScratchSize"] == 0 and rays[0]["VGPRs Spill"] == 0 and rays[0]["LDS Size"] == 0
