"""The compiler's report on the environment kernels (pt_environment_kernels.hip: integrate_kernel_environment; CPU: hipcc cross-compiles
gfx950 without a GPU), read as tests/test_projection_resources.py reads the projection kernels': one environment kernel per skybox
variant and view, no scratch memory, no spilled vector register, the skybox twin's LDS, and the twin's waves per SIMD or, for a pinned list, more
(DESIGN.md section 25)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
ENVIRONMENT = "_ZN2pt28integrate_kernel_environmentILb%dELb%dELb%dELi%dEEEvNS_10RenderArgsE"
# the skybox twin of view 0 .. 5: the kernel's mangled name and its ADAPT argument
TWINS = {0: ("16integrate_kernel", 0), 1: ("16integrate_kernel", 1), 2: ("21integrate_kernel_lens", 1), 3: ("23integrate_kernel_motion", 1),
         4: ("28integrate_kernel_motion_lens", 1), 5: ("27integrate_kernel_projection", 1)}
# The environment kernels compiled for one wave per SIMD fewer than their twin (pt_kernels.hip: environment_waves): none.
FEWER_WAVES = {}
# Without the skybox's double-precision acos and atan2 the lookup needs fewer vector registers (79 ... 90 against 96 ... 108), so the
# compiler's occupancy of some kernels lies ABOVE the twin's.  Pinned here, (big, stats, env, view) -> waves above the twin, so that a
# drift in either direction shows: the box-tree kernels without the envelope test or with statistics and it, and every lens kernel
# (the lens twins are the ones compiled for a wave fewer than the skybox kernels).
_BOX = {(1, 0, 0): 1, (1, 1, 0): 1, (1, 1, 1): 1}
MORE_WAVES = {(b, s, e, v): d for v in (0, 1, 3, 5) for (b, s, e), d in _BOX.items()}
MORE_WAVES.update({(b, s, e, v): 1 for v in (2, 4) for b in (0, 1) for s in (0, 1) for e in (0, 1)})
MORE_WAVES.update({(1, 1, 0, v): 2 for v in (2, 4)})


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
    srcs = [os.path.join(CSRC, f) for f in ("pt_kernels.hip", "pt_environment_kernels.hip", "pt_integrator_body.inc", "pt_environment.hpp", "pt_projection.hpp",
                                            "pt_kernels.hpp", "pt_launch_plan.hpp", "pt_fastfp.hpp", "pt_scene.hpp", "Makefile")]
    newest = max(os.path.getmtime(f) for f in srcs)
    if not os.path.exists(os.path.join(ASM, "environment_resource_usage.txt")) or os.path.getmtime(os.path.join(ASM, "environment_resource_usage.txt")) < newest:
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-environment"])
    if not os.path.exists(os.path.join(ASM, "resource_usage.txt")) or os.path.getmtime(os.path.join(ASM, "resource_usage.txt")) < newest:
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-of-pt_kernels"])
    return _report(os.path.join(ASM, "environment_resource_usage.txt")), _report(os.path.join(ASM, "resource_usage.txt"))


def test_one_environment_kernel_per_skybox_variant_and_view(usage):
    env, twins = usage
    want = sorted(ENVIRONMENT % (b, s, e, v) for b in (0, 1) for s in (0, 1) for e in (0, 1) for v in range(6))
    assert sorted(k for k in env if "integrate_kernel" in k) == want and len(want) == 48
    assert not [k for k in twins if "environment" in k]       # none of them in the kernels' own translation unit


def test_environment_kernels_do_not_spill_and_keep_the_budgets_of_their_twins(usage):
    env, twins = usage
    seen = set()
    for v, (name, adapt) in TWINS.items():
        for b in (0, 1):
            for s in (0, 1):
                for e in (0, 1):
                    k = ENVIRONMENT % (b, s, e, v)
                    r, base = env[k], twins["_ZN2pt%sILb1ELb%dELb%dELb%dELb0ELi%dEEEvNS_10RenderArgsE" % (name, b, s, e, adapt)]
                    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (k, r)
                    assert r["LDS Size"] == base["LDS Size"], (k, r, base)
                    if k in FEWER_WAVES:
                        seen.add(k)
                        assert r["Occupancy"] == base["Occupancy"] - 1 == FEWER_WAVES[k], (k, r, base)
                    else:
                        assert r["Occupancy"] == base["Occupancy"] + MORE_WAVES.get((b, s, e, v), 0), (k, r, base)
    assert seen == set(FEWER_WAVES)
