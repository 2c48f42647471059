"""The compiler's report for the upsampler's kernels (path-tracing_amd/csrc/pt_upsample.hip): no scratch, no spilled registers, the
occupancy of the a-trous kernel it is measured against, and taps read as 16-byte loads."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
USAGE = os.path.join(ASM, "upsample_resource_usage.txt")
DENOISE_USAGE = os.path.join(ASM, "denoise_resource_usage.txt")
SOURCE = os.path.join(CSRC, "pt_upsample.hip")
FULL = ["upsample_kernelILi2E", "upsample_kernelILi3E", "upsample_kernelILi4E"]     # one instantiation per scale
KERNELS = ["upsample_mean_kernel", "upsample_prepare_kernel"] + FULL


def _parse(path):
    kernels, name = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and name:
            kernels[name][m.group(1)] = m.group(2)
    return kernels


@pytest.fixture(scope="module")
def report():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in ("pt_upsample.hip", "pt_upsample.hpp", "pt_feature_weight.hpp"))
    if not os.path.exists(USAGE) or os.path.getmtime(USAGE) < newest:
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-upsample"])
    return _parse(USAGE)


def test_every_kernel_of_the_file_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(SOURCE).read())
    assert declared == ["upsample_mean_kernel", "upsample_prepare_kernel", "upsample_kernel"]
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(report, kernel):
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    # as built: 22, 31 and 49 / 49 / 50 VGPRs, 8 waves per SIMD -- the most a 256-thread workgroup's kernel can have here
    assert int(r["Occupancy"]) == 8, r
    assert int(r["VGPRs"]) <= 64, r
    assert int(r["LDS Size"]) == 0, r       # the taps come from global memory (the L1 / L2); the LDS form is a variant build


def test_occupancy_is_at_least_the_atrous_kernels(report):
    if not os.path.exists(DENOISE_USAGE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    atrous = next(v for name, v in _parse(DENOISE_USAGE).items() if "denoise_atrous_kernel" in name)
    for k in FULL:
        r = next(v for name, v in report.items() if k in name)
        assert int(r["Occupancy"]) >= int(atrous["Occupancy"]), (k, r, atrous)


def test_a_tap_is_three_wide_loads_and_nothing_is_approximated_by_hand():
    asm = open(os.path.join(ASM, "pt_upsample.s")).read()
    bodies = re.findall(r"^_ZN\S*upsample_kernelILi\dE\S*:[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M)
    assert len(bodies) == 3, "the three instantiations' code was not found"
    for body in bodies:
        assert "global_load_dwordx4" in body
    src = open(SOURCE).read() + open(os.path.join(CSRC, "pt_feature_weight.hpp")).read()
    for word in ("__expf", "__powf", "rsqrt", "__frcp", "fmaf("):
        assert word not in src
