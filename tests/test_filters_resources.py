"""The compiler's report for the post-filter kernels (path-tracing_amd/csrc/pt_filters.hip).  Every number below was read from
`make asm`'s -Rpass-analysis=kernel-resource-usage report (lib/asm/filters_resource_usage.txt) for the source as it stood when
this file was added; no kernel was changed to meet it.  (tests/test_denoise_resources.py and tests/test_temporal_resources.py
pin the other image-space kernels, tests/test_kernel_resources.py the integrator.)

    kernel                     VGPRs  scratch B/lane  spills  waves/SIMD
    gauss_lds_kernel              36               0       0           8
    gauss_kernel                  18               0       0           8
    median_small_kernel<1>        44               0       0           8
    median_small_kernel<2>        39               0       0           8
    median_small_kernel<3>        42               0       0           8
    median_kernel                 13             272       0           8
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "filters_resource_usage.txt")
SOURCE = os.path.join(CSRC, "pt_filters.hip")
# as the report's mangled names spell them: the three register-median instantiations are ...kernelILi1EE, ILi2EE, ILi3EE
KERNELS = ["gauss_lds_kernel", "gauss_kernel", "median_small_kernelILi1E", "median_small_kernelILi2E", "median_small_kernelILi3E",
           "13median_kernel"]
# median_kernel keeps its (up to) 64 smallest values in an array that is indexed by a run-time position, so the compiler puts it
# in scratch: 64 floats + bookkeeping = 272 bytes per lane.  A RECORDED STATE, not a goal: the bound only says "no worse".
MEDIAN_KERNEL_SCRATCH_BYTES = 272


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(USAGE) or os.path.getmtime(USAGE) < os.path.getmtime(SOURCE):
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    kernels, name = {}, None
    for line in open(USAGE):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and name:
            kernels[name][m.group(1)] = m.group(2)
    return kernels


def _of(report, kernel):
    return next(v for name, v in report.items() if kernel in name)


def test_every_kernel_of_the_file_is_reported(report):
    declared = set(re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(SOURCE).read()))
    assert declared == {"gauss_lds_kernel", "gauss_kernel", "median_small_kernel", "median_kernel"}
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS[:1] + KERNELS[2:5])
def test_lds_gaussian_and_register_medians_no_scratch_no_spills(report, kernel):
    r = _of(report, kernel)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    # 36 to 44 VGPRs: the REGISTER-side bound, all the waves a 256-thread workgroup's kernel can have here.  Not the achieved
    # occupancy of gauss_lds_kernel: its tile is dynamic LDS (the report says "LDS Size 0"), and at -GAUSS 9 the 48 KB tile, not the
    # registers, limits how many workgroups a compute unit holds.
    assert int(r["Occupancy"]) >= 8, r


def test_global_gaussian_spills_no_vector_registers(report):
    r = _of(report, "gauss_kernel")
    assert r["VGPRs Spill"] == "0" and r["Dynamic Stack"] == "False", r


def test_generic_median_scratch_is_no_worse_than_recorded(report):
    r = _of(report, "13median_kernel")
    assert r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0" and r["Dynamic Stack"] == "False", r
    assert int(r["ScratchSize"]) <= MEDIAN_KERNEL_SCRATCH_BYTES, r


def test_nothing_fused_or_approximated_by_hand():
    src = open(SOURCE).read()
    for word in ("__expf", "__powf", "rsqrt", "__frcp", "fmaf(", "__fmaf"):
        assert word not in src
    assert "#pragma clang fp contract(off)" in src
