"""The compiler's report for the temporal merge kernel (path-tracing_amd/csrc/pt_temporal.hip): no scratch, no spilled registers,
16-byte record loads, nothing fused or approximated by hand.  (tests/test_denoise_resources.py pins the denoiser's kernels.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "temporal_resource_usage.txt")
SOURCE = os.path.join(CSRC, "pt_temporal.hip")
KERNELS = ["temporal_merge_kernel"]


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


def test_every_kernel_of_the_file_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(SOURCE).read())
    assert sorted(declared) == sorted(KERNELS)
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(report, kernel):
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    # 40 VGPRs: the compiler reports 8 waves per SIMD, the most a 256-thread workgroup's kernel can have here and what the
    # denoiser's stencils run at -- a gather-bound kernel hides its latency with waves
    assert int(r["Occupancy"]) >= 8, r


def test_a_tap_is_wide_loads(report):
    asm = open(os.path.join(os.path.dirname(USAGE), "pt_temporal.s")).read()
    m = re.search(r"^_ZN\S*temporal_merge_kernel\S*:[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M)
    assert m, "the merge kernel's code was not found"
    body = m.group(1)
    assert body.count("global_load_dwordx4") >= 4          # the four records of a tap
    assert body.count("global_store_dwordx4") >= 4         # and of the new history
    src = open(SOURCE).read()
    for word in ("__expf", "__powf", "rsqrt", "__frcp", "fmaf(", "__fmaf"):
        assert word not in src
