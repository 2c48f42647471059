"""The compiler's report for the feature and denoiser kernels (path-tracing_amd/csrc/pt_denoise.hip): no scratch, no spilled
registers.  (tests/test_kernel_resources.py pins the integrator's kernels; this file pins the new ones only.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "denoise_resource_usage.txt")
KERNELS = ["feature_rays_kernel", "feature_gather_kernel", "denoise_prepare_kernel", "denoise_variance_kernel", "denoise_atrous_kernel",
           "denoise_finish_kernel"]


@pytest.fixture(scope="module")
def report():
    src = os.path.join(CSRC, "pt_denoise.hip")
    if not os.path.exists(USAGE) or os.path.getmtime(USAGE) < os.path.getmtime(src):
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


def test_every_new_kernel_is_reported(report):
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(report, kernel):
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    assert int(r["Occupancy"]) >= 8, r     # memory-bound stencils: latency is hidden by waves


def test_a_tap_is_three_wide_loads(report):
    """The a-trous kernel reads its records with 16-byte loads and nothing in the file is fused or approximated by hand."""
    asm = open(os.path.join(os.path.dirname(USAGE), "pt_denoise.s")).read()
    m = re.search(r"^_ZN\S*denoise_atrous_kernel\S*:[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M)
    assert m, "the a-trous kernel's code was not found"
    body = m.group(1)
    assert "global_load_dwordx4" in body
    src = open(os.path.join(CSRC, "pt_denoise.hip")).read()
    for word in ("__expf", "__powf", "rsqrt", "__frcp", "fmaf(", "__fmaf"):
        assert word not in src
