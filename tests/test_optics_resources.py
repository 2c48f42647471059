"""The compiler's report for the lens optics kernel (path-tracing_amd/csrc/pt_optics.hip): no scratch, no spilled registers, no
dynamic stack, no LDS; the occupancy recorded; the taps 4-byte loads; nothing fused outside the IEEE divisions, and no fast-math
spelling in the sources."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
REPORT = os.path.join(ASM, "optics_resource_usage.txt")
LISTING = os.path.join(ASM, "pt_optics.s")
SOURCES = ["pt_optics.hip", "pt_optics.hpp"]
# kernel<DIVIDE> -> IEEE divisions: u and v, sd / sw per channel, the gain; and sum / n per tap
EXPECT = {"optics_kernelILb0EE": 2 + 3 + 1, "optics_kernelILb1EE": 2 + 3 + 1 + 12}
# waves per SIMD the compiler reports today (30 and 31 vector registers): recorded, and not to fall below the other image kernels' 8
OCCUPANCY = 8


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
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if any(not os.path.exists(p) or os.path.getmtime(p) < newest for p in (REPORT, LISTING)):
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-optics"])
    return _parse(REPORT)


def test_every_kernel_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_optics.hip")).read())
    assert declared == ["optics_kernel"]
    for k in EXPECT:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(EXPECT)


@pytest.mark.parametrize("kernel", list(EXPECT))
def test_no_scratch_no_spills_no_lds_and_the_occupancy(report, kernel):
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False" and int(r["LDS Size"]) == 0, r
    print(kernel, "VGPRs", r["VGPRs"], "SGPRs", r["TotalSGPRs"], "occupancy", r["Occupancy"])
    assert int(r["Occupancy"]) == OCCUPANCY, r
    assert int(r["VGPRs"]) <= 64, r


def test_taps_are_4_byte_loads_and_nothing_is_fused_outside_the_divisions(report):
    asm = open(LISTING).read()
    for k, divisions in EXPECT.items():
        found = re.findall(r"^_ZN\S*%s\S*:[^\n]*\n(.*?)s_endpgm" % k, asm, re.S | re.M)
        assert len(found) == 1, k
        body = found[0]
        assert "scratch_" not in body and "atomic" not in body and "ds_" not in body, k
        assert "global_load_dwordx" not in body and len(re.findall(r"global_load_dword\b", body)) >= 13, k
        assert body.count("v_div_fmas_f32") == divisions, k
        fused = len(re.findall(r"\bv_fmac?_f32", body))
        assert fused == 5 * divisions, (k, fused)                    # the division's own five, and no other
        assert "v_mad_f32" not in body and "v_mac_f32" not in body and "v_pk_fma" not in body, k
    src = "".join(open(os.path.join(CSRC, f)).read() for f in SOURCES)
    for word in ("__expf", "__powf", "__logf", "rsqrt", "__frcp", "fmaf(", "__fmaf", "__fdividef", "expf(", "logf(", "powf(", "sinf(", "cosf(", "tanf("):
        assert word not in src
