"""The compiler's report for the local exposure kernels (path-tracing_amd/csrc/pt_local.hip): no scratch, no spilled registers, no
dynamic stack; an occupancy not below the graded display kernel's; the staged levels' LDS priced in the granules the hardware hands
it out in; a tap one 4-byte load; nothing fused outside the IEEE divisions, and no fast-math spelling in the sources."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
REPORT = os.path.join(ASM, "local_resource_usage.txt")
LISTING = os.path.join(ASM, "pt_local.s")
GRADED_REPORT = os.path.join(ASM, "display_graded_resource_usage.txt")
SOURCES = ["pt_local.hip", "pt_local.hpp", "pt_grade.hpp"]
# kernel<DIVIDE> or <STAGE> -> (LDS bytes, IEEE divisions)
EXPECT = {"local_luma_kernelILb0EE": (0, 0), "local_luma_kernelILb1EE": (0, 3),                      # sum / n per channel
          "local_atrous_kernelILi1EE": (36 * 12 * 4, 51), "local_atrous_kernelILi2EE": (40 * 16 * 4, 51),   # two per tap and sd / sw
          "local_atrous_kernelILi0EE": (0, 51),
          "local_apply_kernelILb0EE": (0, 2), "local_apply_kernelILb1EE": (0, 5)}                    # (c a) / pivot and the gain; sum / n
LDS_GRANULE, LDS_PER_CU, WAVES_PER_GROUP, SIMDS = 1280, 160 * 1024, 4, 4


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
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-local"])
    return _parse(REPORT)


@pytest.fixture(scope="module")
def graded_occupancy():
    if not os.path.exists(GRADED_REPORT):
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-grade"])
    waves = [int(v["Occupancy"]) for name, v in _parse(GRADED_REPORT).items() if "display_kernel" in name]
    assert len(waves) == 8
    return min(waves)


def test_every_kernel_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_local.hip")).read())
    assert declared == ["local_luma_kernel", "local_atrous_kernel", "local_apply_kernel"]
    for k in EXPECT:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(EXPECT)


@pytest.mark.parametrize("kernel", list(EXPECT))
def test_no_scratch_no_spills_and_the_graded_kernels_occupancy(report, graded_occupancy, kernel):
    lds, _ = EXPECT[kernel]
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    assert int(r["LDS Size"]) == lds, r                              # 36 x 12 and 40 x 16 floats
    assert int(r["Occupancy"]) >= graded_occupancy, r
    # the compiler's calculator divides the compute unit's LDS by the kernel's bytes; the hardware hands it out in 1 280-byte granules
    if lds:
        priced = (lds + LDS_GRANULE - 1) // LDS_GRANULE * LDS_GRANULE
        assert priced == 2 * LDS_GRANULE
        groups = LDS_PER_CU // priced
        assert groups * WAVES_PER_GROUP // SIMDS >= graded_occupancy, (kernel, groups)


def test_taps_are_4_byte_accesses_and_nothing_is_fused_outside_the_divisions(report):
    asm = open(LISTING).read()
    bodies = {k: re.findall(r"^_ZN\S*%s\S*:[^\n]*\n(.*?)s_endpgm" % k, asm, re.S | re.M) for k in EXPECT}
    for k, found in bodies.items():
        assert len(found) == 1, k
        body = found[0]
        assert "scratch_" not in body and "atomic" not in body, k
        divisions = EXPECT[k][1]
        assert body.count("v_div_fmas_f32") == divisions, k
        fused = len(re.findall(r"\bv_fmac?_f32", body))
        assert fused == 5 * divisions, (k, fused)                    # the division's own five, and no other
        assert (divisions == 0) == ("v_div_scale_f32" not in body), k
        assert len(re.findall(r"\bv_rcp_f32", body)) == divisions, k   # (v_rcp_iflag is the integer tile index's)
        assert "v_mad_f32" not in body and "v_mac_f32" not in body and "v_pk_fma" not in body, k
    staged = [bodies["local_atrous_kernelILi1EE"][0], bodies["local_atrous_kernelILi2EE"][0]]
    for body in staged:                                              # the region comes in once, 4 bytes a lane; the taps are LDS reads
        assert len(re.findall(r"global_load_dword\b", body)) == 1 and "global_load_dwordx" not in body
        assert "ds_write_b32" in body and len(re.findall(r"ds_read2?_b32", body)) >= 13
        assert body.count("global_store_dword") == 1
    far = bodies["local_atrous_kernelILi0EE"][0]
    assert len(re.findall(r"global_load_dword\b", far)) == 26 and "ds_" not in far      # the pixel and its 25 taps
    for k in ("local_apply_kernelILb0EE", "local_apply_kernelILb1EE"):
        assert bodies[k][0].count("global_store_dwordx3") == 1, k
    src = "".join(open(os.path.join(CSRC, f)).read() for f in SOURCES)
    for word in ("__expf", "__powf", "__logf", "rsqrt", "__frcp", "fmaf(", "__fmaf", "__fdividef", "expf(", "logf(", "powf("):
        assert word not in src
