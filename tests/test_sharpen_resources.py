"""The compiler's report for the sharpening kernels (path-tracing_amd/csrc/pt_sharpen.hip): both declared and reported once per form;
no scratch, no spilled registers, no dynamic stack, no LDS; an occupancy not below the graded display kernel's; as many IEEE division
sequences in each body as the header states divisions, and nothing fused outside them; a ring tap one 4-byte load; and no fast-math
spelling in the sources."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
REPORT = os.path.join(ASM, "sharpen_resource_usage.txt")
LISTING = os.path.join(ASM, "pt_sharpen.s")
GRADED_REPORT = os.path.join(ASM, "display_graded_resource_usage.txt")
SOURCES = ["pt_sharpen.hip", "pt_sharpen.hpp", "pt_grade.hpp"]
# kernel<DIVIDE> -> IEEE divisions: a / (1 + a); and hmin, hmax, (lobe sd) / den, l0, l1, l1 / l0; the sums form adds sum / n per channel
EXPECT = {"sharpen_luma_kernelILb0EE": 1, "sharpen_luma_kernelILb1EE": 4, "sharpen_apply_kernelILb0EE": 6, "sharpen_apply_kernelILb1EE": 9}


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
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-sharpen"])
    return _parse(REPORT)


@pytest.fixture(scope="module")
def graded_occupancy():
    if not os.path.exists(GRADED_REPORT):
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-grade"])
    waves = [int(v["Occupancy"]) for name, v in _parse(GRADED_REPORT).items() if "display_kernel" in name]
    assert len(waves) == 8
    return min(waves)


def test_every_kernel_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_sharpen.hip")).read())
    assert declared == ["sharpen_luma_kernel", "sharpen_apply_kernel"]
    for k in EXPECT:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(EXPECT)


@pytest.mark.parametrize("kernel", list(EXPECT))
def test_no_scratch_no_spills_no_lds_and_the_graded_kernels_occupancy(report, graded_occupancy, kernel):
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    assert int(r["LDS Size"]) == 0, r                                # the ring is four loads; no tile is staged
    assert int(r["Occupancy"]) >= graded_occupancy, r


def test_the_divisions_are_the_headers_and_nothing_is_fused_outside_them(report):
    asm = open(LISTING).read()
    bodies = {k: re.findall(r"^_ZN\S*%s\S*:[^\n]*\n(.*?)s_endpgm" % k, asm, re.S | re.M) for k in EXPECT}
    for k, found in bodies.items():
        assert len(found) == 1, k
        body = found[0]
        assert "scratch_" not in body and "atomic" not in body and "ds_" not in body, k
        divisions = EXPECT[k]
        assert body.count("v_div_fmas_f32") == divisions, k
        fused = len(re.findall(r"\bv_fmac?_f32", body))
        assert fused == 5 * divisions, (k, fused)                    # the division's own five, and no other
        assert body.count("v_div_scale_f32") == 2 * divisions and body.count("v_div_fixup_f32") == divisions, k
        assert len(re.findall(r"\bv_rcp_f32", body)) == divisions, k   # (v_rcp_iflag is the integer tile index's)
        assert "v_mad_f32" not in body and "v_mac_f32" not in body and "v_pk_fma" not in body, k
        # min and max are the header's single comparisons: a hardware min / max orders zeros and NaNs its own way
        assert not re.search(r"\bv_(min|max)3?_f32", body), k
    for k in ("sharpen_luma_kernelILb0EE", "sharpen_luma_kernelILb1EE"):       # the mean, the count and e in; one float out
        body = bodies[k][0]
        assert body.count("global_load_dwordx3") == 1 and len(re.findall(r"global_load_dword\b", body)) == 1, k
        assert len(re.findall(r"global_store_dword\b", body)) == 1 and "global_store_dwordx" not in body, k
    for k in ("sharpen_apply_kernelILb0EE", "sharpen_apply_kernelILb1EE"):     # the count, the centre and the ring: six 4-byte loads
        body = bodies[k][0]
        assert len(re.findall(r"global_load_dword\b", body)) == 6, k
        assert body.count("global_load_dwordx3") == 1 and body.count("global_store_dwordx3") == 1, k
        assert len(re.findall(r"global_store_dword\b", body)) == 0, k
    src = "".join(open(os.path.join(CSRC, f)).read() for f in SOURCES)
    for word in ("__expf", "__powf", "__logf", "rsqrt", "__frcp", "fmaf(", "__fmaf", "__fdividef", "expf(", "logf(", "powf(", "sqrtf(", "fminf(", "fmaxf("):
        assert word not in src
