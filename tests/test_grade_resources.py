"""The compiler's report for the grading kernels (path-tracing_amd/csrc/pt_meter.hip, pt_display_graded.hip): no scratch, no spilled
registers, no dynamic stack; registers, LDS and occupancy as built; the histogram counted with LDS integer atomics and the graded
kernel's output still dwords."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
REPORTS = {"meter": os.path.join(ASM, "meter_resource_usage.txt"), "graded": os.path.join(ASM, "display_graded_resource_usage.txt")}
SOURCES = ["pt_meter.hip", "pt_meter.hpp", "pt_display_graded.hip", "pt_display_body.inc", "pt_display_kernel.hpp", "pt_grade.hpp"]
GRADED = ["display_kernelILb%dELi%dEE" % (d, c) for c in range(4) for d in (0, 1)]      # means / sums  x  the four curves
# kernel -> (report, VGPRs as built, LDS bytes, waves per SIMD)
EXPECT = {"meter_kernelILb0E": ("meter", 26, 2064, 8), "meter_kernelILb1E": ("meter", 30, 2064, 8), "exposure_kernel": ("meter", 6, 0, 8)}
EXPECT.update({k: ("graded", 53, 16384, 8) for k in GRADED})


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
def reports():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if any(not os.path.exists(p) or os.path.getmtime(p) < newest for p in REPORTS.values()):
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-grade"])
    return {k: _parse(p) for k, p in REPORTS.items()}


def test_every_kernel_is_reported(reports):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_meter.hip")).read())
    assert declared == ["meter_kernel", "exposure_kernel"]
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_display_graded.hip")).read())
    assert declared == ["display_kernel"]
    for k, (which, _, _, _) in EXPECT.items():
        assert sum(k in name for name in reports[which]) == 1, (k, list(reports[which]))
    assert len(reports["meter"]) == 3 and len(reports["graded"]) == len(GRADED)


@pytest.mark.parametrize("kernel", list(EXPECT))
def test_no_scratch_no_spills_and_the_resources_as_built(reports, kernel):
    which, vgprs, lds, waves = EXPECT[kernel]
    r = next(v for name, v in reports[which].items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    assert int(r["VGPRs"]) == vgprs, r
    assert int(r["LDS Size"]) == lds, r
    assert int(r["Occupancy"]) == waves, r          # 8: the most a 256-thread workgroup's kernel can have, the ungraded kernel's


def test_the_histogram_is_lds_atomics_and_the_graded_output_is_dwords():
    asm = open(os.path.join(ASM, "pt_meter.s")).read()
    bodies = re.findall(r"^_ZN\S*meter_kernel\S*:[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M)
    assert len(bodies) == 2
    for body in bodies:
        assert "ds_add_u32" in body and "global_atomic_add" in body
        assert body.count("global_load_dwordx4") >= 4            # 48 bytes of means, 16 of counts
        assert "scratch_" not in body and "cmpswap" not in body
    asm = open(os.path.join(ASM, "pt_display_graded.s")).read()
    bodies = re.findall(r"^_ZN\S*display_kernel\S*:[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M)
    assert len(bodies) == 8
    for body in bodies:
        assert "global_store_byte" not in body and "global_store_short" not in body
        assert body.count("global_store_dwordx3") >= 1 and body.count("global_load_dwordx4") >= 4
        assert "v_fma_f32" not in body.replace("v_div_fmas", "") or "v_div_scale_f32" in body      # fused only inside the IEEE division
        assert "scratch_" not in body
    src = "".join(open(os.path.join(CSRC, f)).read() for f in SOURCES)
    for word in ("__expf", "__powf", "__logf", "rsqrt", "__frcp", "fmaf(", "__fmaf", "__fdividef"):
        assert word not in src
