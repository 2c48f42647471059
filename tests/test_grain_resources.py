"""The compiler's report for the grain display kernels (path-tracing_amd/csrc/pt_display_grain.hip): no scratch, no spilled registers,
no dynamic stack; registers, LDS and occupancy as built; output still dwords, nothing fused outside the IEEE division, the Philox
products one 32 x 32 -> 64 bit multiply each and the floor one instruction.  The lines of the three existing display kernels are
pinned by tests/test_display_resources.py, tests/test_grade_resources.py and tests/test_colour_resources.py, which this change leaves
as they are: pt_display_body.inc gives them the tokens it always did."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
REPORT = os.path.join(ASM, "display_grain_resource_usage.txt")
SOURCES = ["pt_display_grain.hip", "pt_display_body.inc", "pt_display_kernel.hpp", "pt_grade.hpp", "pt_colour.hpp", "pt_grain.hpp", "pt_display.hpp"]
# (with a LUT?, pitch other than 1?) -> VGPRs as built; the exceptions below.  LDS is the threshold table; 8 waves per SIMD are the most
# a 256-thread workgroup's kernel can have, and every instantiation holds them
VGPRS = {(0, 0): 59, (0, 1): 62, (1, 0): 63, (1, 1): 64}
ODD = {(1, 0, 1, 0): 60, (1, 1, 1, 0): 60, (1, 2, 0, 0): 63, (1, 2, 0, 1): 63}     # (sums?, curve, LUT?, pitch?)
EXPECT = {"display_grain_kernelILb%dELi%dELb%dELb%dEE" % (d, c, l, s): (ODD.get((d, c, l, s), VGPRS[(l, s)]), 16384, 8)
          for d in (0, 1) for c in range(4) for l in (0, 1) for s in (0, 1)}


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
    if not os.path.exists(REPORT) or os.path.getmtime(REPORT) < newest:
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-grain"])
    return _parse(REPORT)


def test_every_kernel_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_display_grain.hip")).read())
    assert declared == ["display_grain_kernel"]
    for k in EXPECT:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(EXPECT) == 32


@pytest.mark.parametrize("kernel", list(EXPECT))
def test_no_scratch_no_spills_and_the_resources_as_built(report, kernel):
    vgprs, lds, waves = EXPECT[kernel]
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    assert int(r["VGPRs"]) == vgprs, r
    assert int(r["LDS Size"]) == lds, r
    assert int(r["Occupancy"]) == waves, r


def test_the_output_is_dwords_nothing_is_fused_and_the_generator_is_wide_multiplies(report):
    asm = open(os.path.join(ASM, "pt_display_grain.s")).read()
    bodies = dict(re.findall(r"^(_ZN\S*display_grain_kernel\S*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M))
    assert len(bodies) == 32
    for name, body in bodies.items():
        assert "global_store_byte" not in body and "global_store_short" not in body
        assert body.count("global_store_dwordx3") >= 1
        # the dither's division is in every kernel; fused operations appear inside the IEEE divisions only, five in each
        divisions = body.count("v_div_fixup_f32")
        assert divisions >= 1 and body.count("v_div_scale_f32") == 2 * divisions
        assert len(re.findall(r"\bv_fma_f32|\bv_fmac_f32", body)) == 5 * divisions and "v_pk_fma_f32" not in body, name
        assert "scratch_" not in body and "image_" not in body and "buffer_load" not in body
        assert "v_mad_u64_u32" in body or "v_mul_hi_u32" in body
        assert "v_floor_f32" in body
    src = "".join(open(os.path.join(CSRC, f)).read() for f in SOURCES)
    for word in ("__expf", "__powf", "__logf", "rsqrt", "__frcp", "fmaf(", "__fmaf", "__fdividef", "tex3D", "hipTextureObject"):
        assert word not in src
