"""The compiler's report for the colour display kernels (path-tracing_amd/csrc/pt_display_colour.hip): no scratch, no spilled
registers, no dynamic stack; registers, LDS and occupancy as built; output still dwords, nothing fused, and the LUT read with
plain wide loads.  The lines of the existing display kernels are pinned by tests/test_display_resources.py and
tests/test_grade_resources.py, which this change leaves as they are."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
REPORT = os.path.join(ASM, "display_colour_resource_usage.txt")
SOURCES = ["pt_display_colour.hip", "pt_display_body.inc", "pt_display_kernel.hpp", "pt_grade.hpp", "pt_colour.hpp", "pt_display.hpp"]
# (sums?, curve, with a LUT?) -> VGPRs as built; LDS is the threshold table, 8 waves per SIMD are the most a 256-thread workgroup's
# kernel can have -- the ACES kernel with a LUT holds 7
VGPRS = {(0, False): 48, (1, False): 53, (0, True): 60, (1, True): 62}
EXPECT = {"display_colour_kernelILb%dELi%dELb%dEE" % (d, c, l): (55 if (d, c, l) == (1, 2, 0) else VGPRS[(d, bool(l))], 16384, 7 if (c, l) == (3, 1) else 8)
          for d in (0, 1) for c in range(4) for l in (0, 1)}


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
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-colour"])
    return _parse(REPORT)


def test_every_kernel_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_display_colour.hip")).read())
    assert declared == ["display_colour_kernel"]
    for k in EXPECT:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(EXPECT) == 16


@pytest.mark.parametrize("kernel", list(EXPECT))
def test_no_scratch_no_spills_and_the_resources_as_built(report, kernel):
    vgprs, lds, waves = EXPECT[kernel]
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    assert int(r["VGPRs"]) == vgprs, r
    assert int(r["LDS Size"]) == lds, r
    assert int(r["Occupancy"]) == waves, r


def test_the_output_is_dwords_nothing_is_fused_and_the_lut_is_plain_loads(report):
    asm = open(os.path.join(ASM, "pt_display_colour.s")).read()
    bodies = dict(re.findall(r"^(_ZN\S*display_colour_kernel\S*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M))
    assert len(bodies) == 16
    for name, body in bodies.items():
        lut = "ELb1EEEv" in name
        assert "global_store_byte" not in body and "global_store_short" not in body
        assert body.count("global_store_dwordx3") >= 1
        divides = "ILb1E" in name or "ELi2E" in name or "ELi3E" in name           # sums / count, Reinhard, ACES
        fused = any(op in body.replace("v_div_fmas", "") for op in ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32"))
        assert "v_div_scale_f32" in body if divides else not fused, name            # fused only inside the IEEE division
        assert "scratch_" not in body and "image_" not in body and "buffer_load" not in body
        # 48 bytes of means and 16 of counts; with a LUT four vertices for each of the four pixels, each one wide load
        wide = body.count("global_load_dwordx4") + body.count("global_load_dwordx3")
        assert wide >= (4 + 16 if lut else 4), (name, wide)
    src = "".join(open(os.path.join(CSRC, f)).read() for f in SOURCES)
    for word in ("__expf", "__powf", "__logf", "rsqrt", "__frcp", "fmaf(", "__fmaf", "__fdividef", "tex3D", "hipTextureObject"):
        assert word not in src
