"""The compiler's report for the scene-linear encode kernels (path-tracing_amd/csrc/pt_linear.hip): no scratch, no spilled registers, no
dynamic stack and no LDS; full occupancy; the output written as 16-byte stores and nothing narrower; the aligned PFM kernel and the
RGBE kernel read 16 bytes at a time; nothing fused outside the IEEE division of the instantiations that divide.  The display kernels,
which this stage runs beside and not inside, still compile to what their own tests pin (tests/test_display_resources.py,
tests/test_grain_resources.py): their reports are made again here and held against those tests' figures."""
import os
import re
import subprocess

import pytest

import test_display_resources as display_pins
import test_grain_resources as grain_pins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
REPORT = os.path.join(ASM, "linear_resource_usage.txt")
SOURCES = ["pt_linear.hip", "pt_linear.hpp", "pt_grade.hpp"]
# (sums?, exposed?) and for PFM (.., width a multiple of 4?)
RGBE = ["linear_rgbe_kernelILb%dELb%dEE" % (d, e) for d in (0, 1) for e in (0, 1)]
PFM = ["linear_pfm_kernelILb%dELb%dELb%dEE" % (d, e, r) for d in (0, 1) for e in (0, 1) for r in (0, 1)]

_parse = grain_pins._parse


@pytest.fixture(scope="module")
def report():
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES)
    if not os.path.exists(REPORT) or os.path.getmtime(REPORT) < newest:
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-linear"])
    return _parse(REPORT)


def test_every_kernel_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_linear.hip")).read())
    assert declared == ["linear_rgbe_kernel", "linear_pfm_kernel"]
    for k in RGBE + PFM:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(RGBE + PFM) == 12


@pytest.mark.parametrize("kernel", RGBE + PFM)
def test_no_scratch_no_spills_no_lds(report, kernel):
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    assert int(r["LDS Size"]) == 0, r
    # as built: 16 .. 38 VGPRs; 8 waves per SIMD are the most a 256-thread workgroup's kernel can have, and 64 registers still allow them
    assert int(r["VGPRs"]) <= 64, r
    assert int(r["Occupancy"]) == 8, r


def test_the_accesses_are_wide_and_nothing_is_fused(report):
    asm = open(os.path.join(ASM, "pt_linear.s")).read()
    bodies = dict(re.findall(r"^(_ZN\S*linear_(?:rgbe|pfm)_kernel\S*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M))
    assert len(bodies) == 12
    for name, body in bodies.items():
        stores = re.findall(r"\bglobal_store_\w+", body)
        assert stores and set(stores) == {"global_store_dwordx4"}, (name, stores)       # whole 16-byte groups, nothing else is written
        assert "scratch_" not in body and "buffer_" not in body and "ds_" not in body and "atomic" not in body, name
        divides = "ILb1E" in name.split("kernel")[1][:5]
        divisions = body.count("v_div_fixup_f32")
        assert (divisions >= 1) == divides, name
        assert len(re.findall(r"\bv_fma_f32|\bv_fmac_f32", body)) == 5 * divisions and "v_pk_fma_f32" not in body, name
        if "rgbe" in name:
            assert body.count("global_load_dwordx4") >= 4, name                            # 48 bytes of means, 16 of counts
        elif name.endswith("ELb1EEEvNS_10LinearArgsE"):
            assert body.count("global_load_dwordx4") >= 1, name                            # a row of whole groups: one aligned load
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("pt_linear.hip", "pt_linear.hpp"))
    for word in ("frexp", "ldexp", "logf", "log2", "logb", "__expf", "__powf", "rsqrt", "__frcp", "fmaf(", "__fdividef", "__shared__"):
        assert word not in src, word


def test_the_display_kernels_reports_are_what_their_own_tests_pin():
    """pt_display*.hip and pt_display_body.inc are not touched: made again, their reports satisfy the figures of the tests that pin them."""
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm-of-pt_display", "asm-grain"])
    plain = _parse(display_pins.USAGE)
    assert len(plain) == len(display_pins.KERNELS)
    for k in display_pins.KERNELS:
        r = next(v for name, v in plain.items() if k in name)
        assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0" and int(r["LDS Size"]) == 16384, r
        assert int(r["VGPRs"]) <= 64 and int(r["Occupancy"]) >= 8, r
    grain = _parse(grain_pins.REPORT)
    assert len(grain) == len(grain_pins.EXPECT)
    for k, (vgprs, lds, waves) in grain_pins.EXPECT.items():
        r = next(v for name, v in grain.items() if k in name)
        assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
        assert (int(r["VGPRs"]), int(r["LDS Size"]), int(r["Occupancy"])) == (vgprs, lds, waves), (k, r)
