"""The compiler's report for the bloom kernels (path-tracing_amd/csrc/pt_bloom.hip): no scratch, no spilled registers, no dynamic
stack; registers, LDS and occupancy as built; every tap of a pyramid level one load, every record one 16-byte store; nothing fused outside the IEEE
division, and no fast-math spelling in the sources."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
ASM = os.path.join(ROOT, "path-tracing_amd", "lib", "asm")
REPORT = os.path.join(ASM, "bloom_resource_usage.txt")
LISTING = os.path.join(ASM, "pt_bloom.s")
SOURCES = ["pt_bloom.hip", "pt_bloom.hpp", "pt_grade.hpp"]
# kernel<FIRST / LAST, DIVIDE> -> (VGPRs as built, LDS bytes, waves per SIMD)
EXPECT = {"bloom_down_kernelILb0ELb0EE": (40, 9216, 8), "bloom_down_kernelILb1ELb0EE": (35, 9216, 8), "bloom_down_kernelILb1ELb1EE": (46, 9216, 8),
          "bloom_up_kernelILb0ELb0EE": (16, 3072, 8), "bloom_up_kernelILb1ELb0EE": (15, 3072, 8), "bloom_up_kernelILb1ELb1EE": (15, 3072, 8)}
DIVIDES = {"bloom_down_kernelILb1ELb0EE", "bloom_down_kernelILb1ELb1EE", "bloom_up_kernelILb1ELb1EE"}      # T / e, (l - t) / l, sum / n


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
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm-bloom"])
    return _parse(REPORT)


def test_every_kernel_is_reported(report):
    declared = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", open(os.path.join(CSRC, "pt_bloom.hip")).read())
    assert declared == ["bloom_down_kernel", "bloom_up_kernel"]
    for k in EXPECT:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(EXPECT)


@pytest.mark.parametrize("kernel", list(EXPECT))
def test_no_scratch_no_spills_and_the_resources_as_built(report, kernel):
    vgprs, lds, waves = EXPECT[kernel]
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    assert int(r["VGPRs"]) == vgprs, r
    assert int(r["LDS Size"]) == lds, r            # 32 x 18 and 32 x 6 records of 16 bytes
    assert int(r["Occupancy"]) == waves, r         # 8: the most a 256-thread workgroup's kernel can have


def test_taps_are_16_byte_accesses_and_nothing_is_fused(report):
    asm = open(LISTING).read()
    bodies = {k: re.findall(r"^_ZN\S*%s\S*:[^\n]*\n(.*?)s_endpgm" % k, asm, re.S | re.M) for k in EXPECT}
    for k, found in bodies.items():
        assert len(found) == 1, k
        body = found[0]
        assert "scratch_" not in body and "atomic" not in body, k
        assert "ds_write_b128" in body and "ds_write_b32" not in body, k
        assert ("ds_read_b128" in body or "ds_read_b96" in body) and "ds_read_b32" not in body and "ds_read2_b32" not in body, k
        if k in DIVIDES:                                          # fused only inside the IEEE division
            assert "v_div_scale_f32" in body and "v_div_fixup_f32" in body, k
            fused = len(re.findall(r"\bv_fmac?_f32", body))
            assert fused == 5 * body.count("v_div_fmas_f32"), (k, fused)      # the division's own five, and no other
        else:
            assert "v_fma" not in body and "v_mad_f32" not in body and "v_div_" not in body, k
        assert {"bloom_down_kernelILb1ELb0EE": 5, "bloom_down_kernelILb1ELb1EE": 17, "bloom_up_kernelILb1ELb1EE": 3}.get(k, 0) == \
            body.count("v_div_fmas_f32"), k                           # T / e, four taps' (l - t) / l, and sum / n per channel
        assert "v_rcp_f32" not in body.replace("v_rcp_f32_e32 v", "", 5 * body.count("v_div_fmas_f32")) or k in DIVIDES, k
        assert "v_mac_f32" not in body and "v_pk_fma" not in body, k      # (v_rcp_iflag is the integer tile index's)
    # a pyramid level is read and written record by record: one load per tap (the compiler may leave out the record's zero), one store
    wide = lambda k: len(re.findall(r"global_load_dwordx[34]\b", bodies[k][0]))
    assert wide("bloom_down_kernelILb0ELb0EE") == 4 and wide("bloom_up_kernelILb0ELb0EE") == 3
    for k in ("bloom_down_kernelILb0ELb0EE", "bloom_up_kernelILb0ELb0EE"):
        assert not re.search(r"global_load_dword(x2)?\b", bodies[k][0]), k
    assert all(bodies[k][0].count("global_store_dwordx4") == 1 for k in EXPECT if "down" in k or k == "bloom_up_kernelILb0ELb0EE")
    src = "".join(open(os.path.join(CSRC, f)).read() for f in SOURCES)
    for word in ("__expf", "__powf", "__logf", "rsqrt", "__frcp", "fmaf(", "__fmaf", "__fdividef"):
        assert word not in src
