"""The compiler's report for the display kernel (path-tracing_amd/csrc/pt_display.hip): no scratch, no spilled registers, the
table in 16 KB of LDS, full occupancy, and 12 output bytes per lane as dwords -- no byte stores."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path-tracing_amd", "csrc")
USAGE = os.path.join(ROOT, "path-tracing_amd", "lib", "asm", "display_resource_usage.txt")
SOURCE = os.path.join(CSRC, "pt_display.hip")
KERNELS = ["display_kernelILb0E", "display_kernelILb1E"]     # means as given; sums divided by the count


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
    assert declared == ["display_kernel"]
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, list(report))
    assert len(report) == len(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills(report, kernel):
    r = next(v for name, v in report.items() if kernel in name)
    assert r["ScratchSize"] == "0" and r["VGPRs Spill"] == "0" and r["SGPRs Spill"] == "0", r
    assert r["Dynamic Stack"] == "False"
    # as built: 41 VGPRs, 8 waves per SIMD -- the most a 256-thread workgroup's kernel can have here; the bound leaves the
    # register allocator some room, but not the occupancy
    assert int(r["VGPRs"]) <= 64, r
    assert int(r["Occupancy"]) >= 8, r
    # the table: 4096 floats, nothing else -- eight workgroups of it fit a compute unit's 160 KB
    assert int(r["LDS Size"]) == 16384, r


def test_output_is_dwords_and_the_table_is_searched_in_lds():
    asm = open(os.path.join(os.path.dirname(USAGE), "pt_display.s")).read()
    bodies = re.findall(r"^_ZN\S*display_kernel\S*:[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M)
    assert len(bodies) == 2, "the two instantiations' code was not found"
    for body in bodies:
        assert "global_store_byte" not in body and "global_store_short" not in body
        assert body.count("global_store_dwordx3") >= 1           # 12 bytes: four pixels
        assert body.count("global_load_dwordx4") >= 4            # 48 bytes of means, 16 of counts
        assert body.count("ds_read_b32") >= 12 * 11              # twelve channels, twelve steps each (the first reads one shared entry)
        assert "scratch_" not in body and "buffer_store" not in body
    src = open(SOURCE).read()
    for word in ("__expf", "__powf", "__logf", "rsqrt", "__frcp", "fmaf(", "__fmaf"):
        assert word not in src
