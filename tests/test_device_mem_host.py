"""pt_device_mem.hpp -- the owners of device memory, events and streams and the plane layout of the host layer -- on the CPU:
built with g++ -fsanitize=address,undefined against the HIP headers, the HIP calls stubbed (tests/native/device_mem_main.cpp).
Pins the allocation sizes the layout gives to the expressions the host layer used to write out by hand, and that an owner frees
exactly once, never when it is empty, and holds nothing after a failed allocation.  The same program pins bloom's and local
exposure's views to the offsets their two users each wrote out by hand, and the timed region of pt_capi_internal.hpp to two
event records around its callable on the stream given, one wait, and events that go with the call whether the callable fails or not."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="g++ or the HIP headers are not available")
def test_plane_layout_and_owners_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "device_mem")
    csrc = os.path.join(ROOT, "path-tracing_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", "/opt/rocm/include",
                            os.path.join(ROOT, "tests", "native", "device_mem_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert "device mem ok" in run.stdout
