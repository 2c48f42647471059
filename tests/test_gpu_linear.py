"""The scene-linear encode kernels alone (pt_linear_encode_device_host) against the host's definition of the bytes (pt_linear_encode)
on every case of tests/linear_cases.py, both formats, with and without the exposure -- byte for byte, NaN payloads included; no pixel is
left to the host.  The shapes take every path of the launch: the RGBE kernel's full groups and its tail, the PFM kernel for rows of
whole 16-byte groups (64x1, 8x5) and the one that follows a group across the row flip (every other width), one workgroup and several."""
import importlib

import numpy as np
import pytest

import linear_cases as cases

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("exposed", [0, 1])
@pytest.mark.parametrize("fmt", ["pfm", "hdr"])
@pytest.mark.parametrize("case", list(cases.CASES))
def test_the_kernel_writes_the_hosts_bytes(case, fmt, exposed):
    assert pt.device_count() >= 1, "no HIP device: there is no CPU fallback"
    mean, count, e = cases.CASES[case]
    want = np.frombuffer(pt.linear_encode(mean, count, e, fmt, bool(exposed)), np.uint8)
    body, info = pt.linear_encode_device(0, mean, count, e, fmt, bool(exposed), want_info=True)
    got = np.frombuffer(body, np.uint8)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    print(case, fmt, exposed, "bytes", got.size, "differing", bad.size)
    assert bad.size == 0, (case, fmt, exposed, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert info["deferred_pixels"] == 0 and info["kernel_ms"] > 0
