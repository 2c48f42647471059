"""Argument checks of the display path that need no device (include/pt_hip.h: pt_display_*): NULL pointers, a scene or a
device that is none.  (A session exists only on a device, so the refusal of a band or strided session is checked in
tests/test_gpu_display.py.)"""
import ctypes as C
import importlib

import numpy as np
import pytest

pt = importlib.import_module("path-tracing_amd")
PT_ERR_NO_DEVICE = 4


def test_create_with_null_pointers():
    L = pt.lib()
    h = C.c_void_p(1234)
    assert L.pt_display_create(None, 1e-4, C.byref(h)) == pt.PT_ERR_INVALID_ARGUMENT
    assert h.value is None                      # the output is cleared before anything else
    assert L.pt_display_create(None, 1e-4, None) == pt.PT_ERR_INVALID_ARGUMENT
    h = C.c_void_p(1234)
    assert L.pt_display_create_frame(None, 1e-4, C.byref(h)) == pt.PT_ERR_INVALID_ARGUMENT
    assert h.value is None
    assert L.pt_display_create_frame(None, 1e-4, None) == pt.PT_ERR_INVALID_ARGUMENT


def test_present_reset_destroy_with_null_handle():
    L = pt.lib()
    prm = pt.DisplayParams(0.5, 0, pt.TemporalParams(), pt.DenoiseParams())
    out = np.zeros(3, np.uint8)
    assert L.pt_display_present(None, C.byref(prm), out.ctypes.data_as(C.POINTER(C.c_uint8)), None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_display_reset(None) == pt.PT_ERR_INVALID_ARGUMENT
    L.pt_display_destroy(None)                  # a no-op


def test_bytes_host_checks_its_buffers_before_the_device():
    L = pt.lib()
    m, c, out = np.zeros(3, np.float32), np.ones(1, np.int32), np.zeros(3, np.uint8)
    fp, ip, bp = pt._fp, pt._ip, lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.pt_display_bytes_host(-1, 1, 1, None, ip(c), 0.5, bp(out), None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_display_bytes_host(-1, 1, 1, fp(m), None, 0.5, bp(out), None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_display_bytes_host(-1, 1, 1, fp(m), ip(c), 0.5, None, None) == pt.PT_ERR_INVALID_ARGUMENT
    assert L.pt_display_bytes_host(-1, 0, 1, fp(m), ip(c), 0.5, bp(out), None) == pt.PT_ERR_INVALID_ARGUMENT
    for gamma in (0.0, -2.0, float("nan"), float("inf")):
        assert L.pt_display_bytes_host(-1, 1, 1, fp(m), ip(c), gamma, bp(out), None) == pt.PT_ERR_INVALID_ARGUMENT


def test_bytes_host_without_a_device_is_no_device():
    with pytest.raises(pt.PtError) as e:
        pt.display_bytes(np.zeros((2, 2, 3), np.float32), np.ones(4, np.int32), device=-1)
    assert e.value.status == PT_ERR_NO_DEVICE


def test_a_host_only_scene_has_no_session_to_display(models_dir):
    """pt_display_create takes a session, and a host-only scene gives none: the refusal is PT_ERR_NO_DEVICE at that step."""
    scene = pt.Scene.load_obj(models_dir, "Tor.obj", device=-1)
    with pytest.raises(pt.PtError) as e:
        pt.Session(scene, 8, 8)
    assert e.value.status == PT_ERR_NO_DEVICE


def test_abi_symbols_include_the_display_path():
    for name in ("pt_display_create", "pt_display_create_frame", "pt_display_present", "pt_display_reset", "pt_display_destroy",
                 "pt_display_bytes_host", "pt_display_table"):
        assert name in pt.ABI_SYMBOLS
        getattr(pt.lib(), name)
    assert C.sizeof(pt.DisplayParams) == 4 + 4 + 12 + 20 and C.sizeof(pt.DisplayInfo) == 16
