"""Colour grading on the host (include/pt_hip.h: pt_colour_matrix, pt_colour_host, pt_lut_*): the host stage against the numpy
restatement bit for bit on every case and curve, the exact properties the header states, the matrix against float64 numpy, the
.cube reader's accepted forms and refusals, the argument checks before any device, the deferral cap of the GPU test's inputs,
and the reader and the stage under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import colour_cases as K
import colour_restatement as R
import grade_restatement as G

pt = importlib.import_module("path-tracing_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EXPOSURES = [F(0.6), F(1.0), F(2.5)]


def _same(got, want, where):
    """Bit for bit; a NaN's payload is free, but only where the restatement says NaN too."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), where
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _params(mat, lut):
    return dict(mat, lut=pt.Lut.create(lut) if lut is not None else None)


@pytest.mark.parametrize("name", list(K.CASES))
def test_host_stage_equals_the_restatement(name):
    m, c, M, lut, mat = K.build(name)
    _same(pt.colour_matrix(**mat), M, (name, "matrix"))
    prm = _params(mat, lut)
    for curve in G.CURVES:
        for e in EXPOSURES:
            _same(pt.colour(m, c, e, curve, prm), R.colour(m, c, e, curve, M, lut), (name, curve, e))


@pytest.mark.parametrize("name", [n for n in K.CASES if n not in K.PLANTED])
def test_the_gpu_tests_inputs_defer_at_most_one_per_cent(name):
    """tests/test_gpu_colour.py demands that the kernel defers exactly the predicted pixels; the prediction itself must stay small,
    or a kernel that deferred everything would pass.  Checked here for the manual exposures it uses."""
    m, c, M, lut, _ = K.build(name)
    for gamma in K.GAMMAS:
        table = pt.display_table(gamma)
        for curve in G.CURVES:
            n = K.predict_deferred(R.colour(m, c, F(1.25), curve, M, lut), c, table)
            assert n <= K.DEFER_CAP * c.size, (name, curve, gamma, n, c.size)


def test_constant_lut_gives_its_constant_and_vertices_are_exact():
    rng = np.random.default_rng(3)
    g = np.concatenate([rng.uniform(-0.5, 1.5, (500, 3)), [[np.nan, 0.5, np.inf], [0, 0, 0], [1, 1, 1], [-0.0, 1, 0.5]]]).astype(F)[None]
    c = np.ones((1, g.shape[1]), np.int32)
    for n in K.LUT_SIZES:
        out = pt.colour(g, c, 1.0, "reference", dict(lut=pt.Lut.create(K.lut("constant", n))))
        assert np.array_equal(out.view(np.uint32), np.broadcast_to(K.CONSTANT, out.shape).view(np.uint32)), n
        table = K.lut("random", n)
        idx = rng.integers(0, n - 1, (400, 3))                       # (the last index is reached with f = 1, from the cell below it)
        at = (idx / F(n - 1)).astype(F)[None]
        assert (R.axis(at[0], n)[1] == 0).all()                       # N - 1 is a power of two here: (float)(k / (N - 1)) * (N - 1) is k again
        out = pt.colour(at, np.ones((1, 400), np.int32), 1.0, "reference", dict(lut=pt.Lut.create(table)))[0]
        assert np.array_equal(out.view(np.uint32), table[idx[:, 2], idx[:, 1], idx[:, 0]].view(np.uint32)), n
        # the last vertex is reached from the cell below it, with f = 1 exactly
        assert R.axis(F(1), n) == (n - 2, F(1))


def test_every_tetrahedron_and_every_tie_has_the_headers_answer():
    """A LUT of one cell whose vertices are powers of two apart tells the paths apart; fractions from {0, 1/4, 1/2, 1} in every
    combination visit the six tetrahedra and all ties."""
    lut = (2.0 ** np.arange(24).reshape(2, 2, 2, 3)).astype(F)
    vals = np.array([0, 0.25, 0.5, 1], F)
    g = np.stack(np.meshgrid(vals, vals, vals, indexing="ij"), -1).reshape(1, -1, 3)
    out = pt.colour(g, np.ones((1, g.shape[1]), np.int32), 1.0, "reference", dict(lut=pt.Lut.create(lut)))
    _same(out, R.lut_apply(lut, g), "paths")
    seen = set(R.path_index(g[0, :, 0], g[0, :, 1], g[0, :, 2]).tolist())
    assert seen == set(range(6))
    # the table itself, spelled out: r >= g >= b -> r,g,b; ties go to the first row that holds
    assert R.PATHS[int(R.path_index(F(0.5), F(0.5), F(0.5)))] == (0, 1, 2)
    assert R.PATHS[int(R.path_index(F(0.5), F(0.25), F(0.5)))] == (0, 2, 1)
    assert R.PATHS[int(R.path_index(F(0.25), F(0.5), F(0.5)))] == (1, 2, 0)
    assert R.PATHS[int(R.path_index(F(0.25), F(0.5), F(0.25)))] == (1, 0, 2)


def test_a_zeroed_struct_is_pt_grade_host():
    m, c = K.image("planted", 64, 48)
    for curve in G.CURVES:
        for prm in (None, pt.ColourParams(), dict(), dict(wb=(1, 1, 1), saturation=1.0, matrix=np.eye(3)), dict(wb=(0, 0, 0))):
            _same(pt.colour(m, c, 0.7, curve, prm), pt.grade(m, c, 0.7, curve), (curve, str(prm)))
    # the identity is skipped, not multiplied through: an infinite channel does not turn its neighbours into NaN
    one = np.array([[[np.inf, 1.0, 2.0]]], F)
    assert np.array_equal(pt.colour(one, np.ones((1, 1), np.int32), 1.0, "reference", dict(saturation=1.0)), one)


def test_matrix_against_float64_numpy_and_its_special_values():
    rng = np.random.default_rng(11)
    lum = np.array(R.LUM)
    for _ in range(50):
        wb, s, U = rng.uniform(0.2, 3.0, 3).astype(F), F(rng.uniform(0, 2)), rng.uniform(-1, 2, (3, 3)).astype(F)
        want = U.astype(np.float64) @ (float(s) * np.eye(3) + (1 - float(s)) * np.outer(np.ones(3), lum)) @ np.diag(wb.astype(np.float64))
        got = pt.colour_matrix(wb, s, U)
        assert got.dtype == F and np.all(np.abs(got - want) <= np.spacing(np.abs(want).astype(F))), (got, want)      # one rounding, of a sum whose order is free
        assert np.array_equal(got.view(np.uint32), R.compose(wb, s, U).view(np.uint32))
    assert R.is_identity(pt.colour_matrix()) and R.is_identity(pt.colour_matrix((1, 1, 1), 1.0)) and R.is_identity(pt.colour_matrix(None, None, np.eye(3)))
    grey = pt.colour_matrix(None, 0.0)
    assert np.array_equal(grey, np.broadcast_to(np.array(R.LUM, F), (3, 3)))
    m, c = K.image("random", 7, 5)
    out = pt.colour(m, c, 1.0, "aces", dict(saturation=0.0))[c != 0]
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 1], out[:, 2])
    # saturation 0 without saturation_set is "not set"
    raw, out9 = pt.ColourParams(), np.zeros(9, F)
    assert pt.lib().pt_colour_matrix(C.byref(raw), out9.ctypes.data_as(C.POINTER(C.c_float))) == pt.PT_OK and R.is_identity(out9.reshape(3, 3))
    raw.saturation_set = 1
    assert pt.lib().pt_colour_matrix(C.byref(raw), out9.ctypes.data_as(C.POINTER(C.c_float))) == pt.PT_OK
    assert np.array_equal(out9.reshape(3, 3), grey)


def _status(call):
    with pytest.raises(pt.PtError) as e:
        call()
    return e.value.status, str(e.value)


def test_bad_parameters_are_refused():
    m, c = K.image("random", 7, 5)
    for prm in (dict(wb=(1, -1, 1)), dict(wb=(1, np.nan, 1)), dict(saturation=-0.5), dict(saturation=np.inf), dict(matrix=[[1, 0, 0], [0, np.nan, 0], [0, 0, 1]])):
        assert _status(lambda: pt.colour(m, c, 1.0, "clamp", prm))[0] == pt.PT_ERR_INVALID_ARGUMENT, prm
        assert _status(lambda: pt.colour_matrix(**prm))[0] == pt.PT_ERR_INVALID_ARGUMENT, prm
    for e, curve in ((0.0, 0), (np.nan, 0), (1.0, 9)):
        assert _status(lambda: pt.colour(m, c, e, curve, dict(saturation=0.5)))[0] == pt.PT_ERR_INVALID_ARGUMENT
    assert _status(lambda: pt.Lut.create(np.zeros((1, 1, 1, 3), F)))[0] == pt.PT_ERR_UNSUPPORTED
    assert _status(lambda: pt.Lut.create(np.zeros((66, 66, 66, 3), F)))[0] == pt.PT_ERR_UNSUPPORTED
    bad = K.lut("identity", 3)
    bad[1, 1, 1, 1] = np.nan
    assert _status(lambda: pt.Lut.create(bad))[0] == pt.PT_ERR_INVALID_ARGUMENT
    assert pt.Lut.create(K.lut("identity", 65)).size == 65


@pytest.mark.skipif(pt.device_count() > 0, reason="the order of the checks shows only where there is no device")
def test_arguments_are_checked_before_a_device_is_looked_at():
    m, c = K.image("random", 7, 5)
    lut = pt.Lut.create(K.lut("random", 3))
    assert _status(lambda: pt.display_bytes_colour(m, c, dict(curve="aces"), dict(wb=(1, -1, 1), lut=lut)))[0] == pt.PT_ERR_INVALID_ARGUMENT
    assert _status(lambda: pt.display_bytes_colour(m, c, dict(curve=7), dict(lut=lut)))[0] == pt.PT_ERR_INVALID_ARGUMENT
    assert _status(lambda: pt.display_bytes_colour(m, c, dict(curve="aces"), dict(lut=lut), gamma=-1.0))[0] == pt.PT_ERR_INVALID_ARGUMENT
    assert _status(lambda: pt.display_bytes_colour(m, c, dict(curve="aces"), dict(lut=lut)))[0] == 4          # PT_ERR_NO_DEVICE: only now


def _load(path):
    """(status, handle value or the sentinel the call must leave alone)."""
    L = pt.lib()
    h = C.c_void_p(0xdead0)
    rc = L.pt_lut_load_cube(os.fsencode(str(path)), C.byref(h))
    if rc == pt.PT_OK:
        L.pt_lut_destroy(h)
    return rc, h.value, L.pt_last_error().decode()


def test_cube_reader_accepts_what_the_header_lists(tmp_path):
    table = K.lut("wide", 5)
    forms = [dict(), dict(title="a look", comment="made by the suite"), dict(domain=False), dict(newline="\r\n", title="crlf")]
    for k, form in enumerate(forms):
        path = tmp_path / ("ok%d.cube" % k)
        R.write_cube(path, table, **form)
        assert np.array_equal(R.read_cube(path).view(np.uint32), table.view(np.uint32))
        lut = pt.Lut.load_cube(path)
        assert lut.size == 5
        g = np.random.default_rng(k).uniform(0, 1, (1, 300, 3)).astype(F)
        c = np.ones((1, 300), np.int32)
        _same(pt.colour(g, c, 1.0, "reference", dict(lut=lut)), pt.colour(g, c, 1.0, "reference", dict(lut=pt.Lut.create(table))), form)
    # leading blank space, tabs, exponents, a comment between data lines, no newline at the end
    path = tmp_path / "loose.cube"
    path.write_text("  # c\n\tLUT_3D_SIZE\t2\n" + "".join("  %d\t%de0 0.5\n# mid\n" % (i & 1, (i >> 1) & 1) for i in range(7)) + "1 1 5e-1")
    assert _load(path)[0] == pt.PT_OK


def test_cube_reader_refuses_with_the_status_the_header_states(tmp_path):
    data = lambda n: "".join("0.5 0.25 1\n" for _ in range(n))
    bad = {
        "LUT_1D_SIZE 4\n" + data(4): (pt.PT_ERR_UNSUPPORTED, "line 1"),
        "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0.1\n" + data(8): (pt.PT_ERR_UNSUPPORTED, "line 2"),
        "LUT_3D_SIZE 2\nDOMAIN_MAX 2 2 2\n" + data(8): (pt.PT_ERR_UNSUPPORTED, "line 2"),
        "LUT_3D_SIZE 1\n" + data(1): (pt.PT_ERR_UNSUPPORTED, "line 1"),
        "# big\nLUT_3D_SIZE 66\n": (pt.PT_ERR_UNSUPPORTED, "line 2"),
        "LUT_3D_SIZE 2\n" + data(7): (pt.PT_ERR_INVALID_ARGUMENT, "7 data lines"),
        "LUT_3D_SIZE 2\n" + data(9): (pt.PT_ERR_INVALID_ARGUMENT, "line 10"),
        "LUT_3D_SIZE 2\n" + data(3) + "0.5 zero 1\n" + data(4): (pt.PT_ERR_INVALID_ARGUMENT, "line 5"),
        "LUT_3D_SIZE 2\n" + data(3) + "0.5 0.5\n" + data(4): (pt.PT_ERR_INVALID_ARGUMENT, "line 5"),
        "LUT_3D_SIZE 2\n" + data(3) + "0.5 0.5 1 1\n" + data(4): (pt.PT_ERR_INVALID_ARGUMENT, "line 5"),
        "LUT_3D_SIZE 2\n" + data(2) + "0.5 nan 1\n" + data(5): (pt.PT_ERR_INVALID_ARGUMENT, "line 4"),
        "LUT_3D_SIZE 2\n" + data(2) + "inf 0 1\n" + data(5): (pt.PT_ERR_INVALID_ARGUMENT, "line 4"),
        "LUT_3D_SIZE 2\n" + data(2) + "1e99 0 1\n" + data(5): (pt.PT_ERR_INVALID_ARGUMENT, "line 4"),
        "TITLE \"none\"\n" + data(8): (pt.PT_ERR_INVALID_ARGUMENT, "line 2"),
        "TITLE \"none\"\n\n": (pt.PT_ERR_INVALID_ARGUMENT, "LUT_3D_SIZE"),
        "LUT_3D_SIZE two\n" + data(8): (pt.PT_ERR_INVALID_ARGUMENT, "line 1"),
        "LUT_3D_SIZE 2.5\n" + data(8): (pt.PT_ERR_INVALID_ARGUMENT, "line 1"),
        "LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0 1\n" + data(8): (pt.PT_ERR_INVALID_ARGUMENT, "line 2"),
        "": (pt.PT_ERR_INVALID_ARGUMENT, "LUT_3D_SIZE"),
    }
    for k, (text, (status, word)) in enumerate(bad.items()):
        path = tmp_path / ("bad%d.cube" % k)
        path.write_text(text)
        rc, handle, message = _load(path)
        assert rc == status and handle == 0xdead0 and word in message and str(path) in message, (text[:40], rc, message)
    rc, handle, message = _load(tmp_path / "missing.cube")
    assert rc == 2 and handle == 0xdead0 and "missing.cube" in message          # PT_ERR_IO, as a missing skybox file gives


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"), reason="g++ or the HIP headers are not available")
def test_reader_and_host_stage_are_clean_under_asan_and_ubsan(tmp_path):
    """pt_colour_capi.cpp alone with a stand-alone main: malformed files, a maximal file (N = 65), and the stage on values that
    push every index to its end.  Host code only, run as a program of its own."""
    exe = str(tmp_path / "colour_san")
    csrc = os.path.join(ROOT, "path-tracing_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                            os.path.join(ROOT, "tests", "native", "colour_sanitizer_main.cpp"), os.path.join(csrc, "pt_colour_capi.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe, str(tmp_path) + "/"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert "colour host ok" in run.stdout
