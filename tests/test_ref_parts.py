"""The parts of the reference that build here, against what restates them.

The reference as a whole needs GLM and cannot be compiled in this image; two of its files need nothing: bitmap_image.hpp and
config.h.  `make -C oracle ref` compiles those from the reference's sources where they lie (oracle/ref_parts_main.cpp is the
driver, the output oracle/_ref/ref_parts; __graft_entry__.build() runs it).  With it, three rows of the path stop resting on a
reading of the source alone:

  * the BMP the reference writes (main.cpp:107, 150-156, 197-201: bitmap_image(W, H), clear, set_pixel, save_image) -- the
    oracle's writer and the product's pt_write_bmp produce the same FILE, byte for byte;
  * the skybox the reference reads (scene.cpp:21-23, 136-139: bitmap_image(path), get_pixel(x, y).red/green/blue) -- the numpy
    reader of tests/reference_restatements.py (which tests/test_double_entry.py ties to the oracle's lookup) sees the same texels
    in the same places;
  * the flags the reference parses (config.h:35-99) -- the product's front end (tools/pt_render.cpp) ends up with the same fields,
    for well-formed command lines and for the odd ones (a value-less last flag, a flag in a value's position, -GAUSS / -MEDIAN
    cancelling each other in command-line order).

What ref_parts answered for every case below is stored in tests/golden/ref_parts_vectors.npz (tests/golden/
make_ref_parts_vectors.py): where oracle/_ref/ref_parts exists it is run and must still give those answers; where it does not
(a tree that never saw the reference's sources) the stored answers stand in for it."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import reference_restatements as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "ref_parts")
VECTORS = os.path.join(ROOT, "tests", "golden", "ref_parts_vectors.npz")
BMP_SIZES = [(1, 1), (2, 3), (3, 2), (5, 7), (64, 48), (250, 131)]
SKY_SIZES = [(1, 1), (4, 2), (5, 3), (7, 200), (64, 32)]


@functools.lru_cache(maxsize=None)
def stored():
    with np.load(VECTORS) as f:
        return {k: f[k] for k in f.files}


def live():
    return os.path.exists(REF)


def bmp_input(W, H):
    """W x H x 3 bytes (r, g, b) from the top row; the stored input of the case (the generator draws it from this seed)."""
    return np.random.default_rng(W * 1000 + H).integers(0, 256, (H, W, 3)).astype(np.uint8)


def sky_input(W, H):
    return np.random.default_rng(W * 77 + H).integers(0, 256, (H, W, 3)).astype(np.uint8)


def ref_bmpwrite(rgb, tmp_path):
    H, W = rgb.shape[:2]
    raw, out = str(tmp_path / "in.rgb"), str(tmp_path / "ref.bmp")
    rgb.tofile(raw)
    subprocess.run([REF, "bmpwrite", str(W), str(H), raw, out], check=True)
    return np.fromfile(out, np.uint8)


def ref_bmpread(bmp, tmp_path):
    """(dims the reference printed, texels as get_pixel(x, y) gives them: [y, x] = red, green, blue)."""
    out = str(tmp_path / "sky.rgb")
    r = subprocess.run([REF, "bmpread", bmp, out], check=True, capture_output=True, text=True)
    W, H = (int(x) for x in r.stdout.split())
    return np.array([W, H], np.int32), np.fromfile(out, np.uint8).reshape(H, W, 3)


def ref_config(flags):
    return subprocess.run([REF, "config"] + flags, check=True, capture_output=True, text=True).stdout


@pytest.mark.parametrize("W,H", BMP_SIZES)
def test_bmp_writers_against_the_references(tmp_path, W, H):
    import importlib
    pt = importlib.import_module("path-tracing_amd")
    rgb = stored()[f"bmpwrite_{W}x{H}_in"]
    want = stored()[f"bmpwrite_{W}x{H}"].tobytes()
    if live():
        assert ref_bmpwrite(rgb, tmp_path).tobytes() == want
    orc_bmp, prod_bmp = (str(tmp_path / n) for n in ("orc.bmp", "prod.bmp"))
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    O.write_bmp(orc_bmp, bgr)
    pt.write_bmp(prod_bmp, bgr)
    assert len(want) == 54 + H * ((3 * W + 3) // 4 * 4)
    assert open(orc_bmp, "rb").read() == want
    assert open(prod_bmp, "rb").read() == want


@pytest.mark.parametrize("W,H", SKY_SIZES)
def test_skybox_texels_as_the_reference_reads_them(tmp_path, W, H):
    bgr = stored()[f"bmpread_{W}x{H}_in"]
    bmp = str(tmp_path / "sky.bmp")
    O.write_bmp(bmp, bgr)
    dims, ref = stored()[f"bmpread_{W}x{H}_dims"], stored()[f"bmpread_{W}x{H}"]
    if live():
        d, r = ref_bmpread(bmp, tmp_path)
        assert np.array_equal(d, dims) and np.array_equal(r, ref)
    assert list(dims) == [W, H]
    mine = N.load_bmp_top_down(bmp)                                     # [y, x] = blue, green, red
    assert np.array_equal(ref, mine[:, :, ::-1])
    assert np.array_equal(ref, bgr[:, :, ::-1])                         # and row 0 is the image's top row, as written


CASES = [
    [],
    ["--W", "640", "--H", "360", "-RPP", "64", "-MRR", "5", "-EPS", "0.001", "-ERR", "-1", "-SEED", "7"],
    ["-GAUSS", "2", "-MEDIAN", "3"],                # the later one wins and zeroes the other
    ["-MEDIAN", "3", "-GAUSS", "2"],
    ["-GAMMA", "0.5", "-UPDATE", "0", "-TL", "9", "-SKYBOX", "sky.bmp", "-MODEL_PATH", "m/", "-MODEL_NAME", "x.obj"],
    ["--W", "100", "-SEED"],                        # a flag without its value at the end: never looked at
    ["junk", "--W", "100", "-RPP", "3"],            # one stray word shifts every flag into a value's position
    ["--W", "abc", "-RPP", "12x", "-EPS", "1e-3f", "-ERR", ".5."],      # atoi / atof of malformed numbers
    ["-SEED", "-5"],                                # negative seed: the clock (only checked to differ from 42 and be plausible)
    ["--W", "7", "--W", "9", "-ERR", "1e-40", "-EPS", "1e39"],         # repeated flag, a denormal and an overflow through float
    ["-seed", "9", "-W", "3", "--h", "4"],          # flags are case- and dash-sensitive
]


def _fields(text):
    return dict(l.split(" ", 1) if " " in l else (l, "") for l in text.strip().split("\n"))


@pytest.mark.parametrize("flags", CASES, ids=[" ".join(c) or "(none)" for c in CASES])
def test_flag_parsers_agree(flags):
    exe = os.path.join(ROOT, "path-tracing_amd", "bin", "pt_render")
    if not os.path.exists(exe):
        pytest.skip("path-tracing_amd/bin/pt_render not built")
    clock_seed = "-SEED" in flags and flags[flags.index("-SEED") + 1:][:1] == ["-5"]
    a = _fields(str(stored()[f"config_{CASES.index(flags)}"]))
    if live():
        r = _fields(ref_config(flags))
        unclocked = lambda d: {k: v for k, v in d.items() if not (clock_seed and k == "seed")}
        assert unclocked(r) == unclocked(a), (flags, r, a)      # the stored answer is still the reference's
        a = r
    mine = subprocess.run([exe] + flags, check=True, capture_output=True, text=True, env=dict(os.environ, PT_RENDER_PRINT_CONFIG="1")).stdout
    b = _fields(mine)
    assert set(a) == set(b) and len(a) == 15
    if clock_seed:
        sa, sb = int(a.pop("seed")), int(b.pop("seed"))
        assert sb > 10 ** 9                             # time(nullptr)
        if live():
            assert abs(sa - sb) <= 2                    # read a moment apart
    assert a == b, (flags, a, b)
