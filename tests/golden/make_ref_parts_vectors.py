#!/usr/bin/env python3
"""Generates tests/golden/ref_parts_vectors.npz: what oracle/_ref/ref_parts (the reference's bitmap_image.hpp and config.h,
built by `make -C oracle ref`) answers for every case of tests/test_ref_parts.py, so that the test also runs where the
reference's sources are not at hand.

    make -C oracle ref && python tests/golden/make_ref_parts_vectors.py

Keys:  bmpwrite_<W>x<H>_in   the r, g, b input bytes [H, W, 3]      bmpwrite_<W>x<H>        the BMP file the reference writes
       bmpread_<W>x<H>_in    the b, g, r image the oracle writes     bmpread_<W>x<H>(_dims)  the texels (and W, H) the reference reads
       config_<i>            what the reference's parser prints for CASES[i] (one "name value" line per field)
"""
import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import test_ref_parts as T  # noqa: E402


def main():
    if not T.live():
        raise SystemExit(f"{T.REF} is missing: run `make -C oracle ref` where the reference's sources are")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        tmp = pathlib.Path(td)
        for W, H in T.BMP_SIZES:
            rgb = T.bmp_input(W, H)
            out[f"bmpwrite_{W}x{H}_in"] = rgb
            out[f"bmpwrite_{W}x{H}"] = T.ref_bmpwrite(rgb, tmp)
        for W, H in T.SKY_SIZES:
            bgr = T.sky_input(W, H)
            bmp = str(tmp / "sky.bmp")
            O.write_bmp(bmp, bgr)
            out[f"bmpread_{W}x{H}_in"] = bgr
            out[f"bmpread_{W}x{H}_dims"], out[f"bmpread_{W}x{H}"] = T.ref_bmpread(bmp, tmp)
    for i, flags in enumerate(T.CASES):
        out[f"config_{i}"] = np.array(T.ref_config(flags))
    np.savez_compressed(T.VECTORS, **out)
    print(f"{T.VECTORS}: {len(out)} arrays, {os.path.getsize(T.VECTORS)} bytes")


if __name__ == "__main__":
    main()
