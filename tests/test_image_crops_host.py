"""The crop argument tests/test_gpu_image_kernels.py rests on, checked on the CPU against the uncropped references: a local
operation's result inside a box equals the reference's result on the box padded by the operation's reach, cut at the image's
borders -- for boxes at corners, on edges and in the interior -- and does NOT if the padding is one pixel short or if a crop is cut
just inside a border it should have kept.  Also: the content generators keep -0.0 and NaN out, and the window list covers what
it says; and the mutation table of tools/mutate_image_kernels.py still applies to the sources as they are."""
import os
import sys

import numpy as np
import pytest

import denoise_restatement as R
import image_kernel_cases as K
import oracle_lib as O


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _boxes(W, H, cw, ch):
    return K.windows(W, H, cw, ch, tile_w=8, tile_h=8)


@pytest.mark.parametrize("gauss,median", [(1, 0), (2, 0), (0, 1), (0, 4)])
def test_filter_crops_equal_the_whole(gauss, median):
    W, H = 61, 47
    img = K.image("dense", W, H, seed=11)
    op = (lambda a: O.gauss_blur(a, gauss)) if gauss else (lambda a: O.median_filter(a, median))
    whole = op(img)
    reach = K.gauss_reach(gauss) if gauss else median
    short = 0
    for name, (x0, y0, x1, y1) in _boxes(W, H, 12, 10).items():
        part = K.crop_reference([img], (x0, y0, x1, y1), reach, lambda crops, w, h: op(crops[0]))
        assert np.array_equal(_bits(part), _bits(whole[y0:y1, x0:x1])), name
        less = K.crop_reference([img], (x0, y0, x1, y1), reach - 1, lambda crops, w, h: op(crops[0]))
        short += not np.array_equal(_bits(less), _bits(whole[y0:y1, x0:x1]))
    assert short > 0, "a padding one pixel short went unnoticed: the reach is overstated or the content too smooth"


def test_a_crop_must_keep_the_border_it_touches():
    """Cutting three pixels inside the image's left border clamps to the wrong column."""
    W, H = 40, 30
    img = K.image("dense", W, H, seed=12)
    whole = O.gauss_blur(img, 2)
    cut = O.gauss_blur(np.ascontiguousarray(img[:, 3:]), 2)
    assert not np.array_equal(cut[:, :4], whole[:, 3:7])
    kept = K.crop_reference([img], (0, 0, 7, H), K.gauss_reach(2), lambda crops, w, h: O.gauss_blur(crops[0], 2))
    assert np.array_equal(_bits(kept), _bits(whole[:, 0:7]))


@pytest.mark.parametrize("levels", [1, 3])
def test_denoise_crops_equal_the_whole(levels):
    W, H = 90, 70
    inputs = K.denoise_inputs(W, H, seed=levels, hit="blocks", normal="discrete", position="coplanar", albedo="materials")
    with np.errstate(all="ignore"):
        mean, count = R.denoise(W, H, *inputs, levels=levels)
    mean, count = mean.reshape(H, W, 3), count.reshape(H, W)
    reach = K.denoise_reach(levels)
    assert reach == 3 + 2 * sum(1 << i for i in range(levels)) and K.denoise_reach(5) == 65
    fn = K.denoise_from_planes(R.denoise, levels=levels)
    for name, (x0, y0, x1, y1) in _boxes(W, H, 14, 12).items():
        with np.errstate(all="ignore"):
            pm, pc = K.crop_reference(K.denoise_planes(W, H, *inputs), (x0, y0, x1, y1), reach, fn)
        assert np.array_equal(pc, count[y0:y1, x0:x1]), name
        assert np.array_equal(_bits(pm), _bits(mean[y0:y1, x0:x1])), name
    # the bound is not idle: a padding one pixel short of the colour taps' reach alone (the outermost 3 pixels only carry variances,
    # whose trace in the result can vanish in rounding) changes the interior -- on an all-miss image, where no feature weight is 0
    inputs = K.denoise_inputs(W, H, seed=levels, hit="none", count="sampled")
    with np.errstate(all="ignore"):
        mean = R.denoise(W, H, *inputs, levels=levels)[0].reshape(H, W, 3)
        x0, y0, x1, y1 = _boxes(W, H, 14, 12)["seam"]
        pm, _ = K.crop_reference(K.denoise_planes(W, H, *inputs), (x0, y0, x1, y1), reach, fn)
        lm, _ = K.crop_reference(K.denoise_planes(W, H, *inputs), (x0, y0, x1, y1), reach - K.DENOISE_REACH_VARIANCE - 1, fn)
    assert np.array_equal(_bits(pm), _bits(mean[y0:y1, x0:x1]))
    assert not np.array_equal(_bits(lm), _bits(mean[y0:y1, x0:x1])), "a padding short of the colour taps went unnoticed"


def test_windows_cover_corners_edges_seam_and_last_row():
    W, H = 1920, 1080
    b = K.windows(W, H, 24, 24)
    assert len(set(b.values())) == 10
    assert b["top_left"][:2] == (0, 0) and b["bottom_right"][2:] == (W, H) and b["top_right"][2] == W and b["bottom_left"][3] == H
    x0, y0, x1, y1 = b["seam"]
    assert x0 < 960 < x1 and y0 < 528 < y1 and 960 % 16 == 0 and 528 % 16 == 0 and x0 > 100 and y0 > 100 and x1 < W - 100 and y1 < H - 100
    x0, y0, x1, y1 = b["last_row"]
    assert y0 < 1072 < y1 == H and 1080 == 67 * 16 + 8
    for x0, y0, x1, y1 in K.windows(W, H, 16, 16, tile_w=32, tile_h=8).values():
        assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H


def test_content_is_free_of_negative_zero_and_nan():
    kinds = list(K.CONTENT) + list(K.MEDIAN_ONLY_CONTENT) + ["pos_inf_lines"]
    for kind in kinds:
        for W, H in K.GRID:
            img = K.image(kind, W, H)
            assert img.shape == (H, W, 3) and img.dtype == np.float32
            assert not np.isnan(img).any() and not (np.signbit(img) & (img == 0)).any()
            assert np.array_equal(img, K.image(kind, W, H))          # fixed seeds
    assert (K.image("signed", 33, 31) < 0).any() and np.isinf(K.image("inf_lines", 33, 31)).any()
    assert K.image("huge", 33, 31).max() > 1e30 and 0 < np.abs(K.image("tiny", 33, 31)).max() < 2e-30
    assert len(np.unique(K.image("levels", 33, 31))) == 4 and (K.image("sparse", 83, 85) == 0).mean() > 0.9
    for name in K.NON_NEGATIVE:
        assert (K.image(name, 33, 31) >= 0).all()


def test_grid_covers_what_the_kernels_tile_by():
    ws, hs = {w for w, _ in K.GRID}, {h for _, h in K.GRID}
    for edge in (15, 16, 17, 31, 32, 33):
        assert edge in ws and edge in hs
    assert {(1, 1), (1, 40), (40, 1)} <= set(K.GRID)
    assert any(w < 24 and h < 24 and w * h > 1 for w, h in K.GRID)                   # smaller than -GAUSS 9's halo both ways
    assert any(h >= 10 * w for w, h in K.GRID) and any(w >= 10 * h for w, h in K.GRID)
    assert any((w + 15) // 16 >= 5 and (h + 15) // 16 >= 5 for w, h in K.GRID)
    assert K.gauss_reach(9) == 24 and (16 + 2 * 24) ** 2 * 12 == 48 * 1024 and (16 + 2 * K.gauss_reach(10)) ** 2 * 12 > 48 * 1024


def test_mutation_table_still_applies():
    """Every text the mutation sweep substitutes occurs in its source file exactly as often as the table says, and the substitution
    changes the file: a reformatted kernel line must not let the table go stale until the next sweep on a device."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import mutate_image_kernels as M
    assert len(M.MUTATIONS) == 12 and len({row[0] for row in M.MUTATIONS}) == 12
    for name, rel, edits, occurrences, test, note in M.MUTATIONS:
        text = open(os.path.join(root, rel)).read()
        assert M.mutated_source(text, edits, occurrences, name) != text, name
        assert rel in M.PARENT_TESTS and note
