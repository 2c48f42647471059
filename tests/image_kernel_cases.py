"""Inputs for the image-space kernels' tests (tests/test_gpu_image_kernels.py, tests/test_image_crops_host.py): the shape grid,
synthetic image content, synthetic denoiser inputs, and the crop helper that lets a full-size device result be compared with a
reference that only ever sees small crops.  No device is touched here; everything is numpy with fixed seeds.

-0.0 and NaN are kept out of every image that is compared bit for bit: the reference picks its order statistic from a sorted
window, and which of two equal zeros lands at the chosen rank is unspecified, as is any ordering of a NaN.
"""
import zlib

import numpy as np

F32 = np.float32

# (W, H): 1 pixel, 1 column, 1 row; 15 / 16 / 17 and 31 / 32 / 33 in each direction (one below, at and one above the 16 x 16 tile of
# the post filters and the 32-wide workgroup of the denoiser); tall-narrow and wide-low (a transposed clamp is invisible on a
# near-square image); smaller than the halo of -GAUSS 9 (24) in both directions; 6 x 6 workgroups of 16 x 16 with ragged edges.
GRID = [(1, 1), (1, 40), (40, 1), (15, 16), (16, 17), (17, 15), (16, 16), (31, 32), (32, 33), (33, 31), (32, 32), (17, 33), (32, 15),
        (7, 90), (90, 7), (5, 3), (83, 85)]
GAUSS_RADII = (1, 9, 10)      # 9: the largest halo staged in LDS (exactly 48 KB); 10: the first radius on the global-memory path
MEDIAN_SIZES = (1, 3, 4, 11)  # both ends of the register kernels (1..3) and of the generic kernel (4..11)


def gauss_reach(r):
    return int(np.ceil(r * 2.57))


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


# ---- image content ---------------------------------------------------------------------------------------------------

def _dense(rng, H, W):
    return rng.uniform(0, 255, (H, W, 3))


def _sparse(rng, H, W):
    """Mostly black with isolated bright pixels: what a frame with many pixels without samples looks like."""
    img = np.zeros((H, W, 3))
    lit = rng.random((H, W)) < 0.04
    lit.flat[rng.integers(0, H * W)] = True
    img[lit] = rng.uniform(60, 255, (int(lit.sum()), 3))
    return img


def _levels(rng, H, W):
    """Four integer levels: most of a median window is ties."""
    return rng.integers(0, 4, (H, W, 3)) * 64.0


def _signed(rng, H, W):
    return rng.uniform(-255, 255, (H, W, 3))


def _huge(rng, H, W):
    return rng.uniform(0.5, 1.5, (H, W, 3)) * 1e30 * rng.choice([-1.0, 1.0], (H, W, 3))


def _tiny(rng, H, W):
    return rng.uniform(0.5, 1.5, (H, W, 3)) * 1e-30 * rng.choice([-1.0, 1.0], (H, W, 3))


def _constant(rng, H, W):
    return np.full((H, W, 3), 37.25)


def _inf_lines(rng, H, W):
    """A row of +Inf and a column of -Inf in dense content.  For the median only: an order statistic of values that compare is well
    defined; a Gaussian window holding both signs sums to NaN."""
    img = _dense(rng, H, W)
    img[H // 2, :, :] = np.inf
    img[:, W // 3, :] = -np.inf
    return img


def _pos_inf_lines(rng, H, W):
    """A row and a column of +Inf only: every Gaussian weight is positive, so a window that holds one sums to +Inf and rounds to +Inf."""
    img = _dense(rng, H, W)
    img[H // 2, :, :] = np.inf
    img[:, W // 3, :] = np.inf
    return img


CONTENT = {"dense": _dense, "sparse": _sparse, "levels": _levels, "signed": _signed, "huge": _huge, "tiny": _tiny,
           "constant": _constant}
MEDIAN_ONLY_CONTENT = {"inf_lines": _inf_lines}
NON_NEGATIVE = ("dense", "sparse", "levels", "constant")   # a Gaussian of these cannot round to -0.0, so a median may follow


def image(kind, W, H, seed=0):
    """float32 [H, W, 3] of the named content, without -0.0 and NaN."""
    fn = {**CONTENT, **MEDIAN_ONLY_CONTENT, "pos_inf_lines": _pos_inf_lines}[kind]
    img = fn(np.random.default_rng(_seed(kind, W, H, seed)), H, W).astype(np.float32)
    img = img + F32(0)                        # -0.0 + 0.0 = +0.0
    assert not np.isnan(img).any() and not (np.signbit(img) & (img == 0)).any()
    return img


# ---- crops -----------------------------------------------------------------------------------------------------------

def crop_reference(arrays, box, reach, fn):
    """What a LOCAL image operation with clamped or skipped out-of-image taps gives inside `box`, computed from a crop.

    arrays: the operation's inputs, each [H, W, ...]; box = (x0, y0, x1, y1), half open; reach: how far a result depends on its
    inputs, in pixels; fn(crops, w, h) -> [h, w, ...] array or tuple of such arrays.  The crop is the box padded by `reach` and cut at
    the image's borders.  A result pixel of the box then sees, inside the crop, every input it sees in the whole image: towards a
    cut the padding covers its reach, and a border of the crop that is a border of the image clamps (or skips) exactly as the image
    does -- which is why the crop must KEEP that border and may not be cut a few pixels inside it."""
    H, W = arrays[0].shape[:2]
    x0, y0, x1, y1 = box
    assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
    px0, py0, px1, py1 = max(0, x0 - reach), max(0, y0 - reach), min(W, x1 + reach), min(H, y1 + reach)
    crops = [np.ascontiguousarray(a[py0:py1, px0:px1]) for a in arrays]
    out = fn(crops, px1 - px0, py1 - py0)
    cut = lambda o: o[y0 - py0:y1 - py0, x0 - px0:x1 - px0]
    return tuple(cut(o) for o in out) if isinstance(out, tuple) else cut(out)


def windows(W, H, cw, ch, tile_w=16, tile_h=16):
    """Boxes of cw x ch in a W x H image: the four corners, the middle of each edge, one across a workgroup seam in the interior,
    and one in the last (partial, if the height is no multiple of tile_h) row of workgroups."""
    mx, my = (W // 2 // tile_w) * tile_w - cw // 2, (H // 2 // tile_h) * tile_h - ch // 2     # a seam runs through the middle
    last = ((H - 1) // tile_h) * tile_h
    boxes = {"top_left": (0, 0), "top_right": (W - cw, 0), "bottom_left": (0, H - ch), "bottom_right": (W - cw, H - ch),
             "top": (mx, 0), "bottom": (mx, H - ch), "left": (0, my), "right": (W - cw, my), "seam": (mx, my),
             "last_row": (W // 3, H - ch)}
    assert H - ch < last < H, "the last-row window must span the seam above the last row of workgroups"
    return {k: (x, y, x + cw, y + ch) for k, (x, y) in boxes.items()}


# ---- synthetic denoiser inputs ---------------------------------------------------------------------------------------

ALBEDO_FLOOR = F32(0.01)
SPATIAL_BELOW = 4
_UNIT_SET = np.array([(0, 1, 0), (1, 0, 0), (0, 0, -1), (0.6, 0.8, 0)], np.float32)
HIT_KINDS = ("random", "blocks", "checker", "all", "none")
NORMAL_KINDS = ("unit", "discrete", "opposite", "orthogonal", "some_zero")
POSITION_KINDS = ("coplanar", "random", "scales")
ALBEDO_KINDS = ("floor", "materials")
COUNT_KINDS = ("mixed", "zero", "sampled", "threshold", "two_pow_24", "cancel")


def denoise_inputs(W, H, seed=0, hit="random", normal="discrete", position="coplanar", albedo="floor", count="mixed"):
    """(sum [H*W, 3], sum2 [H*W, 3], count [H*W], features) with every value finite.  Feature values of miss pixels are arbitrary (not
    the zeros the library writes): the header gives a miss centre the feature weight 1 whatever its buffers hold."""
    rng = np.random.default_rng(_seed("denoise", W, H, seed, hit, normal, position, albedo, count))
    y, x = np.mgrid[0:H, 0:W]
    # class
    if hit == "random":
        idx = np.where(rng.random((H, W)) < 0.7, rng.integers(0, 100000, (H, W)), -1)
    elif hit == "blocks":
        idx = np.where((y // 5 + x // 7) % 2 == 0, 7, -1)
    elif hit == "checker":
        idx = np.where((x + y) % 2 == 0, 0, -1)            # index 0 is a hit
    else:
        idx = np.full((H, W), 3 if hit == "all" else -1)
    # normals
    if normal == "unit":
        N = rng.normal(size=(H, W, 3)).astype(np.float32)
        N = N / np.sqrt((N * N).sum(-1, keepdims=True, dtype=np.float32))
    elif normal == "discrete":
        N = _UNIT_SET[rng.integers(0, len(_UNIT_SET), (H // 6 + 1, W // 6 + 1))][y // 6, x // 6]
    elif normal == "opposite":                             # direct neighbours: n_p . n_q = -1
        N = np.zeros((H, W, 3), np.float32)
        N[..., 2] = np.where((x + y) % 2 == 0, 1, -1)
    elif normal == "orthogonal":                           # direct neighbours: n_p . n_q = 0 exactly
        N = np.where(((x + y) % 2 == 0)[..., None], _UNIT_SET[0], _UNIT_SET[1])
    else:                                                  # a zero normal on a hit: every feature weight of that centre is 0
        N = _UNIT_SET[rng.integers(0, 2, (H, W))]
        N = np.where((rng.random((H, W)) < 0.15)[..., None], F32(0), N)
    # positions
    if position == "coplanar":
        P = np.stack([x * 0.05, y * 0.05, np.full((H, W), 2.0)], -1)
    elif position == "random":
        P = rng.uniform(-5, 5, (H, W, 3))
    else:
        P = rng.uniform(-1, 1, (H, W, 3)) * 10.0 ** rng.uniform(-3, 6, (H, W, 1))
    # albedo
    if albedo == "floor":
        below, above = np.nextafter(ALBEDO_FLOOR, F32(0)), np.nextafter(ALBEDO_FLOOR, F32(1))
        A = rng.choice(np.array([0, 0.001, below, ALBEDO_FLOOR, above, 0.02, 0.5, 1.0, 2.5, 40.0], np.float32), (H, W, 3))
    else:
        A = np.array([(0.8, 0.8, 0.8), (0.7, 0.1, 0.1), (0.1, 0.6, 0.2)], np.float32)[rng.integers(0, 3, (H // 4 + 1, W // 4 + 1))][y // 4, x // 4]
    # counts
    if count == "mixed":
        n = rng.choice([0, 0, 0, 1, 2, 3, 4, 5, 16, 100], (H, W))
    elif count == "zero":
        n = np.zeros((H, W), np.int64)
    elif count == "sampled":
        n = rng.integers(1, 64, (H, W))
    elif count == "threshold":
        n = rng.choice([SPATIAL_BELOW - 1, SPATIAL_BELOW, SPATIAL_BELOW + 1], (H, W))
    elif count == "two_pow_24":                            # 2^24 + 1 is the first count a float cannot hold
        n = rng.choice([0, 5, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1], (H, W))
    else:
        n = rng.integers(1, 9, (H, W))
    n = n.astype(np.int32)
    # accumulators: samples of mean m and spread sd, summed in double and rounded once
    m = rng.uniform(0, 2, (H, W, 3)) * np.where(rng.random((H, W, 1)) < 0.1, 20.0, 1.0)       # a few fireflies
    sd = rng.uniform(0, 0.7, (H, W, 3))
    nn = n[..., None].astype(np.float64)
    s = (m * nn).astype(np.float32)
    s2 = ((m * m + sd * sd) * nn).astype(np.float32)
    if count == "cancel":                                  # identical samples: sum2 / n - mean^2 is rounding noise of either sign
        s2 = (s.astype(np.float64) * s / np.maximum(nn, 1)).astype(np.float32)
        s2 = np.where(rng.random((H, W, 3)) < 0.5, np.nextafter(s2, F32(0)), s2).astype(np.float32)
    feat = {"hit_index": idx.astype(np.int32).reshape(-1), "position": P.astype(np.float32).reshape(-1, 3),
            "normal": np.ascontiguousarray(N, np.float32).reshape(-1, 3), "albedo": A.astype(np.float32).reshape(-1, 3)}
    out = (s.reshape(-1, 3), s2.reshape(-1, 3), n.reshape(-1), feat)
    for a in (out[0], out[1], feat["position"], feat["normal"], feat["albedo"]):
        assert np.isfinite(a).all()
    return out


DENOISE_REACH_VARIANCE = 3


def denoise_reach(levels):
    """How far mean_rgb depends on its inputs: 3 for the 7 x 7 variance window, 2 * 2^i for level i."""
    return DENOISE_REACH_VARIANCE + 2 * ((1 << levels) - 1)


def denoise_planes(W, H, s, s2, c, feat):
    """The denoiser's seven inputs as [H, W, ...] planes, for crop_reference."""
    return [s.reshape(H, W, 3), s2.reshape(H, W, 3), c.reshape(H, W), feat["hit_index"].reshape(H, W),
            feat["position"].reshape(H, W, 3), feat["normal"].reshape(H, W, 3), feat["albedo"].reshape(H, W, 3)]


def denoise_from_planes(denoise, **kw):
    """fn for crop_reference: runs denoise(w, h, s, s2, c, feat, **kw) on cropped planes, returns (mean [h, w, 3], count [h, w])."""
    def fn(crops, w, h):
        s, s2, c, idx, P, N, A = crops
        feat = {"hit_index": idx.reshape(-1), "position": P.reshape(-1, 3), "normal": N.reshape(-1, 3), "albedo": A.reshape(-1, 3)}
        mean, cnt = denoise(w, h, s.reshape(-1, 3), s2.reshape(-1, 3), c.reshape(-1), feat, **kw)[:2]
        return mean.reshape(h, w, 3), cnt.reshape(h, w)
    return fn
