"""Inputs of the scene-linear output tests (tests/test_linear_host.py, tests/test_gpu_linear.py): name -> (mean [H, W, 3] float32, count
[H, W] int32, exposure).  Made once, from fixed seeds, and never written to.

  shapes     1x1, 3x2, 5x7, 64x1, 1x64, 67x33 (W x H): W no multiple of 4, one row, one column, more than one workgroup with ragged edges;
             8x5 besides: several rows whose width IS a multiple of 4, the size at which the PFM kernel takes its aligned path
  sweep      255x3: column k's largest channel has exponent field k (0 .. 254) and a mantissa of all ones; the other two lie half a step
             above 0, 1, 127, 128 and 255 steps of the pixel's exponent; the rows put the largest in r, g, b in turn
  specials   NaN with payloads (quiet, signalling, negative), +-inf, -0, negatives, subnormals, 2^-100 and its predecessor, 2^126 and its
             successor, in each channel in turn and in all three; pixels with count == 0 that carry garbage
  divide     sums divided by counts 1, 3 and 7 in float32, the display kernel's own operation: quotients with full mantissas"""
import numpy as np

F = np.float32
U = np.uint32


def _bits(*words):
    return np.array(words, U).view(F)


def _shape(w, h, seed):
    rng = np.random.default_rng(seed)
    mean = np.exp(rng.uniform(-12.0, 12.0, (h, w, 3))).astype(F)
    mean[rng.random((h, w, 3)) < 0.05] *= F(-1)
    mean[rng.random((h, w, 3)) < 0.05] = F(0)
    count = rng.integers(1, 50, (h, w)).astype(np.int32)
    count[rng.random((h, w)) < 0.1] = 0
    if w * h == 1:
        count[:] = 3
    return mean, count, F(np.exp(rng.uniform(-2.0, 2.0)))


def _sweep():
    steps = (0, 1, 127, 128, 255)
    mean = np.zeros((3, 255, 3), F)
    for k in range(255):
        top = _bits((k << 23) | 0x7FFFFF)[0]
        others = [F(np.ldexp(steps[k % 5] + 0.5, k - 134)), F(np.ldexp(steps[(k // 5) % 5] + 0.5, k - 134))]
        for row in range(3):
            px = others[:]
            px.insert(row, top)
            mean[row, k] = px
    return mean, np.ones((3, 255), np.int32), F(1.0)


def _specials():
    special = np.concatenate([_bits(0x7FC00001, 0x7FA5A5A5, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x007FFFFF,
                                    0x80000001, 0x0D800000, 0x0D7FFFFF, 0x0D800001, 0x7E800000, 0x7E800001, 0x7E7FFFFF, 0x7F7FFFFF),
                              np.array([-1.0, -1e-30, 0.0, 1.0, 0.5, 255.0 / 256.0, 1e-30, 3e38], F)])
    assert special[10] == F(2.0 ** -100) and special[13] == F(2.0 ** 126)
    b = lambda x: int(np.array(x, F).view(U))              # pixels are put together as bit patterns: no conversion touches a NaN
    px = []
    for s in special.view(U).tolist():
        px += [(s, b(0.5), b(0.25)), (b(0.5), s, b(0.25)), (b(0.5), b(0.25), s), (s, s, s), (s, b(0), b(0)), (b(1e-40), s, b(-2))]
    garbage = [(int(special.view(U)[0]), int(special.view(U)[4]), b(1e30)), (b(7), int(special.view(U)[5]), int(special.view(U)[3]))] * 3
    mean = np.array(px + garbage, U).view(F)               # the last six have count == 0: all-zero bytes whatever the mean holds
    count = np.concatenate([np.ones(len(px), np.int32), np.zeros(len(garbage), np.int32)])
    w = 13                                                 # 156 pixels: 13 x 12
    assert len(count) % w == 0
    return mean.reshape(-1, w, 3), count.reshape(-1, w), F(0.75)


def _divide():
    rng = np.random.default_rng(77)
    w, h = 7, 3
    count = np.tile(np.array([1, 3, 7], np.int32), (w * h + 2) // 3)[:w * h].reshape(h, w)
    sums = np.exp(rng.uniform(-3.0, 6.0, (h, w, 3))).astype(F)
    return (sums / count[..., None].astype(F)).astype(F), count, F(1.5)


CASES = {f"{w}x{h}": _shape(w, h, 100 * w + h) for w, h in ((1, 1), (3, 2), (5, 7), (64, 1), (1, 64), (67, 33), (8, 5))}
CASES["sweep"] = _sweep()
CASES["specials"] = _specials()
CASES["divide"] = _divide()
for _m, _c, _e in CASES.values():
    _m.setflags(write=False)
    _c.setflags(write=False)
