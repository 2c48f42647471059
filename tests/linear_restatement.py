"""Scene-linear output restated in numpy from the text of include/pt_hip.h alone (uint32 / float32; no library call): the bodies of
PT_LINEAR_PFM and PT_LINEAR_RGBE, and readers of the two files that pt_write_pfm and pt_write_hdr write -- a PFM reader and a reader of
FLAT Radiance pictures (no run-length decoding: a picture this library writes has none)."""
import numpy as np

F = np.float32
U = np.uint32
PFM, RGBE = 1, 2
FORMATS = {"pfm": PFM, "hdr": RGBE}


def _exposed(mean_rgb, exposure, exposed):
    m = np.ascontiguousarray(mean_rgb, F)
    with np.errstate(all="ignore"):
        return m * F(exposure) if exposed else m          # ONE float multiply, or the bits untouched


def clip(c):
    """c' = (c > 0) ? (c < 2^126 ? c : 2^126) : 0: NaN, -0 and negatives give 0, +inf gives 2^126."""
    c = np.asarray(c, F)
    top = F(2.0 ** 126)
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, np.where(c < top, c, top), F(0)).astype(F)


def rgbe_pixels(values):
    """[..., 3] float32 -> [..., 4] uint8 (R, G, B, E) for pixels WITH samples."""
    c = clip(values)
    v = c.max(axis=-1)
    be = (v.view(U) >> U(23)) & U(255)
    zero = be < 27
    scale = ((U(261) - np.where(zero, U(134), be)) << U(23)).astype(U).view(F)
    with np.errstate(all="ignore"):
        prod = c * scale[..., None]                        # exact, or below 1
    byte = prod.astype(np.int32)
    assert (byte >= 0).all() and (byte < 256).all()
    out = np.concatenate([byte.astype(np.uint8), (be + U(2)).astype(np.uint8)[..., None]], axis=-1)
    out[zero] = 0
    return out


def encode(mean_rgb, count, exposure=1.0, format="pfm", exposed=False):
    """The body as bytes: mean_rgb [H, W, 3], count [H, W]."""
    fmt = FORMATS.get(format, format)
    m = _exposed(mean_rgb, exposure, exposed)
    h, w, _ = m.shape
    live = np.ascontiguousarray(count, np.int32).reshape(h, w) != 0
    if fmt == PFM:
        bits = np.where(live[..., None], m.view(U), U(0)).astype("<u4")
        return bits[::-1].tobytes()                        # rows bottom-up
    px = rgbe_pixels(m)
    px[~live] = 0
    return px.tobytes()                                    # rows top-down


def decode_rgbe(body, w, h):
    """(lo, hi) float64 [H, W, 3]: the interval (byte .. byte + 1) * 2^(E - 136) of every channel; mid = (byte + 0.5) * 2^(E - 136)."""
    px = np.frombuffer(body, np.uint8).reshape(h, w, 4).astype(np.int64)
    step = np.ldexp(1.0, px[..., 3] - 136)[..., None]
    return px[..., :3] * step, (px[..., :3] + 1) * step


def read_pfm(data):
    """File bytes -> float32 [H, W, 3] with rows top-down (bits kept)."""
    assert data[:3] == b"PF\n"
    end1 = data.index(b"\n", 3)
    w, h = (int(t) for t in data[3:end1].split())
    end2 = data.index(b"\n", end1 + 1)
    scale = float(data[end1 + 1:end2])
    assert scale == -1.0                                   # negative: little-endian
    body = data[end2 + 1:]
    assert len(body) == 12 * w * h
    return np.frombuffer(body, "<u4").reshape(h, w, 3)[::-1].copy().view(F)


def read_hdr(data):
    """File bytes of a flat Radiance picture -> uint8 [H, W, 4] (R, G, B, E), rows top-down."""
    assert data.startswith(b"#?RADIANCE\n")
    end = data.index(b"\n\n")
    assert b"FORMAT=32-bit_rle_rgbe" in data[:end].split(b"\n")
    line_end = data.index(b"\n", end + 2)
    t = data[end + 2:line_end].split()
    assert t[0] == b"-Y" and t[2] == b"+X"
    h, w = int(t[1]), int(t[3])
    body = data[line_end + 1:]
    assert len(body) == 4 * w * h
    px = np.frombuffer(body, np.uint8).reshape(h, w, 4)
    assert not ((px[..., 0] == 2) & (px[..., 1] == 2) & (px[..., 2] < 128)).any()      # nothing a reader takes for a run-length marker
    assert not ((px[..., 0] == 1) & (px[..., 1] == 1) & (px[..., 2] == 1)).any()
    return px
