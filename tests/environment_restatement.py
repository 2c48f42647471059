"""Environment lighting restated in numpy from the text of include/pt_hip.h alone (no library call): the octahedral map's apron and
lookup (float32, operation by operation), the conversion of an equirectangular picture into the map (float64, rounded once), a
flat and a run-length Radiance encoder with their decoder, and a PFM writer and reader."""
import numpy as np

F = np.float32
U = np.uint32


def with_apron(m):
    """(N, N, 3) -> (N + 2, N + 2, 3): [j + 1, i + 1] is texel (i, j)."""
    m = np.ascontiguousarray(m, F)
    n = m.shape[0]
    t = np.zeros((n + 2, n + 2, 3), F)
    t[1:n + 1, 1:n + 1] = m
    j = np.arange(n)
    t[j + 1, 0] = m[n - 1 - j, 0]               # texel (-1, j) = texel (0, N-1-j)
    t[j + 1, n + 1] = m[n - 1 - j, n - 1]       # texel (N, j) = texel (N-1, N-1-j)
    i = np.arange(-1, n + 1)                    # with the two apron columns: the corners, the two rules in turn
    t[0, i + 1] = t[1, n - 1 - i + 1]           # texel (i, -1) = texel (N-1-i, 0)
    t[n + 1, i + 1] = t[n, n - 1 - i + 1]       # texel (i, N) = texel (N-1-i, N-1)
    return t


def _copysign_bits(mag, sign):
    return ((np.ascontiguousarray(mag, F).view(U) & U(0x7FFFFFFF)) | (np.ascontiguousarray(sign, F).view(U) & U(0x80000000))).view(F)


def map_coordinates(d):
    """qx, qz of unit directions [n, 3] (float32)."""
    d = np.ascontiguousarray(d, F).reshape(-1, 3)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        px, pz = dx / s, dz / s
        fx = _copysign_bits(F(1) - np.abs(pz), px)
        fz = _copysign_bits(F(1) - np.abs(px), pz)
    low = dy < 0                                 # (-0 is not < 0)
    return np.where(low, fx, px).astype(F), np.where(low, fz, pz).astype(F)


def _cell(q, n):
    with np.errstate(all="ignore"):
        f = (q * F(0.5) + F(0.5)) * F(n) - F(0.5)
        fl = np.floor(f)
        i0 = np.where(fl >= -1, np.where(fl <= n - 1, fl, n - 1), -1)
        i0 = np.where(np.isnan(fl), -1, i0).astype(np.int64)
        return i0, (f - i0.astype(F)).astype(F)


def lookup(m, d):
    """L [n, 3] float32 of map (N, N, 3) for unit directions [n, 3]."""
    t = with_apron(m)
    n = t.shape[0] - 2
    qx, qz = map_coordinates(d)
    x0, ax = _cell(qx, n)
    y0, ay = _cell(qz, n)
    ax, ay = ax[:, None], ay[:, None]
    t00, t10 = t[y0 + 1, x0 + 1], t[y0 + 1, x0 + 2]
    t01, t11 = t[y0 + 2, x0 + 1], t[y0 + 2, x0 + 2]
    with np.errstate(all="ignore"):
        bx, by = F(1) - ax, F(1) - ay
        return ((t00 * bx + t10 * ax) * by + (t01 * bx + t11 * ax) * ay).astype(F)


def default_size(h):
    n = 8
    while n < h and n < 2048:
        n *= 2
    return n


def direction_of(qx, qz):
    """The unit direction (float64) of map coordinates in [-1, 1]^2: the inverse of the direction-to-map rule, normalised."""
    qx, qz = np.asarray(qx, np.float64), np.asarray(qz, np.float64)
    dy = 1.0 - np.abs(qx) - np.abs(qz)
    up = dy >= 0
    dx = np.where(up, qx, np.copysign(1.0 - np.abs(qz), qx))
    dz = np.where(up, qz, np.copysign(1.0 - np.abs(qx), qz))
    ln = np.sqrt(dx * dx + dy * dy + dz * dz)
    return dx / ln, dy / ln, dz / ln


def picture_coordinates(ux, uy, uz, w, h, rotate=0.0):
    """fx, fy (float64) at which the picture is looked up for direction u rotated about +y by `rotate` degrees."""
    ang = rotate * np.pi / 180.0
    ca, sa = np.cos(ang), np.sin(ang)
    vx, vz = ca * ux + sa * uz, -sa * ux + ca * uz
    theta = np.arccos(np.clip(uy, -1.0, 1.0)) / np.pi
    phi = np.arctan2(vz, -vx) / (2.0 * np.pi) + 0.5
    return phi * w, theta * h


def from_equirect(pic, n, gain=1.0, rotate=0.0):
    """(h, w, 3) float32 -> (n, n, 3) float32."""
    pic = np.ascontiguousarray(pic, F).astype(np.float64)
    h, w, _ = pic.shape
    k = min(8, max(1, -(-w // n)))
    jj, ii, sj, si = np.meshgrid(np.arange(n), np.arange(n), np.arange(k), np.arange(k), indexing="ij")
    qx = 2.0 * ((ii + (si + 0.5) / k) / n) - 1.0
    qz = 2.0 * ((jj + (sj + 0.5) / k) / n) - 1.0
    ux, uy, uz = direction_of(qx, qz)
    fx, fy = picture_coordinates(ux, uy, uz, w, h, rotate)
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = x0 % w, (x0 + 1) % w
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    v = (pic[ya, xa] * (1.0 - ax) + pic[ya, xb] * ax) * (1.0 - ay) + (pic[yb, xa] * (1.0 - ax) + pic[yb, xb] * ax) * ay
    acc = np.zeros((n, n, 3), np.float64)
    for b in range(k):                           # in the order the header's sum runs: rows of sub-cells, then columns
        for a in range(k):
            acc += v[:, :, b, a]
    return (acc / (k * k) * np.float64(F(gain))).astype(F)


# ---- files ---------------------------------------------------------------------------------------------------------------------
def hdr_header(w, h, magic=b"#?RADIANCE"):
    return magic + b"\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)


def hdr_flat(px):
    """uint8 [H, W, 4] -> the file's bytes with flat scanlines."""
    h, w, _ = px.shape
    return hdr_header(w, h) + np.ascontiguousarray(px, np.uint8).tobytes()


def _rle_channel(row):
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        run = 1
        while i + run < n and run < 127 and row[i + run] == row[i]:
            run += 1
        if run >= 3:
            out += bytes([128 + run, row[i]])
            i += run
        else:
            j = i
            while j < n and j - i < 128 and not (j + 2 < n and row[j] == row[j + 1] == row[j + 2]):
                j += 1
            out += bytes([j - i]) + bytes(row[i:j].tolist())
            i = j
    return bytes(out)


def hdr_rle(px):
    """uint8 [H, W, 4] -> the file's bytes with new-style run-length scanlines (8 <= W < 32768)."""
    h, w, _ = px.shape
    body = bytearray()
    for y in range(h):
        body += bytes([2, 2, w >> 8, w & 255])
        for c in range(4):
            body += _rle_channel(np.ascontiguousarray(px[y, :, c]))
    return hdr_header(w, h) + bytes(body)


def decode_rgbe(px):
    """uint8 [H, W, 4] -> float32 [H, W, 3]: (byte + 0.5) * 2^(E - 136); the pixel 0, 0, 0, 0 is black."""
    p = px.astype(np.int64)
    v = np.ldexp(p[..., :3] + 0.5, (p[..., 3] - 136)[..., None])
    v[(p == 0).all(axis=-1)] = 0.0
    return v.astype(F)


def pfm_bytes(img, big_endian=False):
    """float32 [H, W, 3], rows top-down -> the file's bytes."""
    h, w, _ = img.shape
    body = np.ascontiguousarray(img, F)[::-1].astype(">f4" if big_endian else "<f4").tobytes()
    return b"PF\n%d %d\n%s\n" % (w, h, b"1.0" if big_endian else b"-1.0") + body


def read_pfm(data):
    assert data[:2] == b"PF"
    tok, at = [], 2
    while len(tok) < 3:
        while data[at:at + 1].isspace():
            at += 1
        b = at
        while not data[at:at + 1].isspace():
            at += 1
        tok.append(data[b:at])
    at += 1
    w, h, scale = int(tok[0]), int(tok[1]), float(tok[2])
    return np.frombuffer(data[at:at + 12 * w * h], "<f4" if scale < 0 else ">f4").reshape(h, w, 3)[::-1].astype(F)
