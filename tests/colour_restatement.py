"""Colour grading restated in numpy from the text of include/pt_hip.h alone (pt_colour_matrix, pt_colour_host, pt_lut_load_cube): the
matrix composed in float64, its three lines, the LUT's index and fraction rule, the six tetrahedra with the tie table, and a
.cube writer and reader for the tests.  Every float32 operation is one operation in the order the header writes it."""
import numpy as np

import grade_restatement as G

F = np.float32
LUM = (0.2126, 0.7152, 0.0722)
LUT_MAX_SIZE = 65
# the header's table: (the comparisons that select it, in order) -> the path's axes, 0 = r, 1 = g, 2 = b
PATHS = ((0, 1, 2), (0, 2, 1), (2, 0, 1), (1, 0, 2), (1, 2, 0), (2, 1, 0))


def compose(wb=None, saturation=None, matrix=None):
    """M = U S W in float64 in the header's order, each entry rounded to float32 once.  None: that factor's identity."""
    w = [1.0, 1.0, 1.0] if wb is None or all(float(F(v)) == 0.0 for v in wb) else [float(F(v)) for v in wb]
    s = 1.0 if saturation is None else float(F(saturation))
    U = None if matrix is None else [float(F(v)) for v in np.asarray(matrix, np.float64).reshape(9)]
    if U is None or all(v == 0.0 for v in U):
        U = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    X = [[((s if i == j else 0.0) + ((1.0 - s) * LUM[j])) * w[j] for j in range(3)] for i in range(3)]
    M = np.zeros((3, 3), F)
    for i in range(3):
        for j in range(3):
            M[i, j] = F(((U[3 * i] * X[0][j]) + (U[3 * i + 1] * X[1][j])) + (U[3 * i + 2] * X[2][j]))
    return M


def is_identity(M):
    return np.array_equal(np.asarray(M, F).view(np.uint32), np.eye(3, dtype=F).view(np.uint32))


def apply_matrix(M, m):
    """m [..., 3] float32 -> M m, three lines; skipped when M is the identity bit for bit."""
    m = np.asarray(m, F)
    if is_identity(M):
        return m.copy()
    M = np.asarray(M, F)
    r, g, b = m[..., 0], m[..., 1], m[..., 2]
    with np.errstate(all="ignore"):
        rows = [((M[i, 0] * r) + (M[i, 1] * g)) + (M[i, 2] * b) for i in range(3)]
    return np.stack(rows, axis=-1).astype(F)


def axis(g, n):
    """One channel's cell index (int64) and fraction (float32)."""
    g = np.asarray(g, F)
    with np.errstate(invalid="ignore"):
        x = np.where(~(g >= 0), F(0), np.where(g > 1, F(1), g)).astype(F)
    s = (x * F(n - 1)).astype(F)
    i = np.minimum(s.astype(np.int64), n - 2)
    f = (s - i.astype(F)).astype(F)
    return i, f


def path_index(fr, fg, fb):
    """Which row of PATHS: the header's comparisons in the header's order."""
    first = np.where(fg >= fb, 0, np.where(fr >= fb, 1, 2))
    second = np.where(fr >= fb, 3, np.where(fg >= fb, 4, 5))
    return np.where(fr >= fg, first, second)


def lut_apply(lut, g):
    """lut [N, N, N, 3] indexed [b, g, r]; g [..., 3] float32 -> out [..., 3]."""
    lut = np.asarray(lut, F)
    n = lut.shape[0]
    g = np.asarray(g, F)
    shape = g.shape
    g = g.reshape(-1, 3)
    idx, frac = zip(*(axis(g[:, k], n) for k in range(3)))
    idx, frac = np.stack(idx, 1), np.stack(frac, 1)          # [P, 3] in r, g, b
    which = path_index(frac[:, 0], frac[:, 1], frac[:, 2])
    order = np.asarray(PATHS)[which]                         # [P, 3]: the path's axes
    rows = np.arange(len(g))
    f1, f2, f3 = (frac[rows, order[:, k]] for k in range(3))
    ia = idx.copy()
    ib = ia.copy(); ib[rows, order[:, 0]] += 1
    ic = ib.copy(); ic[rows, order[:, 1]] += 1
    idd = ia + 1
    fetch = lambda i: lut[i[:, 2], i[:, 1], i[:, 0]]         # [P, 3]
    A, B, C, D = fetch(ia), fetch(ib), fetch(ic), fetch(idd)
    with np.errstate(all="ignore"):
        out = ((A + (f1[:, None] * (B - A))) + (f2[:, None] * (C - B))) + (f3[:, None] * (D - C))
    return out.astype(F).reshape(shape)


def colour(mean, count, exposure, curve, M=None, lut=None):
    """pt_colour_host: matrix -> exposure -> curve -> LUT where count != 0, the mean's own value elsewhere."""
    m = np.asarray(mean, F)
    v = m if M is None else apply_matrix(M, m)
    with np.errstate(all="ignore"):
        v = G.curve_value((v * F(exposure)).astype(F), curve)
    if lut is not None:
        v = lut_apply(lut, v)
    return np.where((np.asarray(count).reshape(m.shape[:-1]) != 0)[..., None], v, m).astype(F)


def write_cube(path, lut, title=None, domain=True, newline="\n", comment=None):
    """lut [N, N, N, 3] indexed [b, g, r] -> a .cube file, nine significant digits (every float32 survives)."""
    lut = np.asarray(lut, F)
    lines = []
    if comment:
        lines.append("# " + comment)
    if title is not None:
        lines.append('TITLE "%s"' % title)
    lines += ["", "LUT_3D_SIZE %d" % lut.shape[0]]
    if domain:
        lines += ["DOMAIN_MIN 0 0 0", "DOMAIN_MAX 1.0 1.0 1.0", ""]
    lines += ["%.9g %.9g %.9g" % tuple(float(x) for x in v) for v in lut.reshape(-1, 3)]
    with open(path, "w", newline="") as f:
        f.write(newline.join(lines) + newline)


def read_cube(path):
    """The accepted subset, for the tests: -> lut [N, N, N, 3] float32."""
    n, data = None, []
    for raw in open(path, newline=""):
        line = raw.strip()
        if not line or line.startswith("#") or line.startswith("TITLE"):
            continue
        if line.startswith("LUT_3D_SIZE"):
            n = int(line.split()[1])
        elif line.startswith("DOMAIN_"):
            continue
        else:
            data.append([F(t) for t in line.split()])
    return np.asarray(data, F).reshape(n, n, n, 3)
