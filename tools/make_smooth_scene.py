#!/usr/bin/env python3
"""Writes TorSmooth.obj (and copies the MTL beside it): models/Tor.obj with per-vertex `vn` lines on the torus, so that
`pt_render -SMOOTH vn` has an input -- the shipped models name one vn per face.  The normals are the generator's (welded vertices,
angle-weighted, crease 60 degrees), restated here in numpy so that the tool needs no built library; every other face keeps the vn the
file gives it on all three corners.  A generated normal is written on the side of the vn the face had (Tor.obj winds its lamp against
its vn; the torus agrees with it), so every face of the output names normals of one side.

    python tools/make_smooth_scene.py --out-dir D [--models models/] [--crease 60]
"""
import argparse
import os
import shutil

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORUS_MATERIAL = 4
F32 = np.float32


def numpy_normals(vertices, crease=60.0):
    """pt_smooth_normals restated in numpy (double): welded where positions are bit-identical, angle-weighted, faces with f . g >= cos(crease)."""
    v = np.asarray(vertices, F32).reshape(-1, 3, 3)
    p = v.astype(np.float64)
    c = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(c, axis=1)
    ok = np.isfinite(ln) & (ln > 0)
    fn = np.where(ok[:, None], c / np.where(ok, ln, 1)[:, None], 0)
    ang = np.zeros((len(v), 3))
    for i in range(3):
        a, b = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        with np.errstate(all="ignore"):
            ang[:, i] = np.arccos(np.clip((a * b).sum(1) / np.sqrt((a * a).sum(1) * (b * b).sum(1)), -1, 1))
    at = {}
    for t in np.nonzero(ok)[0]:
        for k in range(3):
            at.setdefault(v[t, k].tobytes(), []).append((t, k))
    out = np.zeros((len(v), 3, 3))
    limit = np.cos(np.radians(float(F32(crease))))
    for corners in at.values():
        for (t, k) in corners:
            acc = np.zeros(3)
            for (u, j) in corners:
                if u == t or fn[t] @ fn[u] >= limit:
                    acc += ang[u, j] * fn[u]
            l = np.linalg.norm(acc)
            if l > 0:
                out[t, k] = acc / l
    return out.astype(F32)


def _index(text, count):
    """An OBJ index as a position in the list read so far: 1-based, or negative and relative to the list's end; None for none or zero."""
    i = int(text) if text else 0
    return i - 1 if i > 0 else count + i if i < 0 else None


def generate(models_dir, out_dir, name="TorSmooth.obj", crease=60.0):
    lines = open(os.path.join(models_dir, "Tor.obj")).read().splitlines()
    pos, nrm, faces, material = [], [], [], 0                     # faces: (line number, vertex positions in `pos`, the first corner's vn or None)
    for i, l in enumerate(lines):
        tok = l.split()
        if tok[:1] == ["v"]:
            pos.append(list(map(float, tok[1:4])))
        elif tok[:1] == ["vn"]:
            nrm.append(list(map(float, tok[1:4])))
        elif tok[:1] == ["usemtl"]:
            material = int(tok[1])
        elif tok[:1] == ["f"] and material == TORUS_MATERIAL:
            parts = [g.split("/") for g in tok[1:4]]
            first = _index(parts[0][2], len(nrm)) if len(parts[0]) == 3 else None
            faces.append((i, [_index(g[0], len(pos)) for g in parts], None if first is None else nrm[first]))
    verts = np.array([[pos[k] for k in idx] for _, idx, _ in faces], F32)
    normals = numpy_normals(verts, crease)
    for f, (_, _, vn) in enumerate(faces):                        # the generator follows the winding; the file's vn names the side
        c = np.cross(verts[f, 1] - verts[f, 0], verts[f, 2] - verts[f, 0])
        if vn is not None and np.dot(c, vn) < 0:
            normals[f] = -normals[f]
    # the new vn lines go first in the file, so every positive vn index the file already uses moves up by their number (a negative
    # one counts from the end of the list read so far, and stays)
    extra = ["vn %.9g %.9g %.9g" % tuple(normals[f, k]) for f in range(len(faces)) for k in range(3)]
    torus = {i: (f, idx) for f, (i, idx, _) in enumerate(faces)}
    for i, l in enumerate(lines):
        tok = l.split()
        if tok[:1] != ["f"]:
            continue
        if i in torus:
            f, idx = torus[i]
            lines[i] = "f " + " ".join("%d//%d" % (idx[k] + 1, 3 * f + k + 1) for k in range(3))
        else:
            groups = []
            for g in tok[1:]:
                part = g.split("/")
                if len(part) == 3 and part[2] and int(part[2]) > 0:
                    part[2] = str(int(part[2]) + len(extra))
                groups.append("/".join(part))
            lines[i] = "f " + " ".join(groups)
    out = [l for l in lines if l.startswith("mtllib")] + extra + [l for l in lines if not l.startswith("mtllib")]
    os.makedirs(out_dir, exist_ok=True)
    open(os.path.join(out_dir, name), "w").write("\n".join(out) + "\n")
    for l in lines:
        if l.startswith("mtllib"):
            shutil.copy(os.path.join(models_dir, l.split()[1]), os.path.join(out_dir, l.split()[1]))
    return os.path.join(out_dir, name)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--models", default=os.path.join(ROOT, "models"))
    ap.add_argument("--crease", type=float, default=60.0)
    a = ap.parse_args()
    print(generate(a.models, a.out_dir, crease=a.crease))
