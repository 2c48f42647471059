#!/usr/bin/env python3
"""models/Tor.obj with texture coordinates: the repository's models have no `vt` lines, so every corner reads (0, 0) and a texture
shows as one texel.  This writes a copy whose every face corner has a `vt` of its own -- planar: u along x + z, v along y - z, one
repeat per `period` scene units -- an MTL whose wall materials name a picture in a `map_Kd` line, and that picture, a checkerboard.

    python tools/make_textured_scene.py --out-dir /tmp/tex        ->  TorUV.obj, TorUV.mtl, checker.bmp
    pt_render --W 640 --H 360 -RPP 64 -MODEL_PATH /tmp/tex/ -MODEL_NAME TorUV.obj -TEXTURE 1:/tmp/tex/checker.bmp      (a checkered wall)
    pt_render ... -TEXTURE mtl                                                                                         (every map_Kd of the MTL)
"""
import argparse
import os
import struct

WALLS = (1, 2, 3)      # Tor.mtl: the white, the green and the red walls (0 is the emitter, 4 the torus)


def write_checker_bmp(path, size=1024, squares=8, dark=40, light=230):
    step = size // squares
    row_a = b"".join(bytes((light if (x // step) % 2 == 0 else dark,)) * 3 for x in range(size))
    row_b = b"".join(bytes((dark if (x // step) % 2 == 0 else light,)) * 3 for x in range(size))
    pad = b"\0" * ((4 - (3 * size) % 4) % 4)
    with open(path, "wb") as f:
        f.write(struct.pack("<HIHHI", 19778, 54 + (3 * size + len(pad)) * size, 0, 0, 54))
        f.write(struct.pack("<IiiHHIIiiII", 40, size, size, 1, 24, 0, (3 * size + len(pad)) * size, 0, 0, 0, 0))
        for y in range(size):
            f.write((row_a if (y // step) % 2 == 0 else row_b) + pad)


def generate(models_dir, out_dir, name="TorUV.obj", picture="checker.bmp", size=1024, period=8.0, source="Tor.obj"):
    """Returns the number of triangles written."""
    os.makedirs(out_dir, exist_ok=True)
    verts, out, n_vt, n_tri = [], [], 0, 0
    for line in open(os.path.join(models_dir, source)).read().split("\n"):
        tok = line.split()
        if tok[:1] == ["v"]:
            verts.append(tuple(float(t) for t in tok[1:4]))
        if tok[:1] == ["mtllib"]:
            line = "mtllib " + name.replace(".obj", ".mtl")
        if tok[:1] == ["f"]:
            corners = []
            for g in tok[1:4]:
                parts = g.split("/")
                x, y, z = verts[int(parts[0]) - 1]
                out.append("vt %.6f %.6f" % ((x + z) / period, (y - z) / period))
                n_vt += 1
                corners.append("%s/%d%s" % (parts[0], n_vt, "/" + parts[2] if len(parts) > 2 and parts[2] else ""))
            line = "f " + " ".join(corners)
            n_tri += 1
        out.append(line)
    open(os.path.join(out_dir, name), "w").write("\n".join(out))
    mtl, current = [], None
    for line in open(os.path.join(models_dir, "Tor.mtl")).read().split("\n"):
        tok = line.split()
        if tok[:1] == ["newmtl"]:
            current = int(tok[1])
        mtl.append(line)
        if tok[:1] == ["Kd"] and current in WALLS:
            mtl.append("map_Kd " + picture)
    open(os.path.join(out_dir, name.replace(".obj", ".mtl")), "w").write("\n".join(mtl))
    write_checker_bmp(os.path.join(out_dir, picture), size)
    return n_tri


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--models", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models"))
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    print(f"{a.out_dir}/TorUV.obj: {generate(a.models, a.out_dir, size=a.size)} triangles with vt, TorUV.mtl with map_Kd, checker.bmp {a.size}x{a.size}")


if __name__ == "__main__":
    main()
