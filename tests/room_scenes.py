"""The scenes the room kernel's tests run (tests/test_room_shape_host.py, tests/test_gpu_room_kernel.py), generated from
models/Tor.obj: three that are room-shaped (pt_scene.hpp: CullTables::room) and four that are not, one per clause a scene can miss.

make(tmp) writes them under tmp and returns {name: Case}.  Case.room = what the TABLES say; Case.sky = a skybox bitmap the handle gets
(the tables of that case are Tor.obj's own, room-shaped: the skybox is the launch's clause)."""
import collections
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "models")
sys.path.insert(0, os.path.join(ROOT, "tools"))

Case = collections.namedtuple("Case", "dir name room sky big")

ROOM = ("tor", "empty_room", "large_light")
OTHER = ("two_objects", "triangle_wall", "skybox", "replica")
NAMES = ROOM + OTHER


def _tor_lines():
    return open(os.path.join(MODELS, "Tor.obj")).read().split("\n")


def _write(d, name, lines):
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, name), "w").write("\n".join(lines))
    shutil.copy(os.path.join(MODELS, "Tor.mtl"), os.path.join(d, "Tor.mtl"))


def make(tmp):
    import make_open_scene as MO
    import make_replicated_scene as MR
    tmp = str(tmp)
    cases = {"tor": Case(MODELS + "/", "Tor.obj", True, None, False)}

    # the room with the torus removed: every face line before "o Main" goes (the vertices stay, so the room's indices hold)
    lines = _tor_lines()
    main = lines.index("o Main")
    d = os.path.join(tmp, "empty") + "/"
    _write(d, "Empty.obj", [l for i, l in enumerate(lines) if not (i < main and l.startswith("f "))])
    cases["empty_room"] = Case(d, "Empty.obj", True, None, False)

    # the light three times as wide and off centre: the first four vertices after "o Main" are its corners (y = 9)
    lines = _tor_lines()
    corners = [i for i in range(main, len(lines)) if lines[i].startswith("v ")][:4]
    for i in corners:
        x, y, z = (float(t) for t in lines[i].split()[1:4])
        assert abs(y - 9.0) < 1e-6 and abs(abs(x) - 1.0) < 1e-6
        lines[i] = "v %.6f %.6f %.6f" % (3.0 * x + 2.0, y, 3.0 * z - 4.0)
    d = os.path.join(tmp, "light") + "/"
    _write(d, "Light.obj", lines)
    cases["large_light"] = Case(d, "Light.obj", True, None, False)

    # two separate objects: two sphere-tree clusters
    d = os.path.join(tmp, "two") + "/"
    MR.generate(MODELS, d, "Two.obj", 2)
    cases["two_objects"] = Case(d, "Two.obj", False, None, False)

    # one wall a single triangle: the last face line (half of a wall) goes, a non-quad record is in the word
    lines = _tor_lines()
    last = max(i for i, l in enumerate(lines) if l.startswith("f "))
    d = os.path.join(tmp, "tri") + "/"
    _write(d, "TriWall.obj", lines[:last] + lines[last + 1:])
    cases["triangle_wall"] = Case(d, "TriWall.obj", False, None, False)

    # Tor.obj under a skybox
    d = os.path.join(tmp, "sky") + "/"
    os.makedirs(d, exist_ok=True)
    MO.write_sky_bmp(os.path.join(d, "sky.bmp"))
    cases["skybox"] = Case(MODELS + "/", "Tor.obj", True, os.path.join(d, "sky.bmp"), False)

    # the smallest replica that is a big scene (4 x 256 + 14 = 1 038 triangles > kBigSceneTriangles)
    d = os.path.join(tmp, "x4") + "/"
    MR.generate(MODELS, d, "TorX4.obj", 4)
    cases["replica"] = Case(d, "TorX4.obj", False, None, True)
    assert sorted(cases) == sorted(NAMES)
    return cases
