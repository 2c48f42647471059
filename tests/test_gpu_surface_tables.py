"""A handle's device keeps ONE set of stand-ins for the surface tables it does not have (pt_capi_internal.hpp: DeviceSurface), uploaded
once and outliving every table they stand in for.  What no unit's own test reaches: a table that comes and goes below a higher one.
On the generated lights_room.obj, 16 x 12 pixels, 4 samples, MRR 3: with direct lighting as the top unit each of textures, dielectrics,
shading normals and roughness is set (the image changes: the table was live), then cleared (the image is the one of direct lighting
alone again, bit for bit -- the stand-in is back in the slot); the same with roughness as the top unit and shading normals below it;
and a copy made by clone_to_device while two tables are set renders what its source renders, bit for bit."""
import importlib

import numpy as np
import pytest

import direct_scenes as DS

pt = importlib.import_module("path-tracing_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32
W, H, SPP, MRR = 16, 12, 4, 3


def _render(sc):
    s, s2, c, _ = sc.render_host(W, H, SPP, MRR, seed=42, want_stats=False)
    return s.view(np.uint32).copy(), s2.view(np.uint32).copy(), c.copy()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("surface_gpu")) + "/"
    DS.lights_room(d)
    sc = pt.Scene.load_obj(d, "lights_room.obj", device=0)
    n_tri = sc.counts()[0]
    rng = np.random.default_rng(5)
    sc.set_texcoords(rng.uniform(0, 1, (n_tri, 3, 2)).astype(F32))
    # name -> (setter, value, cleared): the walls textured, the chalk box of glass, every corner's normal tilted, the floor rough
    tables = {"textures": ("set_textures", [pt.texture(1, rng.uniform(0, 1, (3, 5, 3)).astype(F32), "nearest")], None),
              "glass": ("set_dielectrics", [pt.dielectric(4, 1.5, (0.9, 1.0, 0.8))], None),
              "smooth": ("set_shading_normals", rng.normal(size=(n_tri, 3, 3)).astype(F32), None),
              "rough": ("set_roughness", [pt.rough(2, 0.3)], None)}
    return sc, tables


def _comes_and_goes(sc, tables, names):
    reference = _render(sc)
    for name in names:
        setter, value, cleared = tables[name]
        getattr(sc, setter)(value)
        assert not _same(_render(sc), reference), name + " changed nothing: the table was not live"
        getattr(sc, setter)(cleared)
        assert _same(_render(sc), reference), name + " was cleared and the image is not the reference's"


def test_a_table_below_direct_lighting_comes_and_goes(scene):
    sc, tables = scene
    sc.set_direct_lighting(True)
    try:
        _comes_and_goes(sc, tables, ("textures", "glass", "smooth", "rough"))
    finally:
        sc.set_direct_lighting(False)


def test_shading_normals_below_a_roughness_list_come_and_go(scene):
    sc, tables = scene
    sc.set_roughness(tables["rough"][1])
    try:
        _comes_and_goes(sc, tables, ("smooth",))
    finally:
        sc.set_roughness(None)


def test_a_copy_made_while_two_tables_are_set_renders_what_its_source_renders(scene):
    sc, tables = scene
    sc.set_textures(tables["textures"][1])
    sc.set_roughness(tables["rough"][1])
    try:
        copy = sc.clone_to_device(0)
        assert len(copy.textures()) == 1 and len(copy.roughness()) == 1
        assert _same(_render(copy), _render(sc))
    finally:
        sc.set_roughness(None)
        sc.set_textures(None)
