"""The restatement of mdh_surface_mesh's definition (tests/surface_cases.py) against analytic float32 distances, on the CPU:
YARDSTICK tests -- they hold the yardstick the device tests compare with, and pass without the entry points.  The last test
holds what only the feature brings: the header, the binding table, the C++ mirror and the Ada spec name the two calls, and
meshes.Write_Obj writes what it is given."""
import os
import re

import numpy as np

import surface_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
H, ORIGIN, CELLS = 0.25, (-1.6, -1.5, -1.7), (13, 12, 14)
CENTRE, RADIUS = (0.13, 0.21, -0.07), 1.0


def sphere(centre, radius):
    c = np.asarray(centre, F)

    def D(p):
        d = (np.asarray(p, F) - c).astype(F)
        return ((np.sqrt((d * d).astype(F).sum(axis=1, dtype=F)).astype(F) - F(radius)).astype(F),)
    return D


def box(centre, half):
    c, b = np.asarray(centre, F), np.asarray(half, F)

    def D(p):
        q = (np.abs((np.asarray(p, F) - c).astype(F)) - b).astype(F)
        out = np.maximum(q, F(0.0))
        return ((np.sqrt((out * out).astype(F).sum(axis=1, dtype=F)).astype(F) + np.minimum(q.max(axis=1), F(0.0))).astype(F),)
    return D


def union(*Ds):
    return lambda p: (np.minimum.reduce([D(p)[0] for D in Ds]),)


def test_a_sphere_is_closed_oriented_and_near_its_surface():
    """yardstick: 300 vertices and 298 quads on this grid, every directed edge once and its reverse once, V - E + F = 2, no
    quad's normal towards the centre, and every vertex within h sqrt (3) of the sphere -- it lies in a cell the surface crosses"""
    m = sc.surface_nets(sphere(CENTRE, RADIUS), ORIGIN, H, CELLS)
    top = sc.topology(m["quads"])
    off = np.abs(np.linalg.norm(m["positions"].astype(np.float64) - np.asarray(CENTRE), axis=1) - RADIUS)
    print("sphere: %s vertices and quads, chi %d, largest | |x - c| - R | = %.4f (bound %.4f)" % (m["counts"], top["chi"], off.max(), H * 3 ** 0.5))
    assert tuple(m["counts"]) == (300, 298)
    assert top["closed"] and top["chi"] == 2 and top["components"] == 1
    assert m["border_crossings"] == 0
    assert off.max() <= H * 3 ** 0.5
    P = m["positions"].astype(np.float64)[m["quads"]]
    normal = np.cross(P[:, 2] - P[:, 0], P[:, 3] - P[:, 1])
    outward = P.mean(axis=1) - np.asarray(CENTRE)
    assert ((normal * outward).sum(axis=1) > 0.0).all()
    # the vertices in ascending cell id, the field with x fastest
    cells = m["cells"].astype(np.int64)
    ids = (cells[:, 2] * CELLS[1] + cells[:, 1]) * CELLS[0] + cells[:, 0]
    assert (np.diff(ids) > 0).all()
    assert m["field"].shape == (CELLS[2] + 1, CELLS[1] + 1, CELLS[0] + 1)
    p = sc.corner_points(ORIGIN, H, CELLS)
    assert np.array_equal(p[1] - p[0], [F(ORIGIN[0]) + F(H) - F(ORIGIN[0]), 0.0, 0.0])
    assert np.array_equal(m["field"].ravel(), sphere(CENTRE, RADIUS)(p)[0])


def test_two_spheres_and_a_box():
    """yardstick: two disjoint spheres have chi = 4, a box chi = 2"""
    two = union(sphere(CENTRE, RADIUS), sphere((2.43, 0.21, -0.07), 0.9))
    m = sc.surface_nets(two, ORIGIN, H, (22, 12, 14))
    top = sc.topology(m["quads"])
    assert top["closed"] and top["components"] == 2 and top["chi"] == 4 and top["component_chi"] == [2, 2]
    m = sc.surface_nets(box((0.1, 0.05, -0.1), (0.9, 0.7, 1.1)), ORIGIN, H, CELLS)
    top = sc.topology(m["quads"])
    assert top["closed"] and top["chi"] == 2 and len(m["quads"]) > 100


def test_a_surface_that_leaves_the_grid_is_open_at_the_border_only():
    """yardstick: the sphere at iso = 0.3 leaves the grid in y; every edge without its reverse lies in a cell on the border"""
    m = sc.surface_nets(sphere(CENTRE, RADIUS), ORIGIN, H, CELLS, 0.3)
    top = sc.topology(m["quads"])
    assert not top["closed"] and top["repeated"] == 0 and m["border_crossings"] > 0
    assert len(top["unmatched"]) > 0
    assert sc.on_border(m["cells"][top["unmatched"]], CELLS).all()
    assert np.array_equal(m["field"].ravel(), (sphere(CENTRE, RADIUS)(sc.corner_points(ORIGIN, H, CELLS))[0] - F(0.3)).astype(F))


def test_every_layer_names_the_two_calls(tmp_path):
    from madarch_amd import _binding, meshes, renderers
    header = open(os.path.join(ROOT, "include", "madarch_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("mdh_surface_mesh", "mdh_surface_mesh_device"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name[4:] in _binding.HIP_ONLY_ABI
        assert name in open(os.path.join(ROOT, "include", "madarch.hpp")).read()
        assert '"%s"' % name in open(os.path.join(ROOT, "ada", "madarch_hip.ads")).read()
    assert re.search(r"#define\s+MDH_SURFACE_MAX_CORNERS\s+%d\b" % _binding.SURFACE_MAX_CORNERS, header)
    assert len(_binding.HIP_ONLY_ABI["surface_mesh_device"][1]) == len(_binding.HIP_ONLY_ABI["surface_mesh"][1]) + 1
    assert hasattr(renderers.Renderer, "Surface_Mesh") and hasattr(renderers.Renderer, "Surface_Mesh_Device")
    # Write_Obj: the vertices, the normals and the faces counted from 1
    m = sc.surface_nets(sphere(CENTRE, RADIUS), ORIGIN, H, CELLS)
    path = str(tmp_path / "sphere.obj")
    meshes.Write_Obj(path, m["positions"], m["quads"])
    lines = open(path).read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == 300 and sum(l.startswith("f ") for l in lines) == 298
    back = np.array([l.split()[1:] for l in lines if l.startswith("v ")], np.float64).astype(F)
    assert np.array_equal(back, m["positions"])
    assert [int(x) for x in lines[300].split()[1:]] == list(m["quads"][0] + 1)
    meshes.Write_Obj(path, m["positions"], m["quads"], np.zeros_like(m["positions"]))
    assert sum(l.startswith("vn ") for l in open(path).read().splitlines()) == 300
