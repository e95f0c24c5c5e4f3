"""MDH_OPT_TRIANGLE_BVH on the device: every observable output with the triangles walked through their hierarchy against the
same library scanning them one by one (the same bits), against the oracle (the parity bar), the distance query, the
option's refusals and the hierarchy the renderer reports."""
import ctypes as C

import numpy as np
import pytest

import bvh_scenes as S
import custom_kinds as ck
from helpers import SEED, SMALL_PROBES, assert_parity, make, same_bits, seeded_points, snapshot
from madarch_amd import _binding as B
from madarch_amd import meshes, renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import triangles

pytestmark = pytest.mark.gpu

BVH = B.OPT_TRIANGLE_BVH


def hit_share(snap):
    return float((snap["gb_index"] >= 0).mean())


def on_against_off(build, frames=2):
    """`build(bvh)` -> a renderer; its snapshots with the option on and off, bit for bit"""
    snaps = []
    for bvh in (True, False):
        R = build(bvh)
        assert R.Get_Option(BVH) == (1 if bvh else 0)
        snaps.append(snapshot(R, frames))
        if bvh:
            assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == 1
        R.Destroy()
    on, off = snaps
    print("%.3f of the pixels hit" % hit_share(off))
    assert hit_share(off) >= 0.1  # a frame of misses is no parity
    assert sorted(on) == sorted(off)
    for k in off:
        assert same_bits(on[k], off[k]), k
    return on, off


CASES = {
    "one": lambda: (S.fan(1), {}),
    "five": lambda: (S.fan(5), {}),
    "torus200": lambda: (S.facing_torus(10, 10), {}),
    "torus1000": lambda: (S.facing_torus(25, 20), {}),
    "mixed": lambda: (S.facing_torus(6, 5), {"others": True}),
    "degenerate": lambda: (S.degenerate_mesh(), {}),
    "inside": lambda: (meshes.torus(10, 10), {}),  # the camera at the centre of the ring, inside the mesh's bounding box
    "volumetrics": lambda: (S.facing_torus(6, 5), {"vol": True}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_keep_their_bits(hip, name):
    tris, kw = CASES[name]()
    on, _ = on_against_off(lambda bvh: S.tri_renderer(hip, tris, bvh, **kw))
    if name == "volumetrics":
        assert "visibility" in on and "scattering" in on


def test_coincident_triangles_keep_the_lower_index(hip):
    tris = S.coincident_mesh()
    on, off = on_against_off(lambda bvh: S.tri_renderer(hip, tris, bvh, mats=[0, 1]))
    for snap in (on, off):
        hit = snap["gb_index"] >= 0
        assert hit.mean() >= 0.1 and (snap["gb_index"][hit] == 0).all()


def test_rebuild_with_frames_in_flight(hip):
    """eight frames kept in flight, one triangle moved between frames 3 and 4: the rebuild and the ring of images"""
    tris = S.facing_torus(10, 10)

    def build(bvh):
        R = S.tri_renderer(hip, tris, bvh)
        R.Set_Option(B.OPT_FRAME_OVERLAP, 2)
        for f in range(8):
            if f == 4:
                a, b, c = tris[17] + np.asarray((0.3, -0.2, -0.9), dtype=np.float32)
                R.Set_Primitive(triangles.Triangle, 18, triangles.Create(a, b, c, 1))
            R.Render()
        return R
    on_against_off(build, frames=0)


@pytest.mark.parametrize("seed", range(10))
def test_seeded_scenes(hip, seed):
    tris = S.fuzz_mesh(seed)
    assert 8 <= len(tris) <= 120
    on_against_off(lambda bvh: S.tri_renderer(hip, tris, bvh))


@pytest.mark.parametrize("name", ["torus200", "mixed"])
def test_against_the_oracle(hip, orc, name):
    tris, kw = CASES[name]()
    Rh, Ro = S.tri_renderer(hip, tris, True, **kw), S.tri_renderer(orc, tris, None, **kw)
    sh, so = snapshot(Rh, 2), snapshot(Ro, 2)
    assert hit_share(so) >= 0.1
    assert_parity(sh, so)


@pytest.mark.parametrize("ada_div", [0, 1])
def test_eval_distances(hip, ada_div):
    """the distance query: 4 096 seeded points, points at 1e6, points on vertices and a NaN point (with the Ada division of
    MDH_OPT_ADA_EVAL_DIV the query scans whatever the option says: that value is no distance)"""
    tris = S.facing_torus(10, 10)
    far = np.asarray([(1.0e6, 0.0, 0.0), (0.0, -1.0e6, 3.0), (1.0e6, 1.0e6, 1.0e6), (-1.0e6, 2.0, -1.0e6)], dtype=np.float32)
    pts = np.concatenate((seeded_points(4096, (-3.0, -3.0, 0.0), (3.0, 3.0, 6.0), SEED), far, tris[::13, 0], tris[5::17, 2],
                          np.asarray([(np.nan, 0.5, 3.0)], dtype=np.float32))).astype(np.float32)
    res = []
    for bvh in (True, False):
        R = S.tri_renderer(hip, tris, bvh, W=16, H=16)
        R.Set_Option(B.OPT_ADA_EVAL_DIV, ada_div)
        res.append(R.Eval_Distances_To(pts, (triangles.Triangle,)))
        R.Destroy()
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
    assert np.isfinite(res[1][0][:4096]).all()


def test_refused_where_it_cannot_hold(hip):
    R = make("simple_scene", 32, 24, hip, probes=SMALL_PROBES)  # a space partition
    with pytest.raises(B.MadarchError) as e:
        R.Set_Option(BVH, 1)
    assert e.value.status == B.MDH_E_STATE
    R.Set_Option(BVH, 0)
    scene = scenes.Compile([(ck.My_Sphere, 2), (triangles.Triangle, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(32, 24), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    with pytest.raises(B.MadarchError) as e:
        R.Set_Option(BVH, 1)
    assert e.value.status == B.MDH_E_STATE
    # (a scene cannot declare two Triangle kinds: mdh_create refuses a built-in kind declared twice)
    scene = scenes.Compile([(triangles.Triangle, 2), (triangles.Triangle, 3)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    with pytest.raises(B.MadarchError) as e:
        renderers.Create(windows.Open(32, 24), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    assert e.value.status == B.MDH_E_INVALID
    R = S.tri_renderer(hip, S.fan(2), None)
    for bad in (2, -1):
        with pytest.raises(B.MadarchError) as e:
            R.Set_Option(BVH, bad)
        assert e.value.status == B.MDH_E_INVALID
    # no triangles declared: accepted, and nothing changes
    R = make("global_illumination", 32, 24, hip, probes=SMALL_PROBES)
    R.Set_Option(BVH, 1)
    assert R.Get_Option(BVH) == 1 and R.Get_Option(B.OPT_TABLE_RESIDENCY) == 0
    R.Render()


@pytest.mark.parametrize("name", ["degenerate", "torus1000", "five"])
def test_info_agrees_with_the_builder(hip, name):
    tris, _ = CASES[name]()
    nodes, perm, always, _, _ = S.bvh_build(tris)
    R = S.tri_renderer(hip, tris, True, W=16, H=16)
    out = [C.c_int32(-1) for _ in range(4)]
    hip.check(hip.triangle_bvh_info(R._h, *[C.byref(o) for o in out]))
    n_nodes, leaves, depth, n_always = (o.value for o in out)
    assert n_nodes == len(nodes) and n_always == len(always)
    assert leaves == int((nodes["leaf"] >= 0).sum())
    def deep(i):  # an inner node's children: the next node, and the one its first child's skip link names
        return 1 if nodes[i]["leaf"] >= 0 else 1 + max(deep(i + 1), deep(int(nodes[i + 1]["skip"])))
    assert depth == deep(0)
    R.Set_Option(BVH, 0)
    hip.check(hip.triangle_bvh_info(R._h, *[C.byref(o) for o in out]))
    assert [o.value for o in out] == [0, 0, 0, 0]
