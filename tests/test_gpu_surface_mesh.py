"""mdh_surface_mesh on the device, host arrays, against the restatement of tests/surface_cases.py over the oracle's distances
(tests/test_surface_mesh_host.py holds the restatement itself): positions, quads, counts and the field bit for bit and in
order in every variant k_ray_query is built for, over grids of one cell, of less than a wavefront, of a row across workgroups
and of more workgroups than one round of the scan takes; the device's own consistency with mdh_contacts; listed kinds;
capacities; nothing edited and edits seen; every refusal."""
import ctypes as C

import numpy as np
import pytest

import custom_kinds as ck
import ray_query_cases as rq
import surface_cases as sc
import sweep_cases as sw
import test_gpu_ray_queries as tq
import test_gpu_sweeps as ts
from helpers import SMALL_PROBES, same_bits
from madarch_amd import _binding as B
from madarch_amd import renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import boxes, spheres

pytestmark = pytest.mark.gpu

CASES = tq.CASES
F = np.float32
SHAPES = ((1, 1, 1), (4, 4, 4), (7, 5, 6), (130, 2, 2), (17, 16, 15))
BIG = (41, 41, 41)  # 68 921 cells, 74 088 corners: 290 workgroups, two rounds of the scan (the rooms alone)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def centred(centre, h, shape):
    return tuple(float(F(c - h * n / 2.0)) for c, n in zip(centre, shape))


def around_sphere(centre, radius):
    """grids round a sphere of the scene: the 4 x 4 x 4 one with the surface through its 56 outer cells (radius = 2.1 h),
    4.2 cells across the 7 x 5 x 6 one, 13 cells across the 17 x 16 x 15 one; a little off centre"""
    c = (centre[0] + 0.013, centre[1] - 0.021, centre[2] + 0.017)
    h4, h17 = radius / 2.1, 2.0 * radius / 13.0
    return {(1, 1, 1): (centred((centre[0] + radius, centre[1], centre[2]), h17, (1, 1, 1)), h17, 0.0),
            (4, 4, 4): (centred(c, h4, (4, 4, 4)), h4, 0.0), (7, 5, 6): (centred(c, h4, (7, 5, 6)), h4, 0.0),
            (17, 16, 15): (centred(c, h17, (17, 16, 15)), h17, 0.0)}


# the row of 130 x 2 x 2 cells lies along the floor y = -1 of the rooms and of the open scene, at the level 0.3: the level set
# y = -0.7 runs through its lower layer from end to end (outside the Fallback partition's grid: the border's scan)
FLOOR_ROW = ((-0.5, -0.7 - 0.6 * 0.05, 0.37), 0.05, 0.3)
GRIDS = {
    "rooms": {**around_sphere((3.0, 4.0, 3.0), 1.0), (130, 2, 2): FLOOR_ROW, BIG: ((0.5, -0.9, 0.5), 0.15, 0.0)},
    "partition": {**around_sphere((2.5, 3.5, 2.0), 0.5), (130, 2, 2): FLOOR_ROW},
    "open": {**around_sphere((4.5, 2.5, 3.0), 0.6), (130, 2, 2): FLOOR_ROW},
    # the strip of triangles has no closed body: levels 0.2 and 0.3 round it, and for the row the apex of its level 2
    "mesh": {(1, 1, 1): (centred((0.25, 1.0, 1.3), 0.1, (1, 1, 1)), 0.1, 0.3), (4, 4, 4): (centred((0.25, 1.0, 1.0), 0.35, (4, 4, 4)), 0.35, 0.3),
             (7, 5, 6): (centred((0.2, 0.5, 1.1), 0.3, (7, 5, 6)), 0.3, 0.3), (130, 2, 2): ((0.14, 0.996, 3.64525), 0.004, 2.0),
             (17, 16, 15): (centred((0.2, 1.0, 1.2), 0.1, (17, 16, 15)), 0.1, 0.2)},
}


def grids_of(name):
    key = "rooms" if name.startswith("rooms") else "partition" if name.startswith("partition") else "mesh" if name.startswith("mesh") else "open"
    return GRIDS[key]


_want = {}


def reference(orc, name):
    """the restatement's meshes for the case's grids, computed once (the residencies and the BVH share theirs), and the
    conditions under which they exercise the code -> the oracle's renderer, {shape: mesh}"""
    key = name.replace(", global residency", "").replace("mesh, triangle BVH", "mesh")
    if key not in _want:
        Ro = CASES[name][1](orc)
        D = sw.whole_scene(orc, Ro)
        want = {shape: sc.surface_nets(D, origin, h, shape, iso) for shape, (origin, h, iso) in grids_of(name).items()}
        for shape, m in want.items():
            print("%s, %s: %d vertices, %d quads, %d crossing edges on the border" % (key, shape, m["counts"][0], m["counts"][1], m["border_crossings"]))
            assert shape == (1, 1, 1) or (m["counts"][0] >= 50 and m["counts"][1] >= 30), (key, shape, m["counts"])
        assert max(m["counts"][0] for m in want.values()) > 256
        assert any(m["border_crossings"] > 0 for m in want.values())
        assert want[1, 1, 1]["counts"][1] == 0  # (one cell has no edge with four cells round it)
        _want[key] = (Ro, want)
    return _want[key]


def assert_mesh(got, want, what):
    assert (len(got["positions"]), len(got["quads"])) == tuple(want["counts"]), "%s: counts %s, not %s" % (what, (len(got["positions"]), len(got["quads"])), want["counts"])
    assert same_bits(got["positions"], want["positions"]), "%s: positions, first at %s" % (what, np.argwhere(got["positions"] != want["positions"])[:1])
    assert np.array_equal(got["quads"], want["quads"]), "%s: quads, first at %s" % (what, np.argwhere(got["quads"] != want["quads"])[:1])
    if "field" in got:
        assert same_bits(got["field"], want["field"]), "%s: field" % what


# ------------------------------------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("name", list(CASES))
def test_every_mesh_has_the_restatements_bits(hip, orc, name):
    Ro, want = reference(orc, name)
    R = CASES[name][0](hip)
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == CASES[name][3]
    for shape, (origin, h, iso) in grids_of(name).items():
        got = R.Surface_Mesh(origin, h, shape, iso, Field=True)
        assert_mesh(got, want[shape], "%s, %s" % (name, shape))
    # the largest grid first leaves the scratch larger than the next call needs: the same bits again
    shape = (4, 4, 4)
    origin, h, iso = grids_of(name)[shape]
    assert_mesh(R.Surface_Mesh(origin, h, shape, iso, Field=True), want[shape], "%s, %s again" % (name, shape))


# ------------------------------------------------------------------------------------------------ 2. consistency on the device
@pytest.mark.parametrize("iso", [0.0, 0.3])
@pytest.mark.parametrize("name", list(CASES))
def test_the_mesh_agrees_with_contacts(hip, orc, name, iso):
    """field = Contacts (corners, iso).dist, index and normal = Contacts (positions)'s, and where the scan over all kinds has
    the lookup's distance the normal is Eval_Distances_To's, as test_gpu_sweeps.test_contacts_of_the_whole_scene conditions it"""
    Ro, _ = reference(orc, name)
    R = CASES[name][0](hip)
    shape = (17, 16, 15)
    origin, h, _ = grids_of(name)[shape]
    got = R.Surface_Mesh(origin, h, shape, iso, Field=True)
    assert len(got["positions"]) >= 50 or ("mesh" in name and iso == 0.0)  # (triangles alone enclose nothing: no corner is inside at level 0)
    touch = R.Contacts(sc.corner_points(origin, h, shape), iso)
    assert same_bits(got["field"].ravel(), touch["dist"])
    at = R.Contacts(got["positions"])
    assert np.array_equal(got["index"], at["index"]) and same_bits(got["normals"], at["normal"])
    assert (got["index"] >= 0).all()
    d, i = rq.orc_closest(orc, Ro, got["positions"])
    scan, nrm = sw.listed(Ro, sw.all_kinds(Ro))(got["positions"])
    same = scan.view(np.uint32) == d.view(np.uint32)
    assert same.sum() >= len(same) * 85 // 100 and ("partition" in name or same.all())
    assert np.array_equal(got["index"], i)
    assert same_bits(got["normals"][same], nrm[same])


# ------------------------------------------------------------------------------------------------ 3. listed kinds
LISTED_GRID = ((0.31, -1.83, 0.22), 0.2, (29, 41, 28))  # holds the two spheres and the two boxes of sweep_cases.four_kinds
KIND_LISTS = (("Sphere", "Box"), ("Triangle", "Sphere"))
_listed = {}


def listed_reference(orc):
    if not _listed:
        Ro = sw.make_four_kinds(orc)
        origin, h, shape = LISTED_GRID
        for names in KIND_LISTS:
            for iso in (0.0, 0.1):
                _listed[names, iso] = sc.surface_nets(sw.listed(Ro, sw.kind_types(names)), origin, h, shape, iso)
        m = _listed[("Sphere", "Box"), 0.0]
        top = sc.topology(m["quads"])
        print("(Sphere, Box): %s vertices and quads, %d components, chi %s" % (m["counts"], top["components"], top["component_chi"]))
        # (three bodies, not four: the small sphere and the large box are 0.1 apart, less than a cell, and the net joins them)
        assert m["border_crossings"] == 0 and top["closed"] and top["components"] == 3 and top["component_chi"] == [2, 2, 2]
        assert all(m["counts"][0] >= 50 and m["counts"][1] >= 30 for m in _listed.values())
    return _listed


@pytest.mark.parametrize("variant", list(ts.VARIANTS))
def test_listed_kinds_are_meshed_from_their_exact_scan(hip, orc, variant):
    want = listed_reference(orc)
    partition, residency = ts.VARIANTS[variant]
    R = sw.make_four_kinds(hip, partition=partition, residency=residency)
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == residency
    origin, h, shape = LISTED_GRID
    for (names, iso), m in want.items():
        got = R.Surface_Mesh(origin, h, shape, iso, sw.kind_types(names), Field=True)
        assert_mesh(got, m, "%s, %s, level %g" % (variant, names, iso))
        at = R.Contacts(got["positions"], None, sw.kind_types(names))
        assert np.array_equal(got["index"], at["index"]) and same_bits(got["normals"], at["normal"])
    # the objects without the room's walls: closed bodies, V - E + F = 2 each
    got = R.Surface_Mesh(origin, h, shape, 0.0, (spheres.Sphere, boxes.Box))
    top = sc.topology(got["quads"])
    assert top["closed"] and top["components"] == 3 and top["component_chi"] == [2, 2, 2]
    assert set(np.unique(got["index"])) == {sw.KIND_BASE["Sphere"], sw.KIND_BASE["Sphere"] + 1, sw.KIND_BASE["Box"], sw.KIND_BASE["Box"] + 1}


# ------------------------------------------------------------------------------------------------ 4. capacities
def raw(hip, R, origin, h, shape, iso, vcap, qcap, pos=None, nrm=None, idx=None, quads=None, field=None, counts=None, kinds=None, nk=0, handle=0):
    o, c = np.asarray(origin, F), np.asarray(shape, np.int32)
    return hip.surface_mesh(R._h if handle == 0 else handle, vp(o), h, vp(c), iso, vp(kinds), nk, vcap, qcap, vp(pos), vp(nrm), vp(idx), vp(quads), vp(field), vp(counts))


def test_capacities_bound_what_is_written(hip, orc):
    name = "rooms, LDS scan"
    _, want = reference(orc, name)
    shape = (17, 16, 15)
    m = want[shape]
    origin, h, iso = grids_of(name)[shape]
    R = CASES[name][0](hip)
    counts = np.full(2 + 4, -7, np.int32)
    assert raw(hip, R, origin, h, shape, iso, 0, 0, counts=counts) == B.MDH_OK  # the pure count
    assert np.array_equal(counts[:2], m["counts"]) and (counts[2:] == -7).all()
    nv, nq = 65, 33
    assert m["counts"][0] > nv + 8 and m["counts"][1] > nq + 8
    pos, nrm, idx = np.full((nv + 8, 3), -7.0, F), np.full((nv + 8, 3), -7.0, F), np.full(nv + 8, -7, np.int32)
    quads = np.full((nq + 8, 4), -7, np.int32)
    counts[:] = -7
    assert raw(hip, R, origin, h, shape, iso, nv, nq, pos, nrm, idx, quads, None, counts) == B.MDH_OK
    assert np.array_equal(counts[:2], m["counts"])  # what was found, whatever the capacities
    assert same_bits(pos[:nv], m["positions"][:nv]) and (pos[nv:] == -7.0).all()
    assert np.array_equal(quads[:nq], m["quads"][:nq]) and (quads[nq:] == -7).all()
    full = R.Surface_Mesh(origin, h, shape, iso)
    assert same_bits(nrm[:nv], full["normals"][:nv]) and (nrm[nv:] == -7.0).all()
    assert np.array_equal(idx[:nv], full["index"][:nv]) and (idx[nv:] == -7).all()
    # an optional array left out is not written: the index alone, the quads alone, the field alone
    only = np.full(nv + 8, -7, np.int32)
    assert raw(hip, R, origin, h, shape, iso, nv, 0, idx=only, counts=counts) == B.MDH_OK
    assert np.array_equal(only[:nv], full["index"][:nv]) and (only[nv:] == -7).all()
    quads[:] = -7
    assert raw(hip, R, origin, h, shape, iso, 0, nq, quads=quads, counts=counts) == B.MDH_OK
    assert np.array_equal(quads[:nq], m["quads"][:nq]) and (quads[nq:] == -7).all()
    field = np.full(m["field"].size + 8, -7.0, F)
    assert raw(hip, R, origin, h, shape, iso, 0, 0, field=field, counts=counts) == B.MDH_OK
    assert same_bits(field[:-8], m["field"].ravel()) and (field[-8:] == -7.0).all()
    # capacities beyond what is found: everything, and nothing behind it
    big_pos = np.full((m["counts"][0] + 8, 3), -7.0, F)
    assert raw(hip, R, origin, h, shape, iso, len(big_pos), 0, pos=big_pos, counts=counts) == B.MDH_OK
    assert same_bits(big_pos[:-8], m["positions"]) and (big_pos[-8:] == -7.0).all()


# ------------------------------------------------------------------------------------------------ 5. nothing edited, edits seen
@pytest.mark.parametrize("screen_replay", [0, 1])
def test_meshing_edits_nothing(hip, screen_replay):
    """three frames with a mesh between them, three frames without: the same framebuffer, and the radiance replay, the probe
    settle and the screen replay have counted the same passes of each kind"""
    origin, h, iso = GRIDS["rooms"][17, 16, 15]
    outs = []
    for queries in (True, False):
        R = rq.gi_room(hip)
        R.Set_Option(B.OPT_SCREEN_REPLAY, screen_replay)
        for f in range(3):
            R.Render()
            if queries:
                m = R.Surface_Mesh(origin, h, (17, 16, 15), iso, (None, (spheres.Sphere, boxes.Box), None)[f], Field=f == 2)
                assert len(m["positions"]) > 256
        R.Finish()
        outs.append((R.Read_Framebuffer(), R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats()))
    (fb_q, rad_q, settle_q, scr_q), (fb, rad, settle, scr) = outs
    print("radiance replay %s, probe settle %s, screen replay %s" % (rad, settle, scr))
    assert same_bits(fb_q, fb)
    assert rad_q == rad and settle_q == settle and scr_q == scr
    assert sum(rad) >= 1 and (screen_replay == 0 or scr[1] + scr[2] > 0)  # (the counters do count)


def test_edits_are_seen_with_frames_in_flight(hip, orc):
    Rh, Ro = rq.gi_room(hip), rq.gi_room(orc)
    shape = (17, 16, 15)
    origin, h, iso = GRIDS["rooms"][shape]
    before = Rh.Surface_Mesh(origin, h, shape, iso)
    for _ in range(2):
        Rh.Render()  # (not waited for)
    for R in (Rh, Ro):
        R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.8, 3.9, 2.9), 0.8, 3))
    want = sc.surface_nets(sw.whole_scene(orc, Ro), origin, h, shape, iso)
    assert want["counts"][0] >= 50 and want["counts"][0] != len(before["positions"])  # the move matters to this grid
    assert_mesh(Rh.Surface_Mesh(origin, h, shape, iso, Field=True), want, "after Set_Primitive")
    Rh.Finish()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_rejections_launch_nothing(hip):
    """every refused call returns its status with the outputs and mdh_ray_query_time untouched"""
    shape = (4, 4, 4)
    origin, h, iso = GRIDS["rooms"][shape]
    R = rq.gi_room(hip)
    R.Set_Option(B.OPT_TIMING, 1)
    R.Render()
    ok = R.Surface_Mesh(origin, h, shape, iso)
    ms = R.Ray_Query_Time()
    assert ms > 0.0 and len(ok["positions"]) >= 50
    nv, nq = 8, 8
    pos, nrm, idx, quads = np.full((nv, 3), -3.0, F), np.full((nv, 3), -3.0, F), np.full(nv, -3, np.int32), np.full((nq, 4), -3, np.int32)
    field, counts = np.full(125, -3.0, F), np.full(2, -3, np.int32)
    kinds = np.array([0, 2], np.int32)
    over = float(np.nextafter(rq.MAX_DIST, F(np.inf)))

    def call(origin=origin, h=h, shape=shape, iso=iso, vcap=nv, qcap=nq, pos=pos, nrm=nrm, idx=idx, quads=quads, field=field, counts=counts, kinds=None, nk=0, handle=0):
        return raw(hip, R, origin, h, shape, iso, vcap, qcap, pos, nrm, idx, quads, field, counts, kinds, nk, handle)
    o, c = np.asarray(origin, F), np.asarray(shape, np.int32)
    args = (h, vp(c), iso, None, 0, nv, nq, vp(pos), vp(nrm), vp(idx), vp(quads), vp(field), vp(counts))
    calls = [("no renderer", lambda: hip.surface_mesh(None, vp(o), *args)), ("no origin", lambda: hip.surface_mesh(R._h, None, *args)),
             ("no cells", lambda: hip.surface_mesh(R._h, vp(o), h, None, *args[2:])), ("no counts", lambda: call(counts=None)),
             ("no cell along x", lambda: call(shape=(0, 4, 4))), ("a negative cell count", lambda: call(shape=(4, -1, 4))),
             ("NaN origin", lambda: call(origin=(np.nan, 0.0, 0.0))), ("infinite origin", lambda: call(origin=(0.0, np.inf, 0.0))),
             ("NaN spacing", lambda: call(h=np.nan)), ("infinite spacing", lambda: call(h=np.inf)), ("spacing 0", lambda: call(h=0.0)),
             ("negative spacing", lambda: call(h=-0.25)), ("NaN level", lambda: call(iso=np.nan)), ("infinite level", lambda: call(iso=np.inf)),
             ("level above max_dist", lambda: call(iso=over)), ("level below -max_dist", lambda: call(iso=-over)),
             ("a corner beyond 1024", lambda: call(origin=(1023.0, 0.0, 0.0), h=0.5)), ("an origin below -1024", lambda: call(origin=(0.0, -1025.0, 0.0))),
             ("negative vertex capacity", lambda: call(vcap=-1)), ("negative quad capacity", lambda: call(qcap=-1)),
             ("positions with capacity 0", lambda: call(vcap=0, nrm=None, idx=None)), ("an index with capacity 0", lambda: call(vcap=0, pos=None, nrm=None)),
             ("quads with capacity 0", lambda: call(qcap=0)), ("a vertex capacity without an array", lambda: call(pos=None, nrm=None, idx=None)),
             ("a quad capacity without quads", lambda: call(quads=None)),
             ("kind index 3 of 3 kinds", lambda: call(kinds=np.array([1, 3], np.int32), nk=2)), ("kind index -1", lambda: call(kinds=np.array([-1], np.int32), nk=1)),
             ("kinds without a list", lambda: call(kinds=None, nk=2)), ("n_kinds < 0", lambda: call(kinds=kinds, nk=-1)),
             ("too many kinds", lambda: call(kinds=np.zeros(64, np.int32), nk=64)),
             ("a grid beyond the cap", lambda: call(shape=(255, 256, 255), h=0.001, field=None)),
             ("a grid whose corner count overflows", lambda: call(shape=(2 ** 30, 2 ** 30, 2 ** 30), h=1.0e-9, field=None)),
             ("listed: NaN spacing", lambda: call(h=np.nan, kinds=kinds, nk=2))]
    for what, fn in calls:
        assert fn() == B.MDH_E_INVALID, what
        assert R.Ray_Query_Time() == ms, what
    for a in (pos, nrm, field):
        assert (a == -3.0).all()
    assert (idx == -3).all() and (quads == -3).all() and (counts == -3).all()
    # the limits themselves are accepted: the levels +-max_dist, a corner at 1024, the largest cube
    assert call(iso=float(rq.MAX_DIST)) == B.MDH_OK and call(iso=-float(rq.MAX_DIST)) == B.MDH_OK
    assert call(origin=(1022.0, 0.0, 0.0), h=0.5) == B.MDH_OK
    assert call(shape=(255, 255, 255), h=0.01, vcap=0, qcap=0, pos=None, nrm=None, idx=None, quads=None, field=None) == B.MDH_OK and counts[0] > 256
    # a scene with a user-defined kind
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    for fn in (lambda: Rc.Surface_Mesh(origin, h, shape, iso), lambda: Rc.Surface_Mesh(origin, h, shape, iso, (spheres.Sphere,))):
        assert tq._status(fn) == B.MDH_E_STATE
