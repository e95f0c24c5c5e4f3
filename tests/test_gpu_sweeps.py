"""mdh_spherecast and mdh_contacts on the device, host arrays, against the chain of tests/sweep_cases.py (the march in numpy
float32 over the oracle's distances; tests/test_sweeps_host.py holds the chain itself against orc_probe_raycast): every
variant k_ray_query is built for, batches around the wavefront and the workgroup, three radii and a seeded one, the scene's
max_dist and seeded lengths; the kinds a host lists, in LDS and in device memory, behind a partition that must not be
consulted; contacts; two analytic cases; nothing edited; every refusal; and the ball that a point test lets through a box.
(No ray here can reach the kernels' stall guard: max_dist is 20, where half an ulp is a thousandth of epsilon.)"""
import ctypes as C

import numpy as np
import pytest

import custom_kinds as ck
import ray_query_cases as rq
import ref64_cases
import sweep_cases as sw
import test_gpu_ray_queries as tq
from helpers import SEED, SMALL_PROBES, same_bits
from madarch_amd import _binding as B
from madarch_amd import examples, renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import boxes, planes, spheres

pytestmark = pytest.mark.gpu

N = tq.N
CASES = tq.CASES
INT_KEYS, BIT_KEYS = ("hit", "index", "steps"), ("t", "position", "normal")


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def assert_cast(got, want, n, what, keys=INT_KEYS + BIT_KEYS):
    for k in keys:
        if k in INT_KEYS:
            assert np.array_equal(got[k], want[k][:n]), "%s: %s, first at %s" % (what, k, np.argwhere(got[k] != want[k][:n])[:1])
        else:
            assert same_bits(got[k], want[k][:n]), "%s: %s, first at %s" % (what, k, np.argwhere(got[k] != want[k][:n])[:1])


# ------------------------------------------------------------------------------------------------ 1. the whole scene
_whole = {}


def whole(orc, name):
    """the chain's answers for the case's N rays, computed once: every batch is a prefix of the same rays, and the mesh and
    the residencies share theirs -> the oracle's renderer, rays, radii, lengths, {(radius #, length #): answers}"""
    key = name.replace(", global residency", "").replace("mesh, triangle BVH", "mesh")
    if key not in _whole:
        Ro = CASES[name][1](orc)
        org, drs = CASES[name][2](N)
        radii = list(sw.RADII) + [sw.seeded_radii(N)]
        lengths = [None, rq.seeded_tmax(N, SEED + 31)]
        want = {(i, j): sw.whole_scene_answers(orc, Ro, org, drs, r, t) for i, r in enumerate(radii) for j, t in enumerate(lengths)}
        _whole[key] = (Ro, org, drs, radii, lengths, want)
    return _whole[key]


def cut(v, n):
    return v[:n] if isinstance(v, np.ndarray) else v


@pytest.mark.parametrize("name", list(CASES))
def test_every_sweep_has_the_chains_bits(hip, orc, name):
    Ro, org, drs, radii, lengths, want = whole(orc, name)
    far, near = want[2, 0], want[2, 1]  # radius 0.3
    at_once = ((far["hit"] != 0) & (far["t"] == 0.0) & (far["steps"] == 1)).sum()
    print("%s, radius 0.3: %d of %d hit, %d at t = 0, %d miss; %d rays of radius 0 end at their tmax" % (
        name, (far["hit"] != 0).sum(), N, at_once, (far["hit"] == 0).sum(), ((want[0, 0]["hit"] != 0) & (want[0, 1]["hit"] == 0)).sum()))
    # the inputs exercise the code
    if name == "open scene":
        assert (far["hit"] == 0).sum() >= N // 10
    elif "mesh" in name:
        assert at_once >= N // 20  # (the strip of triangles is thin: 55 of its 1000 rays start within 0.3 of it)
    else:
        assert at_once >= N // 10
    for i in range(len(radii)):
        assert ((want[i, 0]["hit"] != 0) & (want[i, 1]["hit"] == 0)).any()  # rays that end at tmax and hit at max_dist
    R = CASES[name][0](hip)
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == CASES[name][3]
    for n in rq.BATCHES:
        for i, r in enumerate(radii):
            for j, t in enumerate(lengths):
                got = R.Spherecast(org[:n], drs[:n], cut(r, n), cut(t, n))
                assert_cast(got, want[i, j], n, "%s, %d rays, radius #%d, length #%d" % (name, n, i, j))
        # radius 0 (and NULL) up to max_dist: mdh_raycast, bit for bit, in all six outputs
        ray = R.Raycast(org[:n], drs[:n])
        for r in (None, 0.0):
            got = R.Spherecast(org[:n], drs[:n], r, None)
            for k in INT_KEYS + BIT_KEYS:
                assert same_bits(got[k], ray[k]), "%s, %d rays: %s is not Raycast's" % (name, n, k)
    # outputs nobody asked for are not written: the hits alone; and no rays at all
    only = np.full(65 + 8, -7, np.int32)
    rad = np.full(65, 0.3, np.float32)
    hip.check(hip.spherecast(R._h, 65, vp(org), vp(drs), vp(rad), None, None, 0, vp(only), None, None, None, None, None))
    assert np.array_equal(only[:65], far["hit"][:65]) and (only[65:] == -7).all()
    only[:] = -7
    hip.check(hip.spherecast(R._h, 0, vp(org), vp(drs), vp(rad), None, None, 0, vp(only), None, None, None, None, None))
    assert (only == -7).all()


# ------------------------------------------------------------------------------------------------ 3. contacts, whole scene
@pytest.mark.parametrize("name", list(CASES))
def test_contacts_of_the_whole_scene(hip, orc, name):
    Ro, org, drs, radii, _, _ = whole(orc, name)
    d, i = rq.orc_closest(orc, Ro, org)
    scan, nrm = sw.listed(Ro, sw.all_kinds(Ro))(org)
    same = scan.view(np.uint32) == d.view(np.uint32)
    print("%s: the scan over all kinds has the lookup's distance at %d of %d points" % (name, same.sum(), N))
    assert same.sum() >= N * 85 // 100 and ("partition" in name or same.all())
    R = CASES[name][0](hip)
    for n in rq.BATCHES:
        for r in radii[1:] + [None]:
            got = R.Contacts(org[:n], cut(r, n))
            rho = sw.per_ray(0.0 if r is None else cut(r, n), n)
            assert same_bits(got["dist"], (d[:n] - rho).astype(np.float32)), "%s, %d points: dist" % (name, n)
            assert np.array_equal(got["index"], i[:n]), "%s, %d points: index" % (name, n)
            assert same_bits(got["normal"][same[:n]], nrm[:n][same[:n]]), "%s, %d points: normal" % (name, n)
    # the distances alone
    dist = np.full(65 + 8, -7.0, np.float32)
    hip.check(hip.contacts(R._h, 65, vp(org), None, None, 0, vp(dist), None, None))
    assert same_bits(dist[:65], d[:65]) and (dist[65:] == -7.0).all()


# ------------------------------------------------------------------------------------------------ 2. listed kinds
LISTED_N = 257
LISTED_BATCHES = (1, 63, 64, 65, 257)
KIND_LISTS = (("Plane", "Box"), ("Triangle", "Sphere"), ("Sphere", "Plane", "Box", "Triangle"))
VARIANTS = {"LDS scan": (None, 0), "LDS, behind a partition": ("Clamp", 0), "global residency": (None, 1),
            "global residency, behind a partition": ("Fallback", 1)}
_listed = {}


def listed_case(orc):
    if not _listed:
        Ro = sw.make_four_kinds(orc)
        org, drs = sw.four_kinds_rays(LISTED_N)
        radii = [0.0, 0.05, sw.seeded_radii(LISTED_N)]
        lengths = [None, rq.seeded_tmax(LISTED_N, SEED + 37)]
        combos = ((0, 0), (1, 0), (2, 1), (1, 1))
        want, contact = {}, {}
        for names in KIND_LISTS:
            Rl = sw.make_four_kinds(orc, kinds=names)
            for i, j in combos:
                want[names, i, j] = sw.listed_answers(orc, Ro, Rl, names, org, drs, radii[i], lengths[j])
            dist, nrm = sw.listed(Ro, sw.kind_types(names))(org)
            d, ix = rq.orc_closest(orc, Rl, org)
            assert np.array_equal(d, dist)
            contact[names] = (dist, nrm, ix)
        _listed.update(Ro=Ro, org=org, drs=drs, radii=radii, lengths=lengths, combos=combos, want=want, contact=contact)
    return _listed


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_listed_kinds_are_an_exact_scan(hip, orc, variant):
    c = listed_case(orc)
    org, drs = c["org"], c["drs"]
    partition, residency = VARIANTS[variant]
    R = sw.make_four_kinds(hip, partition=partition, residency=residency)
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == residency
    for names in KIND_LISTS:
        prims = sw.kind_types(names)
        for i, j in c["combos"]:
            want = c["want"][names, i, j]
            hit = want["hit"] != 0
            assert hit.sum() >= LISTED_N // 16 and (hit & (want["t"] > 0.0)).any()  # (two triangles and two spheres stop few rays)
            assert j == 0 or (~hit).any()  # ... and a seeded length ends some
            for n in LISTED_BATCHES:
                got = R.Spherecast(org[:n], drs[:n], cut(c["radii"][i], n), cut(c["lengths"][j], n), prims)
                assert_cast(got, want, n, "%s, %s, %d rays, radius #%d, length #%d" % (variant, names, n, i, j))
        # the same answers whatever OPT_ADA_EVAL_DIV says: a march needs a distance
        ada = R.Get_Option(B.OPT_ADA_EVAL_DIV)
        for value in (0, 1):
            R.Set_Option(B.OPT_ADA_EVAL_DIV, value)
            assert_cast(R.Spherecast(org, drs, c["radii"][1], None, prims), c["want"][names, 1, 0], LISTED_N, "%s, %s, ADA_EVAL_DIV %d" % (variant, names, value))
        R.Set_Option(B.OPT_ADA_EVAL_DIV, ada)
        # contacts
        dist, nrm, ix = c["contact"][names]
        for n in LISTED_BATCHES:
            for r in (None, 0.05, c["radii"][2]):
                got = R.Contacts(org[:n], cut(r, n), prims)
                rho = sw.per_ray(0.0 if r is None else cut(r, n), n)
                assert same_bits(got["dist"], (dist[:n] - rho).astype(np.float32)), "%s, %s: dist" % (variant, names)
                assert np.array_equal(got["index"], ix[:n]), "%s, %s: index" % (variant, names)
                assert same_bits(got["normal"], nrm[:n]), "%s, %s: normal" % (variant, names)
    # the ball's case: a sphere of the scene swept from its own centre touches itself at once in the whole scene, and
    # nothing at once among the planes and boxes
    centre, radius = sw.SWEPT_SPHERE
    own = np.tile(np.asarray(centre, np.float32), (64, 1))
    dirs = rq.unit_dirs(np.random.RandomState(SEED % 983), 64)
    everything = R.Spherecast(own, dirs, radius, None)
    assert (everything["hit"] == 1).all() and (everything["t"] == 0.0).all() and (everything["steps"] == 1).all() and (everything["index"] == 1).all()
    walls = R.Spherecast(own, dirs, radius, None, (planes.Plane, boxes.Box))
    assert ((walls["hit"] == 0) | (walls["t"] > 0.0)).all() and (walls["hit"] == 1).any()
    assert (walls["index"][walls["hit"] == 1] >= sw.KIND_BASE["Plane"]).all()


def test_a_listed_kind_without_an_instance(hip):
    R = sw.make_four_kinds(hip, kinds=("Plane", "Box"))
    org, _ = sw.four_kinds_rays(65)
    for r in (None, 0.3):
        got = R.Contacts(org, r, (spheres.Sphere,))
        assert same_bits(got["dist"], np.full(65, sw.NO_INSTANCE - np.float32(r or 0.0), np.float32))
        assert (got["index"] == -1).all() and (got["normal"] == 0.0).all()


# ------------------------------------------------------------------------------------------------ 4. analytic
def test_a_dropped_sphere_and_a_head_on_approach(hip):
    """h - rho - EPS - 4 ulp (h) <= t <= h - rho + 4 ulp (h): the loop returns at the first dist < EPS, and total is a sum
    of distances that never overshoot (tests/test_sweeps_host.py: the same bounds in float64 and for the chain)"""
    R = ref64_cases.make_renderer(sw.floor_alone(), 16, 16, hip)
    org, drs, rho = sw.drop_rays()
    for prims in (None, (planes.Plane,)):
        got = R.Spherecast(org, drs, rho, None, prims)
        for k, (h, r) in enumerate(sw.DROPS):
            lo, hi = sw.analytic_bounds(h - r, h)
            print("drop from %g, radius %g: t = %.9g in [%.9g, %.9g]" % (h, r, got["t"][k], lo, hi))
            assert got["hit"][k] == 1 and lo <= float(got["t"][k]) <= hi
            assert np.array_equal(got["normal"][k], (0.0, 1.0, 0.0)) and got["index"][k] == 2  # (behind the two declared spheres)
    for Rs, L, r in sw.APPROACHES:
        R = ref64_cases.make_renderer(sw.sphere_alone(Rs), 16, 16, hip)
        for prims in (None, (spheres.Sphere,)):
            got = R.Spherecast(np.array([(0.0, 0.0, -L)], np.float32), np.array([(0.0, 0.0, 1.0)], np.float32), r, None, prims)
            lo, hi = sw.analytic_bounds(L - Rs - r, L)
            print("sphere %g from %g, radius %g: t = %.9g in [%.9g, %.9g]" % (Rs, L, r, got["t"][0], lo, hi))
            assert got["hit"][0] == 1 and got["index"][0] == 0 and lo <= float(got["t"][0]) <= hi
            assert np.array_equal(got["normal"][0], (0.0, 0.0, -1.0))


# ------------------------------------------------------------------------------------------------ 5. nothing is edited
@pytest.mark.parametrize("screen_replay", [0, 1])
def test_sweeps_edit_nothing(hip, screen_replay):
    """three frames with a sweep or a contact query between them, three frames without: the same framebuffer, and the
    radiance replay, the probe settle and the screen replay have counted the same passes of each kind"""
    org, drs = rq.room_rays(65)
    kinds = (planes.Plane, boxes.Box)
    outs = []
    for queries in (True, False):
        R = rq.gi_room(hip)
        R.Set_Option(B.OPT_SCREEN_REPLAY, screen_replay)
        for f in range(3):
            R.Render()
            if queries:
                (lambda: (R.Spherecast(org, drs, 0.2, 5.0), R.Contacts(org, 0.2)), lambda: (R.Spherecast(org, drs, 0.2, 5.0, kinds), R.Contacts(org, 0.2, kinds)),
                 lambda: R.Spherecast(org, drs))[f]()
        R.Finish()
        outs.append((R.Read_Framebuffer(), R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats()))
    (fb_q, rad_q, settle_q, scr_q), (fb, rad, settle, scr) = outs
    print("radiance replay %s, probe settle %s, screen replay %s" % (rad, settle, scr))
    assert same_bits(fb_q, fb)
    assert rad_q == rad and settle_q == settle and scr_q == scr
    assert sum(rad) >= 1 and (screen_replay == 0 or scr[1] + scr[2] > 0)  # (the counters do count)


def test_edits_are_seen_with_frames_in_flight(hip, orc):
    Rh, Ro = rq.gi_room(hip), rq.gi_room(orc)
    org, drs = rq.room_rays(257)
    before = Rh.Spherecast(org, drs, 0.05)
    assert np.array_equal(before["index"], sw.whole_scene_answers(orc, Ro, org, drs, 0.05)["index"])
    for _ in range(2):
        Rh.Render()  # (not waited for)
    for R in (Rh, Ro):
        R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.0, 3.0, 2.5), 1.2, 3))
    want = sw.whole_scene_answers(orc, Ro, org, drs, 0.05)
    assert (want["index"] != before["index"]).sum() > 10  # the move matters to these rays
    assert_cast(Rh.Spherecast(org, drs, 0.05), want, 257, "after Set_Primitive")
    # ... by the listed scan and by the contacts too
    listed_want = sw.chain(sw.listed(Ro, [spheres.Sphere]), org, drs, 0.05)
    assert_cast(Rh.Spherecast(org, drs, 0.05, None, (spheres.Sphere,)), listed_want, 257, "listed, after Set_Primitive", keys=("hit", "steps", "t", "position"))
    d, i = rq.orc_closest(orc, Ro, org)
    got = Rh.Contacts(org)
    assert same_bits(got["dist"], d) and np.array_equal(got["index"], i)
    Rh.Finish()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_rejections_launch_nothing(hip):
    """every refused call returns its status with the outputs untouched, and the frame rendered afterwards is the frame of a
    renderer that was never asked"""
    n = 65
    org, drs = rq.room_rays(n)
    R, Rref = rq.gi_room(hip), rq.gi_room(hip)
    hits, dist = np.full(n, -3, np.int32), np.full(n, -3.0, np.float32)
    five = np.full(n, 5.0, np.float32)
    kinds = np.array([1, 2], np.int32)

    def poisoned(a, at, value):
        b = a.copy()
        b[at] = value
        return b
    over = np.nextafter(rq.MAX_DIST, np.float32(np.inf))

    def cast(o=org, d=drs, r=five * 0.01, t=five, k=None, nk=0, h=hits, count=n, handle=R._h):
        return hip.spherecast(handle, count, vp(o), vp(d), vp(r), vp(t), vp(k), nk, vp(h), None, None, None, None, None)

    def touch(c=org, r=five * 0.01, k=None, nk=0, out=dist, count=n, handle=R._h):
        return hip.contacts(handle, count, vp(c), vp(r), vp(k), nk, vp(out), None, None)
    calls = [("no renderer", lambda: cast(handle=None)), ("no origins", lambda: cast(o=None)), ("no directions", lambda: cast(d=None)),
             ("no hits", lambda: cast(h=None)), ("n < 0", lambda: cast(count=-1)),
             ("NaN in a direction", lambda: cast(d=poisoned(drs, (64, 1), np.nan))), ("infinity in an origin", lambda: cast(o=poisoned(org, (3, 0), np.inf))),
             ("NaN radius", lambda: cast(r=poisoned(five, 7, np.nan))), ("negative radius", lambda: cast(r=poisoned(five, 7, -0.001))),
             ("radius above max_dist", lambda: cast(r=poisoned(five, 64, over))),
             ("infinite tmax", lambda: cast(t=poisoned(five, 0, np.inf))), ("negative tmax", lambda: cast(t=poisoned(five, 9, -1.0))),
             ("tmax above max_dist", lambda: cast(t=poisoned(five, 40, over))),
             ("kind index 3 of 3 kinds", lambda: cast(k=np.array([1, 3], np.int32), nk=2)), ("kind index -1", lambda: cast(k=np.array([-1], np.int32), nk=1)),
             ("kinds without a list", lambda: cast(k=None, nk=2)), ("n_kinds < 0", lambda: cast(k=kinds, nk=-1)),
             ("listed: NaN in a direction", lambda: cast(d=poisoned(drs, (64, 1), np.nan), k=kinds, nk=2)),
             ("contacts: no renderer", lambda: touch(handle=None)), ("contacts: no centres", lambda: touch(c=None)), ("contacts: no distances", lambda: touch(out=None)),
             ("contacts: n < 0", lambda: touch(count=-1)), ("contacts: NaN centre", lambda: touch(c=poisoned(org, (1, 2), np.nan))),
             ("contacts: negative radius", lambda: touch(r=poisoned(five, 7, -1.0))), ("contacts: radius above max_dist", lambda: touch(r=poisoned(five, 7, over))),
             ("contacts: infinite radius", lambda: touch(r=poisoned(five, 7, np.inf), k=kinds, nk=2)), ("contacts: kind index", lambda: touch(k=np.array([5], np.int32), nk=1))]
    R.Render()
    Rref.Render()
    for what, call in calls:
        assert call() == B.MDH_E_INVALID, what
    assert (hits == -3).all() and (dist == -3.0).all()
    R.Render()
    Rref.Render()
    assert same_bits(R.Read_Framebuffer(), Rref.Read_Framebuffer())
    assert R.Probe_Settle_Stats() == Rref.Probe_Settle_Stats() and R.Radiance_Replay_Stats() == Rref.Radiance_Replay_Stats()
    # the limits themselves are accepted: a radius and a length of 0 and of max_dist
    assert cast(r=poisoned(five, 7, 0.0), t=poisoned(five, 7, 0.0)) == B.MDH_OK and cast(r=poisoned(five, 7, rq.MAX_DIST), t=poisoned(five, 7, rq.MAX_DIST)) == B.MDH_OK
    assert hits[7] == 0 or hits[7] == 1
    # a scene with a user-defined kind
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    for call in (lambda: Rc.Spherecast(org, drs, 0.1), lambda: Rc.Spherecast(org, drs, 0.1, None, (spheres.Sphere,)), lambda: Rc.Contacts(org, 0.1),
                 lambda: Rc.Contacts(org, 0.1, (spheres.Sphere,))):
        assert tq._status(call) == B.MDH_E_STATE


# ------------------------------------------------------------------------------------------------ 7. the ball
def thrown_at_the_box(hip, swept):
    """a ball from (3, 0.5, 0) straight at the face z = 2.5 of the box (3, 0, 4) +- 1.5, so fast that one step of 0.1 s carries
    its centre from 2.5 in front of the box to 0.5 behind it"""
    G = examples.Ball_Game(16, 16, Probes=SMALL_PROBES, Binding=hip, Swept=swept)
    G.Move_Camera((1.0, -1.5, 0.0))
    G.Throw_Ball()
    G.Ball_Bodies[0][2] = np.array([0.0, 0.0, 60.0], np.float32)
    G.Step_Physics(0.1)
    return G


def test_a_fast_ball_passes_through_the_box_unless_it_is_swept(hip):
    _, pos, vel = thrown_at_the_box(hip, False).Ball_Bodies[0]
    print("the point test: the ball at %s, velocity %s" % (pos, vel))
    assert pos[2] > 5.5 + 0.2 and vel[2] == 60.0  # behind the box, on its way: the point test saw nothing
    G = thrown_at_the_box(hip, True)
    _, pos, vel = G.Ball_Bodies[0]
    print("swept: the ball at %s, velocity %s" % (pos, vel))
    gap = 2.5 - float(pos[2])  # the centre's distance to the face
    radius, slack = float(G.Ball_Radius), 4.0 * sw.ulp32(2.5)
    assert radius - slack <= gap <= radius + float(sw.EPS) + slack
    assert 1.5 < pos[0] < 4.5 and -1.5 < pos[1] < 1.5  # in front of the face itself
    fall = np.float32(-9.81) * np.float32(0.1)
    assert same_bits(vel, np.array([0.0, fall, -60.0], np.float32))  # reflected about (0, 0, -1)
    # the ball is the scene's: the next frame draws it where the physics put it
    G.R.Update_Partitioning()
    G.R.Render()
    G.R.Finish()
