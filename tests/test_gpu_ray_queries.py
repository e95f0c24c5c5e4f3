"""mdh_raycast, mdh_raycast_visibility and mdh_softshadows on the device against the oracle, bit for bit and ray for ray:
every variant k_ray_query is built for (the scan in LDS, the partition with either border, global residency alone, behind
the partition and with the triangle BVH), batches around the wavefront and the workgroup, rays that hit at once, crawl
along a wall or leave the scene.  The yardsticks that are not an oracle export -- visibility from orc_probe_raycast, the
tolerance of soft shadows with min_dist > 0 -- are proved on the CPU in tests/test_ray_queries_host.py.
(No ray here can reach the kernels' stall guard: max_dist is 20, where half an ulp is a thousandth of epsilon.)"""
import ctypes as C

import numpy as np
import pytest

import custom_kinds as ck
import ray_query_cases as rq
from helpers import SEED, SMALL_PROBES, same_bits
from madarch_amd import _binding as B
from madarch_amd import renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import spheres

pytestmark = pytest.mark.gpu

N = max(rq.BATCHES)


def _simple_rays(n):
    """the room's mixture, with origins inside two spheres and two boxes of simple_scene (hits at t = 0)"""
    org, drs = rq.room_rays(n)
    rng = np.random.RandomState(SEED % 997)
    centres = np.array([(0.5, 3.5, 2.0), (3.5, 0.5, 5.0), (3.0, 1.0, 2.0), (2.0, 2.0, -2.0)], np.float32)
    at = np.arange(5, n, 37)
    org[at] = centres[np.arange(len(at)) % 4] + rng.uniform(-0.25, 0.25, (len(at), 3)).astype(np.float32)
    return org, drs


# name -> (the renderer over the HIP library, the same scene over the oracle, the rays, the kernel's residency)
CASES = {
    "rooms, LDS scan": (rq.gi_room, rq.gi_room, rq.room_rays, 0),
    "partition, Clamp": (lambda b: rq.simple_partition(b, scenes.Clamp, 0), rq.simple_partition, _simple_rays, 0),
    "partition, Fallback": (lambda b: rq.simple_partition(b, scenes.Fallback, 0), lambda b: rq.simple_partition(b, scenes.Fallback), _simple_rays, 0),
    "partition, Clamp, global residency": (lambda b: rq.simple_partition(b, scenes.Clamp, 1), rq.simple_partition, _simple_rays, 1),
    "partition, Fallback, global residency": (lambda b: rq.simple_partition(b, scenes.Fallback, 1), lambda b: rq.simple_partition(b, scenes.Fallback), _simple_rays, 1),
    "mesh, global residency": (lambda b: rq.small_mesh(b, residency=1), rq.small_mesh, rq.mesh_rays, 1),
    "mesh, triangle BVH": (lambda b: rq.small_mesh(b, residency=1, bvh=1), rq.small_mesh, rq.mesh_rays, 1),
    "open scene": (lambda b: rq.described(b, "open")[0], lambda b: rq.described(b, "open")[0], rq.open_rays, 0),
}

_answers = {}


def answers(orc, name):
    """the oracle's answers for the case's N rays, computed once: every batch is a prefix of the same rays"""
    key = name.replace(", global residency", "").replace("mesh, triangle BVH", "mesh")
    if key not in _answers:
        Ro = CASES[name][1](orc)
        org, drs = CASES[name][2](N)
        want = rq.oracle_answers(orc, Ro, org, drs)
        tmax = rq.seeded_tmax(N, SEED + 31)
        want["vis_far"] = rq.visibility_from_raycast(want, np.full(N, rq.MAX_DIST))
        want["vis"] = rq.visibility_from_raycast(want, tmax)
        for k in rq.SHADOW_KS:
            want["shadow", k] = rq.orc_softshadow(orc, Ro, org, drs, tmax, k)
        _answers[key] = (org, drs, tmax, want)
    return _answers[key]


def assert_batch(R, n, org, drs, tmax, want, what):
    got = R.Raycast(org[:n], drs[:n])
    for k in ("hit", "index", "steps"):
        assert np.array_equal(got[k], want[k][:n]), "%s, %d rays: %s" % (what, n, k)
    for k in ("t", "position", "normal"):
        assert same_bits(got[k], want[k][:n]), "%s, %d rays: %s, first at %s" % (what, n, k, np.argwhere(got[k] != want[k][:n])[:1])
    assert same_bits(R.Raycast_Visibility(org[:n], drs[:n], float(rq.MAX_DIST)), want["vis_far"][:n]), "%s, %d rays: visibility at max_dist" % (what, n)
    assert same_bits(R.Raycast_Visibility(org[:n], drs[:n], tmax[:n]), want["vis"][:n]), "%s, %d rays: visibility" % (what, n)
    for k in rq.SHADOW_KS:
        assert same_bits(R.Softshadows(org[:n], drs[:n], 0.0, tmax[:n], k), want["shadow", k][:n]), "%s, %d rays: soft shadows, k = %g" % (what, n, k)
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_every_ray_has_the_oracles_bits(hip, orc, name):
    org, drs, tmax, want = answers(orc, name)
    hit = want["hit"] != 0
    print("%s: %d of %d rays hit, %d at t = 0, most steps %d, %d visible below max_dist, %d in a penumbra" % (
        name, hit.sum(), N, (hit & (want["t"] == 0.0)).sum(), want["steps"].max(), int(want["vis"].sum()),
        ((want["shadow", 0.5] > 0.0) & (want["shadow", 0.5] < 1.0)).sum()))
    assert hit.sum() > N // 10 and (want["vis"] == 1.0).any() and (want["vis"] == 0.0).any()
    if name == "open scene":
        assert (~hit).sum() > N // 10  # rays that leave the scene
    elif "mesh" not in name:
        assert (hit & (want["t"] == 0.0) & (want["steps"] == 1)).sum() >= 8  # origins inside a primitive
        assert want["steps"].max() > 1000  # the crawl along the wall
    R = CASES[name][0](hip)
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == CASES[name][3]
    for n in rq.BATCHES:
        assert_batch(R, n, org, drs, tmax, want, name)
    # outputs nobody asked for are not written: the hits alone
    only = np.full(65, -7, np.int32)
    hip.check(hip.raycast(R._h, 65, org.ctypes.data_as(C.c_void_p), drs.ctypes.data_as(C.c_void_p), only.ctypes.data_as(C.c_void_p), None, None, None, None, None))
    assert np.array_equal(only, want["hit"][:65])
    hip.check(hip.raycast(R._h, 0, org.ctypes.data_as(C.c_void_p), drs.ctypes.data_as(C.c_void_p), only.ctypes.data_as(C.c_void_p), None, None, None, None, None))


def test_the_bvh_answers_as_the_scan_does(hip, orc):
    """the triangle BVH against the same renderer with the option off (and, above, against the oracle)"""
    org, drs, tmax, want = answers(orc, "mesh, triangle BVH")
    R = rq.small_mesh(hip, residency=1, bvh=1)
    on = assert_batch(R, N, org, drs, tmax, want, "BVH on")
    nodes = C.c_int32()
    hip.check(hip.triangle_bvh_info(R._h, C.byref(nodes), None, None, None))
    assert nodes.value > 0
    R.Set_Option(B.OPT_TRIANGLE_BVH, 0)
    off = assert_batch(R, N, org, drs, tmax, want, "BVH off")
    hip.check(hip.triangle_bvh_info(R._h, C.byref(nodes), None, None, None))
    assert nodes.value == 0
    for k in on:
        assert same_bits(on[k], off[k]), k


@pytest.mark.parametrize("name", ["room", "open"])
def test_soft_shadows_from_a_min_dist_against_float64(hip, name):
    """min_dist > 0 (the shaders' MIN_STEP * 5, and 0.1) has no oracle export: held against ref64.Run.softshadows with
    ref64.hold_values -- three runs (seeds None, 1, 2), FRAGILE_CAP as it is, and the tolerance of the CPU side:
    COLOUR_RTOL = 3e-3 / COLOUR_ATOL = 3e-4, under which the oracle's own min_dist = 0 results hold (largest error 0.001 of the
    tolerance, no fragile ray; tests/test_ray_queries_host.py, which also keeps these rays under the cap in float64 alone)."""
    R, desc = rq.described(hip, name)
    org, drs, tmax = rq.shadow_rays(name)
    for k in rq.SHADOW_KS:
        for tmin in rq.SHADOW_TMINS:
            got = R.Softshadows(org, drs, tmin, tmax, k)
            rq.hold_shadows("%s k %g min_dist %g" % (name, k, tmin), desc, org, drs, tmin, tmax, k, got)


def test_edits_are_seen_with_frames_in_flight(hip, orc):
    Rh, Ro = rq.gi_room(hip), rq.gi_room(orc)
    org, drs = rq.room_rays(257)
    before = Rh.Raycast(org, drs)
    assert np.array_equal(before["index"], rq.orc_raycast(orc, Ro, org, drs)["index"])
    for _ in range(2):
        Rh.Render()  # (not waited for)
    for R in (Rh, Ro):
        R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.0, 3.0, 2.5), 1.2, 3))
    want = rq.oracle_answers(orc, Ro, org, drs)
    got = Rh.Raycast(org, drs)
    assert (want["index"] != before["index"]).sum() > 10  # the move matters to these rays
    for k in ("hit", "index", "steps"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("t", "position", "normal"):
        assert same_bits(got[k], want[k]), k
    Rh.Finish()


@pytest.mark.parametrize("screen_replay", [0, 1])
def test_queries_edit_nothing(hip, screen_replay):
    """three frames with a query of each kind between them, three frames without: the same framebuffer, and the radiance
    replay, the probe settle and the screen replay have counted the same passes of each kind"""
    org, drs = rq.room_rays(65)
    outs = []
    for queries in (True, False):
        R = rq.gi_room(hip)
        R.Set_Option(B.OPT_SCREEN_REPLAY, screen_replay)
        for f in range(3):
            R.Render()
            if queries:
                (lambda: R.Raycast(org, drs), lambda: R.Raycast_Visibility(org, drs, 5.0), lambda: R.Softshadows(org, drs, 0.25, 5.0, 64.0))[f]()
        R.Finish()
        outs.append((R.Read_Framebuffer(), R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats()))
    (fb_q, rad_q, settle_q, scr_q), (fb, rad, settle, scr) = outs
    print("radiance replay %s, probe settle %s, screen replay %s" % (rad, settle, scr))
    assert same_bits(fb_q, fb)
    assert rad_q == rad and settle_q == settle and scr_q == scr
    assert sum(rad) >= 1 and (screen_replay == 0 or scr[1] + scr[2] > 0)  # (the counters do count)


def _status(call):
    try:
        call()
    except B.MadarchError as e:
        return e.status
    return B.MDH_OK


def test_rejections_launch_nothing(hip):
    """every refused call returns its status with the outputs untouched, and the frame rendered afterwards is the frame of a
    renderer that was never asked"""
    org, drs = rq.room_rays(65)
    R, Rref = rq.gi_room(hip), rq.gi_room(hip)
    bad_dir, bad_org = drs.copy(), org.copy()
    bad_dir[64, 1] = np.nan
    bad_org[3, 0] = np.inf
    five = np.full(65, 5.0, np.float32)
    far = five.copy()
    far[40] = np.nextafter(rq.MAX_DIST, np.float32(np.inf))
    sentinel = np.full(65, -3.0, np.float32)
    hits = np.full(65, -3, np.int32)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)
    calls = [
        ("NaN in a direction", lambda: hip.raycast(R._h, 65, vp(org), vp(bad_dir), vp(hits), None, None, None, None, None)),
        ("NaN in a direction", lambda: hip.raycast_visibility(R._h, 65, vp(org), vp(bad_dir), vp(five), vp(sentinel))),
        ("infinity in an origin", lambda: hip.raycast(R._h, 65, vp(bad_org), vp(drs), vp(hits), None, None, None, None, None)),
        ("infinity in an origin", lambda: hip.softshadows(R._h, 65, vp(bad_org), vp(drs), 0.0, vp(five), 64.0, vp(sentinel))),
        ("tmax above max_dist", lambda: hip.raycast_visibility(R._h, 65, vp(org), vp(drs), vp(far), vp(sentinel))),
        ("tmax above max_dist", lambda: hip.softshadows(R._h, 65, vp(org), vp(drs), 0.0, vp(far), 64.0, vp(sentinel))),
        ("tmin < 0", lambda: hip.softshadows(R._h, 65, vp(org), vp(drs), -0.001, vp(five), 64.0, vp(sentinel))),
        ("k not finite", lambda: hip.softshadows(R._h, 65, vp(org), vp(drs), 0.0, vp(five), float("inf"), vp(sentinel))),
        ("n < 0", lambda: hip.raycast(R._h, -1, vp(org), vp(drs), vp(hits), None, None, None, None, None)),
        ("no hit_out", lambda: hip.raycast(R._h, 65, vp(org), vp(drs), None, None, None, None, None, None)),
    ]
    R.Render()
    Rref.Render()
    for what, call in calls:
        assert call() == B.MDH_E_INVALID, what
    assert (sentinel == -3.0).all() and (hits == -3).all()
    R.Render()
    Rref.Render()
    assert same_bits(R.Read_Framebuffer(), Rref.Read_Framebuffer())
    assert R.Probe_Settle_Stats() == Rref.Probe_Settle_Stats() and R.Radiance_Replay_Stats() == Rref.Radiance_Replay_Stats()
    # a scene with a user-defined kind: neither the interpreter nor the hiprtc kernels answer ray queries
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rc.Raycast(org, drs)) == B.MDH_E_STATE
    assert _status(lambda: Rc.Raycast_Visibility(org, drs, 5.0)) == B.MDH_E_STATE
    assert _status(lambda: Rc.Softshadows(org, drs, 0.0, 5.0, 64.0)) == B.MDH_E_STATE
