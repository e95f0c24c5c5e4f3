"""The checks of the device-array ray queries (mdh_raycast_device, mdh_raycast_visibility_device, mdh_softshadows_device,
mdh_ray_query_wait) on the device, with torch tensors as the device memory.  They run in a process of their own, started
once by tests/test_gpu_ray_streams.py: a process that uses PyTorch beside the library has to import torch BEFORE the library
is loaded (the wheel carries its own ROCm runtime under the system's SONAMEs), which the suite's
shared process -- where the library has long been loaded without torch -- cannot arrange, and should not: every other test
keeps the runtime it has always run on.  main () imports torch, loads the library, runs the named checks (all by default)
and writes one JSON object: check -> {ok, log, seconds}.  After a device error nothing more is started.

The scenes, rays and oracle answers are those of tests/ray_query_cases.py; the eight cases are the table of
tests/test_gpu_ray_queries.py, rebuilt here from the same helpers.  The host-array calls are the second yardstick: the
existing test holds them against the oracle, bit for bit."""
import ctypes as C
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import custom_kinds as ck  # noqa: E402
import ray_query_cases as rq  # noqa: E402
from helpers import SEED, SMALL_PROBES, same_bits  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402
from madarch_amd import renderers, scenes, windows  # noqa: E402
from madarch_amd.lights import point_lights  # noqa: E402
from madarch_amd.primitives import spheres  # noqa: E402

torch = None  # main (): imported before the library is loaded
hip = orc = None

N = max(rq.BATCHES)
SCHEDULES = ((1, 1), (16, 1), (64, 1), (16, 0), (64, 0))  # (MDH_OPT_RAY_STREAM_REFILL, MDH_OPT_RAY_STREAM_GROUPS)
PAD, FILL = 64, -7
BAD_BITS = 0x7FC00000


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
KEYS = ("hit", "index", "steps", "t", "position", "normal", "vis_far", "vis") + tuple(("shadow", k) for k in rq.SHADOW_KS)

CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


# ------------------------------------------------------------------------------------ device memory
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(n, dtype):
    return torch.full((n,), FILL, dtype=dtype, device="cuda")


def set_schedule(R, refill, groups):
    R.Set_Option(B.OPT_RAY_STREAM_REFILL, refill)
    R.Set_Option(B.OPT_RAY_STREAM_GROUPS, groups)


def device_rays(org, drs, tmax):
    return {"org": dev(org), "dir": dev(drs), "tmax": dev(tmax), "far": dev(np.full(len(org), rq.MAX_DIST, np.float32))}


def device_queries(R, d, n, stream=0, pad=0):
    """all five queries for the first n rays of d, into fresh tensors of n + pad entries filled with FILL -> the tensors"""
    out = {"hit": filled(n + pad, torch.int32), "index": filled(n + pad, torch.int32), "steps": filled(n + pad, torch.int32),
           "t": filled(n + pad, torch.float32), "position": filled(3 * (n + pad), torch.float32), "normal": filled(3 * (n + pad), torch.float32),
           "vis_far": filled(n + pad, torch.float32), "vis": filled(n + pad, torch.float32)}
    for k in rq.SHADOW_KS:
        out["shadow", k] = filled(n + pad, torch.float32)
    R.Raycast_Device(d["org"], d["dir"], out["hit"], out["index"], out["t"], out["steps"], out["position"], out["normal"], Stream=stream, N=n)
    R.Raycast_Visibility_Device(d["org"], d["dir"], d["far"], out["vis_far"], Stream=stream, N=n)
    R.Raycast_Visibility_Device(d["org"], d["dir"], d["tmax"], out["vis"], Stream=stream, N=n)
    for k in rq.SHADOW_KS:
        R.Softshadows_Device(d["org"], d["dir"], 0.0, d["tmax"], k, out["shadow", k], Stream=stream, N=n)
    return out


def to_host(out):
    """(a copy on torch's current stream: ordered behind the queries that were given that stream)"""
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("position", "normal"):
        if k in got:
            got[k] = got[k].reshape(-1, 3)
    return got


def host_queries(R, org, drs, tmax):
    """the host-array calls: the yardstick tests/test_gpu_ray_queries.py holds against the oracle"""
    want = R.Raycast(org, drs)
    want["vis_far"] = R.Raycast_Visibility(org, drs, float(rq.MAX_DIST))
    want["vis"] = R.Raycast_Visibility(org, drs, tmax)
    for k in rq.SHADOW_KS:
        want["shadow", k] = R.Softshadows(org, drs, 0.0, tmax, k)
    return want


def assert_same(got, want, n, what, keys=KEYS, at=None):
    """the first n entries of got (or those at `at`) have want's bits"""
    for k in keys:
        g, w = np.asarray(got[k])[:n], np.asarray(want[k])[:n]
        if at is not None:
            g, w = g[at], w[at]
        if g.dtype.kind == "i":
            assert np.array_equal(g, w), "%s: %s, first at %s" % (what, k, np.argwhere(g != w)[:1])
        else:
            assert same_bits(g, w), "%s: %s, first at %s" % (what, k, np.argwhere(~((g == w) | ((g != g) & (w != w))))[:1])


def assert_tail_untouched(got, n, what):
    for k, v in got.items():
        assert (np.asarray(v)[n:] == FILL).all(), "%s: %s written behind ray %d" % (what, k, n)


_answers = {}


def answers(name):
    """the oracle's answers for the case's N rays, computed once (the mesh and the residencies share theirs)"""
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


# ------------------------------------------------------------------------------------------- checks
def oracle_bits(name):
    """1000 rays through one workgroup that refills at 16 idle lanes: four wavefronts serve them all by refills"""
    org, drs, tmax, want = answers(name)
    R = CASES[name][0](hip)
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == CASES[name][3]
    set_schedule(R, 16, 1)
    got = to_host(device_queries(R, device_rays(org, drs, tmax), N))
    print("%s: %d of %d rays hit, most steps %d, mean %.1f" % (name, (want["hit"] != 0).sum(), N, want["steps"].max(), want["steps"].mean()))
    assert_same(got, want, N, name)


def schedule_changes_no_bit(name):
    org, drs, tmax, _ = answers(name)
    R = CASES[name][0](hip)
    d = device_rays(org, drs, tmax)
    perm = np.random.RandomState((SEED + 41) & 0x7FFFFFFF).permutation(N)
    for n in rq.BATCHES:
        want = host_queries(R, org[:n], drs[:n], tmax[:n])
        for refill, groups in SCHEDULES:
            set_schedule(R, refill, groups)
            got = to_host(device_queries(R, d, n))
            assert_same(got, want, n, "%s, %d rays, refill %d, groups %d" % (name, n, refill, groups))
        # the same rays in another order: other neighbours in the wavefront, other rays taken behind them
        p = perm[perm < n]
        dp = device_rays(org[p], drs[p], tmax[p])
        for refill, groups in ((16, 1), (1, 0)):
            set_schedule(R, refill, groups)
            got = to_host(device_queries(R, dp, n))
            back = {k: np.empty_like(v) for k, v in got.items()}
            for k in got:
                back[k][p] = got[k]
            assert_same(back, want, n, "%s, %d rays permuted, refill %d, groups %d" % (name, n, refill, groups))


for _name in CASES:
    CHECKS["the oracle's bits: " + _name] = (lambda name: lambda: oracle_bits(name))(_name)
for _name in CASES:
    CHECKS["the schedule changes no bit: " + _name] = (lambda name: lambda: schedule_changes_no_bit(name))(_name)


@check("every ray is answered once and nothing else is written")
def answered_once():
    for name in ("rooms, LDS scan", "partition, Fallback, global residency", "mesh, triangle BVH"):
        org, drs, tmax, _ = answers(name)
        R = CASES[name][0](hip)
        d = device_rays(org, drs, tmax)
        for n in (65, 257):
            want = host_queries(R, org[:n], drs[:n], tmax[:n])
            for refill in (1, 16, 64):
                set_schedule(R, refill, 1)
                what = "%s, %d rays, refill %d" % (name, n, refill)
                got = to_host(device_queries(R, d, n, pad=PAD))
                assert_same(got, want, n, what)  # (no FILL among them: every entry was written)
                for k in ("hit", "index", "steps", "t", "vis", "vis_far"):
                    assert (got[k][:n] != FILL).all(), k
                flat = {k: v.reshape(-1) if k in ("position", "normal") else v for k, v in got.items()}
                assert_tail_untouched({k: v for k, v in flat.items() if k not in ("position", "normal")}, n, what)
                assert_tail_untouched({k: flat[k] for k in ("position", "normal")}, 3 * n, what)
                # the hits alone: the optional outputs are null
                only = filled(n + PAD, torch.int32)
                R.Raycast_Device(d["org"], d["dir"], only, N=n)
                only = only.cpu().numpy()
                assert np.array_equal(only[:n], want["hit"]) and (only[n:] == FILL).all(), what
        # no rays: MDH_OK, nothing launched
        none = filled(PAD, torch.int32)
        R.Raycast_Device(d["org"], d["dir"], none, N=0)
        assert (none.cpu().numpy() == FILL).all()


@check("bad rays are refused, not marched")
def bad_rays():
    n = 257
    for name in ("rooms, LDS scan", "partition, Clamp, global residency"):
        org, drs, tmax, _ = answers(name)
        org, drs, tmax = org[:n].copy(), drs[:n].copy(), tmax[:n].copy()
        R = CASES[name][0](hip)
        clean = host_queries(R, org, drs, tmax)
        rng = np.random.RandomState((SEED + 53) & 0x7FFFFFFF)
        places = rng.permutation(n)[:40]
        poison = (np.nan, np.inf, -np.inf)
        bad_ray, bad_len = places[:24], places[24:]
        for i, q in enumerate(bad_ray):  # every component of origin and direction, every poison
            (org if i % 6 < 3 else drs)[q, i % 3] = poison[(i // 6) % 3]
        long_ = tmax.copy()
        for i, q in enumerate(bad_len):
            long_[q] = (np.nan, np.inf, np.nextafter(rq.MAX_DIST, np.float32(np.inf)), np.float32(1e30))[i % 4]
        good = np.ones(n, bool)
        good[bad_ray] = False
        good_len = good.copy()
        good_len[bad_len] = False
        d = device_rays(org, drs, long_)
        for refill, groups in ((1, 1), (16, 1), (64, 0)):
            set_schedule(R, refill, groups)
            what = "%s, refill %d, groups %d" % (name, refill, groups)
            got = to_host(device_queries(R, d, n, pad=PAD))
            assert_same(got, clean, n, what, keys=("hit", "index", "steps", "t", "position", "normal", "vis_far"), at=good)
            assert_same(got, clean, n, what, keys=("vis",) + tuple(("shadow", k) for k in rq.SHADOW_KS), at=good_len)
            assert (got["hit"][:n][bad_ray] == -1).all() and (got["index"][:n][bad_ray] == -1).all() and (got["steps"][:n][bad_ray] == 0).all(), what
            for k in ("t", "position", "normal"):
                assert (got[k][:n][bad_ray] == 0.0).all(), "%s: %s" % (what, k)
            assert (got["vis_far"][:n].view(np.uint32)[bad_ray] == BAD_BITS).all(), what
            for k in ("vis",) + tuple(("shadow", k) for k in rq.SHADOW_KS):
                assert (got[k][:n].view(np.uint32)[~good_len] == BAD_BITS).all(), "%s: %s" % (what, k)
                assert (got[k][n:] == FILL).all()


@check("ordered with the caller's stream")
def ordering():
    n = 1000
    org, drs, tmax, _ = answers("rooms, LDS scan")
    R = rq.gi_room(hip)
    set_schedule(R, 16, 0)
    want = host_queries(R, org, drs, tmax)
    pinned = {k: torch.from_numpy(v).pin_memory() for k, v in (("org", org), ("dir", drs), ("tmax", tmax))}
    for side in (torch.cuda.Stream(), None):  # a stream of torch's own, then the default stream (Stream = 0)
        handle = 0 if side is None else side.cuda_stream
        d = {k: torch.zeros_like(v, device="cuda") for k, v in pinned.items()}  # (zeros: rays that answer otherwise)
        d["far"] = dev(np.full(n, rq.MAX_DIST, np.float32))
        ballast = torch.ones(1 << 24, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
            for _ in range(8):
                ballast = ballast * 1.0001 + 0.5  # (work in front of the rays: the query has something to wait for)
            for k, v in pinned.items():
                d[k].copy_(v, non_blocking=True)
                d[k].add_(0.0)
            out = device_queries(R, d, n, stream=handle)
            used = {k: (v + 0 if v.dtype == torch.int32 else v * 1.0) for k, v in out.items()}  # consumed on the same stream, no host wait between
        if side is not None:
            side.synchronize()
        got = to_host(used)
        assert_same(got, want, n, "stream %#x" % handle)
        R.Ray_Query_Wait()
    # a Set_Primitive before the call is seen, with frames in flight
    Ro = rq.gi_room(orc)
    org, drs = org[:257], drs[:257]
    d = device_rays(org, drs, tmax[:257])
    before = to_host(device_queries(R, d, 257))
    for _ in range(2):
        R.Render()  # (not waited for)
    for X in (R, Ro):
        X.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.0, 3.0, 2.5), 1.2, 3))
    want = rq.oracle_answers(orc, Ro, org, drs)
    got = to_host(device_queries(R, d, 257))
    assert (want["index"] != before["index"]).sum() > 10  # the move matters to these rays
    assert_same(got, want, 257, "after Set_Primitive", keys=("hit", "index", "steps", "t", "position", "normal"))
    R.Finish()


@check("queries edit nothing")
def edit_nothing():
    """three frames with a device query of each kind and the two options between them, three frames without: the same
    framebuffer, and the radiance replay, the probe settle and the screen replay have counted the same passes"""
    org, drs = rq.room_rays(65)
    d = device_rays(org, drs, np.full(65, 5.0, np.float32))
    for screen_replay in (0, 1):
        outs = []
        for queries in (True, False):
            R = rq.gi_room(hip)
            R.Set_Option(B.OPT_SCREEN_REPLAY, screen_replay)
            held = []
            for f in range(3):
                R.Render()
                if queries:
                    set_schedule(R, (1, 16, 64)[f], (0, 1, 3)[f])
                    o = filled(65, torch.int32 if f == 0 else torch.float32)
                    (lambda: R.Raycast_Device(d["org"], d["dir"], o), lambda: R.Raycast_Visibility_Device(d["org"], d["dir"], d["tmax"], o),
                     lambda: R.Softshadows_Device(d["org"], d["dir"], 0.25, d["tmax"], 64.0, o))[f]()
                    held.append(o)
            R.Ray_Query_Wait()
            R.Finish()
            outs.append((R.Read_Framebuffer(), R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats()))
            if queries:
                assert all((o.cpu().numpy() != FILL).all() for o in held)
        (fb_q, rad_q, settle_q, scr_q), (fb, rad, settle, scr) = outs
        print("screen replay %d: radiance replay %s, probe settle %s, screen replay %s" % (screen_replay, rad, settle, scr))
        assert same_bits(fb_q, fb)
        assert rad_q == rad and settle_q == settle and scr_q == scr
        assert sum(rad) >= 1 and (screen_replay == 0 or scr[1] + scr[2] > 0)  # (the counters do count)


def _status(call):
    try:
        rc = call()
    except B.MadarchError as e:
        return e.status
    return B.MDH_OK if rc is None else rc


@check("rejections launch nothing")
def rejections():
    n = 65
    org, drs = rq.room_rays(n)
    five = np.full(n, 5.0, np.float32)
    R = rq.gi_room(hip)
    d = device_rays(org, drs, five)
    out_f, out_i = filled(n, torch.float32), filled(n, torch.int32)
    host_f, host_i = np.full(3 * n, -3.0, np.float32), np.full(n, -3, np.int32)

    def p(x):
        return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    o, v, t = d["org"], d["dir"], d["tmax"]
    calls = [("host origins", lambda a: hip.raycast_device(R._h, n, p(a), p(v), p(out_i), None, None, None, None, None, None), host_f),
             ("host directions", lambda a: hip.raycast_device(R._h, n, p(o), p(a), p(out_i), None, None, None, None, None, None), host_f),
             ("host hits", lambda a: hip.raycast_device(R._h, n, p(o), p(v), p(a), None, None, None, None, None, None), host_i)]
    for slot, what in enumerate(("index", "t", "steps", "positions", "normals")):
        def optional(a, slot=slot):
            args = [None] * 5
            args[slot] = p(a)
            return hip.raycast_device(R._h, n, p(o), p(v), p(out_i), *args, None)
        calls.append(("host " + what, optional, host_f))
    calls += [("host lengths", lambda a: hip.raycast_visibility_device(R._h, n, p(o), p(v), p(a), p(out_f), None), host_f),
              ("host visibility", lambda a: hip.raycast_visibility_device(R._h, n, p(o), p(v), p(t), p(a), None), host_f),
              ("host origins of shadow rays", lambda a: hip.softshadows_device(R._h, n, p(a), p(v), 0.0, p(t), 64.0, p(out_f), None), host_f),
              ("host lengths of shadow rays", lambda a: hip.softshadows_device(R._h, n, p(o), p(v), 0.0, p(a), 64.0, p(out_f), None), host_f),
              ("host shadows", lambda a: hip.softshadows_device(R._h, n, p(o), p(v), 0.0, p(t), 64.0, p(a), None), host_f)]
    for what, call, array in calls:
        assert call(array) == B.MDH_E_INVALID, what
        # the error did not stick: a valid call behind it succeeds, and answers
        fresh = filled(n, torch.int32)
        R.Raycast_Device(o, v, fresh)
        assert (fresh.cpu().numpy() != FILL).all(), what
    plain = [("no hits", lambda: hip.raycast_device(R._h, n, p(o), p(v), None, None, None, None, None, None, None)),
             ("n < 0", lambda: hip.raycast_device(R._h, -1, p(o), p(v), p(out_i), None, None, None, None, None, None)),
             ("no renderer", lambda: hip.raycast_device(None, n, p(o), p(v), p(out_i), None, None, None, None, None, None)),
             ("no lengths", lambda: hip.raycast_visibility_device(R._h, n, p(o), p(v), None, p(out_f), None)),
             ("tmin < 0", lambda: hip.softshadows_device(R._h, n, p(o), p(v), -0.001, p(t), 64.0, p(out_f), None)),
             ("k not finite", lambda: hip.softshadows_device(R._h, n, p(o), p(v), 0.0, p(t), float("inf"), p(out_f), None)),
             ("tmin not finite", lambda: hip.softshadows_device(R._h, n, p(o), p(v), float("nan"), p(t), 64.0, p(out_f), None)),
             ("refill 0", lambda: hip.set_option(R._h, B.OPT_RAY_STREAM_REFILL, 0)),
             ("refill 65", lambda: hip.set_option(R._h, B.OPT_RAY_STREAM_REFILL, 65)),
             ("groups -1", lambda: hip.set_option(R._h, B.OPT_RAY_STREAM_GROUPS, -1))]
    for what, call in plain:
        assert call() == B.MDH_E_INVALID, what
    R.Ray_Query_Wait()
    assert (out_f.cpu().numpy() == FILL).all() and (out_i.cpu().numpy() == FILL).all()
    assert (host_f == -3.0).all() and (host_i == -3).all()
    assert R.Get_Option(B.OPT_RAY_STREAM_REFILL) == refill_default() and R.Get_Option(B.OPT_RAY_STREAM_GROUPS) == 0
    assert hip.ray_query_wait(None) == B.MDH_E_INVALID
    # a scene with a user-defined kind
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rc.Raycast_Device(o, v, out_i)) == B.MDH_E_STATE
    assert _status(lambda: Rc.Raycast_Visibility_Device(o, v, t, out_f)) == B.MDH_E_STATE
    assert _status(lambda: Rc.Softshadows_Device(o, v, 0.0, t, 64.0, out_f)) == B.MDH_E_STATE
    assert (out_f.cpu().numpy() == FILL).all() and (out_i.cpu().numpy() == FILL).all()


def refill_default():
    import re
    with open(os.path.join(ROOT, "madarch_amd", "csrc", "mdh_ray_stream.h")) as f:
        return int(re.search(r"#define MDH_RAY_STREAM_REFILL_DEFAULT (\d+)", f.read()).group(1))


@check("the kernel's time is read off its events")
def timing():
    org, drs, tmax, _ = answers("rooms, LDS scan")
    R = rq.gi_room(hip)
    R.Set_Option(B.OPT_TIMING, 1)
    d = device_rays(org, drs, tmax)
    out = filled(N, torch.int32)
    R.Raycast_Device(d["org"], d["dir"], out)
    ms = R.Ray_Query_Time()  # (waits for the query's end event by itself)
    assert 0.0 < ms < 1000.0, ms
    R.Raycast_Device(d["org"], d["dir"], out)
    R.Ray_Query_Wait()
    assert 0.0 < R.Ray_Query_Time() < 1000.0


# ------------------------------------------------------------------------------------------- the process
DEVICE_ERRORS = ("illegal memory access", "HIP error", "hipError", "device-side", "unspecified launch failure")


def main(argv):
    global torch, hip, orc
    out_path, names = argv[0], argv[1:] or list(CHECKS)
    import torch as _torch  # BEFORE the library: one ROCm runtime serves both
    torch = _torch
    results = {}

    def flush():
        with open(out_path + ".tmp", "w") as f:
            json.dump(results, f)
        os.replace(out_path + ".tmp", out_path)
    if not torch.cuda.is_available():
        results["__error__"] = "torch sees no device"
        flush()
        return 1
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    from oracle_engine import oracle_binding
    hip, orc = B.hip_binding(), oracle_binding()
    dead = None
    for name in names:
        if dead:
            results[name] = {"ok": False, "log": "not run: a device error in '%s'" % dead, "seconds": 0.0}
            continue
        t0 = time.time()
        try:
            CHECKS[name]()
            torch.cuda.synchronize()
            results[name] = {"ok": True, "log": "", "seconds": time.time() - t0}
        except BaseException as e:  # noqa: B902
            log = traceback.format_exc()
            results[name] = {"ok": False, "log": log[-4000:], "seconds": time.time() - t0}
            if (isinstance(e, B.MadarchError) and e.status == B.MDH_E_DEVICE) or any(s in log for s in DEVICE_ERRORS) or not isinstance(e, Exception):
                dead = name
        print("%-72s %s %.1f s" % (name, "ok" if results[name]["ok"] else "FAILED", results[name]["seconds"]), flush=True)
        flush()
    return 0 if all(r["ok"] for r in results.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
