"""The checks of mdh_spherecast_device and mdh_contacts_device on the device, with torch tensors as the device memory.  They
run in a process of their own, started once by tests/test_gpu_sweep_streams.py, for the reason
tests/ray_stream_device_checks.py gives: torch has to be imported BEFORE the library is loaded.  main () is that module's
(the same loop, the same JSON object: check -> {ok, log, seconds}; after a device error nothing more is started).

The yardstick is the host-array calls, which tests/test_gpu_sweeps.py holds against the chain over the oracle, bit for
bit; the scenes and rays are that test's."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import custom_kinds as ck  # noqa: E402
import ray_query_cases as rq  # noqa: E402
import ray_stream_device_checks as rs  # noqa: E402
import sweep_cases as sw  # noqa: E402
from helpers import SEED, SMALL_PROBES, same_bits  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402
from madarch_amd import renderers, scenes, windows  # noqa: E402
from madarch_amd.lights import point_lights  # noqa: E402
from madarch_amd.primitives import boxes, planes, spheres  # noqa: E402

N = rs.N
PAD, FILL, BAD_BITS = rs.PAD, rs.FILL, rs.BAD_BITS
CAST_KEYS = ("hit", "index", "steps", "t", "position", "normal")
TOUCH_KEYS = ("dist", "index", "normal")
LISTS = (None, ("Plane", "Box"), ("Triangle", "Sphere"))

CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


def torch():
    return rs.torch


def hip():
    return rs.hip


def prims_of(names):
    return None if names is None else sw.kind_types(names)


def rays_of(name):
    """the case's N rays with a seeded radius and length each"""
    org, drs = rs.CASES[name][2](N)
    return org, drs, sw.seeded_radii(N), rq.seeded_tmax(N, SEED + 31)


def to_device(org, drs, rad, tmax):
    return {"org": rs.dev(org), "dir": rs.dev(drs), "rad": rs.dev(rad), "tmax": rs.dev(tmax)}


def device_cast(R, d, n, prims=None, stream=0, pad=0, radii=True, lengths=True):
    t = torch()
    out = {"hit": rs.filled(n + pad, t.int32), "index": rs.filled(n + pad, t.int32), "steps": rs.filled(n + pad, t.int32),
           "t": rs.filled(n + pad, t.float32), "position": rs.filled(3 * (n + pad), t.float32), "normal": rs.filled(3 * (n + pad), t.float32)}
    R.Spherecast_Device(d["org"], d["dir"], out["hit"], d["rad"] if radii else None, d["tmax"] if lengths else None, prims,
                        out["index"], out["t"], out["steps"], out["position"], out["normal"], Stream=stream, N=n)
    return out


def device_touch(R, d, n, prims=None, stream=0, pad=0):
    t = torch()
    out = {"dist": rs.filled(n + pad, t.float32), "index": rs.filled(n + pad, t.int32), "normal": rs.filled(3 * (n + pad), t.float32)}
    R.Contacts_Device(d["org"], out["dist"], d["rad"], prims, out["index"], out["normal"], Stream=stream, N=n)
    return out


def host_cast(R, org, drs, rad, tmax, prims=None):
    return R.Spherecast(org, drs, rad, tmax, prims)


def host_touch(R, org, rad, prims=None):
    return R.Contacts(org, rad, prims)


def four_kinds(name):
    """the scene of four kinds of tests/test_gpu_sweeps.py: in LDS, or in device memory behind a partition"""
    return sw.make_four_kinds(hip(), partition="Fallback" if "residency" in name else None, residency=1 if "residency" in name else 0)


def four_kinds_rays():
    org, drs = sw.four_kinds_rays(N)
    return org, drs, sw.seeded_radii(N), rq.seeded_tmax(N, SEED + 37)


# ------------------------------------------------------------------------------------------- checks
def host_bits(name):
    """every batch, every schedule and a permutation of the rays: the bits of the host-array calls"""
    org, drs, rad, tmax = rays_of(name)
    R = rs.CASES[name][0](hip())
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == rs.CASES[name][3]
    d = to_device(org, drs, rad, tmax)
    perm = np.random.RandomState((SEED + 41) & 0x7FFFFFFF).permutation(N)
    for n in rq.BATCHES:
        want = host_cast(R, org[:n], drs[:n], rad[:n], tmax[:n])
        touch = host_touch(R, org[:n], rad[:n])
        for refill, groups in rs.SCHEDULES:
            rs.set_schedule(R, refill, groups)
            what = "%s, %d rays, refill %d, groups %d" % (name, n, refill, groups)
            rs.assert_same(rs.to_host(device_cast(R, d, n)), want, n, what, keys=CAST_KEYS)
            rs.assert_same(rs.to_host(device_touch(R, d, n)), touch, n, what, keys=TOUCH_KEYS)
        p = perm[perm < n]
        dp = to_device(org[p], drs[p], rad[p], tmax[p])
        for refill, groups in ((16, 1), (1, 0)):
            rs.set_schedule(R, refill, groups)
            got = rs.to_host(device_cast(R, dp, n))
            back = {k: np.empty_like(v) for k, v in got.items()}
            for k in got:
                back[k][p] = got[k]
            rs.assert_same(back, want, n, "%s, %d rays permuted, refill %d, groups %d" % (name, n, refill, groups), keys=CAST_KEYS)
    # no radii and no lengths: radius 0 up to max_dist, mdh_raycast's bits
    rs.set_schedule(R, 16, 1)
    ray = R.Raycast(org, drs)
    rs.assert_same(rs.to_host(device_cast(R, d, N, radii=False, lengths=False)), ray, N, name + ", no radii, no lengths", keys=CAST_KEYS)


for _name in rs.CASES:
    CHECKS["the host-array calls' bits: " + _name] = (lambda name: lambda: host_bits(name))(_name)


def listed_bits(name):
    org, drs, rad, tmax = four_kinds_rays()
    R = four_kinds(name)
    d = to_device(org, drs, rad, tmax)
    for names in LISTS[1:] + (("Sphere", "Plane", "Box", "Triangle"),):
        prims = prims_of(names)
        for n in rq.BATCHES:
            want, touch = host_cast(R, org[:n], drs[:n], rad[:n], tmax[:n], prims), host_touch(R, org[:n], rad[:n], prims)
            for refill, groups in ((16, 1), (64, 0)):  # (k_listed takes neither: no bit may move all the same)
                rs.set_schedule(R, refill, groups)
                what = "%s, %s, %d rays, refill %d" % (name, names, n, refill)
                rs.assert_same(rs.to_host(device_cast(R, d, n, prims)), want, n, what, keys=CAST_KEYS)
                rs.assert_same(rs.to_host(device_touch(R, d, n, prims)), touch, n, what, keys=TOUCH_KEYS)


for _name in ("listed kinds, LDS scan", "listed kinds, global residency behind a partition"):
    CHECKS["the host-array calls' bits: " + _name] = (lambda name: lambda: listed_bits(name))(_name)


def flat(got):
    return {k: np.asarray(v).reshape(-1) for k, v in got.items()}


@check("every ray and centre is answered once and nothing else is written")
def answered_once():
    t = torch()
    for name in ("rooms, LDS scan", "partition, Fallback, global residency", "mesh, triangle BVH"):
        org, drs, rad, tmax = rays_of(name)
        R = rs.CASES[name][0](hip())
        d = to_device(org, drs, rad, tmax)
        for n in (65, 257):
            want, touch = host_cast(R, org[:n], drs[:n], rad[:n], tmax[:n]), host_touch(R, org[:n], rad[:n])
            for refill in (1, 16, 64):
                rs.set_schedule(R, refill, 1)
                what = "%s, %d rays, refill %d" % (name, n, refill)
                for got, yard, keys in ((rs.to_host(device_cast(R, d, n, pad=PAD)), want, CAST_KEYS), (rs.to_host(device_touch(R, d, n, pad=PAD)), touch, TOUCH_KEYS)):
                    rs.assert_same(got, yard, n, what, keys=keys)
                    f = flat(got)
                    for k in keys:
                        w = 3 if k in ("position", "normal") else 1
                        assert (f[k][w * n:] == FILL).all(), "%s: %s written behind item %d" % (what, k, n)
                    for k in ("hit", "dist", "steps"):
                        assert k not in f or (f[k][:n] != FILL).all(), "%s: %s" % (what, k)
                # the hits and the distances alone: the optional outputs are null
                only, dist = rs.filled(n + PAD, t.int32), rs.filled(n + PAD, t.float32)
                R.Spherecast_Device(d["org"], d["dir"], only, d["rad"], d["tmax"], N=n)
                R.Contacts_Device(d["org"], dist, d["rad"], N=n)
                only, dist = only.cpu().numpy(), dist.cpu().numpy()
                assert np.array_equal(only[:n], want["hit"]) and (only[n:] == FILL).all(), what
                assert same_bits(dist[:n], touch["dist"]) and (dist[n:] == FILL).all(), what
        none = rs.filled(PAD, t.int32)
        R.Spherecast_Device(d["org"], d["dir"], none, N=0)
        R.Contacts_Device(d["org"], none.view(t.float32), N=0)
        assert (none.cpu().numpy() == FILL).all()
    # the listed scan
    org, drs, rad, tmax = four_kinds_rays()
    R = four_kinds("LDS")
    d = to_device(org, drs, rad, tmax)
    prims = prims_of(LISTS[1])
    for n in (65, 257):
        for got, yard, keys in ((rs.to_host(device_cast(R, d, n, prims, pad=PAD)), host_cast(R, org[:n], drs[:n], rad[:n], tmax[:n], prims), CAST_KEYS),
                                (rs.to_host(device_touch(R, d, n, prims, pad=PAD)), host_touch(R, org[:n], rad[:n], prims), TOUCH_KEYS)):
            rs.assert_same(got, yard, n, "listed, %d" % n, keys=keys)
            f = flat(got)
            for k in keys:
                assert (f[k][(3 if k in ("position", "normal") else 1) * n:] == FILL).all(), "listed: %s written behind item %d" % (k, n)


@check("bad rays and centres are refused, not marched")
def bad_items():
    n = 257
    poison = (np.nan, np.inf, -np.inf)
    over = np.nextafter(rq.MAX_DIST, np.float32(np.inf))
    for name, names in (("rooms, LDS scan", None), ("partition, Clamp, global residency", None), ("listed kinds, LDS scan", LISTS[1]),
                        ("listed kinds, global residency behind a partition", LISTS[2])):
        if names is None:
            org, drs, rad, tmax = (a[:n].copy() for a in rays_of(name))
            R = rs.CASES[name][0](hip())
        else:
            org, drs, rad, tmax = (a[:n].copy() for a in four_kinds_rays())
            R = four_kinds(name)
        prims = prims_of(names)
        clean, clean_touch = host_cast(R, org, drs, rad, tmax, prims), host_touch(R, org, rad, prims)
        places = np.random.RandomState((SEED + 53) & 0x7FFFFFFF).permutation(n)[:48]
        bad_org, bad_dir, bad_rad, bad_len = places[:12], places[12:24], places[24:36], places[36:]
        for i, q in enumerate(bad_org):
            org[q, i % 3] = poison[(i // 3) % 3]
        for i, q in enumerate(bad_dir):
            drs[q, i % 3] = poison[(i // 3) % 3]
        for i, q in enumerate(bad_rad):
            rad[q] = (np.nan, np.inf, -np.inf, np.float32(-1e-6), over, np.float32(1e30))[i % 6]
        for i, q in enumerate(bad_len):
            tmax[q] = (np.nan, np.inf, -np.inf, np.float32(-1e-6), over, np.float32(1e30))[i % 6]
        bad_ray = np.zeros(n, bool)
        bad_ray[places] = True
        bad_centre = np.zeros(n, bool)
        bad_centre[np.concatenate((bad_org, bad_rad))] = True
        d = to_device(org, drs, rad, tmax)
        for refill, groups in ((1, 1), (16, 1), (64, 0)):
            rs.set_schedule(R, refill, groups)
            what = "%s, refill %d, groups %d" % (name, refill, groups)
            got = rs.to_host(device_cast(R, d, n, prims, pad=PAD))
            rs.assert_same(got, clean, n, what, keys=CAST_KEYS, at=~bad_ray)
            assert (got["hit"][:n][bad_ray] == -1).all() and (got["index"][:n][bad_ray] == -1).all() and (got["steps"][:n][bad_ray] == 0).all(), what
            for k in ("t", "position", "normal"):
                assert (got[k][:n][bad_ray] == 0.0).all(), "%s: %s" % (what, k)
            assert (got["hit"][n:] == FILL).all()
            got = rs.to_host(device_touch(R, d, n, prims, pad=PAD))
            rs.assert_same(got, clean_touch, n, what, keys=TOUCH_KEYS, at=~bad_centre)
            assert (got["dist"][:n].view(np.uint32)[bad_centre] == BAD_BITS).all() and (got["index"][:n][bad_centre] == -1).all(), what
            assert (got["normal"][:n][bad_centre] == 0.0).all() and (got["dist"][n:] == FILL).all(), what


@check("ordered with the caller's stream")
def ordering():
    t = torch()
    n = 1000
    org, drs, rad, tmax = rays_of("rooms, LDS scan")
    R = rq.gi_room(hip())
    rs.set_schedule(R, 16, 0)
    kinds = (planes.Plane, boxes.Box)
    want = {None: (host_cast(R, org, drs, rad, tmax), host_touch(R, org, rad)), kinds: (host_cast(R, org, drs, rad, tmax, kinds), host_touch(R, org, rad, kinds))}
    pinned = {k: t.from_numpy(v).pin_memory() for k, v in (("org", org), ("dir", drs), ("rad", rad), ("tmax", tmax))}
    for side in (t.cuda.Stream(), None):  # a stream of torch's own, then the default stream (Stream = 0)
        handle = 0 if side is None else side.cuda_stream
        d = {k: t.zeros_like(v, device="cuda") for k, v in pinned.items()}  # (zeros: rays that answer otherwise)
        ballast = t.ones(1 << 24, device="cuda")
        t.cuda.synchronize()
        used = {}
        with t.cuda.stream(side if side is not None else t.cuda.default_stream()):
            for _ in range(8):
                ballast = ballast * 1.0001 + 0.5  # (work in front of the rays: the query has something to wait for)
            for k, v in pinned.items():
                d[k].copy_(v, non_blocking=True)
                d[k].add_(0.0)
            for prims in want:
                outs = (device_cast(R, d, n, prims, stream=handle), device_touch(R, d, n, prims, stream=handle))
                used[prims] = [{k: (v + 0 if v.dtype == t.int32 else v * 1.0) for k, v in o.items()} for o in outs]  # consumed on the same stream, no host wait between
        if side is not None:
            side.synchronize()
        for prims, (cast, touch) in used.items():
            rs.assert_same(rs.to_host(cast), want[prims][0], n, "stream %#x, %s" % (handle, prims), keys=CAST_KEYS)
            rs.assert_same(rs.to_host(touch), want[prims][1], n, "stream %#x, %s" % (handle, prims), keys=TOUCH_KEYS)
        R.Ray_Query_Wait()
    # a Set_Primitive before the call is seen, with frames in flight
    d = to_device(org[:257], drs[:257], rad[:257], tmax[:257])
    before = rs.to_host(device_cast(R, d, 257))
    for _ in range(2):
        R.Render()  # (not waited for)
    R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.0, 3.0, 2.5), 1.2, 3))
    got = rs.to_host(device_cast(R, d, 257))
    after = host_cast(R, org[:257], drs[:257], rad[:257], tmax[:257])
    assert (after["index"] != before["index"]).sum() > 10  # the move matters to these rays
    rs.assert_same(got, after, 257, "after Set_Primitive", keys=CAST_KEYS)
    R.Finish()


@check("sweeps edit nothing")
def edit_nothing():
    t = torch()
    org, drs = rq.room_rays(65)
    d = to_device(org, drs, np.full(65, 0.2, np.float32), np.full(65, 5.0, np.float32))
    kinds = (planes.Plane, boxes.Box)
    for screen_replay in (0, 1):
        outs = []
        for queries in (True, False):
            R = rq.gi_room(hip())
            R.Set_Option(B.OPT_SCREEN_REPLAY, screen_replay)
            held = []
            for f in range(3):
                R.Render()
                if queries:
                    rs.set_schedule(R, (1, 16, 64)[f], (0, 1, 3)[f])
                    prims = (None, kinds, None)[f]
                    held += [device_cast(R, d, 65, prims)["hit"], device_touch(R, d, 65, prims)["dist"]]
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


@check("rejections launch nothing")
def rejections():
    t = torch()
    n = 65
    org, drs = rq.room_rays(n)
    R = rq.gi_room(hip())
    d = to_device(org, drs, np.full(n, 0.2, np.float32), np.full(n, 5.0, np.float32))
    out_f, out_i = rs.filled(3 * n, t.float32), rs.filled(n, t.int32)
    host_f, host_i = np.full(3 * n, -3.0, np.float32), np.full(n, -3, np.int32)
    kinds = np.array([1, 2], np.int32)

    def p(x):
        return None if x is None else C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    h = hip()

    def cast(o=d["org"], v=d["dir"], r=d["rad"], l=d["tmax"], k=None, nk=0, hit=out_i, opt=(None,) * 5, count=n, handle=R._h):
        return h.spherecast_device(handle, count, p(o), p(v), p(r), p(l), p(k), nk, p(hit), *[p(x) for x in opt], None)

    def touch(c=d["org"], r=d["rad"], k=None, nk=0, dist=out_f, index=None, normal=None, count=n, handle=R._h):
        return h.contacts_device(handle, count, p(c), p(r), p(k), nk, p(dist), p(index), p(normal), None)
    calls = [("host origins", lambda: cast(o=host_f)), ("host directions", lambda: cast(v=host_f)), ("host radii", lambda: cast(r=host_f)),
             ("host lengths", lambda: cast(l=host_f)), ("host hits", lambda: cast(hit=host_i)), ("host origins, listed", lambda: cast(o=host_f, k=kinds, nk=2)),
             ("host centres", lambda: touch(c=host_f)), ("host radii of centres", lambda: touch(r=host_f)), ("host distances", lambda: touch(dist=host_f)),
             ("host indices", lambda: touch(index=host_i)), ("host normals", lambda: touch(normal=host_f)), ("host normals, listed", lambda: touch(normal=host_f, k=kinds, nk=2))]
    for slot, what in enumerate(("index", "t", "steps", "positions", "normals")):
        calls.append(("host " + what, (lambda slot: lambda: cast(opt=tuple(host_f if s == slot else None for s in range(5))))(slot)))
    for what, call in calls:
        assert call() == B.MDH_E_INVALID, what
        fresh = rs.filled(n, t.int32)  # the error did not stick: a valid call behind it succeeds, and answers
        R.Spherecast_Device(d["org"], d["dir"], fresh, d["rad"], d["tmax"])
        assert (fresh.cpu().numpy() != FILL).all(), what
    plain = [("no hits", lambda: cast(hit=None)), ("no origins", lambda: cast(o=None)), ("no directions", lambda: cast(v=None)), ("n < 0", lambda: cast(count=-1)),
             ("no renderer", lambda: cast(handle=None)), ("kind index", lambda: cast(k=np.array([1, 3], np.int32), nk=2)), ("kinds without a list", lambda: cast(nk=1)),
             ("n_kinds < 0", lambda: cast(k=kinds, nk=-1)), ("no centres", lambda: touch(c=None)), ("no distances", lambda: touch(dist=None)),
             ("contacts: n < 0", lambda: touch(count=-1)), ("contacts: no renderer", lambda: touch(handle=None)), ("contacts: kind index", lambda: touch(k=np.array([-1], np.int32), nk=1))]
    for what, call in plain:
        assert call() == B.MDH_E_INVALID, what
    R.Ray_Query_Wait()
    assert (out_f.cpu().numpy() == FILL).all() and (out_i.cpu().numpy() == FILL).all()
    assert (host_f == -3.0).all() and (host_i == -3).all()
    # a scene with a user-defined kind
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=h)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    for call in (lambda: Rc.Spherecast_Device(d["org"], d["dir"], out_i), lambda: Rc.Spherecast_Device(d["org"], d["dir"], out_i, Prims=(spheres.Sphere,)),
                 lambda: Rc.Contacts_Device(d["org"], out_f), lambda: Rc.Contacts_Device(d["org"], out_f, Prims=(spheres.Sphere,))):
        assert rs._status(call) == B.MDH_E_STATE
    assert (out_f.cpu().numpy() == FILL).all() and (out_i.cpu().numpy() == FILL).all()


@check("the kernel's time is read off its events")
def timing():
    t = torch()
    org, drs, rad, tmax = rays_of("rooms, LDS scan")
    R = rq.gi_room(hip())
    R.Set_Option(B.OPT_TIMING, 1)
    d = to_device(org, drs, rad, tmax)
    for prims in (None, (planes.Plane, boxes.Box)):
        out = rs.filled(N, t.int32)
        R.Spherecast_Device(d["org"], d["dir"], out, d["rad"], d["tmax"], prims)
        assert 0.0 < R.Ray_Query_Time() < 1000.0  # (waits for the query's end event by itself)
        dist = rs.filled(N, t.float32)
        R.Contacts_Device(d["org"], dist, d["rad"], prims)
        R.Ray_Query_Wait()
        assert 0.0 < R.Ray_Query_Time() < 1000.0


def main(argv):
    """tests/ray_stream_device_checks.py's process, over this module's checks"""
    rs.CHECKS.clear()
    rs.CHECKS.update(CHECKS)
    return rs.main(argv)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
