"""The checks of mdh_inscatter_points_device and mdh_inscatter_rays_device on the device, with torch tensors as the device
memory.  They run in a process of their own, started once by tests/test_gpu_inscatter.py, for the reason
tests/ray_stream_device_checks.py gives: torch has to be imported BEFORE the library is loaded.  main () imports torch, loads
the library, runs the named checks (all by default) and writes one JSON object: check -> {ok, log, seconds}.  After a device
error nothing more is started.  The host-array calls are the yardstick: tests/test_gpu_inscatter.py holds them against the
frame's textures, the chain and float64."""
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

import inscatter_cases as IC  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402

torch = None  # main (): imported before the library is loaded
hip = None

PAD, FILL = 16, -7
STEP = 0.1

CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(n, dtype, value=FILL):
    return torch.full((n,), value, dtype=dtype, device="cuda")


def ray_outputs(n, pad=PAD):
    return {"rgb": filled(3 * (n + pad), torch.float32), "len": filled(n + pad, torch.float32), "steps": filled(n + pad, torch.int32)}


def rays_device(R, d_org, d_dir, d_tmax, n, step=STEP, march=False, out=None, stream=0):
    out = out or ray_outputs(n)
    R.Inscatter_Rays_Device(d_org, d_dir, d_tmax, step, out["rgb"], out["len"], out["steps"], March=march, Stream=stream, N=n)
    return out


def to_host(out):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["rgb"] = got["rgb"].reshape(-1, 3)
    return got


def assert_rays(got, want, n, what, at=None):
    rows = np.arange(n) if at is None else np.asarray(at)
    for k in ("rgb", "len"):
        IC.assert_bits(got[k][rows], want[k][rows], "%s: %s" % (what, k))
    assert np.array_equal(got["steps"][rows], want["steps"][rows]), "%s: steps" % what
    for k in ("rgb", "len", "steps"):
        assert (got[k][n:] == FILL).all(), "%s: %s written past its %d rays" % (what, k, n)


def batch(name, n):
    """n rays of the chain's construction with its step counts in turn, and lengths for both march settings"""
    org, drs, counts = IC.chain_rays(name, n, 0)
    return org, drs, np.array([IC.tmax_for(STEP, c) for c in counts], np.float32)


@check("device arrays have the host arrays' bits")
def same_bits_as_host():
    for name in ("room", "partition, Fallback", "mesh, triangle BVH"):
        R = IC.VARIANTS[name](hip)
        org, drs, tmax = batch(name, 9)
        d_org, d_dir, d_tmax = dev(org), dev(drs), dev(tmax)
        for march in (False, True):
            want = R.Inscatter_Rays(org, drs, tmax, STEP, March=march)
            for n in (1, 3, 4, 5, 9):
                got = to_host(rays_device(R, d_org, d_dir, d_tmax, n, march=march))
                assert_rays(got, {k: v[:n] for k, v in want.items()}, n, "%s, march %d, n %d" % (name, march, n))
        # the optional outputs may be left out
        rgb = filled(3 * 9, torch.float32)
        R.Inscatter_Rays_Device(d_org, d_dir, d_tmax, STEP, rgb, N=9)
        IC.assert_bits(rgb.cpu().numpy().reshape(-1, 3), R.Inscatter_Rays(org, drs, tmax, STEP)["rgb"], name + ": the colours alone")
        # the points, with and without f: more than one workgroup, a partial wavefront
        P, D, F, _ = IC.sample_points(org, drs, STEP, [65, 129, 128, 64, 63, 1, 0, 65, 129])
        n = len(P)
        assert n > 512 and n % 64 != 0
        d_P, d_D, d_F = dev(P), dev(D), dev(F)
        for f, d_f in ((None, None), (F, d_F)):
            out = filled(3 * (n + PAD), torch.float32)
            R.Inscatter_Points_Device(d_P, d_D, out, F=d_f, N=n)
            got = out.cpu().numpy()
            IC.assert_bits(got[:3 * n].reshape(-1, 3), R.Inscatter_Points(P, D, f), "%s: points, f %s" % (name, "given" if f is not None else "absent"))
            assert (got[3 * n:] == FILL).all()
        R.Destroy()


@check("a ray or point that is not marched is answered in its place, its neighbours keep their bits, the host call refuses the batch")
def bad_lanes():
    R = IC.room(hip)
    n = 9
    org, drs, tmax = batch("room", n)
    want = R.Inscatter_Rays(org, drs, tmax, STEP)
    b_org, b_dir, b_tmax = org.copy(), drs.copy(), tmax.copy()
    b_org[1, 0] = np.nan
    b_dir[3, 2] = np.inf
    b_tmax[4] = -0.5
    b_tmax[6] = np.nextafter(np.float32(20.0), np.float32(np.inf))
    bad, good = [1, 3, 4, 6], [0, 2, 5, 7, 8]
    got = to_host(rays_device(R, dev(b_org), dev(b_dir), dev(b_tmax), n))
    assert (IC.bits(got["rgb"][bad]) == IC.BAD_BITS).all() and (IC.bits(got["len"][bad]) == IC.BAD_BITS).all(), (got["rgb"][bad], got["len"][bad])
    assert (got["steps"][bad] == -1).all()
    assert_rays(got, want, n, "neighbours of the planted rays", at=good)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rgb = np.full((n, 3), -3.0, np.float32)
    for o, d, t in ((b_org, drs, tmax), (org, b_dir, tmax), (org, drs, b_tmax)):
        assert hip.inscatter_rays(R._h, n, vp(o), vp(d), vp(t), 0, STEP, vp(rgb), None, None) == B.MDH_E_INVALID
    assert (rgb == -3.0).all()
    # the points: a NaN position, an infinite direction, a NaN f
    P, D, F, _ = IC.sample_points(org, drs, STEP, [20] * n)
    m = len(P)
    want = R.Inscatter_Points(P, D, F)
    b_P, b_D, b_F = P.copy(), D.copy(), F.copy()
    b_P[5, 1] = np.nan
    b_D[64, 0] = -np.inf
    b_F[130] = np.nan
    bad = [5, 64, 130]
    good = [q for q in range(m) if q not in bad]
    out = filled(3 * (m + PAD), torch.float32)
    R.Inscatter_Points_Device(dev(b_P), dev(b_D), out, F=dev(b_F), N=m)
    got = out.cpu().numpy()
    assert (got[3 * m:] == FILL).all()
    got = got[:3 * m].reshape(-1, 3)
    assert (IC.bits(got[bad]) == IC.BAD_BITS).all(), got[bad]
    IC.assert_bits(got[good], want[good], "neighbours of the planted points")
    assert hip.inscatter_points(R._h, m, vp(b_P), vp(D), vp(F), vp(rgb)) == B.MDH_E_INVALID
    assert hip.inscatter_points(R._h, m, vp(P), vp(D), vp(b_F), vp(rgb)) == B.MDH_E_INVALID
    assert (rgb == -3.0).all()
    R.Destroy()


@check("the answers are ordered with the caller's stream")
def stream_order():
    R = IC.room(hip)
    n = 9
    org, drs, tmax = batch("room", n)
    want = R.Inscatter_Rays(org, drs, tmax, STEP)
    P, D, F, _ = IC.sample_points(org, drs, STEP, [30] * n)
    want_points = R.Inscatter_Points(P, D, F)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # (kernels on the side stream fill the inputs: the query has to start behind them, and the copies behind the query)
        d_org, d_dir, d_tmax = torch.from_numpy(org).cuda() * 1.0, torch.from_numpy(drs).cuda() * 1.0, torch.from_numpy(tmax).cuda() * 1.0
        got = to_host(rays_device(R, d_org, d_dir, d_tmax, n, stream=side.cuda_stream))
        d_P, d_D, d_F = torch.from_numpy(P).cuda() * 1.0, torch.from_numpy(D).cuda() * 1.0, torch.from_numpy(F).cuda() * 1.0
        out = filled(3 * len(P), torch.float32)
        R.Inscatter_Points_Device(d_P, d_D, out, F=d_F, Stream=side.cuda_stream)
        got_points = out.cpu().numpy().reshape(-1, 3)
    assert_rays(got, want, n, "a side stream")
    IC.assert_bits(got_points, want_points, "points on a side stream")
    with torch.cuda.stream(side):
        out = rays_device(R, d_org, d_dir, d_tmax, n, stream=side.cuda_stream)
    R.Ray_Query_Wait()
    side.synchronize()
    assert_rays(to_host(out), want, n, "Ray_Query_Wait")
    R.Destroy()


@check("pageable host pointers, arrays that end outside their allocation and bad arguments are refused before a launch")
def refusals():
    R = IC.room(hip)
    n = 9
    org, drs, tmax = batch("room", n)
    d_org, d_dir, d_tmax = dev(org), dev(drs), dev(tmax)
    out = ray_outputs(n, 0)
    # an array whose last 40 bytes alone lie inside its allocation: 32 MiB get an allocation of their own from torch, exactly as large
    big = torch.full((8 << 20,), FILL, dtype=torch.float32, device="cuda")
    tail = C.c_void_p(big.data_ptr() + (big.numel() - 10) * 4)
    assert 3 * n * 4 > 40
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    host_rgb = np.zeros((n, 3), np.float32)

    def rays(count=n, o=None, d=None, t=None, march=0, step=STEP, rgb=None, no_rgb=False):
        return hip.inscatter_rays_device(R._h, count, o or p(d_org), d or p(d_dir), t or p(d_tmax), march, step, None if no_rgb else (rgb or p(out["rgb"])),
                                         p(out["len"]), p(out["steps"]), None)

    def points(count=n, pos=None, f=None, rgb=None, no_rgb=False):
        return hip.inscatter_points_device(R._h, count, pos or p(d_org), p(d_dir), f, None if no_rgb else (rgb or p(out["rgb"])), None)
    calls = {
        "rays: pageable origins": lambda: rays(o=vp(org)), "rays: pageable directions": lambda: rays(d=vp(drs)), "rays: pageable lengths": lambda: rays(t=vp(tmax)),
        "rays: pageable colours": lambda: rays(rgb=vp(host_rgb)), "rays: colours that end outside their allocation": lambda: rays(rgb=tail),
        "rays: n < 0": lambda: rays(count=-1), "rays: no colours": lambda: rays(no_rgb=True), "rays: march 2": lambda: rays(march=2),
        "rays: step 0": lambda: rays(step=0.0), "rays: step NaN": lambda: rays(step=float("nan")), "rays: step < 0": lambda: rays(step=-1.0),
        "rays: more than 4096 steps in max_dist": lambda: rays(step=20.0 / 4097.0),
        "points: pageable positions": lambda: points(pos=vp(org)), "points: pageable f": lambda: points(f=vp(tmax)),
        "points: colours that end outside their allocation": lambda: points(rgb=tail), "points: n < 0": lambda: points(count=-1),
        "points: no colours": lambda: points(no_rgb=True),
    }
    for what, call in calls.items():
        assert call() == B.MDH_E_INVALID, what
    assert torch.cuda.is_available() and torch.zeros(1, device="cuda").item() == 0.0  # (HIP's error state was cleared)
    assert rays(count=0) == B.MDH_OK and points(count=0) == B.MDH_OK  # (no launch)
    torch.cuda.synchronize()
    for k in out:
        assert (out[k].cpu().numpy() == FILL).all(), k
    assert (big[-16:].cpu().numpy() == FILL).all()
    want = R.Inscatter_Rays(org, drs, tmax, STEP)
    assert_rays(to_host(rays_device(R, d_org, d_dir, d_tmax, n)), want, n, "after the refusals")
    R.Destroy()


@check("nothing is edited: all four queries between frames in flight")
def edits_nothing():
    n = 9
    org, drs, tmax = batch("room", n)
    outs = []
    for queries in (True, False):
        R = IC.room(hip, IC.VOL_B)
        d_org, d_dir, d_tmax = dev(org), dev(drs), dev(tmax)
        rgb = filled(3 * n, torch.float32)
        for f in range(4):
            R.Render()  # (not waited for)
            if queries:
                (lambda: R.Inscatter_Points(org, drs), lambda: R.Inscatter_Rays(org, drs, tmax, STEP, March=True),
                 lambda: R.Inscatter_Points_Device(d_org, d_dir, rgb, N=n), lambda: R.Inscatter_Rays_Device(d_org, d_dir, d_tmax, STEP, rgb, N=n))[f]()
        R.Ray_Query_Wait()
        R.Finish()
        outs.append((R.Read_Framebuffer(), R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats()))
        R.Destroy()
    (fb_q, rad_q, settle_q, scr_q), (fb, rad, settle, scr) = outs
    assert np.array_equal(IC.bits(fb_q), IC.bits(fb))
    assert rad_q == rad and settle_q == settle and scr_q == scr


# ------------------------------------------------------------------------------------------- the process
DEVICE_ERRORS = ("illegal memory access", "HIP error", "hipError", "device-side", "unspecified launch failure")


def main(argv):
    global torch, hip
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
    hip = B.hip_binding()
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
