"""The checks of mdh_path_trace_device on the device, with torch tensors as the device memory.  They run in a process of their
own, started once by tests/test_gpu_path_trace.py, for the reason tests/ray_stream_device_checks.py gives: torch has to be
imported BEFORE the library is loaded.  main () imports torch, loads the library, runs the named checks (all by default) and
writes one JSON object: check -> {ok, log, seconds}.  After a device error nothing more is started.  The host-array call is
the yardstick: tests/test_gpu_path_trace.py holds it against the pixel program, the public queries and float64."""
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

import path_trace_cases as PT  # noqa: E402
import ray_query_cases as rq  # noqa: E402
import shade_rays_cases as S  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402

torch = None  # main (): imported before the library is loaded
hip = None

N = 257
PAD, FILL = 64, -7
KEYS = ("rgb", "hit", "index", "t")
SEED, BOUNCES = PT.SEED_PATHS, 3

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


def outputs(n, pad=PAD):
    """the sums start at zero over the rays and hold FILL behind them"""
    rgb = filled(3 * (n + pad), torch.float32)
    rgb[:3 * n] = 0.0
    return {"rgb": rgb, "hit": filled(n + pad, torch.int32), "index": filled(n + pad, torch.int32), "t": filled(n + pad, torch.float32)}


def trace_device(R, org, drs, n, out=None, stream=0, **kw):
    out = out or outputs(n)
    R.Path_Trace_Device(org, drs, out["rgb"], out["hit"], out["index"], out["t"], Seed=SEED, Bounces=BOUNCES, Stream=stream, N=n, **kw)
    return out


def to_host(out):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["rgb"] = got["rgb"].reshape(-1, 3)
    return got


def assert_same(got, want, n, what, at=None):
    rows = np.arange(n) if at is None else np.asarray(at)
    for k in KEYS:
        g, w = S.bits(got[k][rows]), S.bits(want[k][rows] if at is not None else want[k][:n])
        assert np.array_equal(g, w), "%s: %s differs at %s" % (what, k, np.argwhere(g != w)[:3].tolist())


def assert_untouched(got, n, what):
    for k in KEYS:
        assert (got[k][n:] == FILL).all(), "%s: %s written past its %d rays" % (what, k, n)


@check("device arrays have the host arrays' bits")
def same_bits_as_host():
    for name in ("rooms", "partition, Fallback", "mesh, triangle BVH"):
        with S.frame_size(16, 16):
            R = S.FRAME_SCENES[name](hip)
        org, drs = rq.room_rays(N) if name != "mesh, triangle BVH" else rq.mesh_rays(N)
        d_org, d_dir = dev(org), dev(drs)
        want = R.Path_Trace(org, drs, Seed=SEED, Sample_Count=2, Bounces=BOUNCES)
        for n in (1, 65, N):
            got = to_host(trace_device(R, d_org, d_dir, n, Sample_Count=2))
            assert_same(got, want, n, "%s n %d" % (name, n))
            assert_untouched(got, n, "%s n %d" % (name, n))
        # the sums stay on the device from call to call: 0 .. 1 and then 2 .. 3 are 0 .. 3
        whole = R.Path_Trace(org, drs, Seed=SEED, Sample_Count=4, Bounces=BOUNCES)
        out = trace_device(R, d_org, d_dir, N, Sample_Count=2)
        out = trace_device(R, d_org, d_dir, N, out=out, Sample_First=2, Sample_Count=2)
        assert_same(to_host(out), whole, N, "%s: two slices" % name)
        # every output but the sums may be left out
        rgb = torch.zeros(3 * N, dtype=torch.float32, device="cuda")
        R.Path_Trace_Device(d_org, d_dir, rgb, Seed=SEED, Sample_Count=4, Bounces=BOUNCES, N=N)
        assert np.array_equal(S.bits(rgb.cpu().numpy().reshape(-1, 3)), S.bits(whole["rgb"]))
        R.Destroy()


@check("a ray that is not traced is answered by its lane, its neighbours keep their bits, the host call refuses the batch")
def bad_rays():
    R = rq.gi_room(hip)
    org, drs = rq.room_rays(N)
    want = R.Path_Trace(org, drs, Seed=SEED, Sample_Count=2, Bounces=BOUNCES)
    bad_org, bad_dir = org.copy(), drs.copy()
    planted = {5: (bad_dir, 1, np.nan), 63: (bad_org, 0, np.inf), 64: (bad_org, 2, 2000.0), 70: (bad_dir, 0, 3.0), 130: (bad_org, 1, -np.inf), 256: (bad_dir, 2, -3.0)}
    for q, (arr, c, v) in planted.items():
        arr[q, c] = v
    bad_dir[200] = 0.0  # a zero direction
    planted[200] = (bad_dir, 0, 0.0)
    got = to_host(trace_device(R, dev(bad_org), dev(bad_dir), N, Sample_Count=2))
    bad = sorted(planted)
    good = [q for q in range(N) if q not in planted]
    assert (got["rgb"][bad].view(np.uint32) == PT.BAD_BITS).all(), got["rgb"][bad]
    assert (got["hit"][bad] == -1).all() and (got["index"][bad] == -1).all() and (got["t"][bad] == 0.0).all()
    assert_same(got, want, N, "neighbours of the planted rays", at=good)
    assert_untouched(got, N, "planted rays")
    import ctypes as C
    rgb = np.zeros((N, 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert hip.path_trace(R._h, N, vp(bad_org), vp(bad_dir), SEED, 0, 0, 2, BOUNCES, vp(rgb), None, None, None) == B.MDH_E_INVALID
    assert (rgb == 0.0).all()
    R.Destroy()


@check("the sums are ordered with the caller's stream")
def stream_order():
    R = rq.gi_room(hip)
    org, drs = rq.room_rays(N)
    want = R.Path_Trace(org, drs, Seed=SEED, Sample_Count=2, Bounces=BOUNCES)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_org = torch.from_numpy(org).cuda(non_blocking=False) * 1.0  # (kernels on the side stream: the query has to start behind them)
        d_dir = torch.from_numpy(drs).cuda(non_blocking=False) * 1.0
        out = outputs(N)
        out = trace_device(R, d_org, d_dir, N, out=out, stream=side.cuda_stream, Sample_Count=2)
        got = to_host(out)  # (copies on the side stream: behind the query)
    assert_same(got, want, N, "a side stream")
    with torch.cuda.stream(side):
        out = outputs(N)
        out = trace_device(R, d_org, d_dir, N, out=out, stream=side.cuda_stream, Sample_Count=2)
    R.Ray_Query_Wait()
    side.synchronize()
    assert_same(to_host(out), want, N, "Ray_Query_Wait")
    R.Destroy()


@check("pageable host pointers and bad arguments are refused before a launch")
def refusals():
    import ctypes as C
    R = rq.gi_room(hip)
    org, drs = rq.room_rays(N)
    d_org, d_dir = dev(org), dev(drs)
    out = {k: filled(len(v), v.dtype) for k, v in outputs(N, 0).items()}
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    host_rgb = np.zeros((N, 3), np.float32)

    def raw(n=N, o=None, d=None, rgb=None, s0=0, sc=1, nb=3, no_rgb=False):
        return hip.path_trace_device(R._h, n, o or p(d_org), d or p(d_dir), SEED, 0, s0, sc, nb, None if no_rgb else (rgb or p(out["rgb"])), p(out["hit"]), None, None, None)
    calls = {
        "pageable origins": lambda: raw(o=vp(org)), "pageable directions": lambda: raw(d=vp(drs)), "pageable sums": lambda: raw(rgb=vp(host_rgb)),
        "n < 0": lambda: raw(n=-1), "no sums": lambda: raw(no_rgb=True), "seven bounces": lambda: raw(nb=7), "negative bounces": lambda: raw(nb=-1),
        "a negative first sample": lambda: raw(s0=-1), "a negative count": lambda: raw(sc=-1), "a sum that overflows": lambda: raw(s0=2 ** 31 - 1, sc=1),
    }
    for what, call in calls.items():
        assert call() == B.MDH_E_INVALID, what
    assert raw(n=0) == B.MDH_OK and raw(sc=0) == B.MDH_OK  # (no launch)
    torch.cuda.synchronize()
    for k in KEYS:
        assert (out[k].cpu().numpy() == FILL).all(), k
    want = R.Path_Trace(org, drs, Seed=SEED, Bounces=BOUNCES)
    assert_same(to_host(trace_device(R, d_org, d_dir, N)), want, N, "after the refusals")
    R.Destroy()


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
