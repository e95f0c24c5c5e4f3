"""The checks of mdh_shade_rays_device and mdh_camera_rays_device on the device, with torch tensors as the device memory.
They run in a process of their own, started once by tests/test_gpu_shade_rays.py, for the reason
tests/ray_stream_device_checks.py gives: torch has to be imported BEFORE the library is loaded.  main () imports torch,
loads the library, runs the named checks (all by default) and writes one JSON object: check -> {ok, log, seconds}.  After a
device error nothing more is started.  The host-array calls are the yardstick: tests/test_gpu_shade_rays.py holds them
against the frame and against float64."""
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

import ray_query_cases as rq  # noqa: E402
import shade_rays_cases as S  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402

torch = None  # main (): imported before the library is loaded
hip = None

N = 257
PAD, FILL = 64, -7
BAD_BITS = 0x7FC00000
KEYS = ("rgb", "hit", "index", "t", "steps")

CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(n, dtype):
    return torch.full((n,), FILL, dtype=dtype, device="cuda")


def outputs(n):
    return {"rgb": filled(3 * n, torch.float32), "hit": filled(n, torch.int32), "index": filled(n, torch.int32),
            "t": filled(n, torch.float32), "steps": filled(n, torch.int32)}


def shade_device(R, org, drs, n, mode, tone, stream=0, pad=PAD):
    out = outputs(n + pad)
    R.Shade_Rays_Device(org, drs, out["rgb"], out["hit"], out["index"], out["t"], out["steps"], Mode=mode, Tone_Map=tone, Stream=stream, N=n)
    return out


def to_host(out):
    got = {k: v.cpu().numpy() for k, v in out.items()}  # (on torch's current stream: ordered behind a query that was given it)
    got["rgb"] = got["rgb"].reshape(-1, 3)
    return got


def assert_same(got, want, n, what, at=None):
    rows = np.arange(n) if at is None else np.asarray(at)
    for k in KEYS:
        g, w = S.bits(got[k][rows]), S.bits(want[k][rows] if at is not None else want[k][:n])
        assert np.array_equal(g, w), "%s: %s differs at %s" % (what, k, np.argwhere(g != w)[:3].tolist())


def assert_untouched(got, n, what):
    """nothing behind the first n entries was written"""
    for k in KEYS:
        tail = got[k][n:]
        assert (tail == FILL).all(), "%s: %s written past its %d rays" % (what, k, n)


@check("device arrays have the host arrays' bits, both modes, linear and tone-mapped")
def same_bits_as_host():
    for name in ("rooms", "partition, Fallback", "mesh, triangle BVH"):
        for mode in S.MODES:
            R = S.frame_renderer(hip, name, mode)
            org, drs = rq.room_rays(N) if name != "mesh, triangle BVH" else rq.mesh_rays(N)
            d_org, d_dir = dev(org), dev(drs)
            for tone in (False, True):
                want = R.Shade_Rays(org, drs, Mode=mode, Tone_Map=tone)
                for n in (1, 65, N):
                    got = to_host(shade_device(R, d_org, d_dir, n, mode, tone))
                    assert_same(got, want, n, "%s mode %d tone %d n %d" % (name, mode, tone, n))
                    assert_untouched(got, n, "%s n %d" % (name, n))
            R.Destroy()


@check("camera rays on the device are the host call's, and shade to the frame")
def camera_rays():
    W, H = S.FRAME_W, S.FRAME_H
    R = S.frame_renderer(hip, "rooms", 0)
    org, drs = R.Camera_Rays(W, H)
    d_org, d_dir = filled(3 * W * H + PAD, torch.float32), filled(3 * W * H + PAD, torch.float32)
    R.Camera_Rays_Device(W, H, d_org, d_dir)  # (on the default stream, torch's: the copies below are behind it)
    g_org, g_dir = d_org.cpu().numpy(), d_dir.cpu().numpy()
    assert np.array_equal(S.bits(g_org[:3 * W * H].reshape(-1, 3)), S.bits(org)) and np.array_equal(S.bits(g_dir[:3 * W * H].reshape(-1, 3)), S.bits(drs))
    assert (g_org[3 * W * H:] == FILL).all() and (g_dir[3 * W * H:] == FILL).all()
    R.Render_Pass(B.PASS_SCREEN)
    fb = R.Read_Framebuffer().reshape(-1, 3)
    got = to_host(shade_device(R, d_org, d_dir, W * H, 0, True))
    assert np.array_equal(S.bits(got["rgb"][:W * H]), S.bits(fb))
    # every output but the colours may be left out
    rgb = filled(3 * W * H, torch.float32)
    R.Shade_Rays_Device(d_org, d_dir, rgb, Mode=0, Tone_Map=True, N=W * H)
    assert np.array_equal(S.bits(rgb.cpu().numpy().reshape(-1, 3)), S.bits(fb))
    R.Destroy()


@check("a ray that is not shaded is answered by its lane, its neighbours keep their bits, the host call refuses the batch")
def bad_rays():
    R = S.frame_renderer(hip, "rooms", 0)
    org, drs = rq.room_rays(N)
    want = R.Shade_Rays(org, drs, Tone_Map=False)
    bad_org, bad_dir = org.copy(), drs.copy()
    planted = {5: (bad_dir, 1, np.nan), 63: (bad_org, 0, np.inf), 64: (bad_org, 2, 2000.0), 70: (bad_dir, 0, 3.0), 130: (bad_org, 1, -np.inf), 256: (bad_dir, 2, -3.0)}
    for q, (arr, c, v) in planted.items():
        arr[q, c] = v
    got = to_host(shade_device(R, dev(bad_org), dev(bad_dir), N, 0, False))
    bad = sorted(planted)
    good = [q for q in range(N) if q not in planted]
    assert (got["rgb"][bad].view(np.uint32) == BAD_BITS).all(), got["rgb"][bad]
    assert (got["hit"][bad] == -1).all() and (got["index"][bad] == -1).all() and (got["t"][bad] == 0.0).all() and (got["steps"][bad] == 0).all()
    assert_same(got, want, N, "neighbours of the planted rays", at=good)
    assert_untouched(got, N, "planted rays")
    assert B.MDH_E_INVALID == _raw_host(R, bad_org, bad_dir)
    R.Destroy()


def _raw_host(R, org, drs):
    import ctypes as C
    rgb = np.zeros((len(org), 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return hip.shade_rays(R._h, len(org), vp(org), vp(drs), 0, 0, vp(rgb), None, None, None, None)


@check("the answers are ordered with the caller's stream")
def stream_order():
    R = S.frame_renderer(hip, "rooms", 0)
    org, drs = rq.room_rays(N)
    want = R.Shade_Rays(org, drs)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_org = torch.from_numpy(org).cuda(non_blocking=False)
        d_dir = torch.from_numpy(drs).cuda(non_blocking=False)
        d_org = d_org * 1.0  # (kernels on the side stream: the query has to start behind them)
        d_dir = d_dir * 1.0
        out = shade_device(R, d_org, d_dir, N, 0, False, stream=side.cuda_stream)
        got = to_host(out)  # (copies on the side stream: behind the query)
    assert_same(got, want, N, "a side stream")
    # and the host's wait
    with torch.cuda.stream(side):
        out = shade_device(R, d_org, d_dir, N, 0, False, stream=side.cuda_stream)
    R.Ray_Query_Wait()
    side.synchronize()
    assert_same(to_host(out), want, N, "Ray_Query_Wait")
    R.Destroy()


@check("pageable host pointers and bad arguments are refused before a launch")
def refusals():
    import ctypes as C
    R = S.frame_renderer(hip, "rooms", 0)
    org, drs = rq.room_rays(N)
    d_org, d_dir = dev(org), dev(drs)
    out = outputs(N)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    host_rgb = np.zeros((N, 3), np.float32)
    calls = {
        "pageable origins": lambda: hip.shade_rays_device(R._h, N, vp(org), p(d_dir), 0, 0, p(out["rgb"]), None, None, None, None, None),
        "pageable directions": lambda: hip.shade_rays_device(R._h, N, p(d_org), vp(drs), 0, 0, p(out["rgb"]), None, None, None, None, None),
        "pageable colours": lambda: hip.shade_rays_device(R._h, N, p(d_org), p(d_dir), 0, 0, vp(host_rgb), None, None, None, None, None),
        "mode 1": lambda: hip.shade_rays_device(R._h, N, p(d_org), p(d_dir), 1, 0, p(out["rgb"]), None, None, None, None, None),
        "n < 0": lambda: hip.shade_rays_device(R._h, -1, p(d_org), p(d_dir), 0, 0, p(out["rgb"]), None, None, None, None, None),
        "no colours": lambda: hip.shade_rays_device(R._h, N, p(d_org), p(d_dir), 0, 0, None, None, None, None, None, None),
        "pageable camera rays": lambda: hip.camera_rays_device(R._h, 4, 4, vp(host_rgb), p(d_dir), None),
    }
    for what, call in calls.items():
        assert call() == B.MDH_E_INVALID, what
    torch.cuda.synchronize()
    for k in KEYS:
        assert (out[k].cpu().numpy() == FILL).all(), k
    assert hip.shade_rays_device(R._h, 0, p(d_org), p(d_dir), 0, 0, p(out["rgb"]), None, None, None, None, None) == B.MDH_OK
    # the renderer still answers
    want = R.Shade_Rays(org, drs)
    assert_same(to_host(shade_device(R, d_org, d_dir, N, 0, False)), want, N, "after the refusals")
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
