"""The checks of mdh_path_frame_read_device and mdh_path_frame_rays_device on the device, with torch tensors as the device memory.
They run in a process of their own, started once by tests/test_gpu_path_frame.py, for the reason
tests/ray_stream_device_checks.py gives: torch has to be imported BEFORE the library is loaded.  main () imports torch, loads
the library, runs the named checks (all by default) and writes one JSON object: check -> {ok, log, seconds}.  After a device
error nothing more is started.  The host forms are the yardstick: tests/test_gpu_path_frame.py holds them against the ray
queries and numpy."""
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

import path_frame_cases as PF  # noqa: E402
import ray_query_cases as rq  # noqa: E402
import shade_rays_cases as S  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402

torch = None  # main (): imported before the library is loaded
hip = None

W, H = PF.W, PF.H
N = W * H
PAD, FILL = 64, -7
SEED = PF.SEED

CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


def filled(n, dtype, value=FILL):
    return torch.full((n,), value, dtype=dtype, device="cuda")


def opened(jitter=True, samples=3):
    R = rq.gi_room(hip)
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=jitter)
    R.Path_Frame_Accumulate(samples)
    return R


def outputs():
    return {"rgb": filled(3 * N + PAD, torch.float32), "rgba8": filled(N + PAD, torch.int32), "sums": filled(3 * N + PAD, torch.float32)}


def assert_read(out, want, what):
    rgb, rgba8, sums = (out[k].cpu().numpy() for k in ("rgb", "rgba8", "sums"))
    assert np.array_equal(S.bits(rgb[:3 * N]), S.bits(want["rgb"].reshape(-1))), what + ": rgb"
    assert np.array_equal(rgba8[:N].view(np.uint8).reshape(H, W, 4), want["rgba8"]), what + ": rgba8"
    assert np.array_equal(S.bits(sums[:3 * N]), S.bits(want["sums"].reshape(-1))), what + ": sums"
    assert (rgb[3 * N:] == FILL).all() and (rgba8[N:] == FILL).all() and (sums[3 * N:] == FILL).all(), what + ": written past the frame"


@check("the device forms have the host forms' bits")
def same_bits_as_host():
    for jitter in (False, True):
        R = opened(jitter)
        for tone_map in (False, True):
            want = R.Path_Frame_Read(Tone_Map=tone_map, Rgb=True, Rgba8=True, Sums=True)
            out = outputs()
            assert R.Path_Frame_Read_Device(W, H, out["rgb"], out["rgba8"], out["sums"], Tone_Map=tone_map) == 3
            R.Ray_Query_Wait()
            assert_read(out, want, "jitter %s tone map %s" % (jitter, tone_map))
        # every output may be left out
        only = filled(N, torch.int32)
        R.Path_Frame_Read_Device(W, H, Rgba8=only, Tone_Map=True)
        R.Ray_Query_Wait()
        assert np.array_equal(only.cpu().numpy().view(np.uint8).reshape(H, W, 4), want["rgba8"])
        for s in (0, 4):
            org, drs = R.Path_Frame_Rays(s)
            d_org, d_dir = filled(3 * N + PAD, torch.float32), filled(3 * N + PAD, torch.float32)
            R.Path_Frame_Rays_Device(W, H, d_org, d_dir, Sample=s)
            torch.cuda.synchronize()
            for got, host in ((d_org, org), (d_dir, drs)):
                got = got.cpu().numpy()
                assert np.array_equal(S.bits(got[:3 * N]), S.bits(host.reshape(-1))) and (got[3 * N:] == FILL).all(), (jitter, s)
        R.Destroy()


@check("the resolve and the rays are ordered with the caller's stream")
def stream_order():
    R = opened(True)
    want = R.Path_Frame_Read(Tone_Map=True, Rgb=True, Rgba8=True, Sums=True)
    rays = R.Path_Frame_Rays(2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = {k: v * 1 for k, v in outputs().items()}  # (kernels on the side stream: the resolve has to start behind them)
        R.Path_Frame_Read_Device(W, H, out["rgb"], out["rgba8"], out["sums"], Tone_Map=True, Stream=side.cuda_stream)
        host = {k: v.cpu() for k, v in out.items()}  # (copies on the side stream: behind the resolve)
        d_org, d_dir = filled(3 * N, torch.float32) * 1, filled(3 * N, torch.float32) * 1
        R.Path_Frame_Rays_Device(W, H, d_org, d_dir, Sample=2, Stream=side.cuda_stream)
        h_org, h_dir = d_org.cpu(), d_dir.cpu()
    side.synchronize()
    assert_read(host, want, "a side stream")
    assert np.array_equal(S.bits(h_org.numpy()), S.bits(rays[0].reshape(-1))) and np.array_equal(S.bits(h_dir.numpy()), S.bits(rays[1].reshape(-1)))
    # more samples behind a read in flight: the read has the sums of its moment, Ray_Query_Wait is the host's wait
    with torch.cuda.stream(side):
        out = outputs()
        R.Path_Frame_Read_Device(W, H, out["rgb"], out["rgba8"], out["sums"], Tone_Map=True, Stream=side.cuda_stream)
    R.Path_Frame_Accumulate(2)
    R.Ray_Query_Wait()
    side.synchronize()
    assert_read(out, want, "Ray_Query_Wait")
    assert R.Path_Frame_Info()["samples"] == 5
    R.Destroy()


@check("pageable host pointers and short tensors are refused before a launch")
def refusals():
    R = opened(True)
    R.Set_Option(B.OPT_TIMING, 1)
    R.Path_Frame_Accumulate(1)
    R.Ray_Query_Wait()
    before = R.Ray_Query_Time()
    h = R._h
    out = outputs()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    host = np.zeros(3 * N, np.float32)
    vp = C.c_void_p(host.ctypes.data)
    # arrays that end outside their allocation: 32 MiB get an allocation of their own from torch, exactly as large, once the
    # blocks it kept from the checks before are given back; a tensor that reaches its end is one float or one word short
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    big = torch.full((8 << 20,), FILL, dtype=torch.float32, device="cuda")
    short3, short1 = big[big.numel() - (3 * N - 1):], big[big.numel() - (N - 1):]
    n = C.c_int32(-5)
    calls = {
        "pageable colours": lambda: hip.path_frame_read_device(h, 0, vp, None, None, C.byref(n), None),
        "pageable bytes": lambda: hip.path_frame_read_device(h, 0, None, vp, None, C.byref(n), None),
        "pageable sums": lambda: hip.path_frame_read_device(h, 0, p(out["rgb"]), None, vp, C.byref(n), None),
        "short colours": lambda: hip.path_frame_read_device(h, 0, p(short3), None, None, C.byref(n), None),
        "short bytes": lambda: hip.path_frame_read_device(h, 0, None, p(short1), None, C.byref(n), None),
        "short sums": lambda: hip.path_frame_read_device(h, 0, None, None, p(short3), C.byref(n), None),
        "a tone map of 2": lambda: hip.path_frame_read_device(h, 2, p(out["rgb"]), None, None, C.byref(n), None),
        "pageable origins": lambda: hip.path_frame_rays_device(h, 0, vp, p(out["sums"]), None),
        "pageable directions": lambda: hip.path_frame_rays_device(h, 0, p(out["rgb"]), vp, None),
        "short origins": lambda: hip.path_frame_rays_device(h, 0, p(short3), p(out["sums"]), None),
        "short directions": lambda: hip.path_frame_rays_device(h, 0, p(out["rgb"]), p(short3), None),
        "no directions": lambda: hip.path_frame_rays_device(h, 0, p(out["rgb"]), None, None),
        "a negative sample": lambda: hip.path_frame_rays_device(h, -1, p(out["rgb"]), p(out["sums"]), None),
    }
    for what, call in calls.items():
        assert call() == B.MDH_E_INVALID, what
    assert n.value == -5
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v.cpu().numpy() == FILL).all(), k
    assert (host == 0.0).all() and (big.cpu().numpy() == FILL).all()
    assert R.Ray_Query_Time() == before  # nothing was launched
    # Python's own checks come first
    for what, call in {"a short tensor": lambda: R.Path_Frame_Read_Device(W, H, short3), "a host tensor": lambda: R.Path_Frame_Read_Device(W, H, torch.zeros(3 * N))}.items():
        try:
            call()
        except ValueError:
            continue
        raise AssertionError(what + " was accepted")
    # the resolve does not take the timing pair: the accumulate kernel stays what is timed
    R.Path_Frame_Read_Device(W, H, out["rgb"], out["rgba8"], out["sums"])
    R.Ray_Query_Wait()
    assert R.Ray_Query_Time() == before
    want = R.Path_Frame_Read(Rgb=True, Rgba8=True, Sums=True)
    assert_read(out, want, "after the refusals")
    R.Path_Frame_End()
    assert hip.path_frame_read_device(h, 0, p(out["rgb"]), None, None, None, None) == B.MDH_E_STATE
    assert hip.path_frame_rays_device(h, 0, p(out["rgb"]), p(out["sums"]), None) == B.MDH_E_STATE
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
