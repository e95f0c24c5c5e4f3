"""The checks of mdh_path_frame_stats_device and, on an adaptive frame, mdh_path_frame_read_device on the device, with torch tensors as
the device memory.  They run in a process of their own, started once by tests/test_gpu_path_adaptive.py, for the reason
tests/ray_stream_device_checks.py gives: torch has to be imported BEFORE the library is loaded.  main () is
tests/path_frame_device_checks.py's.  The host forms are the yardstick: tests/test_gpu_path_adaptive.py holds them against the
chain of public queries."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import path_adaptive_cases as PA  # noqa: E402
import path_frame_cases as PF  # noqa: E402
import path_frame_device_checks as base  # noqa: E402
import ray_query_cases as rq  # noqa: E402
import shade_rays_cases as S  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402

W, H = PF.W, PF.H
N = W * H
PAD, FILL = base.PAD, base.FILL
SEED = PA.SEED

CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


def torch():
    return base.torch


def opened(rounds=(2, 2)):
    R = rq.gi_room(base.hip)
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=2, Jitter=True, Min_Samples=PA.MIN_SAMPLES, Max_Samples=PA.MAX_SAMPLES, Tolerance=PA.TOLERANCE["rooms"], Floor=PA.FLOOR)
    for k in rounds:
        R.Path_Frame_Accumulate(k)
    return R


def stat_outputs():
    t = torch()
    return {"count": base.filled(N + PAD, t.int32), "moments": base.filled(2 * N + PAD, t.float32), "active": base.filled(1 + PAD, t.int64), "total": base.filled(1 + PAD, t.int64)}


def assert_stats(out, want, what):
    count, mom, active, total = (out[k].cpu().numpy() for k in ("count", "moments", "active", "total"))
    assert np.array_equal(count[:N], want["count"].reshape(-1)), what + ": count"
    assert np.array_equal(S.bits(mom[:2 * N]), S.bits(want["moments"].reshape(-1))), what + ": moments"
    assert active[0] == want["active"] and total[0] == want["total_samples"], what + ": %d active, %d samples against %d, %d" % (active[0], total[0], want["active"], want["total_samples"])
    assert (count[N:] == FILL).all() and (mom[2 * N:] == FILL).all() and (active[1:] == FILL).all() and (total[1:] == FILL).all(), what + ": written past the frame"


@check("the device forms have the host forms' bits")
def same_bits_as_host():
    R = opened()
    want = R.Path_Frame_Stats()
    assert 0 < want["active"] < N and len(np.unique(want["count"])) > 1
    out = stat_outputs()
    R.Path_Frame_Stats_Device(W, H, out["count"], out["moments"], out["active"], out["total"])
    R.Ray_Query_Wait()
    assert_stats(out, want, "all four")
    # every output may be left out
    only = base.filled(1, torch().int64)
    R.Path_Frame_Stats_Device(W, H, Total_Samples=only)
    R.Ray_Query_Wait()
    assert only.cpu().numpy()[0] == want["total_samples"]
    R.Path_Frame_Stats_Device(W, H)
    # the resolve by each pixel's own count
    for tone_map in (False, True):
        image = R.Path_Frame_Read(Tone_Map=tone_map, Rgb=True, Rgba8=True, Sums=True)
        got = base.outputs()
        assert R.Path_Frame_Read_Device(W, H, got["rgb"], got["rgba8"], got["sums"], Tone_Map=tone_map) == 4
        R.Ray_Query_Wait()
        base.assert_read(got, image, "tone map %s" % tone_map)
    R.Destroy()


@check("the statistics are ordered with the caller's stream")
def stream_order():
    t = torch()
    R = opened()
    want = R.Path_Frame_Stats()
    side = t.cuda.Stream()
    with t.cuda.stream(side):
        out = {k: v * 1 for k, v in stat_outputs().items()}  # (kernels on the side stream: the statistics have to start behind them)
        R.Path_Frame_Stats_Device(W, H, out["count"], out["moments"], out["active"], out["total"], Stream=side.cuda_stream)
        host = {k: v.cpu() for k, v in out.items()}  # (copies on the side stream: behind the statistics)
    side.synchronize()
    assert_stats(host, want, "a side stream")
    # a round behind statistics in flight: they have the state of their moment, Ray_Query_Wait is the host's wait
    with t.cuda.stream(side):
        out = stat_outputs()
        R.Path_Frame_Stats_Device(W, H, out["count"], out["moments"], out["active"], out["total"], Stream=side.cuda_stream)
    R.Path_Frame_Accumulate(3)
    R.Ray_Query_Wait()
    side.synchronize()
    assert_stats(out, want, "Ray_Query_Wait")
    assert R.Path_Frame_Info()["samples"] == 7 and R.Path_Frame_Stats()["total_samples"] > want["total_samples"]
    R.Destroy()


@check("pageable host pointers and short tensors are refused before a launch")
def refusals():
    t = torch()
    hip = base.hip
    R = opened()
    R.Set_Option(B.OPT_TIMING, 1)
    R.Path_Frame_Accumulate(1)
    R.Ray_Query_Wait()
    before = R.Ray_Query_Time()
    h = R._h
    out = stat_outputs()
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    host = np.zeros(2 * N, np.float32)
    vp = C.c_void_p(host.ctypes.data)
    t.cuda.synchronize()
    t.cuda.empty_cache()
    big = t.full((8 << 20,), FILL, dtype=t.float32, device="cuda")  # (an allocation of its own: a tensor that reaches its end is one word short)
    short2, short1 = big[big.numel() - (2 * N - 1):], big[big.numel() - (N - 1):]
    odd = C.c_void_p(out["active"].data_ptr() + 4)
    calls = {
        "pageable counts": lambda: hip.path_frame_stats_device(h, vp, None, None, None, None),
        "pageable moments": lambda: hip.path_frame_stats_device(h, None, vp, None, None, None),
        "a pageable active word": lambda: hip.path_frame_stats_device(h, None, None, vp, None, None),
        "a pageable total": lambda: hip.path_frame_stats_device(h, p(out["count"]), None, None, vp, None),
        "short counts": lambda: hip.path_frame_stats_device(h, p(short1), None, None, None, None),
        "short moments": lambda: hip.path_frame_stats_device(h, None, p(short2), None, None, None),
        "a total one word before the end": lambda: hip.path_frame_stats_device(h, None, None, None, p(big[big.numel() - 1:]), None),
        "an active word that is not aligned": lambda: hip.path_frame_stats_device(h, None, None, odd, None, None),
    }
    for what, call in calls.items():
        assert call() == B.MDH_E_INVALID, what
    t.cuda.synchronize()
    for k, v in out.items():
        assert (v.cpu().numpy() == FILL).all(), k
    assert (host == 0.0).all() and (big.cpu().numpy() == FILL).all()
    assert R.Ray_Query_Time() == before  # nothing was launched
    # Python's own checks come first
    for what, call in {"a short tensor": lambda: R.Path_Frame_Stats_Device(W, H, short1.view(t.int32)), "a host tensor": lambda: R.Path_Frame_Stats_Device(W, H, t.zeros(N, dtype=t.int32))}.items():
        try:
            call()
        except ValueError:
            continue
        raise AssertionError(what + " was accepted")
    # the statistics do not take the timing pair: the round stays what is timed
    want = R.Path_Frame_Stats()
    R.Path_Frame_Stats_Device(W, H, out["count"], out["moments"], out["active"], out["total"])
    R.Ray_Query_Wait()
    assert R.Ray_Query_Time() == before
    assert_stats(out, want, "after the refusals")
    # a plain frame, and none
    R.Path_Frame_Begin(W, H, Seed=SEED)
    assert hip.path_frame_stats_device(h, p(out["count"]), None, None, None, None) == B.MDH_E_STATE
    R.Path_Frame_End()
    assert hip.path_frame_stats_device(h, p(out["count"]), None, None, None, None) == B.MDH_E_STATE
    R.Destroy()


if __name__ == "__main__":
    base.CHECKS = CHECKS  # (main () runs the checks of the table it finds there)
    sys.exit(base.main(sys.argv[1:]))
