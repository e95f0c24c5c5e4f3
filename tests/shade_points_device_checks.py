"""The checks of mdh_shade_points_device on the device, with torch tensors as the device memory.  They run in a process of
their own, started once by tests/test_gpu_shade_points.py, for the reason tests/ray_stream_device_checks.py gives: torch has
to be imported BEFORE the library is loaded.  main () imports torch, loads the library, runs the named checks (all by
default) and writes one JSON object: check -> {ok, log, seconds}.  After a device error nothing more is started.  The
host-array call is the yardstick: tests/test_gpu_shade_points.py holds it against the oracle, the frame and float64."""
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

import ray_query_cases as rq  # noqa: E402
import shade_points_cases as P  # noqa: E402
import shade_rays_cases as S  # noqa: E402
from helpers import SEED  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402

torch = None  # main (): imported before the library is loaded
hip = None

N = 257
PAD, FILL = 64, -7

CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(n):
    return torch.full((n,), FILL, dtype=torch.float32, device="cuda")


def points(R, name="rooms", n=N):
    """n points of the scene's five classes with seeded view directions and materials (host arrays)"""
    pos, nrm, _ = P.irradiance_points(R, name, P.scene_rays(name, n), n)
    rng = np.random.RandomState(SEED % 1000 + 67)
    return pos, nrm, rq.unit_dirs(rng, n), rng.randint(0, 5, n).astype(np.int32)


def shade_device(R, d, n, mode, tone, stream=0, pad=PAD):
    rgb = filled(3 * n + pad)
    R.Shade_Points_Device(d[0], d[1], None if mode == 3 else d[2], None if mode == 3 else d[3], rgb, Mode=mode, Tone_Map=tone, Stream=stream, N=n)
    return rgb


def to_host(rgb, n):
    got = rgb.cpu().numpy()  # (on torch's current stream: ordered behind a query that was given it)
    assert (got[3 * n:] == FILL).all(), "written past its %d points" % n
    return got[:3 * n].reshape(-1, 3)


def host(R, h, mode, tone=False):
    return R.Shade_Points(h[0], h[1], *(() if mode == 3 else (h[2], h[3])), Mode=mode, Tone_Map=tone)


@check("device arrays have the host arrays' bits, all three modes, linear and tone-mapped")
def same_bits_as_host():
    for name in ("rooms", "partition, Fallback", "mesh, triangle BVH"):
        R = S.frame_renderer(hip, name, 0)
        h = points(R, name)
        d = [dev(a) for a in h]
        for mode in (0, 2, 3):
            for tone in ((False,) if mode == 3 else (False, True)):
                want = host(R, h, mode, tone)
                for n in (1, 65, N):
                    got = to_host(shade_device(R, d, n, mode, tone), n)
                    assert np.array_equal(S.bits(got), S.bits(want[:n])), "%s mode %d tone %d n %d" % (name, mode, tone, n)
        R.Destroy()


@check("a point that is not shaded is answered by its lane, its neighbours keep their bits")
def bad_points():
    R = S.frame_renderer(hip, "rooms", 0)
    h = points(R)
    want = {mode: host(R, h, mode) for mode in (0, 2, 3)}
    pos, nrm, view, mat = (a.copy() for a in h)
    # a NaN, a position beyond the bound, a normal and a view direction beyond theirs, material ids outside the table
    pos[5, 1] = np.nan
    pos[63, 0] = 2000.0
    nrm[64, 2] = np.inf
    nrm[70, 0] = 1.5
    pos[130, 2] = -np.inf
    view[200, 1] = -2.0
    view[201, 0] = np.nan
    mat[256] = 20
    mat[100] = -1
    bad_all = [5, 63, 64, 70, 130]            # what mode 3 reads too
    bad_full = bad_all + [100, 200, 201, 256]  # view directions and material ids: modes 0 and 2 only
    d = [dev(a) for a in (pos, nrm, view, mat)]
    for mode in (0, 2, 3):
        got = to_host(shade_device(R, d, N, mode, False), N)
        bad = bad_all if mode == 3 else bad_full
        good = [q for q in range(N) if q not in bad]
        assert (got[bad].view(np.uint32) == P.BAD_BITS).all(), (mode, got[bad])
        assert np.array_equal(S.bits(got[good]), S.bits(want[mode][good])), "mode %d: the neighbours of the planted points" % mode
    R.Destroy()


@check("the answers are ordered with the caller's stream")
def stream_order():
    R = S.frame_renderer(hip, "rooms", 0)
    h = points(R)
    want = host(R, h, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d = [torch.from_numpy(a).cuda(non_blocking=False) for a in h]
        d = [d[0] * 1.0, d[1] * 1.0, d[2] * 1.0, d[3] + 0]  # (kernels on the side stream: the query has to start behind them)
        rgb = shade_device(R, d, N, 0, False, stream=side.cuda_stream)
        got = to_host(rgb * 1.0, N)  # (a kernel and a copy on the side stream, no host wait between: behind the query)
    assert np.array_equal(S.bits(got), S.bits(want)), "a side stream"
    # and the host's wait
    with torch.cuda.stream(side):
        rgb = shade_device(R, d, N, 3, False, stream=side.cuda_stream)
    R.Ray_Query_Wait()
    side.synchronize()
    assert np.array_equal(S.bits(to_host(rgb, N)), S.bits(host(R, h, 3))), "Ray_Query_Wait"
    R.Destroy()


@check("pageable host pointers, arrays that end outside their allocation and bad arguments are refused before a launch")
def refusals():
    R = S.frame_renderer(hip, "rooms", 0)
    R.Set_Option(B.OPT_TIMING, 1)
    h = points(R)
    d = [dev(a) for a in h]
    want = host(R, h, 0)
    t_before = R.Ray_Query_Time()
    assert t_before > 0.0
    rgb = filled(3 * N)
    hv = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    host_rgb = np.zeros((N, 3), np.float32)
    # an array whose last 40 bytes alone lie inside its allocation: 32 MiB get an allocation of their own from torch, exactly as large
    big = torch.full((8 << 20,), FILL, dtype=torch.float32, device="cuda")
    tail = C.c_void_p(big.data_ptr() + (big.numel() - 10) * 4)

    def call(n=N, pos=p(d[0]), nrm=p(d[1]), view=p(d[2]), mat=p(d[3]), mode=0, tone=0, out=p(rgb)):
        return hip.shade_points_device(R._h, n, pos, nrm, view, mat, mode, tone, out, None)
    refused = {
        "pageable positions": lambda: call(pos=hv(h[0])), "pageable normals": lambda: call(nrm=hv(h[1])), "pageable view directions": lambda: call(view=hv(h[2])),
        "pageable material ids": lambda: call(mat=hv(h[3])), "pageable colours": lambda: call(out=hv(host_rgb)),
        "positions that end outside their allocation": lambda: call(pos=tail), "colours that end outside theirs": lambda: call(out=tail),
        "material ids that end outside theirs": lambda: call(mat=tail), "mode 3: normals that end outside theirs": lambda: call(nrm=tail, mode=3, view=None, mat=None),
        "mode 1": lambda: call(mode=1), "n < 0": lambda: call(n=-1), "no colours": lambda: call(out=None), "mode 3 tone-mapped": lambda: call(mode=3, tone=1),
        "mode 0 without view directions": lambda: call(view=None), "mode 0 without material ids": lambda: call(mat=None),
        "mode 2 without view directions": lambda: call(mode=2, view=None), "mode 2 without material ids": lambda: call(mode=2, mat=None),
    }
    for what, fn in refused.items():
        assert fn() == B.MDH_E_INVALID, what
    torch.cuda.synchronize()
    assert (rgb.cpu().numpy() == FILL).all() and (big[-16:].cpu().numpy() == FILL).all()
    assert R.Ray_Query_Time() == t_before  # (no kernel was timed since: none was launched)
    assert call(n=0) == B.MDH_OK
    # mode 3 takes NULL for both, and pointers it does not read are not looked at
    assert call(mode=3, view=None, mat=None) == B.MDH_OK
    R.Ray_Query_Wait()
    i3 = rgb.cpu().numpy().reshape(-1, 3).copy()
    assert call(mode=3, view=hv(h[2]), mat=hv(h[3])) == B.MDH_OK
    R.Ray_Query_Wait()
    assert np.array_equal(S.bits(rgb.cpu().numpy().reshape(-1, 3)), S.bits(i3)) and np.array_equal(S.bits(i3), S.bits(host(R, h, 3)))
    # the renderer still answers
    assert np.array_equal(S.bits(to_host(shade_device(R, d, N, 0, False), N)), S.bits(want)), "after the refusals"
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
