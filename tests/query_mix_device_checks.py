"""Every family of queries in turn on ONE renderer -- host form, then device form, the device forms on two caller streams
alternately -- with torch tensors as the device memory.  The families share one bridge to the caller's stream and to the
frames, one pair of timing events and one staging buffer; what a query answers must not depend on which family ran before
it.  The yardstick is the same call made alone on a fresh renderer, never the renderer under test in the same state.

The checks run in a process of their own, started once by tests/test_gpu_query_mix.py, for the reason
tests/ray_stream_device_checks.py gives: torch has to be imported BEFORE the library is loaded.  main () imports torch, loads
the library, runs the named checks (all by default) and writes one JSON object: check -> {ok, log, seconds}.  After a device
error nothing more is started."""
import json
import math
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
from helpers import SEED  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402

torch = None  # main (): imported before the library is loaded
hip = None

FIRST = 64          # the first host batch: d_rays at its floor of 256 rays
SIZES = (65, 300)   # one past a wavefront; past the floor, so that d_rays grows
FILL = -7
STEP = 0.1

CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


def renderer(timing):
    """the rooms scene with seeded atlases (what a shaded ray or point reads is not all zero)"""
    R = rq.gi_room(hip)
    if timing:
        R.Set_Option(B.OPT_TIMING, 1)
    irr, rad = S.seeded_atlases(R)
    R.Write_Texture(B.TEX_IRRADIANCE, irr)
    R.Write_Texture(B.TEX_RADIANCE, rad)
    return R


def inputs(n):
    """host arrays for every family: rays of the room's mixture, lengths, radii, free points with normals, views, materials"""
    org, drs = rq.room_rays(n)
    rng = np.random.RandomState(SEED % 1000 + 71)
    return {"org": org, "drs": drs, "tmax": rq.seeded_tmax(n, SEED + 13), "short": rq.seeded_tmax(n, SEED + 17, 0.2, 3.0),
            "radii": rng.uniform(0.0, 0.4, n).astype(np.float32), "pos": rq.rays_inside(n, rq.ROOM_LO, rq.ROOM_HI, SEED + 19)[0],
            "nrm": rq.unit_dirs(rng, n), "view": rq.unit_dirs(rng, n), "mat": rng.randint(0, 5, n).astype(np.int32)}


def out(n, **kinds):
    """device outputs: name -> 'f' (a float per ray), 'f3' (three), 'i' (an int)"""
    return {k: torch.full((n * (3 if v == "f3" else 1),), FILL, dtype=torch.int32 if v == "i" else torch.float32, device="cuda") for k, v in kinds.items()}


RAYCAST_OUT = dict(hit="i", index="i", t="f", steps="i", position="f3", normal="f3")


def families(R):
    """name -> (host form (h) -> dict of arrays, device form (d, n, stream) -> dict of tensors), in the order they are called.
    A device form runs with its torch stream current: the kernels that fill its outputs are on the stream the query is given."""
    kinds = [p for p, _ in R.Scene.Prims_Count]

    def raycast_d(d, n, s):
        o = out(n, **RAYCAST_OUT)
        R.Raycast_Device(d["org"], d["drs"], o["hit"], Index=o["index"], T=o["t"], Steps=o["steps"], Position=o["position"], Normal=o["normal"], Stream=s.cuda_stream, N=n)
        return o

    def visibility_d(d, n, s):
        o = out(n, vis="f")
        R.Raycast_Visibility_Device(d["org"], d["drs"], d["tmax"], o["vis"], Stream=s.cuda_stream, N=n)
        return o

    def shadows_d(d, n, s):
        o = out(n, shadow="f")
        R.Softshadows_Device(d["org"], d["drs"], 0.1, d["tmax"], 8.0, o["shadow"], Stream=s.cuda_stream, N=n)
        return o

    def spherecast_d(prims):
        def run(d, n, s):
            o = out(n, **RAYCAST_OUT)
            R.Spherecast_Device(d["org"], d["drs"], o["hit"], Radii=d["radii"], Max_Dists=d["tmax"], Prims=prims, Index=o["index"], T=o["t"], Steps=o["steps"],
                                Position=o["position"], Normal=o["normal"], Stream=s.cuda_stream, N=n)
            return o
        return run

    def contacts_d(prims):
        def run(d, n, s):
            o = out(n, dist="f", index="i", normal="f3")
            R.Contacts_Device(d["org"], o["dist"], Radii=d["radii"], Prims=prims, Index=o["index"], Normal=o["normal"], Stream=s.cuda_stream, N=n)
            return o
        return run

    def shade_rays_d(mode):
        def run(d, n, s):
            o = out(n, rgb="f3", hit="i", index="i", t="f", steps="i")
            R.Shade_Rays_Device(d["org"], d["drs"], o["rgb"], Hit=o["hit"], Index=o["index"], T=o["t"], Steps=o["steps"], Mode=mode, Stream=s.cuda_stream, N=n)
            return o
        return run

    def shade_points_d(mode):
        def run(d, n, s):
            o = out(n, rgb="f3")
            R.Shade_Points_Device(d["pos"], d["nrm"], None if mode == 3 else d["view"], None if mode == 3 else d["mat"], o["rgb"], Mode=mode, Stream=s.cuda_stream, N=n)
            return o
        return run

    def path_trace_d(d, n, s):
        o = out(n, hit="i", index="i", t="f")
        o["rgb"] = torch.zeros(3 * n, dtype=torch.float32, device="cuda")  # (the sums so far)
        R.Path_Trace_Device(d["org"], d["drs"], o["rgb"], Hit=o["hit"], Index=o["index"], T=o["t"], Seed=5, Sample_Count=2, Bounces=2, Stream=s.cuda_stream, N=n)
        return o

    def inscatter_points_d(d, n, s):
        o = out(n, rgb="f3")
        R.Inscatter_Points_Device(d["pos"], d["view"], o["rgb"], F=d["short"], Stream=s.cuda_stream, N=n)
        return o

    def inscatter_rays_d(d, n, s):
        o = out(n, rgb="f3", len="f", steps="i")
        R.Inscatter_Rays_Device(d["org"], d["drs"], d["short"], STEP, o["rgb"], Len=o["len"], Steps=o["steps"], March=True, Stream=s.cuda_stream, N=n)
        return o

    return {
        "raycast": (lambda h: R.Raycast(h["org"], h["drs"]), raycast_d),
        "visibility": (lambda h: {"vis": R.Raycast_Visibility(h["org"], h["drs"], h["tmax"])}, visibility_d),
        "soft shadows": (lambda h: {"shadow": R.Softshadows(h["org"], h["drs"], 0.1, h["tmax"], 8.0)}, shadows_d),
        "spherecast": (lambda h: R.Spherecast(h["org"], h["drs"], h["radii"], h["tmax"]), spherecast_d(None)),
        "spherecast, listed kinds": (lambda h: R.Spherecast(h["org"], h["drs"], h["radii"], h["tmax"], Prims=kinds), spherecast_d(kinds)),
        "contacts": (lambda h: R.Contacts(h["org"], h["radii"]), contacts_d(None)),
        "contacts, listed kinds": (lambda h: R.Contacts(h["org"], h["radii"], Prims=kinds), contacts_d(kinds)),
        "shaded rays, mode 0": (lambda h: R.Shade_Rays(h["org"], h["drs"], Mode=0), shade_rays_d(0)),
        "shaded rays, mode 2": (lambda h: R.Shade_Rays(h["org"], h["drs"], Mode=2), shade_rays_d(2)),
        "shaded points, mode 0": (lambda h: {"rgb": R.Shade_Points(h["pos"], h["nrm"], h["view"], h["mat"], Mode=0)}, shade_points_d(0)),
        "shaded points, mode 3": (lambda h: {"rgb": R.Shade_Points(h["pos"], h["nrm"], Mode=3)}, shade_points_d(3)),
        "path trace": (lambda h: R.Path_Trace(h["org"], h["drs"], Seed=5, Sample_Count=2, Bounces=2), path_trace_d),
        "in-scattering at points": (lambda h: {"rgb": R.Inscatter_Points(h["pos"], h["view"], h["short"])}, inscatter_points_d),
        "in-scattering along rays": (lambda h: R.Inscatter_Rays(h["org"], h["drs"], h["short"], STEP, March=True), inscatter_rays_d),
    }


def device_form(forms, d, n, stream):
    with torch.cuda.stream(stream):
        return forms[1](d, n, stream)


def to_host(o):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)).reshape(-1) for k, v in o.items()}


def same_bits(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s" % (what, k)
        assert np.array_equal(S.bits(g), S.bits(w)), "%s: %s differs from the call made alone on a fresh renderer (%d of %d words)" % (
            what, k, int((S.bits(g) != S.bits(w)).sum()), g.size)


def timed(R, call, device, what):
    """runs the call and holds its kernel time against the host's clock around it.  A host form has waited for its kernel when
    it returns; a device form returns behind the enqueue, and Ray_Query_Time waits for the kernel's end event: its wall
    time ends there."""
    t0 = time.perf_counter()
    result = call()
    t1 = time.perf_counter()
    ms = R.Ray_Query_Time()
    t2 = time.perf_counter()
    wall = ((t2 if device else t1) - t0) * 1000.0
    print("   %-52s kernel %8.4f ms, wall %8.4f ms" % (what, ms, wall), flush=True)
    assert math.isfinite(ms) and ms > 0.0, "%s: a kernel time of %r ms" % (what, ms)
    assert ms <= wall, "%s: a kernel time of %r ms in a call of %r ms" % (what, ms, wall)
    return result


@check("every family after every other on one renderer has the bits of the call made alone; its kernel time is its own")
def mixed():
    h = {n: inputs(n) for n in (FIRST,) + SIZES}
    d = {n: {k: torch.from_numpy(v).cuda() for k, v in h[n].items()} for n in SIZES}
    torch.cuda.synchronize()
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    R = renderer(True)
    fam = families(R)
    got = []  # (what, family, form, n, answers)
    timed(R, lambda: R.Raycast(h[FIRST]["org"], h[FIRST]["drs"]), False, "the first host batch")
    turn = 0
    for n in SIZES:
        if n == SIZES[-1]:  # a device query nobody waits for, and at once the host batch that outgrows d_rays
            got.append(("raycast, device form, n %d, not waited for" % SIZES[0], "raycast", 1, SIZES[0], device_form(fam["raycast"], d[SIZES[0]], SIZES[0], sides[turn % 2])))
            turn += 1
        for name, forms in fam.items():
            what = "%s, host form, n %d" % (name, n)
            got.append((what, name, 0, n, timed(R, lambda: forms[0](h[n]), False, what)))
            what = "%s, device form, n %d" % (name, n)
            side = sides[turn % 2]
            turn += 1
            got.append((what, name, 1, n, timed(R, lambda: device_form(forms, d[n], n, side), True, what)))
    R.Ray_Query_Wait()
    torch.cuda.synchronize()
    got = [(what, name, form, n, to_host(o)) for what, name, form, n, o in got]
    R.Destroy()
    for what, name, form, n, answers in got:  # the yardstick: the call alone, on a renderer that has done nothing else
        Rf = renderer(False)
        alone = families(Rf)[name]
        want = to_host(alone[0](h[n]) if form == 0 else device_form(alone, d[n], n, torch.cuda.current_stream()))
        same_bits(answers, want, what)
        Rf.Destroy()


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
