#!/usr/bin/env python3
"""Times the 1080p frame of the obj_mesh example (1000 triangles, the example's camera) three ways, alternating them in one
process so that they share the session's clocks and neighbours:

    a  MDH_OPT_TRIANGLE_BVH on, no partition   -- the exact scan, walked through the hierarchy
    b  the option off, no partition             -- the same bits, every triangle at every march step: the fair baseline
    c  the GPU_Fast partition (the example)     -- another picture (cells cut at Index_Count): context only

Each run, like scripts/bench_mesh.py: frames kept in flight, then one device-synchronised frame at a time, then each pass's
kernel time from the strictly serial schedule.  A run stops after --steps frames or --seconds, whichever comes first (the
scan of b takes a large part of a second per frame).  Prints one JSON line: every run, and per variant the median and the
spread (max - min) over the rounds.

    python scripts/bench_mesh_bvh.py [--width 1920 --height 1080] [--rounds 3] [--steps 30] [--seconds 6] [--variants abc]

With a library built by `make -C madarch_amd/csrc bvhstats` (MADARCH_HIP_LIBRARY) variant a also reports the share of node
visits that skipped their subtree."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args, variant):
    from madarch_amd import examples
    if variant == "c":
        return examples.obj_mesh(args.width, args.height)
    R = examples.obj_mesh(args.width, args.height, Triangle_BVH=True)
    if variant == "b":
        from madarch_amd import _binding as B
        R.Set_Option(B.OPT_TRIANGLE_BVH, 0)
    return R


def timed(R, steps, seconds, sync):
    n, t0 = 0, time.perf_counter()
    while n < steps:
        R.Render()
        if sync:
            R.Finish()
        n += 1
        if time.perf_counter() - t0 > seconds:
            break
    R.Finish()
    return (time.perf_counter() - t0) / n, n


def run(args, variant):
    from madarch_amd import _binding as B
    lib = B.hip_binding().lib
    R = build(args, variant)
    mpix = args.width * args.height / 1e6
    for _ in range(2):
        R.Render()
    R.Finish()
    stats = None
    if variant == "a" and hasattr(lib, "mdh_diag_bvh"):
        out = (ctypes.c_ulonglong * 2)()
        lib.mdh_diag_bvh(out)
        R.Render()
        R.Finish()
        lib.mdh_diag_bvh(out)
        stats = {"node_visits": out[0], "skipped": out[1], "share_skipped": round(out[1] / max(1, out[0]), 4)}
    dt, n = timed(R, args.steps, args.seconds, False)
    overlap = R.Get_Option(B.OPT_FRAME_OVERLAP)
    R.Set_Option(B.OPT_FRAME_OVERLAP, 0)
    R.Set_Option(B.OPT_TIMING, 1)
    R.Render()
    R.Finish()
    R.Reset_Pass_Times()
    timed(R, 5, args.seconds / 2, True)
    passes = {}
    for p, name in enumerate(B.PASS_NAMES):
        ms, k = R.Pass_Time(p)
        if k:
            passes[name] = round(ms / k, 4)
    R.Set_Option(B.OPT_TIMING, 0)
    dts, ns = timed(R, args.steps, args.seconds, True)
    res = {"variant": variant, "mpixels_per_s": round(mpix / dt, 3), "ms_per_frame": round(dt * 1e3, 3), "frames": n,
           "mpixels_per_s_serial": round(mpix / dts, 3), "ms_per_frame_serial": round(dts * 1e3, 3), "frames_serial": ns,
           "frame_overlap": overlap, "pass_ms": passes, "table_residency": R.Get_Option(B.OPT_TABLE_RESIDENCY),
           "triangle_bvh": R.Get_Option(B.OPT_TRIANGLE_BVH)}
    if stats:
        res["bvh_stats"] = stats
    R.Destroy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--variants", default="abc")
    args = ap.parse_args()
    from madarch_amd import _binding as B
    runs = []
    for _ in range(args.rounds):
        for v in args.variants:
            runs.append(run(args, v))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    summary = {}
    for v in args.variants:
        for key in ("mpixels_per_s", "mpixels_per_s_serial"):
            vals = [r[key] for r in runs if r["variant"] == v]
            summary["%s_%s" % (v, key)] = {"median": round(statistics.median(vals), 3), "spread": round(max(vals) - min(vals), 3)}
    print(json.dumps({"metric": "obj_mesh_%dx%d_triangle_bvh" % (args.width, args.height), "unit": "Mpixels/s", "summary": summary,
                      "runs": runs, "version": (B.hip_binding().version() or b"").decode()}))


if __name__ == "__main__":
    main()
