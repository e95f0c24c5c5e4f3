#!/usr/bin/env python3
"""Times the 1080p frame of the obj_mesh example (1000 triangles behind a 30 x 20 x 20 partition: a scene table larger
than LDS, read from device memory) the way bench.py times a workload: frames kept in flight (MDH_OPT_FRAME_OVERLAP as the
library sets it), then one device-synchronised frame at a time, then each pass's kernel time from the strictly serial
schedule.  Prints one JSON line.

    python scripts/bench_mesh.py [--width 1920 --height 1080] [--steps 50] [--warmup 5] [--camera example|parity]
                                 [--force-residency] [--scene obj_mesh|simple_scene] [--cpu-baseline]

--scene simple_scene with and without --force-residency is the A/B of the residency by itself on a scene that fits LDS.
--camera parity looks at the mesh from (1.5, 1, -1.5) (the example's own camera sees the torus edge-on)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args, binding):
    from madarch_amd import _binding as B
    from madarch_amd import examples
    R = examples.SCENES[args.scene](args.width, args.height, Binding=binding)
    if args.scene == "obj_mesh" and args.camera == "parity":
        R.Set_Camera_Position((1.5, 1.0, -1.5))
    if args.force_residency and binding.prefix == "mdh_":
        R.Set_Option(B.OPT_TABLE_RESIDENCY, 1)
    return R


def cpu_baseline(args):
    """the CPU oracle on the same frame (test infrastructure, as bench.py's cpu_baseline): context, not a yardstick"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_engine import ORC_OPT_THREADS, oracle_binding
    R = build(args, oracle_binding())
    R.Set_Option(ORC_OPT_THREADS, min(16, len(os.sched_getaffinity(0))))
    R.Render()
    frames, t = 0, time.perf_counter()
    while True:
        R.Render()
        frames += 1
        dt = time.perf_counter() - t
        if dt > 10.0 or frames >= 16:
            break
    return {"value": round(args.width * args.height * frames / dt / 1e6, 4), "unit": "Mpixels/s", "cores": R.Get_Option(ORC_OPT_THREADS), "frames": frames}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prewarm-s", type=float, default=0.4)
    ap.add_argument("--scene", default="obj_mesh", choices=["obj_mesh", "simple_scene"])
    ap.add_argument("--camera", default="example", choices=["example", "parity"])
    ap.add_argument("--force-residency", action="store_true")
    ap.add_argument("--cpu-baseline", action="store_true")
    args = ap.parse_args()
    from madarch_amd import _binding as B
    R = build(args, B.hip_binding())
    mpix = args.width * args.height / 1e6
    t_pre = time.perf_counter()
    while True:  # (the clocks of an idle GPU ramp up over the first few hundred milliseconds of load)
        for _ in range(5):
            R.Render()
        R.Finish()
        if time.perf_counter() - t_pre >= args.prewarm_s:
            break
    for _ in range(args.warmup):
        R.Render()
    R.Finish()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        R.Render()
    R.Finish()
    dt = (time.perf_counter() - t0) / args.steps
    overlap = R.Get_Option(B.OPT_FRAME_OVERLAP)
    # each kernel on its own, then SURVEY.md 8(d)'s frame: one device-synchronised Renderers.Render at a time
    R.Set_Option(B.OPT_FRAME_OVERLAP, 0)
    R.Set_Option(B.OPT_TIMING, 1)
    for _ in range(3):
        R.Render()
    R.Finish()
    R.Reset_Pass_Times()
    for _ in range(10):
        R.Render()
    R.Finish()
    passes = {}
    for p, name in enumerate(B.PASS_NAMES):
        ms, n = R.Pass_Time(p)
        if n:
            passes[name] = {"ms_avg": round(ms / n, 4), "launches": n}
    R.Set_Option(B.OPT_TIMING, 0)
    n_serial = max(10, min(args.steps, 50))
    R.Finish()
    ts = time.perf_counter()
    for _ in range(n_serial):
        R.Render()
        R.Finish()
    dts = (time.perf_counter() - ts) / n_serial
    out = {"metric": "%s_%dx%d_mpixels_per_s" % (args.scene, args.width, args.height), "value": round(mpix / dt, 3), "unit": "Mpixels/s",
           "ms_per_step": round(dt * 1e3, 4), "value_serial": round(mpix / dts, 3), "ms_per_step_serial": round(dts * 1e3, 4),
           "frame_overlap": overlap, "steps": args.steps, "warmup": args.warmup, "camera": args.camera,
           "table_residency": R.Get_Option(B.OPT_TABLE_RESIDENCY), "forced_residency": bool(args.force_residency),
           "partition_warnings": R.Partition_Warnings(), "passes_serial": passes, "version": (B.hip_binding().version() or b"").decode()}
    R.Destroy()
    if args.cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
