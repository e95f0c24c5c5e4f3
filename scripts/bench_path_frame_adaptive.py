#!/usr/bin/env python3
"""Times an adaptive path-traced frame (Path_Frame_Begin_Adaptive: a count and two moments a pixel, a stopping rule, a compaction
of the pixels still running) against the plain accumulator it extends.  Run by hand on one MI355X; bench.py does not call it
and there is no threshold.

Per scene (the headline scene, global_illumination with config 3's probes, and examples.obj_mesh behind its partition), over the
width x height pixels with --bounces bounces and jitter, three forms ALTERNATED in one process:
  - plain     Path_Frame_Accumulate to --max samples in rounds of --round: what the parent can do
  - in_place  adaptive, the same rounds, OPT_PATH_FRAME_COMPACT 0: retired pixels keep their lanes and idle
  - compact   the same with OPT_PATH_FRAME_COMPACT 1
Each figure is the host's time from the first enqueue to Ray_Query_Wait's return (the accumulator opened and the device idle
before it), the median of --repeats rounds behind a warm-up round, with the spread (max - min) beside it.  Beside the times:
total_samples, the active count behind every round (from a pass of its own, which waits between the rounds and is not timed),
and the mean absolute linear error against a plain frame of --reference samples of the same seed.

    python scripts/bench_path_frame_adaptive.py [--width 1920 --height 1080] [--bounces 3] [--repeats 5] [--scenes a,b] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def med(xs):
    return {"ms": round(statistics.median(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min", type=int, default=4, dest="lo")
    ap.add_argument("--max", type=int, default=16, dest="hi")
    ap.add_argument("--round", type=int, default=4, dest="per_round")
    ap.add_argument("--tolerance", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--reference", type=int, default=1024)
    ap.add_argument("--scenes", default="global_illumination_ddgi8x8x8,obj_mesh_partition")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # before the library is loaded
    if not torch.cuda.is_available():
        sys.exit("bench_path_frame_adaptive.py measures on a GPU: none is visible")
    torch.zeros(1, device="cuda")
    import bench_ray_queries as brq
    from madarch_amd import _binding as B
    W, H = args.width, args.height
    rounds = [min(args.per_round, args.hi - first) for first in range(0, args.hi, args.per_round)]
    rule = dict(Min_Samples=args.lo, Max_Samples=args.hi, Tolerance=args.tolerance, Floor=args.floor)
    results = []
    for name, build, _cam, _box in brq.scenes(W, H):
        if name not in args.scenes.split(","):
            continue
        R = build()
        kw = dict(Seed=args.seed, Bounces=args.bounces, Jitter=True)

        def begin(form):
            if form == "plain":
                R.Path_Frame_Begin(W, H, **kw)
            else:
                R.Set_Option(B.OPT_PATH_FRAME_COMPACT, 1 if form == "compact" else 0)
                R.Path_Frame_Begin_Adaptive(W, H, **kw, **rule)
            R.Ray_Query_Wait()

        # the reference: a plain frame of many samples, in slices
        begin("plain")
        for first in range(0, args.reference, 64):
            R.Path_Frame_Accumulate(min(64, args.reference - first))
            R.Ray_Query_Wait()
        reference = R.Path_Frame_Read()["rgb"].astype(np.float64)
        forms = ("plain", "in_place", "compact")
        times = {k: [] for k in forms}
        for rnd in range(args.repeats + 1):  # round 0 is the warm-up
            for form in forms:
                begin(form)
                t0 = time.perf_counter()
                for k in rounds:
                    R.Path_Frame_Accumulate(k)
                R.Ray_Query_Wait()
                ms = (time.perf_counter() - t0) * 1e3
                if rnd > 0:
                    times[form].append(ms)
        row = {"scene": name, "pixels": W * H, "bounces": args.bounces, "rounds": rounds, "rule": rule}
        states = {}
        for form in forms:  # once more, not timed: the counts behind every round, the image
            begin(form)
            active = []
            for k in rounds:
                R.Path_Frame_Accumulate(k)
                if form != "plain":
                    active.append(R.Path_Frame_Stats(Count=False, Moments=False)["active"])
            image = R.Path_Frame_Read(Sums=True)
            total = W * H * args.hi if form == "plain" else R.Path_Frame_Stats(Count=False, Moments=False)["total_samples"]
            if form != "plain":
                states[form] = (image["sums"], R.Path_Frame_Stats()["count"])
            row[form] = dict(med(times[form]), total_samples=int(total), active_behind_each_round=active,
                             mean_abs_error=float(np.nanmean(np.abs(image["rgb"].astype(np.float64) - reference))), rounds_ms=[round(x, 4) for x in times[form]])
        a, b = states["in_place"], states["compact"]
        row["both_mappings_give_the_same_bits"] = bool(np.array_equal(a[1], b[1]) and ((a[0].view(np.uint32) == b[0].view(np.uint32)) | (np.isnan(a[0]) & np.isnan(b[0]))).all())
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        R.Destroy()
    line = json.dumps({"metric": "path_frame_adaptive_%dx%d" % (W, H), "unit": "ms", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
                       "reference_samples": args.reference, "library": os.path.basename(B.HIP_LIBRARY), "results": results, "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
