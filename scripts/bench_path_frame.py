#!/usr/bin/env python3
"""Times Path_Frame_Accumulate (k_path_frame: an 8 x 8 tile of pixels per wavefront, the sums in the renderer's own memory)
against what a host could do for the same pixels before it: Camera_Rays_Device + Path_Trace_Device on device arrays
(k_path_trace: a row of 64 rays per wavefront).  Run by hand on one MI355X; bench.py does not call it and there is no threshold.

Per scene (the headline scene, global_illumination with config 3's probes, and examples.obj_mesh behind its partition), over the
width x height pixels with --bounces bounces, in slices of 1 and 16 samples, three forms ALTERNATED in one process:
  - rays    Path_Trace_Device over Camera_Rays_Device's rays: the baseline
  - frame0  Path_Frame_Accumulate without jitter: tiles, and the primary segment evaluated once per launch and pixel
  - frame1  Path_Frame_Accumulate with jitter: tiles, every sample's own primary ray
Each figure is the kernel's time (OPT_TIMING, two events on the query stream: Ray_Query_Time), the median of --repeats
rounds behind a warm-up round, with the spread (max - min) beside it; a round times the three forms one after the other, so
that drift of the clocks meets all three alike.  The un-jittered sums are held against the baseline's bit for bit while at it.

    python scripts/bench_path_frame.py [--width 1920 --height 1080] [--bounces 3] [--repeats 5] [--scenes a,b] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

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
    ap.add_argument("--slices", default="1,16")
    ap.add_argument("--scenes", default="global_illumination_ddgi8x8x8,obj_mesh_partition")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # before the library is loaded
    if not torch.cuda.is_available():
        sys.exit("bench_path_frame.py measures on a GPU: none is visible")
    torch.zeros(1, device="cuda")
    import bench_ray_queries as brq
    from madarch_amd import _binding as B
    W, H = args.width, args.height
    n = W * H
    results = []
    for name, build, _cam, _box in brq.scenes(W, H):
        if name not in args.scenes.split(","):
            continue
        # one renderer per form: an accumulator belongs to its renderer, and all three see the same scene and camera
        Rs = {"rays": build(), "frame0": build(), "frame1": build()}
        for R in Rs.values():
            R.Set_Option(B.OPT_TIMING, 1)
        d_org, d_dir = torch.empty(3 * n, device="cuda"), torch.empty(3 * n, device="cuda")
        Rs["rays"].Camera_Rays_Device(W, H, d_org, d_dir)
        d_rgb = torch.zeros(3 * n, device="cuda")
        torch.cuda.synchronize()
        for count in [int(s) for s in args.slices.split(",")]:
            d_rgb.zero_()
            torch.cuda.synchronize()
            Rs["frame0"].Path_Frame_Begin(W, H, Seed=args.seed, Bounces=args.bounces, Jitter=False)
            Rs["frame1"].Path_Frame_Begin(W, H, Seed=args.seed, Bounces=args.bounces, Jitter=True)
            done = [0]

            def rays():
                Rs["rays"].Path_Trace_Device(d_org, d_dir, d_rgb, Seed=args.seed, Sample_First=done[0], Sample_Count=count, Bounces=args.bounces)
                Rs["rays"].Ray_Query_Wait()
                return Rs["rays"].Ray_Query_Time()

            def frame(which):
                def call():
                    Rs[which].Path_Frame_Accumulate(count)
                    Rs[which].Ray_Query_Wait()
                    return Rs[which].Ray_Query_Time()
                return call
            forms = {"rays": rays, "frame0": frame("frame0"), "frame1": frame("frame1")}
            times = {k: [] for k in forms}
            for rnd in range(args.repeats + 1):  # round 0 is the warm-up
                for k, call in forms.items():
                    ms = call()
                    if rnd > 0:
                        times[k].append(ms)
                done[0] += count
            sums = Rs["frame0"].Path_Frame_Read(Rgb=False, Sums=True)["sums"].reshape(-1)
            base = d_rgb.cpu().numpy()
            same = bool(((sums.view(np.uint32) == base.view(np.uint32)) | (np.isnan(sums) & np.isnan(base))).all())
            m = {k: med(v) for k, v in times.items()}
            row = {"scene": name, "n": n, "bounces": args.bounces, "samples_per_call": count, "rays": m["rays"], "frame_no_jitter": m["frame0"], "frame_jitter": m["frame1"],
                   "no_jitter_over_rays": round(m["frame0"]["ms"] / m["rays"]["ms"], 4), "jitter_over_rays": round(m["frame1"]["ms"] / m["rays"]["ms"], 4),
                   "no_jitter_sums_are_the_rays_bits": same, "rounds_ms": {k: [round(x, 4) for x in v] for k, v in times.items()}}
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        for R in Rs.values():
            R.Destroy()
    line = json.dumps({"metric": "path_frame_%dx%d" % (W, H), "unit": "ms", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
                       "library": os.path.basename(B.HIP_LIBRARY), "results": results, "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
