#!/usr/bin/env python3
"""Times Inscatter_Rays (k_ray_inscatter: one wavefront per ray, a ray's steps spread over the lanes in chunks of 64) on one
MI355X.  Run by hand; bench.py does not call it and there is no threshold.

Over the light_shafts scene with its default volumetrics, under OPT_TIMING (two events on the query stream around the kernel:
Ray_Query_Time, without the copies), the median of --repeats calls behind a warm-up, and the spread:
  - the camera rays of the 250 x 250 scattering texels, step 0.1, tmax 10: the work of the frame's scattering texture, with
    the integrand evaluated at every step instead of tapped from the froxels;
  - the camera rays of a --width x --height frame with tmax = the primary ray's t (max_dist on a miss), step 0.1;
  - steps per second, and the share of lane slots that held a live step: sum (steps) / sum (64 * ceil (steps / 64));
  - for context, the visibility and scattering passes' times of --frames frames of the same scene (Pass_Time).
And the froxel approximation against its ground truth: the mean absolute difference, per channel of the tone-mapped image,
between examples.foggy_fisheye_view over the pinhole's own rays and the frame (--view pixels square).

    python scripts/bench_inscatter.py [--width 1920 --height 1080] [--repeats 5] [--frames 20] [--view 256] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(xs):
    return {"ms": round(statistics.median(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def timed(R, org, drs, tmax, step, repeats):
    def call():
        out = R.Inscatter_Rays(org, drs, tmax, step)
        return R.Ray_Query_Time(), out
    call()  # the warm-up
    runs = [call() for _ in range(repeats)]
    steps = runs[-1][1]["steps"].astype(np.int64)
    m = med([t for t, _ in runs])
    slots = (64 * ((steps + 63) // 64)).sum()
    return {"n": int(len(org)), "step": step, "kernel": m, "steps": int(steps.sum()), "mean_steps_per_ray": round(float(steps.mean()), 2),
            "steps_per_s": round(float(steps.sum()) / (m["ms"] * 1e-3), 1), "live_lane_share": round(float(steps.sum()) / max(int(slots), 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--view", type=int, default=256)
    ap.add_argument("--step", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from madarch_amd import _binding as B
    from madarch_amd import examples
    W, H = args.width, args.height
    R = examples.light_shafts(W, H)
    R.Set_Option(B.OPT_TIMING, 1)
    results = {}
    org, drs = R.Camera_Rays(250, 250)
    results["scattering_texels_250x250_tmax_10"] = timed(R, org, drs, 10.0, args.step, args.repeats)
    print(json.dumps(results["scattering_texels_250x250_tmax_10"]), file=sys.stderr, flush=True)
    org, drs = R.Camera_Rays(W, H)
    rc = R.Raycast(org, drs)
    tmax = np.where(rc["hit"] == 1, np.minimum(rc["t"], np.float32(R.Scene.Max_Dist)), np.float32(R.Scene.Max_Dist)).astype(np.float32)
    results["camera_rays_%dx%d_tmax_t" % (W, H)] = timed(R, org, drs, tmax, args.step, args.repeats)
    print(json.dumps(results["camera_rays_%dx%d_tmax_t" % (W, H)]), file=sys.stderr, flush=True)
    R.Reset_Pass_Times()
    for _ in range(args.frames):
        R.Render()
    R.Finish()
    passes = {}
    for name, p in (("visibility", B.PASS_VISIBILITY), ("scattering", B.PASS_SCATTERING)):
        ms, launches = R.Pass_Time(p)
        passes[name] = {"ms_per_launch": round(ms / max(launches, 1), 4), "launches": int(launches)}
    results["frame_passes_%dx%d" % (W, H)] = passes
    R.Destroy()
    view = None
    if args.view > 0:
        V = args.view
        R = examples.light_shafts(V, V)
        for _ in range(4):
            R.Render()
        R.Finish()
        frame = R.Read_Framebuffer().astype(np.float64)
        foggy = examples.foggy_fisheye_view(R, V, V, Step=args.step, Rays=R.Camera_Rays(V, V)).astype(np.float64)
        both = np.isfinite(frame).all(axis=-1) & np.isfinite(foggy).all(axis=-1)
        view = {"pixels": int(both.sum()), "mean_abs_difference_rgb_tone_mapped": [round(float(np.abs(frame - foggy)[both][:, c].mean()), 6) for c in range(3)],
                "largest": round(float(np.abs(frame - foggy)[both].max()), 6)}
        print(json.dumps(view), file=sys.stderr, flush=True)
        R.Destroy()
    line = json.dumps({"metric": "inscatter_rays", "unit": "ms", "scene": "light_shafts", "repeats": args.repeats, "library": os.path.basename(B.HIP_LIBRARY),
                       "results": results, "foggy_view_against_the_frame_%dx%d" % (args.view, args.view): view,
                       "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
