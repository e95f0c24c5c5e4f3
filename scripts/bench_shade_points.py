#!/usr/bin/env python3
"""Times Shade_Points and Shade_Points_Device (k_point_shade: the lighting of a point the host owns, one point per lane)
against Shade_Rays_Device over the rays of the same pixels (k_ray_shade: the same lighting behind a primary march) on one
MI355X.  Run by hand; bench.py does not call it and there is no threshold.

Per scene (the headline scene, global_illumination with config 3's probes, and examples.obj_mesh behind its partition) the
frame's hit points are taken as a host would take them -- Camera_Rays -> Raycast -> Primitive_Material -- and then
  - k_point_shade in modes 0, 2 and 3 and k_ray_shade in modes 0 and 2 over the hit pixels' rays are timed ALTERNATELY in one
    process (OPT_TIMING, two events on the query stream; device arrays), median of --repeats rounds behind a warm-up, and the spread;
  - the device-array call followed by Ray_Query_Wait and the host-array call are timed end to end on the host's clock.
Before anything is timed the points' colours are compared with their rays' and with the frame's pixels, bit for bit.

    python scripts/bench_shade_points.py [--width 1920 --height 1080] [--repeats 5] [--scenes a,b] [--out FILE]
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default="global_illumination_ddgi8x8x8,obj_mesh_partition")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # before the library is loaded
    if not torch.cuda.is_available():
        sys.exit("bench_shade_points.py measures on a GPU: none is visible")
    torch.zeros(1, device="cuda")
    import bench_ray_queries as brq
    from madarch_amd import _binding as B
    W, H = args.width, args.height
    results = []
    for name, build, _cam, _box in brq.scenes(W, H):
        if name not in args.scenes.split(","):
            continue
        R = build()
        R.Set_Option(B.OPT_FRAME_OVERLAP, 0)
        R.Set_Option(B.OPT_SCREEN_REPLAY, 0)
        R.Set_Option(B.OPT_TIMING, 1)
        for _ in range(4):  # the probes hold light
            R.Render()
        R.Finish()
        org, drs = R.Camera_Rays(W, H)
        rc = R.Raycast(org, drs)
        mat = R.Primitive_Material(rc["index"])
        rows = np.nonzero(rc["hit"] == 1)[0]
        n = len(rows)
        c = np.ascontiguousarray
        h = {"org": c(org[rows]), "dir": c(drs[rows]), "pos": c(rc["position"][rows]), "nrm": c(rc["normal"][rows]), "mat": c(mat[rows])}
        d = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
        d_rgb = torch.empty(3 * n, device="cuda")
        row = {"scene": name, "pixels": W * H, "n": n}

        def points(mode, tone=False):
            R.Shade_Points_Device(d["pos"], d["nrm"], None if mode == 3 else d["dir"], None if mode == 3 else d["mat"], d_rgb, Mode=mode, Tone_Map=tone)
            R.Ray_Query_Wait()

        def rays(mode, tone=False):
            R.Shade_Rays_Device(d["org"], d["dir"], d_rgb, Mode=mode, Tone_Map=tone)
            R.Ray_Query_Wait()

        def host_points(mode, tone=False):
            return R.Shade_Points(h["pos"], h["nrm"], *(() if mode == 3 else (h["dir"], h["mat"])), Mode=mode, Tone_Map=tone)
        # the same bits first: the points' colours are their rays' and the frame's
        same = True
        for mode in (0, 2):
            R.Set_Option(B.OPT_SCREEN_MODE, mode)
            R.Render_Pass(B.PASS_SCREEN)
            fb = R.Read_Framebuffer().reshape(-1, 3)[rows]
            points(mode, True)
            got = d_rgb.cpu().numpy().reshape(-1, 3).copy()
            rays(mode, True)
            same = same and np.array_equal(got.view(np.uint32), fb.view(np.uint32)) and np.array_equal(got.view(np.uint32), d_rgb.cpu().numpy().reshape(-1, 3).view(np.uint32))
            same = same and np.array_equal(host_points(mode, True).view(np.uint32), fb.view(np.uint32))
        row["same_bits_as_rays_and_frame"] = bool(same)
        calls = [("points_mode0", lambda: points(0)), ("rays_mode0", lambda: rays(0)), ("points_mode2", lambda: points(2)), ("rays_mode2", lambda: rays(2)),
                 ("points_mode3", lambda: points(3))]
        kernel, wall = {k: [] for k, _ in calls}, {k: [] for k, _ in calls}
        for rep in range(args.repeats + 1):  # (round 0: the warm-up)
            for key, call in calls:  # alternated: every round runs each kernel once
                t0 = time.perf_counter()
                call()
                ms = (time.perf_counter() - t0) * 1e3
                if rep:
                    wall[key].append(ms)
                    kernel[key].append(R.Ray_Query_Time())
        for key, _ in calls:
            row[key] = {"kernel": med(kernel[key]), "end_to_end": med(wall[key])}
        hw = {m: [] for m in (0, 2, 3)}
        for rep in range(args.repeats + 1):
            for m in hw:
                t0 = time.perf_counter()
                host_points(m)
                if rep:
                    hw[m].append((time.perf_counter() - t0) * 1e3)
        row["host_arrays_end_to_end"] = {"mode%d" % m: med(v) for m, v in hw.items()}
        row["points_over_rays"] = {"mode0": round(row["points_mode0"]["kernel"]["ms"] / row["rays_mode0"]["kernel"]["ms"], 3),
                                   "mode2": round(row["points_mode2"]["kernel"]["ms"] / row["rays_mode2"]["kernel"]["ms"], 3),
                                   "mode3_over_points_mode0": round(row["points_mode3"]["kernel"]["ms"] / row["points_mode0"]["kernel"]["ms"], 3)}
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        R.Destroy()
    line = json.dumps({"metric": "shade_points_%dx%d" % (W, H), "unit": "ms", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
                       "results": results, "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
