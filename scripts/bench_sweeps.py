#!/usr/bin/env python3
"""Times the swept-sphere casts and the contact queries (Spherecast, Contacts and their _Device forms) on one MI355X.  Run
by hand; bench.py does not call it and there is no threshold.

The protocol is scripts/bench_ray_queries.py's, whose scenes, rays and clock this script imports: per workload the median
and the spread of --repeats calls behind one warm-up call, end to end by the host's clock and the kernel alone between two
HIP events on the query stream (OPT_TIMING, Ray_Query_Time).

  * the headline room's camera rays and incoherent rays, swept over the whole scene at radius 0, 0.05 and 0.3 -- beside
    Raycast and Raycast_Visibility over the same rays, alternated call by call in one process: the sweep at radius 0 does
    raycast's work (a hit's index, position and normal) in the visibility query's marching form (no arg-min in the march);
  * the listed (Plane, Box) sweep and the contacts, whole scene and listed;
  * examples.obj_mesh behind its partition;
  * the device-array forms at MDH_OPT_RAY_STREAM_REFILL 64 and 16 (torch tensors; the kernel's time alone).

    python scripts/bench_sweeps.py [--width 1920 --height 1080] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import bench_ray_queries as brq  # noqa: E402

RADII = (0.0, 0.05, 0.3)


def alternated(R, calls, repeats, n):
    """name -> call, run in turns (one warm-up turn first): every workload meets the same clocks -> name -> figures"""
    for call in calls.values():
        call()
    wall, kernel = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(repeats):
        for k, call in calls.items():
            t0 = time.perf_counter()
            call()
            wall[k].append(time.perf_counter() - t0)
            kernel[k].append(R.Ray_Query_Time())
    out = {}
    for k in calls:
        w, ms = statistics.median(wall[k]), statistics.median(kernel[k])
        out[k] = {"ms_end_to_end": round(w * 1e3, 3), "ms_end_to_end_spread": round((max(wall[k]) - min(wall[k])) * 1e3, 3), "kernel_ms": round(ms, 4),
                  "kernel_ms_spread": round(max(kernel[k]) - min(kernel[k]), 4), "mrays_per_s_kernel": round(n / (ms * 1e-3) / 1e6, 2) if ms > 0 else None}
    return out


def device_forms(R, torch, B, org, drs, kinds, repeats, n):
    """the device-array forms: nothing is copied, so the kernel's time is the call's"""
    d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(drs).cuda()
    d_rad = torch.full((n,), 0.05, dtype=torch.float32, device="cuda")
    hit, dist = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
    index, t = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
    out = {}
    for refill in (64, 16):
        R.Set_Option(B.OPT_RAY_STREAM_REFILL, refill)

        def waited(call):
            def run():
                call()
                R.Ray_Query_Wait()
            return run
        calls = {"spherecast_device_radius_0.05": waited(lambda: R.Spherecast_Device(d_org, d_dir, hit, d_rad, None, None, index, t)),
                 "spherecast_device_plane_box_radius_0.05": waited(lambda: R.Spherecast_Device(d_org, d_dir, hit, d_rad, None, kinds, index, t)),
                 "contacts_device_radius_0.05": waited(lambda: R.Contacts_Device(d_org, dist, d_rad, None, index))}
        out["refill_%d" % refill] = alternated(R, calls, repeats, n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # (before the library is loaded: INTEGRATION.md section 5)
    if not torch.cuda.is_available():
        sys.exit("bench_sweeps.py measures on a GPU: none is visible")
    torch.zeros(1, device="cuda")
    from madarch_amd import _binding as B
    from madarch_amd.primitives import boxes, planes, triangles
    W, H = args.width, args.height
    n = W * H
    results = []
    for name, build, cam, (lo, hi) in list(brq.scenes(W, H))[:2]:  # the headline room, obj_mesh behind its partition
        R = build()
        R.Set_Option(B.OPT_TIMING, 1)
        room = name.startswith("global_illumination")
        kinds = (planes.Plane, boxes.Box) if room else (triangles.Triangle,)
        tmax = np.full(n, np.float32(0.5) * np.float32(R.Scene.Max_Dist), np.float32)
        for rays, (org, drs) in (("camera", brq.camera_rays(W, H, cam)), ("incoherent", brq.incoherent_rays(n, lo, hi, brq.SEED))):
            calls = {"raycast": lambda: R.Raycast(org, drs), "raycast_visibility": lambda: R.Raycast_Visibility(org, drs, tmax)}
            for r in RADII:
                calls["spherecast_radius_%g" % r] = (lambda r: lambda: R.Spherecast(org, drs, r))(r)
            if room:
                calls["spherecast_plane_box_radius_0.05"] = lambda: R.Spherecast(org, drs, 0.05, None, kinds)
                calls["contacts_plane_box_radius_0.05"] = lambda: R.Contacts(org, 0.05, kinds)
            calls["contacts_radius_0.05"] = lambda: R.Contacts(org, 0.05)
            cast = R.Spherecast(org, drs, 0.05)
            row = {"scene": name, "rays": rays, "n": n, "hit_share_radius_0.05": round(float(cast["hit"].mean()), 4), "mean_steps_radius_0.05": round(float(cast["steps"].mean()), 2),
                   "table_residency": R.Get_Option(B.OPT_TABLE_RESIDENCY), "host_arrays": alternated(R, calls, args.repeats, n)}
            if room:
                row["device_arrays"] = device_forms(R, torch, B, org, drs, kinds, args.repeats, n)
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        R.Destroy()
    line = json.dumps({"metric": "sweeps_%dx%d" % (W, H), "unit": "ms", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "results": results,
                       "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
