#!/usr/bin/env python3
"""Times the device-array ray queries (Raycast_Device, Raycast_Visibility_Device, Softshadows_Device: k_ray_stream, whose
lanes take the next ray when their own has ended) against the host-array ones (k_ray_query) on one MI355X.  Run by hand;
bench.py does not call it and there is no threshold.

The batches are those of scripts/bench_ray_queries.py: the camera rays and as many seeded incoherent rays of
global_illumination (config 3's probes) and of examples.obj_mesh behind its partition and with the triangle BVH, 1920 x
1080 rays each.  Per batch and query:
  - the kernel's time of the host-array call (OPT_TIMING, two events on the query stream), median of --repeats calls behind
    a warm-up, and the spread (max - min);
  - the same of the device call at MDH_OPT_RAY_STREAM_REFILL = 64 (lock step), 48, 32, 16, 8 and 1;
  - end to end on the host's clock: the host-array call against the device call followed by Ray_Query_Wait, its arrays
    already on the device (at the renderer's default threshold).
The answers of the device call at every threshold are compared with the host-array call's, bit for bit, before they are timed.

    python scripts/bench_ray_streams.py [--width 1920 --height 1080] [--repeats 5] [--scenes a,b] [--out FILE]
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

REFILLS = (64, 48, 32, 16, 8, 1)


def med(xs):
    return {"ms": round(statistics.median(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", default=None, help="comma-separated names of bench_ray_queries.scenes (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # before the library is loaded
    if not torch.cuda.is_available():
        sys.exit("bench_ray_streams.py measures on a GPU: none is visible")
    torch.zeros(1, device="cuda")
    import bench_ray_queries as brq
    from madarch_amd import _binding as B
    W, H = args.width, args.height
    n = W * H
    results = []
    for name, build, cam, (lo, hi) in brq.scenes(W, H):
        if args.scenes and name not in args.scenes.split(","):
            continue
        R = build()
        R.Set_Option(B.OPT_TIMING, 1)
        default_refill = R.Get_Option(B.OPT_RAY_STREAM_REFILL)
        tmax = np.full(n, np.float32(0.5) * np.float32(R.Scene.Max_Dist), np.float32)
        d_tmax = torch.from_numpy(tmax).cuda()
        for rays, (org, drs) in (("camera", brq.camera_rays(W, H, cam)), ("incoherent", brq.incoherent_rays(n, lo, hi, brq.SEED))):
            d_org, d_dir = torch.from_numpy(org).cuda(), torch.from_numpy(drs).cuda()
            out_i = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in ("hit", "index", "steps")}
            out_f = {"t": torch.empty(n, device="cuda"), "position": torch.empty(3 * n, device="cuda"), "normal": torch.empty(3 * n, device="cuda")}
            out_s = torch.empty(n, device="cuda")
            queries = {
                "raycast": (lambda: R.Raycast(org, drs),
                            lambda: R.Raycast_Device(d_org, d_dir, out_i["hit"], out_i["index"], out_f["t"], out_i["steps"], out_f["position"], out_f["normal"]),
                            lambda want: all(np.array_equal(out_i[k].cpu().numpy(), want[k]) for k in out_i) and
                            all(np.array_equal(out_f[k].cpu().numpy().reshape(want[k].shape), want[k]) for k in out_f)),
                "raycast_visibility": (lambda: R.Raycast_Visibility(org, drs, tmax), lambda: R.Raycast_Visibility_Device(d_org, d_dir, d_tmax, out_s),
                                       lambda want: np.array_equal(out_s.cpu().numpy(), want)),
                "softshadows_k64": (lambda: R.Softshadows(org, drs, 0.25, tmax, 64.0), lambda: R.Softshadows_Device(d_org, d_dir, 0.25, d_tmax, 64.0, out_s),
                                    lambda want: np.array_equal(out_s.cpu().numpy(), want, equal_nan=True)),
            }
            row = {"scene": name, "rays": rays, "n": n}
            for qname, (host_call, device_call, same) in queries.items():
                want = host_call()  # (the warm-up)
                if qname == "raycast":
                    row["mean_steps"], row["max_steps"] = round(float(want["steps"].mean()), 2), int(want["steps"].max())
                kernel, wall = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    host_call()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    kernel.append(R.Ray_Query_Time())
                q = {"host_kernel": med(kernel), "host_end_to_end": med(wall), "device_kernel": {}, "same_bits": True}
                for refill in REFILLS:
                    R.Set_Option(B.OPT_RAY_STREAM_REFILL, refill)
                    device_call()  # (the warm-up)
                    R.Ray_Query_Wait()
                    q["same_bits"] = bool(q["same_bits"] and same(want))
                    kernel = []
                    for _ in range(args.repeats):
                        device_call()
                        R.Ray_Query_Wait()
                        kernel.append(R.Ray_Query_Time())
                    q["device_kernel"][str(refill)] = med(kernel)
                R.Set_Option(B.OPT_RAY_STREAM_REFILL, default_refill)
                device_call()
                R.Ray_Query_Wait()
                wall = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    device_call()
                    R.Ray_Query_Wait()
                    wall.append((time.perf_counter() - t0) * 1e3)
                q["device_end_to_end"] = med(wall)
                row[qname] = q
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        R.Destroy()
    line = json.dumps({"metric": "ray_streams_%dx%d" % (W, H), "unit": "ms", "device": torch.cuda.get_device_name(0), "refills": list(REFILLS),
                       "default_refill": default_refill if results else None, "repeats": args.repeats, "results": results,
                       "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
