#!/usr/bin/env python3
"""Times the batched ray queries (Raycast, Raycast_Visibility, Softshadows) on one MI355X.  Run by hand; bench.py does not
call it and there is no threshold.

Scenes: global_illumination with config 3's probes (bench.py's headline scene), and examples.obj_mesh behind its partition
and with the triangle BVH instead.  Rays, 1920 x 1080 of each: the frame's camera rays, generated on the host as
camera_ray (mdh_device.h) does -- a wavefront's 64 rays are neighbours in a row -- and as many seeded incoherent rays
(origins in the scene's bounds, directions uniform on the sphere).

Per scene, ray set and query: Mrays/s end to end (host clock around the call: the host's check of the rays, both copies
and the kernel) and the kernel's own time between two HIP events on the query stream (OPT_TIMING, Ray_Query_Time); the
median and the spread over --repeats calls behind one warm-up call.  For orientation the scene's mode-2 screen pass at the
same size by mdh_pass_time: it runs the same primary march plus shading, in kernels this feature leaves as they were.
--resources FILE adds the registers and wavefronts per SIMD of every k_ray_query instantiation from a saved output of
madarch_amd/csrc/resource_usage.sh (the script compiles the library for minutes: run it where no GPU waits).

    python scripts/bench_ray_queries.py [--width 1920 --height 1080] [--repeats 7] [--resources FILE] [--out FILE]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x4D414441


def camera_rays(W, H, position, orientation=np.eye(3, dtype=np.float32)):
    """camera_ray (mdh_device.h; draw_screen.glsl:20-24) for every pixel centre, row 0 = top, in float32"""
    u = ((2 * np.arange(W) + 1).astype(np.float32) / np.float32(W) - np.float32(1.0))
    v = -((2 * np.arange(H) + 1).astype(np.float32) / np.float32(H) - np.float32(1.0))
    frag = np.zeros((H, W, 3), np.float32)
    frag[..., 0], frag[..., 1] = u[None, :], v[:, None]
    d = frag - np.array([0.0, 0.0, -1.5], np.float32)
    d = d / np.sqrt((d * d).sum(axis=-1, keepdims=True, dtype=np.float32))
    m = np.asarray(orientation, np.float32)
    org = frag.reshape(-1, 3) @ m.T + np.asarray(position, np.float32)
    return np.ascontiguousarray(org, np.float32), np.ascontiguousarray(d.reshape(-1, 3) @ m.T, np.float32)


def incoherent_rays(n, lo, hi, seed):
    rng = np.random.RandomState(seed & 0x7FFFFFFF)
    org = (np.asarray(lo) + (np.asarray(hi) - np.asarray(lo)) * rng.rand(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    return org, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def scenes(W, H):
    from madarch_amd import examples
    yield ("global_illumination_ddgi8x8x8", lambda: examples.global_illumination(W, H, Probes=examples.GI_8X8X8_PROBES),
           (2.0, 2.0, 0.0), ((-0.9, -0.9, -5.9), (6.9, 6.9, 6.9)))
    yield ("obj_mesh_partition", lambda: examples.obj_mesh(W, H), (0.0, 1.0, -5.0), ((0.0, 0.0, 0.0), (3.0, 2.0, 2.0)))
    yield ("obj_mesh_triangle_bvh", lambda: examples.obj_mesh(W, H, Triangle_BVH=True), (0.0, 1.0, -5.0), ((0.0, 0.0, 0.0), (3.0, 2.0, 2.0)))


def timed(R, call, repeats, n):
    call()  # warm-up: the code object, the batch's device buffer
    wall, kernel = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
        kernel.append(R.Ray_Query_Time())
    w, k = statistics.median(wall), statistics.median(kernel)
    return {"mrays_per_s_end_to_end": round(n / w / 1e6, 2), "ms_end_to_end": round(w * 1e3, 3), "ms_end_to_end_spread": round((max(wall) - min(wall)) * 1e3, 3),
            "kernel_ms": round(k, 4), "kernel_ms_spread": round(max(kernel) - min(kernel), 4), "mrays_per_s_kernel": round(n / (k * 1e-3) / 1e6, 2) if k > 0 else None}


def screen_mode2_ms(R, frames=8):
    """the scene's mode-2 screen pass (direct light and occlusion behind the same primary march), serial frames, HIP events"""
    from madarch_amd import _binding as B
    R.Set_Option(B.OPT_SCREEN_MODE, 2)
    R.Set_Option(B.OPT_FRAME_OVERLAP, 0)
    R.Set_Option(B.OPT_TIMING, 1)
    for _ in range(2):
        R.Render()
    R.Finish()
    R.Reset_Pass_Times()
    for _ in range(frames):
        R.Render()
        R.Finish()
    ms, k = R.Pass_Time(B.PASS_SCREEN)
    return round(ms / k, 4) if k else None


def resources(path):
    rows = {}
    for line in open(path):
        m = re.match(r"\S*k_ray_queryILi(\d+)ELi(\d+)E\S*\s+VGPR\s+(\d+)\s+AGPR\s+\d+\s+SGPR\s+(\d+)\s+scratch\s+(\d+)\s+occ\s+(\d+)", line)
        if m:
            pf, what, vgpr, sgpr, scratch, occ = map(int, m.groups())
            rows["k_ray_query<%d, %s>" % (pf, ("raycast", "visibility", "softshadow")[what])] = {"vgpr": vgpr, "sgpr": sgpr, "scratch_bytes_per_lane": scratch, "waves_per_simd": occ}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--resources", default=None, help="a saved output of madarch_amd/csrc/resource_usage.sh")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ray_queries.py measures on a GPU: none is visible")
    from madarch_amd import _binding as B
    W, H = args.width, args.height
    n = W * H
    results = []
    for name, build, cam, (lo, hi) in scenes(W, H):
        R = build()
        R.Set_Option(B.OPT_TIMING, 1)
        max_dist = np.float32(R.Scene.Max_Dist)
        tmax = np.full(n, np.float32(0.5) * max_dist, np.float32)
        for rays, (org, drs) in (("camera", camera_rays(W, H, cam)), ("incoherent", incoherent_rays(n, lo, hi, SEED))):
            hits = R.Raycast(org, drs)
            row = {"scene": name, "rays": rays, "n": n, "hit_share": round(float(hits["hit"].mean()), 4), "mean_steps": round(float(hits["steps"].mean()), 2),
                   "max_steps": int(hits["steps"].max()), "table_residency": R.Get_Option(B.OPT_TABLE_RESIDENCY), "triangle_bvh": R.Get_Option(B.OPT_TRIANGLE_BVH),
                   "raycast": timed(R, lambda: R.Raycast(org, drs), args.repeats, n),
                   "raycast_visibility": timed(R, lambda: R.Raycast_Visibility(org, drs, tmax), args.repeats, n),
                   "softshadows_k64": timed(R, lambda: R.Softshadows(org, drs, 0.25, tmax, 64.0), args.repeats, n)}
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        results.append({"scene": name, "screen_pass_mode2_ms": screen_mode2_ms(R), "width": W, "height": H})
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)
        R.Destroy()
    line = json.dumps({"metric": "ray_queries_%dx%d" % (W, H), "unit": "Mrays/s", "device": torch.cuda.get_device_name(0), "results": results,
                       "resources": resources(args.resources) if args.resources else None, "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
