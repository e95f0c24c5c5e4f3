#!/usr/bin/env python3
"""Times Shade_Rays and Shade_Rays_Device (k_ray_shade: the frame's pixel program in a general kernel, one ray per lane,
64 consecutive rays per wavefront) against the screen pass of the same pixels on one MI355X.  Run by hand; bench.py does not
call it and there is no threshold.

Per scene (the headline scene, global_illumination with config 3's probes, and examples.obj_mesh behind its partition) and
mode (0, 2), over the width x height rays of Camera_Rays:
  - the kernel's time (OPT_TIMING, two events on the query stream), median of --repeats calls behind a warm-up, and the spread;
  - end to end on the host's clock: the host-array call, and the device-array call followed by Ray_Query_Wait with its
    arrays already on the device;
  - beside them the scene's screen pass at the same size and in the same mode by Pass_Time, serial frames: for mode 0 of the
    rooms that is the census kernel over 8 x 8 tiles.
Before anything is timed the tone-mapped answers are compared with the framebuffer of a screen pass over the same atlases,
bit for bit.

    python scripts/bench_shade_rays.py [--width 1920 --height 1080] [--repeats 5] [--scenes a,b] [--out FILE]
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


def screen_pass_ms(R, B, frames=8):
    """the screen pass alone over the atlases as they stand (Render_Pass: no probe pass moves them), HIP events"""
    R.Finish()
    R.Reset_Pass_Times()
    for _ in range(frames):
        R.Render_Pass(B.PASS_SCREEN)
        R.Finish()
    ms, k = R.Pass_Time(B.PASS_SCREEN)
    return round(ms / k, 4) if k else None


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
        sys.exit("bench_shade_rays.py measures on a GPU: none is visible")
    torch.zeros(1, device="cuda")
    import bench_ray_queries as brq
    from madarch_amd import _binding as B
    W, H = args.width, args.height
    n = W * H
    results = []
    for name, build, _cam, _box in brq.scenes(W, H):
        if name not in args.scenes.split(","):
            continue
        for mode in (0, 2):
            R = build()
            R.Set_Option(B.OPT_SCREEN_MODE, mode)
            R.Set_Option(B.OPT_FRAME_OVERLAP, 0)
            R.Set_Option(B.OPT_SCREEN_REPLAY, 0)  # (the pass that marches: what the query's kernel does too)
            R.Set_Option(B.OPT_TIMING, 1)
            for _ in range(4):  # the probes hold light
                R.Render()
            R.Finish()
            org, drs = R.Camera_Rays(W, H)
            d_org, d_dir = torch.empty(3 * n, device="cuda"), torch.empty(3 * n, device="cuda")
            R.Camera_Rays_Device(W, H, d_org, d_dir)
            d_rgb = torch.empty(3 * n, device="cuda")
            d_int = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
            d_t = torch.empty(n, device="cuda")
            host_call = lambda: R.Shade_Rays(org, drs, Mode=mode, Tone_Map=True)  # noqa: E731

            def device_call():
                R.Shade_Rays_Device(d_org, d_dir, d_rgb, d_int[0], d_int[1], d_t, d_int[2], Mode=mode, Tone_Map=True)
                R.Ray_Query_Wait()
            row = {"scene": name, "mode": mode, "n": n}
            R.Render_Pass(B.PASS_SCREEN)
            fb = R.Read_Framebuffer().reshape(-1, 3)
            want = host_call()  # (the warm-up)
            device_call()
            row["same_bits_as_frame"] = bool(np.array_equal(want["rgb"].view(np.uint32), fb.view(np.uint32)) and
                                             np.array_equal(d_rgb.cpu().numpy().view(np.uint32).reshape(-1, 3), fb.view(np.uint32)))
            row["hit_share"], row["mean_steps"], row["max_steps"] = round(float(want["hit"].mean()), 4), round(float(want["steps"].mean()), 2), int(want["steps"].max())
            kernel, wall = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                host_call()
                wall.append((time.perf_counter() - t0) * 1e3)
                kernel.append(R.Ray_Query_Time())
            row["host_kernel"], row["host_end_to_end"] = med(kernel), med(wall)
            kernel, wall = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                device_call()
                wall.append((time.perf_counter() - t0) * 1e3)
                kernel.append(R.Ray_Query_Time())
            row["device_kernel"], row["device_end_to_end"] = med(kernel), med(wall)
            row["screen_pass_ms"] = screen_pass_ms(R, B)
            row["kernel_over_screen_pass"] = round(row["device_kernel"]["ms"] / row["screen_pass_ms"], 3) if row["screen_pass_ms"] else None
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            R.Destroy()
    line = json.dumps({"metric": "shade_rays_%dx%d" % (W, H), "unit": "ms", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
                       "results": results, "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
