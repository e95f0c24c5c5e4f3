#!/usr/bin/env python3
"""Times Path_Trace_Device (k_path_trace: one ray per lane, a flat loop over the segments of the lane's paths) on one MI355X.
Run by hand; bench.py does not call it and there is no threshold.

Per scene (the headline scene, global_illumination with config 3's probes, and examples.obj_mesh behind its partition), over
the width x height rays of Camera_Rays with --bounces bounces, in slices of 1 and 16 samples:
  - the kernel's time (OPT_TIMING, two events on the query stream: Ray_Query_Time), median of --repeats calls behind a
    warm-up, and the spread;
  - paths per second (rays x samples / kernel time) and segments per second, with the mean number of segments of a path
    counted on the host for sample 0 of every 64th ray (--segments-every): Raycast, Primitive_Material and Path_Scatter chained as the kernel
    chains them.
With MADARCH_HIP_LIBRARY naming a build made with EXTRA=-DMDH_PATH_LOCKSTEP=1 the same script times the kernel whose
wavefronts wait for their slowest path before the next sample: the difference is what the flat loop buys.
--view N,M: the mean absolute difference between examples.path_traced_view's two linear images of the room at N and M samples.

    python scripts/bench_path_trace.py [--width 1920 --height 1080] [--bounces 3] [--repeats 5] [--scenes a,b] [--view 64,1024] [--out FILE]
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


def roughness_log(renderers, materials):
    """{material id: roughness} as the scene builders hand the materials over"""
    table = {}
    set_m, add_m = renderers.Renderer.Set_Material, renderers.Renderer.Add_Material

    def set_material(self, index, e):
        table[int(index)] = np.float32(e.Get(materials.Roughness).data)
        return set_m(self, index, e)

    def add_material(self, e):
        i = add_m(self, e)
        table[int(i)] = np.float32(e.Get(materials.Roughness).data)
        return i
    renderers.Renderer.Set_Material, renderers.Renderer.Add_Material = set_material, add_material
    return table


def mean_segments(R, table, org, drs, seed, bounces, every=64):
    """segments per path of sample 0 over every `every`-th ray, chained on the host as the kernel chains them"""
    rows = np.arange(0, len(org), every)
    O, D = np.ascontiguousarray(org[rows]), np.ascontiguousarray(drs[rows])
    segments = 0
    for b in range(bounces + 1):
        if not len(rows):
            break
        segments += len(rows)
        rc = R.Raycast(O, D)
        hit = rc["hit"] == 1
        if b == bounces or not hit.any():
            break
        rows, D = rows[hit], np.ascontiguousarray(D[hit])
        P, N = rc["position"][hit], np.ascontiguousarray(rc["normal"][hit])
        mat = R.Primitive_Material(rc["index"][hit])
        rough = np.array([table.get(int(m), np.float32(1.0)) for m in mat], np.float32)
        nd = np.zeros_like(D)
        for q in range(len(rows)):  # (ids are no longer consecutive)
            nd[q] = R.Path_Scatter(D[q:q + 1], N[q:q + 1], rough[q:q + 1], Seed=seed, Id_First=int(rows[q]), Sample=0, Bounce=b)[0]
        ok = np.isfinite(nd).all(axis=1)
        O = np.ascontiguousarray((P + (N * np.float32(0.05)) * np.float32(5.0))[ok])
        rows, D = rows[ok], np.ascontiguousarray(nd[ok])
    return segments / float(len(np.arange(0, len(org), every)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slices", default="1,16")
    ap.add_argument("--scenes", default="global_illumination_ddgi8x8x8,obj_mesh_partition")
    ap.add_argument("--view", default="")
    ap.add_argument("--segments-every", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # before the library is loaded
    if not torch.cuda.is_available():
        sys.exit("bench_path_trace.py measures on a GPU: none is visible")
    torch.zeros(1, device="cuda")
    import bench_ray_queries as brq
    from madarch_amd import _binding as B
    from madarch_amd import examples, materials, renderers
    table = roughness_log(renderers, materials)
    W, H = args.width, args.height
    n = W * H
    results = []
    for name, build, _cam, _box in brq.scenes(W, H):
        if name not in args.scenes.split(","):
            continue
        table.clear()
        R = build()
        R.Set_Option(B.OPT_TIMING, 1)
        org, drs = R.Camera_Rays(W, H)
        d_org, d_dir = torch.empty(3 * n, device="cuda"), torch.empty(3 * n, device="cuda")
        R.Camera_Rays_Device(W, H, d_org, d_dir)
        d_rgb = torch.zeros(3 * n, device="cuda")
        d_hit = torch.empty(n, dtype=torch.int32, device="cuda")
        seg = mean_segments(R, table, org, drs, args.seed, args.bounces, args.segments_every) if args.segments_every > 0 else None
        for count in [int(s) for s in args.slices.split(",")]:
            def call(first):
                R.Path_Trace_Device(d_org, d_dir, d_rgb, d_hit, Seed=args.seed, Sample_First=first, Sample_Count=count, Bounces=args.bounces)
                R.Ray_Query_Wait()
                return R.Ray_Query_Time()
            call(0)  # the warm-up
            kernel = [call((k + 1) * count) for k in range(args.repeats)]
            m = med(kernel)
            row = {"scene": name, "n": n, "bounces": args.bounces, "samples_per_call": count, "kernel": m, "hit_share": round(float(d_hit.float().mean()), 4),
                   "paths_per_s": round(n * count / (m["ms"] * 1e-3), 1), "mean_segments_per_path": None if seg is None else round(seg, 4),
                   "segments_per_s": None if seg is None else round(seg * n * count / (m["ms"] * 1e-3), 1)}
            results.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        R.Destroy()
    view = []
    for samples in [int(s) for s in args.view.split(",") if s]:
        R = examples.global_illumination(256, 256)
        for _ in range(16):
            R.Render()
        _, _, traced, frame = examples.path_traced_view(R, 256, 256, Samples=samples, Bounces=args.bounces, Seed=args.seed)
        hit = R.Raycast(*R.Camera_Rays(256, 256))["hit"].reshape(256, 256) == 1
        row = {"samples": samples, "bounces": args.bounces, "hit_pixels": int(hit.sum()),
               "mean_abs_difference_rgb": [round(float(np.abs(traced[hit] - frame[hit])[:, c].mean()), 6) for c in range(3)]}
        view.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        R.Destroy()
    line = json.dumps({"metric": "path_trace_%dx%d" % (W, H), "unit": "ms", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
                       "library": os.path.basename(B.HIP_LIBRARY), "results": results, "view_room_256x256": view,
                       "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
