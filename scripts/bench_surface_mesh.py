#!/usr/bin/env python3
"""Times the surface mesher (Surface_Mesh_Device: mdh_surface_mesh_device) on one MI355X.  Run by hand; bench.py does not call
it and there is no threshold.

Per workload -- the headline room over the whole scene and over (Sphere, Box), examples.obj_mesh behind its partition, at
64^3 and 128^3 cells -- three calls alternate in one process, --repeats rounds behind one warm-up round, each timed between
two HIP events on the query stream (OPT_TIMING, Ray_Query_Time):

  * contacts   Contacts_Device over the grid's corner points passed as an array, radius = the level: THE YARDSTICK, the
               kernel the field kernel has to match (it reads no point array);
  * field      the pure count: the field kernel, the count and the scan;
  * mesh       the whole call: those, the vertices with index and normal, and the quads.

The whole call is reported as a multiple of the yardstick with the spread over the rounds.

    python scripts/bench_surface_mesh.py [--repeats 7] [--out profiles/r25_surface_mesh.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import bench_ray_queries as brq  # noqa: E402


def corner_points(origin, h, cells):
    """the grid's corners as the kernel computes them, x fastest"""
    f = np.float32
    axes = [(f(origin[c]) + (np.arange(cells[c] + 1).astype(f) * f(h)).astype(f)).astype(f) for c in range(3)]
    Z, Y, X = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack((X.ravel(), Y.ravel(), Z.ravel()), axis=1))


def workload(R, torch, origin, h, cells, iso, prims, repeats):
    n = int(np.prod(np.asarray(cells) + 1))
    pts = torch.from_numpy(corner_points(origin, h, cells)).cuda()
    rad = torch.full((n,), float(iso), dtype=torch.float32, device="cuda")
    dist = torch.zeros(n, dtype=torch.float32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    R.Surface_Mesh_Device(origin, h, cells, counts, iso, prims)
    R.Ray_Query_Wait()
    nv, nq = (int(x) for x in counts.cpu().numpy())
    pos, nrm = torch.zeros(3 * max(nv, 1), dtype=torch.float32, device="cuda"), torch.zeros(3 * max(nv, 1), dtype=torch.float32, device="cuda")
    idx, quads = torch.zeros(max(nv, 1), dtype=torch.int32, device="cuda"), torch.zeros(4 * max(nq, 1), dtype=torch.int32, device="cuda")
    calls = {"contacts": lambda: R.Contacts_Device(pts, dist, rad, prims),
             "field": lambda: R.Surface_Mesh_Device(origin, h, cells, counts, iso, prims),
             "mesh": lambda: R.Surface_Mesh_Device(origin, h, cells, counts, iso, prims, max(nv, 1), max(nq, 1), pos, nrm, idx, quads)}
    ms = {k: [] for k in calls}
    for turn in range(repeats + 1):
        for k, call in calls.items():
            call()
            R.Ray_Query_Wait()
            if turn:
                ms[k].append(R.Ray_Query_Time())
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = [m / c for m, c in zip(ms["mesh"], ms["contacts"])]
    fields = [f / c for f, c in zip(ms["field"], ms["contacts"])]
    return {"corners": n, "vertices": nv, "quads": nq,
            "kernel_ms": {k: round(med[k], 4) for k in calls}, "kernel_ms_spread": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
            "field_count_scan_over_contacts": round(statistics.median(fields), 3), "field_count_scan_over_contacts_range": [round(min(fields), 3), round(max(fields), 3)],
            "mesh_over_contacts": round(statistics.median(ratios), 3), "mesh_over_contacts_range": [round(min(ratios), 3), round(max(ratios), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # (before the library is loaded: INTEGRATION.md section 5)
    if not torch.cuda.is_available():
        sys.exit("bench_surface_mesh.py measures on a GPU: none is visible")
    torch.zeros(1, device="cuda")
    from madarch_amd import _binding as B
    from madarch_amd.primitives import boxes, spheres
    results = []
    for name, build, _, (lo, hi) in list(brq.scenes(64, 64))[:2]:  # the headline room, obj_mesh behind its partition
        R = build()
        R.Set_Option(B.OPT_TIMING, 1)
        room = name.startswith("global_illumination")
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        if room:
            lo[2] = hi[2] - (hi - lo).min()  # (a cube of cells: the room's half with the sphere and the box in it)
        for cells in (64, 128):
            h = float((hi - lo).min() / cells)
            for what, prims, iso in (("whole scene", None, 0.1),) + ((("(Sphere, Box)", (spheres.Sphere, boxes.Box), 0.0),) if room else ()):
                row = {"scene": name, "kinds": what, "cells": cells, "spacing": round(h, 5), "level": iso, "table_residency": R.Get_Option(B.OPT_TABLE_RESIDENCY)}
                row.update(workload(R, torch, tuple(float(x) for x in lo), h, (cells,) * 3, iso, prims, args.repeats))
                results.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        R.Destroy()
    line = json.dumps({"metric": "surface_mesh", "unit": "ms", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "results": results,
                       "version": (B.hip_binding().version() or b"").decode()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
