"""How many 8x8 tiles of a frame can share their cage irradiance taps (MDH_SHARE_TAPS, mdh_march.h)?  A CPU estimate.

The screen pass gives a wavefront one 8x8 tile.  At the first shaded point the wavefront fetches its eight irradiance taps once
when every lane that hit holds the same cage cell and the same bits of the normal, and at least 8 lanes hit.  This script
renders the frame of one of bench.py's workloads with the CPU oracle and the geometry buffer on, derives every pixel's hit
point P = origin + dir * t from the camera model of camera_ray (mdh_device.h) in float32 and its cage cell
gp = floor (P / spacing), and counts the tiles whose hit pixels name ONE primitive and ONE cell -- per primitive, since the
primitive decides the normal: a plane's is uniform, a box's unless the tile spans two faces, a sphere's never.

    python scripts/tile_uniformity.py [--workload global_illumination_1080p_ddgi8x8x8]

(numpy and the oracle only; no GPU.  The camera is where the examples put it: at (2, 2, 0), looking along +z.)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402
from oracle_engine import oracle_binding  # noqa: E402

F = np.float32
CAMERA = np.array([2.0, 2.0, 0.0], np.float32)  # examples.py: Set_Camera_Position ((2, 2, 0)), identity orientation
NORMAL_OF = {"Plane": "uniform", "Box": "uniform unless the tile spans two faces", "Sphere": "not uniform"}


def hit_points(W, H, t):
    """camera_ray and the hit point, float32 operation for operation (draw_screen.glsl:21-24)"""
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    u = ((2 * i + 1).astype(F) / F(W) - F(1.0)).astype(F)
    v = (-((2 * j + 1).astype(F) / F(H) - F(1.0))).astype(F)
    d = np.stack([u, v, np.full_like(u, F(1.5))], axis=-1)  # frag - (0, 0, -1.5)
    d = (d / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]).astype(F)
    origin = np.stack([u, v, np.zeros_like(u)], axis=-1) + CAMERA
    return (origin + d * t[..., None].astype(F)).astype(F)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", default="global_illumination_1080p_ddgi8x8x8", choices=sorted(w for w, v in bench.WORKLOADS.items() if v[0] != "ball_game"))
    args = ap.parse_args()
    R = bench.make_renderer(args.workload, oracle_binding())
    R.Set_Option(B.OPT_GBUFFER, 1)
    R.Render()
    index, t, _ = R.Read_Gbuffer()
    W, H = R.Width, R.Height
    spacing = np.array(R.Probes.Grid_Spacing, np.float32)
    names, at = {}, 0
    for prim, count in R.Scene.Prims_Count:  # the geometry buffer numbers primitives kind after kind, by declared count
        for k in range(count):
            names[at + k] = "%s %d" % (prim.name, k + 1)
        at += count
    R.Destroy()
    hit = index >= 0
    gp = np.floor(hit_points(W, H, t) / spacing).astype(np.int64)
    cell = (gp[..., 0] + 64) + 1024 * (gp[..., 1] + 64) + 1024 * 1024 * (gp[..., 2] + 64)
    ty, tx = (H + 7) // 8, (W + 7) // 8
    pad = lambda a, fill: np.pad(a, ((0, ty * 8 - H), (0, tx * 8 - W)), constant_values=fill)
    tiles = lambda a: a.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64)
    hit_t, index_t, cell_t = tiles(pad(hit, False)), tiles(pad(index, -1)), tiles(pad(cell, -1))
    n_hit = hit_t.sum(axis=1)
    big = np.iinfo(np.int64).max
    lo = lambda a: np.where(hit_t, a, big).min(axis=1)
    hi = lambda a: np.where(hit_t, a, -big).max(axis=1)
    one_prim, one_cell = lo(index_t) == hi(index_t), lo(cell_t) == hi(cell_t)
    shares = (n_hit >= 8) & one_prim & one_cell
    n = ty * tx
    print("%s: %d x %d pixels, %d tiles of 8x8 (one wavefront each), cage cells of %s" % (args.workload, W, H, n, tuple(float(s) for s in spacing)))
    print("tiles with a hit pixel                          %6d  %5.1f %%" % ((n_hit > 0).sum(), 100.0 * (n_hit > 0).sum() / n))
    print("... with at least 8                             %6d  %5.1f %%" % ((n_hit >= 8).sum(), 100.0 * (n_hit >= 8).sum() / n))
    print("... that hit ONE primitive                      %6d  %5.1f %%" % (((n_hit >= 8) & one_prim).sum(), 100.0 * ((n_hit >= 8) & one_prim).sum() / n))
    print("... in ONE cage cell                            %6d  %5.1f %%" % (shares.sum(), 100.0 * shares.sum() / n))
    print("by first primitive (the normal of its tiles):")
    by_kind = {}
    first = lo(index_t)
    for p in sorted(set(first[shares].tolist())):
        k = int((shares & (first == p)).sum())
        kind = names[p].split()[0]
        by_kind[kind] = by_kind.get(kind, 0) + k
        print("  %-12s %6d  %5.1f %%  %s" % (names[p], k, 100.0 * k / n, NORMAL_OF.get(kind, "?")))
    sure, maybe = by_kind.get("Plane", 0), by_kind.get("Plane", 0) + by_kind.get("Box", 0)
    print("wavefronts that share their taps at the first point: between %d (%.1f %%, planes) and %d (%.1f %%, with every box tile)" % (
        sure, 100.0 * sure / n, maybe, 100.0 * maybe / n))


if __name__ == "__main__":
    main()
