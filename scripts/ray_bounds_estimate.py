#!/usr/bin/env python3
"""What ray-constant bounds on the sphere's and the box's distance would save k_screen's marches (MDH_RAY_BOUNDS, DESIGN.md
section 4 item 19): the set-up and the cull restated in numpy on the room model of scripts/vis_clearance.py, float32, the kernel's
operations in the kernel's order (mdh_device.h: ray_bounds, closest_primitive).

march_plain evaluates the SDF at fl(o + fl(d * total)), 0 <= total < tmax.  At every evaluation closest_primitive takes the
planes' minimum, then runs the sphere's cull test and the box's (a square root behind each, skipped when no live lane of the
wavefront needs it).  A lower bound of a solid's distance over the whole segment o + d [0, tmax] is one number per lane for the
whole march:

    hs   |c - p*| - r - E                    p* the segment's point closest to the sphere's centre c
    hb   |q| - sum |q_a| e_a / |q| - E_b     q = c_b - p*_b, the box's support function along q

and where it exceeds the running minimum in every live lane the solid's block is skipped without its own test.

For a sample of 8x8 tiles this script marches every pixel's primary and reflection ray in lock step per tile, live lanes only,
and counts per tile: wave-steps; steps in which today's sphere and box culls fire; steps in which each bound clears every live
lane; the same for one register min(hs, hb) in front of both blocks.  It prices the net in vector instructions per tile with the
static counts of scripts/probes/ray_bounds_probe.hip and as a share of the 185.3 M of one 1080p launch.

    python scripts/ray_bounds_estimate.py [--stride S] [--small]

--small adds the 64x64 cameras of tests/test_gpu_ray_bounds.py."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_first_estimate as BF  # noqa: E402
import vis_clearance as V  # noqa: E402

f32 = np.float32
UNIT_TOL = f32(2.0 ** -18)  # | |d|^2 - 1 | above this: the bounds are off
MARGIN = f32(2.0 ** -14)  # E = (lim + tmax) * MARGIN
# static counts (vector instructions, gfx950, the Makefile's flags): scripts/probes/ray_bounds_probe.hip gives b_base 8, b_sphere 24,
# b_box 25, b_cmp 10, r_base 11, r_setup 94 -- each block carries one v_cndmask of the probe's own select, the compare one v_cmp beside
# it.  The sphere's test 15, the box's 16; priced at the lower 13 and 11 that the blocks cost inside the kernel's step, where the
# subtractions c - x are shared with what follows.  The set-up 83 per march.
COST = dict(sphere_block=13, box_block=11, compare=1, setup=83, launch_valu=185.3e6, tiles=32400)


def ray_bounds(sc, thr, lim, o, d, tmax):
    """ray_bounds (mdh_device.h) in float32: (hs, hb) per ray, NaN where the bounds are off or fail closed (v_med3_f32 is the
    clamp below for 0 <= tmax, and a ray with another tmax is off)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        o = o.astype(f32); d = d.astype(f32); tmax = np.broadcast_to(np.asarray(tmax, f32), o.shape[:1])
        ok = np.full(len(o), bool(thr > 0))
        ok &= np.all(np.abs(o) <= lim, axis=1)
        ok &= np.abs(V.dot(d, d) - f32(1)) <= UNIT_TOL
        ok &= tmax >= 0
        E = ((lim + tmax) * MARGIN).astype(f32)
        s = sc["spheres"][0]
        w = (s[:3] - o).astype(f32)
        t = np.fmin(np.fmax(V.dot(w, d), f32(0)), tmax)
        q = (w - d * t[:, None]).astype(f32)
        hs = ((np.sqrt(V.dot(q, q)) - s[3]) - E).astype(f32)
        b = sc["boxes"][0]
        w = (b[:3] - o).astype(f32)
        t = np.fmin(np.fmax(V.dot(w, d), f32(0)), tmax)
        q = (w - d * t[:, None]).astype(f32)
        q2 = V.dot(q, q)
        rq = (f32(1) / np.sqrt(q2)).astype(f32)  # (the kernel: v_rsq_f32, one ulp)
        aq = np.abs(q)
        sup = (((aq[:, 0] * b[3] + aq[:, 1] * b[4]) + aq[:, 2] * b[5]) * rq).astype(f32)
        se = f32(2) * ((b[3] + b[4]) + b[5])
        hb = ((q2 * rq - sup) - E * (f32(1) + se * rq)).astype(f32)
        off = f32(np.nan)  # (the kernel: all ones)
        return np.where(ok, hs, off).astype(f32), np.where(ok, hb, off).astype(f32)


def sdf_parts(sc, x):
    """closest_primitive (ROOM) at x [n, 3] in float32: the planes' minimum, the sphere's cull test and distance, the box's
    m = max(q) and distance -- the box's own test needs the running minimum, which the caller holds."""
    x = x.astype(f32)
    c = np.full(len(x), sc["max_dist"], f32)
    o = sc["off"]
    for a in range(3):
        c = np.minimum(c, np.minimum(x[:, a] + o[2 * a], -x[:, a] + o[2 * a + 1]))
    s = sc["spheres"][0]
    dv = (s[:3] - x).astype(f32)
    d2 = V.dot(dv, dv)
    ds = (np.sqrt(d2) - s[3]).astype(f32)
    b = sc["boxes"][0]
    q = (np.abs(b[:3] - x) - b[3:]).astype(f32)
    m = np.maximum(q[:, 0], np.maximum(q[:, 1], q[:, 2]))
    qp = np.maximum(q, f32(0))
    db = (np.sqrt(V.dot(qp, qp)) + np.minimum(m, f32(0))).astype(f32)
    return c, d2, ds, m, db


def sphere_need(closest, d2, r):
    """MDH_SPHERE_STEP's `need` (false: this lane lets the root go)."""
    tsum = (closest + r).astype(f32)
    return ~(tsum < 0) & ~(d2 > (tsum * tsum) * f32(1.000001))


def box_need(closest, m):
    thr = np.where(closest > 0, closest * f32(1.000001), closest).astype(f32)
    return ~(m > thr)


def tile_march(sc, o, d, live, hs, hb, tile, nt, check=None):
    """march_plain in lock step per tile.  o, d [n, 3]; live, hs, hb, tile [n] (tile: each ray's wavefront, 0 .. nt - 1).
    Returns (hit, total, counts) -- counts: per tile, wave-steps and the steps in which each cull clears the wavefront.
    check (a list) receives (what, position, closest, float32 distance) wherever a bound skips a block."""
    n = len(o)
    total = np.zeros(n, f32)
    hit = np.zeros(n, bool)
    live = live.copy()
    names = ("steps", "sphere_today", "box_today", "sphere_bound", "box_bound", "box_bound_alone", "one_register", "both_today")
    cnt = {k: np.zeros(nt, np.int64) for k in names}

    def waves(flag, idx):  # per tile: does `flag` hold in EVERY live lane (flag given on the live rays idx)
        bad = np.zeros(nt, np.int64)
        np.add.at(bad, tile[idx], ~flag)
        on = np.zeros(nt, np.int64)
        np.add.at(on, tile[idx], 1)
        return (bad == 0) & (on > 0), on > 0

    with np.errstate(invalid="ignore"):
        while live.any():
            idx = np.nonzero(live)[0]
            x = (o[idx] + d[idx] * total[idx, None]).astype(f32)
            c, d2, ds, m, db = sdf_parts(sc, x)
            r = sc["spheres"][0][3]
            s_clear, on = waves(~sphere_need(c, d2, r), idx)
            cnt["steps"] += on
            cnt["sphere_today"] += s_clear
            sb_lane = hs[idx] > c
            sb_clear, _ = waves(sb_lane, idx)
            cnt["sphere_bound"] += sb_clear
            # the sphere's block runs in the whole wavefront or not at all: today's code and the bound's differ in when, never in
            # what `closest` is behind it (a skipped block would have left it unchanged)
            c1 = np.where(s_clear[tile[idx]], c, np.minimum(c, ds)).astype(f32)
            b_clear, _ = waves(~box_need(c1, m), idx)
            cnt["box_today"] += b_clear
            cnt["both_today"] += s_clear & b_clear
            bb_lane = hb[idx] > c1
            bb_clear, _ = waves(bb_lane, idx)
            cnt["box_bound"] += bb_clear
            cnt["box_bound_alone"] += bb_clear & ~sb_clear
            one_clear, _ = waves((np.minimum(hs[idx], hb[idx]) > c), idx)
            cnt["one_register"] += one_clear
            if check is not None:
                ks = sb_clear[tile[idx]]
                check.append(("sphere", x[ks], c[ks], ds[ks]))
                kb = bb_clear[tile[idx]]
                check.append(("box", x[kb], c1[kb], db[kb]))
            sd = np.minimum(c1, db).astype(f32)
            h = sd < V.EPS
            hit[idx[h]] = True
            total[idx[~h]] = total[idx[~h]] + sd[~h]
            live[idx] = ~h & (total[idx] < sc["max_dist"])
    return hit, total, cnt


def frame(sc, thr, lim, W, H, pos, yaw, pitch, tiles, check=None):
    """Both marches of every pixel of the tiles: per-march counts."""
    o, d, valid = BF.camera_rays(W, H, pos, BF.rotation(yaw, pitch), tiles)
    nt = len(tiles)
    o = o.reshape(-1, 3); d = d.reshape(-1, 3); valid = valid.reshape(-1)
    tile = np.repeat(np.arange(nt), 64)
    hs, hb = ray_bounds(sc, thr, lim, o, d, sc["max_dist"])
    h0, t0, c0 = tile_march(sc, o, d, valid, hs, hb, tile, nt, check)
    P0 = (o + d * t0[:, None]).astype(f32)
    N0 = BF.normals(sc, P0)
    from0 = (P0 + (N0 * V.MIN_STEP) * f32(5)).astype(f32)
    rd = (d - N0 * (f32(2) * V.dot(N0, d))[:, None]).astype(f32)
    hs1, hb1 = ray_bounds(sc, thr, lim, from0, rd, sc["max_dist"])
    h1, t1, c1 = tile_march(sc, from0, rd, valid & h0, hs1, hb1, tile, nt, check)
    return c0, c1


def price(c0, c1):
    """Net vector instructions per tile of the two-ballot form, of each part alone and of the one-register form."""
    tot = {k: float((c0[k] + c1[k]).mean()) for k in c0}
    steps = tot["steps"]
    C = COST
    sphere = C["sphere_block"] * tot["sphere_bound"] - C["compare"] * steps
    box = C["box_block"] * tot["box_bound"] - C["compare"] * steps
    one = (C["sphere_block"] + C["box_block"]) * tot["one_register"] - C["compare"] * steps
    setup = 2 * C["setup"]
    return dict(sphere=sphere - setup / 2, box=box - setup / 2, both=sphere + box - setup, one_register=one - setup)


def report(name, c0, c1):
    m = lambda c, k: float(c[k].mean())  # noqa: E731
    print(f"{name}: {len(c0['steps'])} tiles; wave-steps per tile (mean)      primary   reflection   both")
    rows = [("wave-steps", "steps"), ("today's sphere cull fires", "sphere_today"), ("sphere bound clears every live lane", "sphere_bound"),
            ("today's box cull fires", "box_today"), ("box bound clears every live lane", "box_bound"),
            ("... and the sphere bound does not", "box_bound_alone"), ("today's culls both fire", "both_today"),
            ("min(hs, hb) clears every live lane", "one_register")]
    for label, k in rows:
        print(f"  {label:44s} {m(c0, k):7.2f}   {m(c1, k):10.2f}   {m(c0, k) + m(c1, k):6.2f}")
    p = price(c0, c1)
    per_tile = COST["launch_valu"] / COST["tiles"]
    for k in ("sphere", "box", "both", "one_register"):
        print(f"  net of {k:12s} {p[k]:8.1f} vector instructions per tile = {100 * p[k] / per_tile:5.2f} % of {per_tile:.0f}")
    return p


SMALL = {  # tests/test_gpu_ray_bounds.py's cameras in the room: position, yaw, pitch
    "edge": ((6.37, 6.37, 6.7), 0.0, 0.0), "floor": ((2.0, 2.0, 0.0), 0.0, 0.7), "corner": ((4.0, 4.0, 3.0), 0.6, -0.5),
    "default": ((2.0, 2.0, 0.0), 0.0, 0.0), "gap": ((0.77, -0.69, 2.16), -0.44, 0.1), "low_wall": ((6.25, -0.69, 1.55), 1.67, 0.45),
    "sphere": ((3.0, 4.0, 1.9), 0.0, 0.0), "box": ((3.0, 0.3, 1.8), 0.0, 0.0), "graze": ((3.0, 5.0005, -2.0), 0.0, 0.0),
    "box_edge": ((-0.5, 1.5, 2.5), float(np.pi / 2), 0.0), "outside": ((3.0, 3.0, -30.0), 0.0, 0.0),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--stride", type=int, default=6, help="every stride-th tile of the 1080p frame along x and y")
    ap.add_argument("--small", action="store_true", help="the 64x64 test cameras too")
    a = ap.parse_args(argv)
    sc = V.scene_arrays(V.ROOM)
    thr, lim = V.margins(sc)
    print(f"room: thr {thr:.6g}, lim {lim:.6g}, max_dist {sc['max_dist']:.6g}; E = {float((lim + sc['max_dist']) * MARGIN):.3g}; static counts {COST}")
    tx, ty = 1920 // 8, 1080 // 8
    tiles = np.array([(x, y) for y in range(0, ty, a.stride) for x in range(0, tx, a.stride)])
    c0, c1 = frame(sc, thr, lim, 1920, 1080, (2.0, 2.0, 0.0), 0.0, 0.0, tiles)
    report(f"headline 1920x1080, every {a.stride}th tile", c0, c1)
    if a.small:
        tiles = np.array([(x, y) for y in range(8) for x in range(8)])
        for name in sorted(SMALL):
            pos, yaw, pitch = SMALL[name]
            c0, c1 = frame(sc, thr, lim, 64, 64, pos, yaw, pitch, tiles)
            report(f"{name} 64x64", c0, c1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
