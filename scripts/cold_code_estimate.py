#!/usr/bin/env python3
"""What the straight-line code around k_screen's march loops would shed: (a) the hit points' arg-min behind closest_primitive's
culls (MDH_INFO_CULL; DESIGN.md section 4 "Exact work elimination" item 18), (b) segment_clear's cross axes and solids behind wave
ballots and (c) the reflection ray's first step taken from the first point's sd0 (both built, measured and dropped in round 23:
"What was tried and dropped").  An estimate in numpy on the room model of scripts/vis_clearance.py and
scripts/best_first_estimate.py, before any kernel is changed.  Per 8x8 tile, with the lanes grouped as the kernel groups
them (one wavefront per tile), it counts

    (a) hit points (the primary ray's and the reflection ray's) whose whole wavefront culls the sphere, the box or both in the
        typed arg-min -- closest_primitive's two ballots against the minimum the six planes left;
    (b) segment_clear calls (the first point's unfolded corners, the second point's best-first rounds and fallback passes)
        whose candidate lanes are all separated from the box by one of its three face axes, and calls that no candidate lane's
        `ok` survives the bound on lim and the planes;
    (c) tiles that trace a reflection ray, and which roots that ray's first evaluation takes.

Each count is multiplied by the static VALU count of the block it skips and divided by the launch's 187.43 M VALU instructions
(DESIGN.md section 8).  The static counts are of the probe kernels of scripts/probes/cold_code_probe.hip, cross-compiled for gfx950
with the Makefile's flags, one block per kernel, less an empty kernel with the same loads and stores (the commands are in that file's
header; scripts/probes/count_valu.py counts).  Not of k_screen's own disassembly: inlined there, a block's instructions are scheduled
among its neighbours' and have no boundary to count between.  The counts are upper bounds -- in the kernel a candidate shares its
distance with its cull -- and the counted drop of (a) was 64 instructions per wavefront where this script says 137
(profiles/r23_cold_code_ab.log):

    sphere candidate (root, subtract, MDH_CAND)   47, of which the cull's own distance and test keep 13  -> 34 saved
    box candidate                                 55, of which the cull keeps 12                         -> 43 saved
    segment_clear: sphere block 27, the box's three face axes 23, its three cross axes 27
    sdf <ROOM>: 47 with both roots culled, + 26 for the sphere's, + 33 for the box's (106 with both)

    python scripts/cold_code_estimate.py [--width W --height H] [--stride S] [--camera X Y Z YAW PITCH]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_first_estimate as E  # noqa: E402
import vis_clearance as V  # noqa: E402

f32 = np.float32
K1 = f32(1.000001)
LAUNCH_VALU = 187.43e6
SAVE_SPHERE, SAVE_BOX = 34, 43
CLEAR_SPHERE, CLEAR_FACES, CLEAR_CROSS = 27, 23, 27
SDF_BASE, SDF_SPHERE, SDF_BOX = 47, 26, 33


def tile_any(x, nt):
    return x.reshape(nt, 64).any(axis=1)


def info_culls(sc, P, lanes, nt):
    """Per tile: (has a hit point, culls the sphere, culls the box) -- the typed arg-min's ballots, float32."""
    o = sc["off"]
    closest = np.full(len(P), sc["max_dist"], f32)
    with np.errstate(invalid="ignore"):
        for a in range(3):
            closest = np.fmin(closest, np.fmin(P[:, a] + o[2 * a], -P[:, a] + o[2 * a + 1]))
        s = sc["spheres"][0]
        v = s[:3] - P
        d2 = V.dot(v, v)
        tsum = closest + s[3]
        need_s = tile_any(lanes & ~(tsum < 0) & ~(d2 > (tsum * tsum) * K1), nt)
        ds = np.sqrt(d2) - s[3]
        closest = np.where(np.repeat(need_s, 64) & (ds < closest), ds, closest)
        b = sc["boxes"][0]
        q = np.abs(b[:3] - P) - b[3:]
        m = np.maximum(q[:, 0], np.maximum(q[:, 1], q[:, 2]))
        thr = np.where(closest > 0, closest * K1, closest)
        need_b = tile_any(lanes & ~(m > thr), nt)
    has = tile_any(lanes, nt)
    return has, has & ~need_s, has & ~need_b


def clear_parts(sc, thr, lim, A, vd, vmax):
    """segment_clear's stages per ray: ok behind lim and the planes, ok behind the sphere too, separated by a face axis."""
    with np.errstate(invalid="ignore", over="ignore"):
        B = A + vd * vmax[:, None]
        ok = np.full(len(A), thr > 0) & np.all(np.abs(A) <= lim, axis=1) & np.all(np.abs(B) <= lim, axis=1)
        lo, hi = np.fmin(A, B), np.fmax(A, B)
        o = sc["off"]
        pl = np.fmin(lo[:, 0] + o[0], -hi[:, 0] + o[1])
        pl = np.fmin(pl, np.fmin(lo[:, 1] + o[2], -hi[:, 1] + o[3]))
        pl = np.fmin(pl, np.fmin(lo[:, 2] + o[4], -hi[:, 2] + o[5]))
        ok &= pl > thr
        s = sc["spheres"][0]
        w = s[:3] - A
        t = np.fmin(np.fmax(V.dot(w, vd), f32(0)), vmax)
        q = w - vd * t[:, None]
        rt = s[3] + thr
        ok_s = ok & (V.dot(q, q) > rt * rt)
        hv = vd * (vmax * f32(0.5))[:, None]
        ah = np.abs(hv)
        b = sc["boxes"][0]
        am = np.abs((A + hv) - b[:3])
        e = b[3:] + thr
        faces = (am[:, 0] > e[0] + ah[:, 0]) | (am[:, 1] > e[1] + ah[:, 1]) | (am[:, 2] > e[2] + ah[:, 2])
    return ok, ok_s, faces


def corner_stages(sc, thr, lim, P, N):
    """Per point and cage corner [n, 8]: the stages of clear_parts for the corner's visibility ray."""
    s = np.array(V.PROBE_SPACING, f32)
    g = np.array(V.PROBE_DIMS)
    gp = np.floor(P / s).astype(np.int64)
    A = (P + (N * V.MIN_STEP) * f32(5)).astype(f32)
    n = len(P)
    ok, ok_s, faces = (np.zeros((n, 8), bool) for _ in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(8):
            bits = np.array([(i >> a) & 1 for a in range(3)])
            pw = (np.clip(gp + bits, 0, g - 1).astype(f32) * s).astype(f32)
            hvec = (P - pw).astype(f32)
            dist = np.sqrt(V.dot(hvec, hvec)).astype(f32)
            vd = (-(hvec / dist[:, None])).astype(f32)
            ok[:, i], ok_s[:, i], faces[:, i] = clear_parts(sc, thr, lim, A, vd, (dist - V.MIN_STEP * f32(5)).astype(f32))
    return ok, ok_s, faces


def count_calls(cand, st, nt):
    """cand [n, k] candidate lanes per call slot -> (calls, calls with no `ok` lane, calls whose needy lanes the faces all separate)."""
    ok, ok_s, faces = st
    W = lambda x: x.reshape(nt, 64, -1)  # noqa: E731
    calls = W(cand).any(axis=1)
    none_ok = calls & ~W(cand & ok).any(axis=1)
    faces_do = calls & ~none_ok & ~W(cand & ok_s & ~faces).any(axis=1)
    return int(calls.sum()), int(none_ok.sum()), int(faces_do.sum())


def estimate(a):
    sc = V.scene_arrays(V.ROOM)
    thr, lim = V.margins(sc)
    tx, ty = (a.width + 7) // 8, (a.height + 7) // 8
    tiles = np.array([(x, y) for y in range(0, ty, a.stride) for x in range(0, tx, a.stride)])
    nt = len(tiles)
    o, d, valid = E.camera_rays(a.width, a.height, a.camera[:3], E.rotation(a.camera[3], a.camera[4]), tiles)
    o, d, valid = o.reshape(-1, 3), d.reshape(-1, 3), valid.reshape(-1)
    h0, t0 = E.march_hit(sc, o, d, valid)
    h0 &= valid
    P0 = (o + d * t0[:, None]).astype(f32)
    N0 = E.normals(sc, P0)
    from0 = (P0 + (N0 * V.MIN_STEP) * f32(5)).astype(f32)
    rd = (d - N0 * (f32(2) * V.dot(N0, d))[:, None]).astype(f32)
    h1, t1 = E.march_hit(sc, from0, rd, h0)
    h1 &= h0
    P1 = (from0 + rd * t1[:, None]).astype(f32)
    N1 = E.normals(sc, P1)
    # (a)
    has0, cs0, cb0 = info_culls(sc, P0, h0, nt)
    has1, cs1, cb1 = info_culls(sc, P1, h1, nt)
    n_points = int(has0.sum() + has1.sum())
    n_sphere, n_box, n_both = int(cs0.sum() + cs1.sum()), int(cb0.sum() + cb1.sum()), int((cs0 & cb0).sum() + (cs1 & cb1).sum())
    valu_a = n_sphere * SAVE_SPHERE + n_box * SAVE_BOX
    # (b) the first point: every unfolded corner behind the immediate outcomes; the second: the best-first rounds and the fallback
    t0c = E.corner_terms(sc, thr, lim, P0, N0, V.PROBE_SPACING, V.PROBE_DIMS)
    st0 = corner_stages(sc, thr, lim, P0, N0)
    first = count_calls(t0c["unfolded"] & ~t0c["imm"] & h0[:, None], st0, nt)
    t1c = E.corner_terms(sc, thr, lim, P1, N1, V.PROBE_SPACING, V.PROBE_DIMS)
    st1 = corner_stages(sc, thr, lim, P1, N1)
    rnd, fb = E.best_first(t1c, h1)
    rows = np.arange(len(P1))
    cand_r = np.zeros((len(P1), 8), bool)
    st_r = tuple(np.zeros((len(P1), 8), bool) for _ in range(3))
    for r in range(8):  # call slot r: the corner each lane tries in round r
        c = np.argmax(rnd == r, axis=1)
        go = (rnd == r).any(axis=1)
        cand_r[:, r] = go & ~t1c["imm"][rows, c]
        for k in range(3):
            st_r[k][:, r] = st1[k][rows, c]
    second = count_calls(cand_r, st_r, nt)
    ftest, _ = E.in_order(t1c, fb)
    fallback = count_calls(ftest, st1, nt)
    calls, none_ok, faces_do = (first[k] + second[k] + fallback[k] for k in range(3))
    valu_b = none_ok * (CLEAR_SPHERE + CLEAR_FACES + CLEAR_CROSS) + faces_do * CLEAR_CROSS
    # (c) the reflection ray's first evaluation, at from0: the roots its wavefront takes there
    _, rs, rb = info_culls(sc, from0, h0, nt)  # (closest_primitive's culls behind the planes: the same ballots)
    n_refl = int(has0.sum())
    valu_c = n_refl * SDF_BASE + int((has0 & ~rs).sum()) * SDF_SPHERE + int((has0 & ~rb).sum()) * SDF_BOX
    scale = (tx * ty) / nt
    pct = lambda v: 100.0 * v * scale / LAUNCH_VALU  # noqa: E731
    print(f"camera {a.camera}, {a.width}x{a.height}, every {a.stride}th tile: {nt} of {tx * ty} tiles")
    print(f"  (a) hit points (tile-wavefronts) {n_points}: cull the sphere {n_sphere}, the box {n_box}, both {n_both}"
          f"  -> {valu_a / max(nt, 1):7.1f} VALU per tile, {pct(valu_a):.2f} % of the launch")
    print(f"  (b) segment_clear calls {calls} ({calls / max(nt, 1):.2f} per tile; first point {first[0]}, second point {second[0]}, fallback {fallback[0]}):"
          f" no candidate left behind the planes {none_ok}, faces separate every candidate {faces_do}"
          f"  -> {valu_b / max(nt, 1):7.1f} VALU per tile, {pct(valu_b):.2f} % of the launch")
    print(f"  (c) tiles with a reflection ray {n_refl}: its first evaluation takes the sphere's root in {int((has0 & ~rs).sum())}, the box's in {int((has0 & ~rb).sum())}"
          f"  -> {valu_c / max(nt, 1):7.1f} VALU per tile, {pct(valu_c):.2f} % of the launch")
    return pct(valu_a), pct(valu_b), pct(valu_c)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--stride", type=int, default=5, help="every stride-th tile along x and y")
    ap.add_argument("--camera", type=float, nargs=5, default=[2.0, 2.0, 0.0, 0.0, 0.0], metavar=("X", "Y", "Z", "YAW", "PITCH"))
    a = ap.parse_args(argv)
    pa, pb, pc = estimate(a)
    if (a.width, a.height) == (1920, 1080):
        for name, p in (("(a) the arg-min's culls", pa), ("(b) the clearance test's ballots", pb), ("(c) the reflection ray's first step", pc)):
            print(f"=> {name}: {p:.2f} % of k_screen's VALU instructions: " + ("worth building." if p >= 0.5 else "below 0.5 %, not built."))
    return 0


if __name__ == "__main__":
    sys.exit(main())
