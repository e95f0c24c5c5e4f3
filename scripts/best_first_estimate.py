#!/usr/bin/env python3
"""What visiting the reflection point's cage probes best first would save the screen pass's wavefronts (MDH_BEST_FIRST,
DESIGN.md section 4): an estimate in numpy on the room model of scripts/vis_clearance.py, before any kernel is written.

The second shaded point of a pixel (render_probes.glsl:170-183) names ONE probe: the first cage corner in index order whose
dot(probe_to_spec, -N) * vis is the strict maximum.  Today the wavefront of an 8x8 tile walks the corners in index order; a
corner's clearance test (segment_clear) runs while ANY lane still needs it, its march while any lane is not cleared.  Best
first, every lane tries its untried corner of largest d = dot(probe_to_spec, -N) > 0 per round until one is visible; a lane
without a visible candidate of positive d takes today's loop (the fallback, wave-uniform).

For a sample of 8x8 tiles this script follows each pixel's primary and reflection ray in float32 and counts, per tile,

    today        corner passes with a clearance test, and with a march, in the in-order loop;
    best first   rounds (the maximum over the tile's lanes), of them with a test and with a march; lanes and tiles in the
                 fallback, and the fallback's own passes.

    python scripts/best_first_estimate.py [--width W --height H] [--stride S] [--camera X Y Z YAW PITCH] [--map]

--map prints, per tile, the best-first rounds and an F where the tile has fallback lanes (how the cameras of
tests/test_gpu_best_first.py were chosen)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_clearance as V  # noqa: E402

f32 = np.float32
MATERIAL_ROUGHNESS = dict(plane=0.6, sphere=0.1, box=0.3)  # examples.global_illumination: every surface reflects (< 0.75)


def rotation(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])).astype(f32)


def camera_rays(W, H, pos, m, tiles):
    """camera_ray (mdh_device.h) for the 64 pixels of each tile (tx, ty): origins and directions [n, 64, 3], validity [n, 64]."""
    lane = np.arange(64)
    i = tiles[:, 0, None] * 8 + (lane & 7)[None, :]
    j = tiles[:, 1, None] * 8 + (lane >> 3)[None, :]
    valid = (i < W) & (j < H)
    u = (2 * i + 1).astype(f32) / f32(W) - f32(1)
    v = -((2 * j + 1).astype(f32) / f32(H) - f32(1))
    frag = np.stack([u, v, np.zeros_like(u)], axis=-1).astype(f32)
    d = frag - np.array([0, 0, -1.5], f32)
    d = (d / np.sqrt(V.dot(d, d))[..., None]).astype(f32)
    return (frag @ m.T + np.array(pos, f32)).astype(f32), (d @ m.T).astype(f32), valid


def march_hit(sc, o, d, live):
    """march_plain: (hit, t) of rays o + d t up to max_dist."""
    total = np.zeros(len(o), f32)
    hit = np.zeros(len(o), bool)
    live = live.copy()
    while live.any():
        idx = np.nonzero(live)[0]
        sd = V.sdf(sc, o[idx] + d[idx] * total[idx, None])
        h = sd < V.EPS
        hit[idx[h]] = True
        total[idx[~h]] = total[idx[~h]] + sd[~h]
        live[idx] = ~h & (total[idx] < sc["max_dist"])
    return hit, total


def normals(sc, P):
    """The normal of the primitive nearest to P (primitive_info's: a plane's own, a sphere's radial, a box's nearest face)."""
    best = np.full(len(P), np.inf, f32)
    N = np.zeros((len(P), 3), f32)
    o = sc["off"]
    for g in range(6):
        a, s = g // 2, (1.0 if g % 2 == 0 else -1.0)
        dist = f32(s) * P[:, a] + o[g]
        n = np.zeros(3, f32); n[a] = s
        take = dist < best
        best = np.where(take, dist, best); N[take] = n
    for s in sc["spheres"]:
        dv = P - s[:3]
        ln = np.sqrt(V.dot(dv, dv))
        take = ln - s[3] < best
        best = np.where(take, ln - s[3], best); N[take] = (dv / ln[:, None])[take]
    for b in sc["boxes"]:
        q = np.abs(P - b[:3]) - b[3:]
        qp = np.maximum(q, f32(0))
        dist = np.sqrt(V.dot(qp, qp)) + np.minimum(q.max(axis=1), f32(0))
        ax = np.argmax(q, axis=1)
        n = np.zeros((len(P), 3), f32)
        n[np.arange(len(P)), ax] = np.sign(P - b[:3])[np.arange(len(P)), ax]
        take = dist < best
        best = np.where(take, dist, best); N[take] = n[take]
    return N


def second_points(sc, o, d, valid):
    """The reflection ray's hit of every pixel: (active, P, N) -- active where the primary and the reflection ray both hit."""
    h0, t0 = march_hit(sc, o, d, valid)
    P0 = (o + d * t0[:, None]).astype(f32)
    N0 = normals(sc, P0)
    from0 = (P0 + (N0 * V.MIN_STEP) * f32(5)).astype(f32)
    rd = (d - N0 * (f32(2) * V.dot(N0, d))[:, None]).astype(f32)
    h1, t1 = march_hit(sc, from0, rd, valid & h0)
    P1 = (from0 + rd * t1[:, None]).astype(f32)
    return valid & h0 & h1, P1, normals(sc, P1)


def corner_terms(sc, thr, lim, P, N, spacing, dims):
    """Per point and cage corner [n, 8]: unfolded, d, and the visibility ray's outcome (immediate, cleared, marched; vis)."""
    s = np.array(spacing, f32)
    g = np.array(dims)
    gp = np.floor(P / s).astype(np.int64)
    fold = (gp < 0) | (gp >= g - 1)  # [n, 3]
    folded = fold[:, 0] * 1 + fold[:, 1] * 2 + fold[:, 2] * 4
    A = (P + (N * V.MIN_STEP) * f32(5)).astype(f32)
    sd0 = V.sdf(sc, A)
    n = len(P)
    out = dict(unfolded=np.zeros((n, 8), bool), d=np.zeros((n, 8), f32), vmax=np.zeros((n, 8), f32), imm=np.zeros((n, 8), bool),
               clear=np.zeros((n, 8), bool), vis=np.ones((n, 8), bool))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(8):
            bits = np.array([(i >> a) & 1 for a in range(3)])
            q = np.clip(gp + bits, 0, g - 1)
            pw = (q.astype(f32) * s).astype(f32)
            hvec = (P - pw).astype(f32)
            dist = np.sqrt(V.dot(hvec, hvec)).astype(f32)
            vd = (-(hvec / dist[:, None])).astype(f32)
            out["unfolded"][:, i] = (i & folded) == 0
            out["d"][:, i] = V.dot(-vd, -N)
            vmax = (dist - V.MIN_STEP * f32(5)).astype(f32)
            out["vmax"][:, i] = vmax
            need = (vmax > 0) & ~(sd0 < V.EPS) & (sd0 < vmax)  # behind the immediate outcomes
            out["imm"][:, i] = ~need
            vis = np.ones(n, bool)
            vis[(vmax > 0) & (sd0 < V.EPS)] = False
            k = np.nonzero(need & out["unfolded"][:, i])[0]
            if len(k):
                c = V.segment_clear(sc, thr, lim, A[k], vd[k], vmax[k])
                out["clear"][k, i] = c
                m = k[~c]
                if len(m):
                    vis[m] = V.march(sc, A[m], vd[m], vmax[m], sd0[m])[0]
            out["vis"][:, i] = vis
    return out


def in_order(t, lanes):
    """Today's loop for the lanes `lanes` [n] of each point: per corner [n, 8] whether the lane runs a test and a march."""
    n = len(lanes)
    accw = np.full(n, -2.0, f32)
    test = np.zeros((n, 8), bool); mar = np.zeros((n, 8), bool)
    for i in range(8):
        on = lanes & t["unfolded"][:, i]
        d = t["d"][:, i]
        with np.errstate(invalid="ignore"):
            skip = (accw >= 0) & (d <= accw)
        ray = on & ~skip & ~t["imm"][:, i]
        test[:, i] = ray
        mar[:, i] = ray & ~t["clear"][:, i]
        vis = np.where(skip | (t["vmax"][:, i] <= 0), True, t["vis"][:, i])
        w = (d * vis.astype(f32)).astype(f32)
        with np.errstate(invalid="ignore"):
            up = on & (w > accw)
        accw = np.where(up, w, accw)
    return test, mar


def best_first(t, active):
    """The rounds of every lane: tried [n, 8] in order of decreasing d (ties: lowest index), its round number, the fallback lanes."""
    n = len(active)
    with np.errstate(invalid="ignore"):
        cand = t["unfolded"] & (t["d"] > 0) & active[:, None]
    key = np.where(cand, t["d"], -np.inf)
    order = np.argsort(-key, axis=1, kind="stable")  # largest first, lowest index among equals
    rnd = np.full((n, 8), -1)
    searching = active.copy()
    won = np.zeros(n, bool)
    rows = np.arange(n)
    for r in range(8):
        c = order[:, r]
        go = searching & cand[rows, c]
        rnd[rows[go], c[go]] = r
        win = go & t["vis"][rows, c]
        won |= win
        searching &= go & ~win
    return rnd, active & ~won


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--stride", type=int, default=5, help="every stride-th tile along x and y")
    ap.add_argument("--camera", type=float, nargs=5, default=[2.0, 2.0, 0.0, 0.0, 0.0], metavar=("X", "Y", "Z", "YAW", "PITCH"))
    ap.add_argument("--map", action="store_true")
    a = ap.parse_args(argv)
    sc = V.scene_arrays(V.ROOM)
    thr, lim = V.margins(sc)
    tx, ty = (a.width + 7) // 8, (a.height + 7) // 8
    tiles = np.array([(x, y) for y in range(0, ty, a.stride) for x in range(0, tx, a.stride)])
    o, d, valid = camera_rays(a.width, a.height, a.camera[:3], rotation(a.camera[3], a.camera[4]), tiles)
    nt = len(tiles)
    active, P, N = second_points(sc, o.reshape(-1, 3), d.reshape(-1, 3), valid.reshape(-1))
    t = corner_terms(sc, thr, lim, P, N, V.PROBE_SPACING, V.PROBE_DIMS)
    W = lambda x: x.reshape(nt, 64, 8)  # noqa: E731
    test, mar = in_order(t, active)
    corners_today = W(t["unfolded"] & active[:, None]).any(axis=1).sum(axis=1)
    tests_today, marches_today = W(test).any(axis=1).sum(axis=1), W(mar).any(axis=1).sum(axis=1)
    rnd, fb = best_first(t, active)
    need_test = ~t["imm"]; need_mar = need_test & ~t["clear"]
    rounds = W(rnd).max(axis=(1, 2)) + 1
    r_test = np.array([len(np.unique(W(np.where(need_test, rnd, -1))[k][W(np.where(need_test, rnd, -1))[k] >= 0])) for k in range(nt)])
    r_mar = np.array([len(np.unique(W(np.where(need_mar, rnd, -1))[k][W(np.where(need_mar, rnd, -1))[k] >= 0])) for k in range(nt)])
    fb_tile = fb.reshape(nt, 64).any(axis=1)
    ftest, fmar = in_order(t, fb)
    fb_corners = W(t["unfolded"] & fb[:, None]).any(axis=1).sum(axis=1)
    fb_tests, fb_marches = W(ftest).any(axis=1).sum(axis=1), W(fmar).any(axis=1).sum(axis=1)
    lanes = active.reshape(nt, 64).sum(axis=1)
    live = lanes > 0
    print(f"camera {a.camera}, {a.width}x{a.height}, every {a.stride}th tile: {nt} tiles, {int(live.sum())} with a second point, {int(active.sum())} lanes")
    print(f"per tile with a second point (mean)        today   best first   fallback   best first + fallback")
    m = lambda x: float(x[live].mean())  # noqa: E731
    print(f"  corner passes (straight-line code)      {m(corners_today):6.2f}   {m(rounds):10.2f}   {m(fb_corners):8.2f}   {m(rounds) + m(fb_corners):8.2f}   (+ one first pass of {m(corners_today):.2f} directions)")
    print(f"  passes with a clearance test            {m(tests_today):6.2f}   {m(r_test):10.2f}   {m(fb_tests):8.2f}   {m(r_test) + m(fb_tests):8.2f}")
    print(f"  passes with a march                     {m(marches_today):6.2f}   {m(r_mar):10.2f}   {m(fb_marches):8.2f}   {m(r_mar) + m(fb_marches):8.2f}")
    print(f"  rounds histogram (tiles): " + ", ".join(f"{r}: {int((rounds[live] == r).sum())}" for r in range(0, 9) if (rounds[live] == r).any()))
    print(f"  tiles with fallback lanes {int(fb_tile.sum())} of {int(live.sum())}; fallback lanes {int(fb.sum())} of {int(active.sum())}; lanes that win in round 2 or later {int(((rnd.max(axis=1) >= 1) & ~fb).sum())}")
    if a.map:
        grid = {}
        for k, (x, y) in enumerate(tiles):
            grid[(x, y)] = ("." if not live[k] else str(rounds[k])) + ("F" if fb_tile[k] else " ")
        for y in range(0, ty, a.stride):
            print("".join(grid[(x, y)] for x in range(0, tx, a.stride)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
