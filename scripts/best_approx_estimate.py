#!/usr/bin/env python3
"""What ranking the second point's cage probes by an approximate d and directing the winner only would save the screen pass
(MDH_BEST_APPROX): an estimate in numpy on the room model of scripts/vis_clearance.py and
scripts/best_first_estimate.py, before any kernel is run.

The first round of the best-first search (shade_structured, mdh_march.h) scans every unfolded corner's exact direction --
probes_fresh, cage_probe, grid_to_world, a correctly rounded root, three IEEE divisions, the dot product -- to pick ONE corner.
Under the rule (best_approx, mdh_march.h) every lane ranks the corners by a_i = -dot(h_i, N) * rsq(dot2(h_i)); a lane whose
largest a leads the runner-up by more than 2 eps and exceeds eps has its winner, a lane whose a are all below -eps has none,
any other lane is undecided.  A wavefront without an undecided lane runs the exact statements once, for the winners' corners;
one with an undecided lane scans as today.

Per 8x8 tile, lock-step, this script counts

    today     the corner passes of the exact scan's first round (a corner some lane of the tile has unfolded);
    the rule  the approximate corners (8, 4, 2 or 1: every corner not folded in all lanes), the exact passes (1 where the rule
              decides for the tile and some lane has a winner, today's otherwise), undecided lanes and tiles;
    net       vector instructions per tile, from the static counts of scripts/probes/best_approx_probe.hip, and as a share
              of the 177.08 M of one 1080p launch (profiles/r26_ray_bounds_ab.log).

It also checks the rule against the scan on every lane it meets: a decided lane names the scan's corner (or none).

    python scripts/best_approx_estimate.py [--width W --height H] [--stride S] [--camera X Y Z YAW PITCH]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_first_estimate as BF  # noqa: E402

V = BF.V
f32 = np.float32
EPS_A = f32(2.0 ** -19)  # MDH_BEST_APPROX_EPS (mdh_march.h, where the argument is)
D2_LO, D2_HI = f32(2.0 ** -40), f32(2.0 ** 40)  # the smallest dot2 the rule accepts; the largest one that lim <= 2^18 lets through
LIM_HI = f32(2.0 ** 18)
# static counts (vector instructions, gfx950, the Makefile's flags): scripts/probes/best_approx_probe.hip gives a_base 15, a_skip 20,
# a_scan1 121, a_winner 109, a_root_base 5, a_root_full 22, a_rank0 173, a_rank1 122, a_rank3 96, a_rank7 78.  A scan pass is
# a_scan1 - a_base less the root's full expansion (a_root_full - a_root_base = 17: code behind sqrt_'s guard that a dot2 of 2^-96 or
# more never runs) plus the loop's skip test (a_skip - a_base); the winner's block likewise; the ranking by its number of corners.
COST = dict(scan_pass=121 - 15 - 17 + 5, winner=109 - 15 - 17, rank={8: 173 - 15, 4: 122 - 15, 2: 96 - 15, 1: 78 - 15}, launch_valu=177.08e6, tiles=32400)


def rsq32(x):
    """v_rsq_f32 to within its ulp: the float64 inverse root, rounded once"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (1.0 / np.sqrt(x.astype(np.float64))).astype(f32)


def cage(P, spacing, dims):
    """world_to_grid and the folds: gp [n, 3] (int64), fold [n, 3]"""
    s = np.array(spacing, f32)
    g = np.array(dims)
    with np.errstate(invalid="ignore"):
        q = np.floor((P / s).astype(f32))
    gp = np.clip(np.where(np.isfinite(q), q, 0), -2.0 ** 30, 2.0 ** 30).astype(np.int64)  # (far outside the grid either way)
    return gp, (gp < 0) | (gp >= g - 1)


def exact_scan(P, N, spacing, dims):
    """The first round's exact scan: d [n, 8] in float32 (the kernel's operations), unfolded [n, 8], and its choice bi [n]
    (-1: no candidate): the largest d > 0, the lowest index among equals."""
    s = np.array(spacing, f32)
    g = np.array(dims)
    gp, fold = cage(P, spacing, dims)
    folded = fold[:, 0] * 1 + fold[:, 1] * 2 + fold[:, 2] * 4
    n = len(P)
    d = np.zeros((n, 8), f32)
    unf = np.zeros((n, 8), bool)
    bd = np.zeros(n, f32)
    bi = np.full(n, -1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(8):
            bits = np.array([(i >> a) & 1 for a in range(3)])
            q = np.clip(gp + bits, 0, g - 1)
            pw = (q.astype(f32) * s).astype(f32)
            h = (P - pw).astype(f32)
            dist = np.sqrt(V.dot(h, h)).astype(f32)
            v = (h / dist[:, None]).astype(f32)
            d[:, i] = V.dot(v, -N)  # dot(-vd, -N), vd = -(h / dist)
            unf[:, i] = (i & folded) == 0
            up = unf[:, i] & (d[:, i] > bd)
            bd = np.where(up, d[:, i], bd)
            bi = np.where(up, i, bi)
    return d, unf, bi


def rule(P, N, spacing, dims, lim):
    """best_approx: (state [n]: 1 winner, 2 no candidate, 0 undecided; bi [n]; a [n, 8], below -8 at a folded corner)."""
    s = np.array(spacing, f32)
    g = np.array(dims)
    gp, fold = cage(P, spacing, dims)
    n = len(P)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.all(np.abs(P) <= lim, axis=1) & np.all(np.abs(N) <= f32(1), axis=1)
        ok &= bool(np.all(np.abs((g - 1).astype(f32) * s) <= lim)) and bool(f32(0) <= lim <= LIM_HI)
        out = f32(lim * f32(32))  # a folded corner's place holder
        h0 = (P - (np.clip(gp, 0, g - 1).astype(f32) * s).astype(f32)).astype(f32)
        h1 = (P - ((gp + 1).astype(f32) * s).astype(f32)).astype(f32)
        sq = np.stack([h0 * h0, np.where(fold, h0 * h0, h1 * h1)], axis=-1).astype(f32)  # [n, 3, 2]
        pn = np.stack([h0 * N, np.where(fold, out, h1 * N)], axis=-1).astype(f32)
        a = np.zeros((n, 8), f32)
        a1 = np.full(n, -4.0, f32); a2 = np.full(n, -4.0, f32)
        bi = np.full(n, -1)
        dmin = np.full(n, 4.0, f32)
        for i in range(8):
            bx, by, bz = i & 1, (i >> 1) & 1, (i >> 2) & 1
            d2 = ((sq[:, 0, bx] + sq[:, 1, by]) + sq[:, 2, bz]).astype(f32)
            dn = ((pn[:, 0, bx] + pn[:, 1, by]) + pn[:, 2, bz]).astype(f32)
            ai = (-dn * rsq32(d2)).astype(f32)
            a[:, i] = ai
            dmin = np.fmin(dmin, d2)  # (v_min_f32: minNum)
            up = ai > a1
            bi = np.where(up, i, bi)
            a2 = np.where(up, a1, np.where(ai > a2, ai, a2))  # (the median of a, a1 and a2 <= a1)
            a1 = np.where(up, ai, a1)
        ok &= dmin >= D2_LO
        win = ok & (a1 - a2 > f32(2) * EPS_A) & (a1 > EPS_A)
        none = ok & ~win & (a1 < -EPS_A)
    state = np.where(win, 1, np.where(none, 2, 0))
    return state, np.where(win, bi, -1), a


def tiles_of(sc, a):
    tx, ty = (a.width + 7) // 8, (a.height + 7) // 8
    tiles = np.array([(x, y) for y in range(0, ty, a.stride) for x in range(0, tx, a.stride)])
    o, d, valid = BF.camera_rays(a.width, a.height, a.camera[:3], BF.rotation(a.camera[3], a.camera[4]), tiles)
    active, P, N = BF.second_points(sc, o.reshape(-1, 3), d.reshape(-1, 3), valid.reshape(-1))
    return len(tiles), active, P, N


def tile_counts(active, P, N, lim, nt):
    """Per tile [nt]: today's scan passes, the ranking's corners, the exact passes under the rule, undecided lanes; and the lanes' states."""
    d, unf, bi_x = exact_scan(P, N, V.PROBE_SPACING, V.PROBE_DIMS)
    state, bi_r, _ = rule(P, N, V.PROBE_SPACING, V.PROBE_DIMS, lim)
    dec = active & (state != 0)
    assert np.array_equal(bi_r[dec], bi_x[dec]), "the rule names another corner than the scan"
    W = lambda x: x.reshape(nt, 64, -1)  # noqa: E731
    act = active.reshape(nt, 64)
    passes = W(unf & active[:, None]).any(axis=1).sum(axis=1)
    _, fold = cage(P, V.PROBE_SPACING, V.PROBE_DIMS)
    wave_unfolded = W(~fold & active[:, None]).any(axis=1).sum(axis=1)  # axes some lane has unfolded
    rank_corners = np.where(act.any(axis=1), 2 ** wave_unfolded, 0)
    und = (active & (state == 0)).reshape(nt, 64).sum(axis=1)
    wins = (active & (state == 1)).reshape(nt, 64).any(axis=1)
    exact = np.where(und > 0, passes, wins.astype(int))
    return passes, rank_corners, exact, und, state


def report(name, nt, active, P, N, lim):
    passes, rank_corners, exact, und, state = tile_counts(active, P, N, lim, nt)
    live = active.reshape(nt, 64).any(axis=1)
    C = COST
    today = passes * C["scan_pass"]
    new = np.array([C["rank"].get(int(k), 0) for k in rank_corners]) + np.where(und > 0, passes * C["scan_pass"], exact * C["winner"])
    per_tile = C["launch_valu"] / C["tiles"]
    m = lambda x: float(np.asarray(x, float)[live].mean()) if live.any() else 0.0  # noqa: E731
    lanes = int(active.sum())
    print(f"{name}: {nt} tiles, {int(live.sum())} with a second point, {lanes} lanes")
    print(f"  exact corner passes per tile today            {m(passes):6.2f}")
    print(f"  under the rule: approximate corners           {m(rank_corners):6.2f}   exact passes {m(exact):6.2f}")
    print(f"  undecided lanes {int(und.sum())} of {lanes} ({100.0 * und.sum() / max(lanes, 1):.2f} %), tiles with one {int((und > 0).sum())} of {int(live.sum())}; "
          f"winners {int((active & (state == 1)).sum())}, without a candidate {int((active & (state == 2)).sum())}")
    net = m(today) - m(new)
    print(f"  vector instructions per tile: today {m(today):7.1f}, the rule {m(new):7.1f}, net {net:+7.1f} = {100.0 * net / per_tile:+.2f} % of the launch's {per_tile:.0f} per tile")
    return net / per_tile


CAMERAS_64 = {"default": (2.0, 2.0, 0.0, 0.0, 0.0), "edge": (6.37, 6.37, 6.7, 0.0, 0.0), "floor": (2.0, 2.0, 0.0, 0.0, 0.7), "corner": (4.0, 4.0, 3.0, 0.6, -0.5),
              "gap": (0.77, -0.69, 2.16, -0.44, 0.1), "low_wall": (6.25, -0.69, 1.55, 1.67, 0.45)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--stride", type=int, default=5, help="every stride-th tile along x and y")
    ap.add_argument("--camera", type=float, nargs=5, default=None, metavar=("X", "Y", "Z", "YAW", "PITCH"))
    a = ap.parse_args(argv)
    sc = V.scene_arrays(V.ROOM)
    _, lim = V.margins(sc)
    print(f"room: lim {lim:.6g}, eps 2^-19 = {float(EPS_A):.3g}; static counts {COST}")
    if a.camera is not None:
        report(f"camera {a.camera}, {a.width}x{a.height}, every {a.stride}th tile", *tiles_of(sc, a), lim)
        return 0
    a.camera = [2.0, 2.0, 0.0, 0.0, 0.0]
    share = report(f"## the headline frame, camera {a.camera}, {a.width}x{a.height}, every {a.stride}th tile", *tiles_of(sc, a), lim)
    print("## the 64x64 frames of tests/test_gpu_best_first.py (every tile)")
    for name in sorted(CAMERAS_64):
        b = argparse.Namespace(width=64, height=64, stride=1, camera=list(CAMERAS_64[name]))
        report(f"{name} {b.camera}", *tiles_of(sc, b), lim)
    print(f"=> the headline frame: {100.0 * share:+.2f} % of the launch's vector instructions; the project's bar for building a part is 0.5 %: "
          + ("the kernel change goes on." if share >= 0.005 else "below the bar: not built."))
    return 0


if __name__ == "__main__":
    sys.exit(main())
