"""MDH_BEST_APPROX (mdh_march.h: best_approx) restated in numpy (scripts/best_approx_estimate.py), float32, the kernel's
operations, beside the exact first-round scan of the second point's best-first search and a float64 reference.  More than 10^5
points over three scenes (the room, the sphere tangent to a wall, the box in a wall) and both probe grids:

    wherever the rule decides, the exact float32 scan names the same corner, or none;
    the measured max |a_i - d_i| over every unfolded corner of every point inside the rule's range tests stays below eps / 2
    (eps = 2^-19 is derived beside the code from the roundings, not from this measurement), and both stay within their
    derived shares of the float64 value: 13 u and 11.3 u, u = 2^-24;
    the rule decides for at least 90 % of the lanes of the headline camera's sample (the condition under which it pays).

Point families: the scenes' surfaces with their normals; random points with random unit normals; points ON the cage's
symmetry planes (midway between two probes along one, two or three axes, with a normal that makes the two sides equal: exact
ties), within 2^-16 .. 2^-22 of them, AT a probe and within a few ulps of one; normals with a zero component, with -0, with a
NaN, with a component above 1; coordinates beyond lim, infinite and NaN."""
import importlib.util
import os
import sys

import numpy as np
import pytest

_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")


def _load(name):
    if _DIR not in sys.path:
        sys.path.insert(0, _DIR)
    spec = importlib.util.spec_from_file_location(name, os.path.join(_DIR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


E = _load("best_approx_estimate")
V = E.V
f32 = np.float32
U = 2.0 ** -24
EPS = float(E.EPS_A)

SCENES = {
    "room": V.ROOM,
    "tangent_sphere": dict(V.ROOM, spheres=[((0.0, 4.0, 3.0), 1.0)]),
    "box_in_wall": dict(V.ROOM, boxes=[((3.0, 0.5, 4.0), (1.5, 1.5, 1.5))]),
}
GRIDS = {"8x8x8": ((0.95, 0.95, 0.9), (8, 8, 8)), "default": ((2.0, 3.0, 3.0), (4, 3, 3))}


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def surface_points(scene, rng, n):
    """points of the scene's surfaces with their normals: the walls, the sphere, the box's faces"""
    c, r = (np.array(v, float) for v in scene["spheres"][0])
    bc, be = (np.array(v, float) for v in scene["boxes"][0])
    lo, hi = np.array([-1.0, -1.0, -6.0]), np.array([7.0, 7.0, 7.0])
    k = n // 3
    a = rng.integers(0, 3, k); s = rng.choice([-1.0, 1.0], k)
    P = lo + rng.random((k, 3)) * (hi - lo)
    P[np.arange(k), a] = np.where(s > 0, lo[a], hi[a])
    N = np.zeros((k, 3)); N[np.arange(k), a] = s
    d = unit(rng.normal(size=(k, 3)))
    a2 = rng.integers(0, 3, k); s2 = rng.choice([-1.0, 1.0], k)
    u = rng.random((k, 3)) * 2 - 1
    u[np.arange(k), a2] = s2
    N2 = np.zeros((k, 3)); N2[np.arange(k), a2] = s2
    return np.concatenate([P, c + r * d, bc + u * be]), np.concatenate([N, d, N2])


def families(scene, grid, rng):
    """{family: (P, N)} in float64; the checks run their float32 roundings"""
    sp, dm = (np.array(v, float) for v in grid)
    lo, hi = np.array([-1.0, -1.0, -6.0]), np.array([7.0, 7.0, 7.0])
    out = {}
    out["surfaces"] = surface_points(scene, rng, 9000)
    n = 4000
    out["random"] = (lo + rng.random((n, 3)) * (hi - lo), unit(rng.normal(size=(n, 3))))
    # on the symmetry planes of a cage cell: midway between the probes along the axes of a mask, the normal without a component
    # along them (both sides get the same a, bit for bit where the midpoint is a float: the default grid's are)
    n = 3000
    cell = np.stack([rng.integers(0, int(dm[a]) - 1, n) for a in range(3)], axis=1)
    frac = rng.random((n, 3))
    mask = rng.integers(1, 8, n)[:, None] >> np.arange(3)[None, :] & 1
    frac = np.where(mask == 1, 0.5, frac)
    P = (cell + frac) * sp
    N = unit(np.where(mask == 1, 0.0, rng.normal(size=(n, 3))) + 1e-30)
    N = np.where(mask == 1, 0.0, N)
    allm = mask.sum(axis=1) == 3
    N[allm] = unit(rng.normal(size=(int(allm.sum()), 3)))  # (the cell's centre: any normal)
    out["symmetric"] = (P, N)
    off = 2.0 ** -rng.integers(16, 23, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    out["near_symmetric"] = (P + mask * off, N)
    out["symmetric_tilted"] = (P, unit(N + 2.0 ** -rng.integers(16, 23, (n, 1)) * rng.normal(size=(n, 3)) + 1e-30))
    n = 1000  # at a probe and a few ulps from one
    q = np.stack([rng.integers(0, int(dm[a]), n) for a in range(3)], axis=1)
    pw = (q.astype(f32) * sp.astype(f32)).astype(np.float64)
    Nq = unit(rng.normal(size=(n, 3)))
    out["at_probe"] = (pw, Nq)
    out["near_probe"] = (pw * (1.0 + rng.integers(-4, 5, (n, 3)) * 2.0 ** -23) + rng.integers(-4, 5, (n, 3)) * 2.0 ** -149, Nq)
    n = 2000  # the normal's edge cases
    P = lo + rng.random((n, 3)) * (hi - lo)
    N = unit(rng.normal(size=(n, 3)))
    k = n // 4
    N[:k][np.arange(k), rng.integers(0, 3, k)] = 0.0
    N[k:2 * k][np.arange(k), rng.integers(0, 3, k)] = -0.0
    N[2 * k:3 * k][np.arange(k), rng.integers(0, 3, k)] = np.nan
    N[3 * k:][np.arange(n - 3 * k), rng.integers(0, 3, n - 3 * k)] = rng.choice([-1.0, 1.0], n - 3 * k) * rng.uniform(1.0001, 3.0, n - 3 * k)
    out["normals"] = (P, N)
    out["axis_normals"] = (lo + rng.random((n, 3)) * (hi - lo), np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1)))
    n = 1000
    P = (rng.random((n, 3)) * 2 - 1) * 40.0
    P[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n) * rng.uniform(16.001, 60.0, n)
    P[:100][np.arange(100), rng.integers(0, 3, 100)] = np.inf
    P[100:200][np.arange(100), rng.integers(0, 3, 100)] = np.nan
    P[200:300] *= 1e30
    out["beyond_lim"] = (P, unit(rng.normal(size=(n, 3))))
    return out


OFF = ("beyond_lim",)  # families the rule must leave undecided


def reference(P, N, grid):
    """t_i = -dot(h, N) / |h| in float64 from the float32 h of the scan [n, 8]"""
    s = np.array(grid[0], f32); g = np.array(grid[1])
    gp, _ = E.cage(P, *grid)
    t = np.zeros((len(P), 8))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(8):
            bits = np.array([(i >> a) & 1 for a in range(3)])
            h = (P - (np.clip(gp + bits, 0, g - 1).astype(f32) * s).astype(f32)).astype(f32).astype(np.float64)
            t[:, i] = -np.sum(h * N.astype(np.float64), axis=1) / np.sqrt(np.sum(h * h, axis=1))
    return t


_seen = {"points": 0, "worst": 0.0}


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_decided_lane_names_the_scans_corner(name, grid):
    sc = V.scene_arrays(SCENES[name])
    _, lim = V.margins(sc)
    assert lim == 16.0
    fam = families(SCENES[name], GRIDS[grid], np.random.default_rng(29))
    total = sum(len(P) for P, _ in fam.values())
    assert total * len(SCENES) * len(GRIDS) >= 100000
    for key, (P, N) in sorted(fam.items()):
        P = P.astype(f32); N = N.astype(f32)
        d, unf, bi_x = E.exact_scan(P, N, *GRIDS[grid])
        state, bi_r, a = E.rule(P, N, *GRIDS[grid], lim)
        dec = state != 0
        assert np.array_equal(bi_r[dec], bi_x[dec]), (key, int((bi_r[dec] != bi_x[dec]).sum()))
        assert np.all(bi_x[state == 2] == -1) and np.all(bi_r[state == 1] >= 0)
        if key in OFF:
            assert not dec.any(), key
        if key == "symmetric" and grid == "default":  # exact ties (the midpoints are floats): never a winner between two equals
            assert (state == 0).mean() > 0.5, (state == 0).mean()
        if key == "normals":
            bad = np.isnan(N).any(axis=1) | (np.abs(N) > 1).any(axis=1)
            assert bad.any() and not dec[bad].any()
        # the bound: every unfolded corner of every lane inside the range tests (decided or a near tie), against each other and
        # against float64
        with np.errstate(invalid="ignore"):
            inr = np.all(np.abs(P) <= lim, axis=1) & np.all(np.abs(N) <= 1, axis=1)
        t = reference(P, N, GRIDS[grid])
        with np.errstate(invalid="ignore"):
            fin = unf & inr[:, None] & np.isfinite(a) & np.isfinite(d) & np.isfinite(t)
            h2ok = fin.copy()
        # (dot2 in [2^-40, 2^40]: at a probe the scan's d is 0 / 0 and the rule is undecided)
        rng_ok = np.zeros_like(fin)
        s = np.array(GRIDS[grid][0], f32); g = np.array(GRIDS[grid][1])
        gp, _ = E.cage(P, *GRIDS[grid])
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(8):
                bits = np.array([(i >> k) & 1 for k in range(3)])
                h = (P - (np.clip(gp + bits, 0, g - 1).astype(f32) * s).astype(f32)).astype(f32)
                d2 = V.dot(h, h)
                rng_ok[:, i] = (d2 >= E.D2_LO) & (d2 <= E.D2_HI)
        m = h2ok & rng_ok
        if m.any():
            a64, d64 = np.where(m, a, 0).astype(np.float64), np.where(m, d, 0).astype(np.float64)
            t = np.where(m, t, 0.0)
            worst = float(np.abs(a64 - d64).max())
            wa = float(np.abs(a64 - t).max()); wd = float(np.abs(d64 - t).max())
            print("%s %s %s: %d points, decided %.1f %%, max |a - d| %.2f u, |a - t| %.2f u, |d - t| %.2f u"
                  % (name, grid, key, len(P), 100.0 * dec.mean(), worst / U, wa / U, wd / U))
            assert worst < EPS / 2, (key, worst / U)
            assert wa <= 13.0 * U and wd <= 11.3 * U, (key, wa / U, wd / U)
            _seen["worst"] = max(_seen["worst"], worst)
        _seen["points"] += len(P)


def test_an_exact_tie_and_a_probe_are_undecided():
    sc = V.scene_arrays(V.ROOM)
    _, lim = V.margins(sc)
    grid = GRIDS["default"]
    P = np.array([[3.0, 1.0, 1.0], [3.0, 4.5, 4.5], [2.0, 3.0, 3.0], [2.5, 1.0, 1.0]], f32)
    N = np.array([[0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], f32)
    state, bi, a = E.rule(P, N, *grid, lim)
    d, unf, bx = E.exact_scan(P, N, *grid)
    assert state[0] == 0 and a[0, 0] == a[0, 1]  # midway along x, the normal across: a tie
    assert state[1] == 0  # the cell's centre along all three axes
    assert state[2] == 0 and np.isnan(d[2]).any()  # at a probe: dot2 = 0
    assert state[3] == 1 and bi[3] == bx[3]  # off the plane: decided, and the scan's


def test_the_rule_decides_for_the_headline_cameras_lanes():
    """the condition of the issue, on the room model: every 12th tile of the 1080p frame"""
    import argparse
    sc = V.scene_arrays(V.ROOM)
    _, lim = V.margins(sc)
    a = argparse.Namespace(width=1920, height=1080, stride=12, camera=[2.0, 2.0, 0.0, 0.0, 0.0])
    nt, active, P, N = E.tiles_of(sc, a)
    passes, rank_corners, exact, und, state = E.tile_counts(active, P, N, lim, nt)
    lanes = int(active.sum())
    decided = int((active & (state != 0)).sum())
    print("headline sample: %d lanes, %d decided (%.2f %%), tiles with an undecided lane %d of %d" % (lanes, decided, 100.0 * decided / lanes, int((und > 0).sum()), nt))
    assert lanes > 10000 and decided >= 0.9 * lanes
