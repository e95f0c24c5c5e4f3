"""MDH_RAY_BOUNDS (mdh_device.h: ray_bounds, closest_primitive) restated in numpy (scripts/ray_bounds_estimate.py), float32,
the kernel's operations: two numbers per ray, hs and hb, below the sphere's and the box's distance at every position the
march can evaluate.  Held along float32 marches of scripts/vis_clearance.py's sdf, more than 10^5 rays over three scenes:

    wherever a bound exceeds the running minimum `closest` -- where the kernel may skip the solid's block -- the float32
    distance of that solid at that position is >= closest (min_raw(closest, d) would have returned closest), and the float64
    distance at the ideal point o + d * total exceeds closest by at least half the margin: the margin E = 2^-14 (lim + tmax)
    (the box's: E (1 + 2 (e_x + e_y + e_z) / |q|)) less an error budget of half of it.

Ray families: random rays from inside the room; rays tangent to the sphere within 1e-3 .. 1e-6; rays along and just off the
box's faces, edges and corners; rays that start on the sphere or the box and leave (the clamped parameter); origins beyond
lim; non-unit, zero, infinite and NaN directions (the bounds must be off: NaN).  And in the room, from the headline camera's
tiles, the sphere bound must skip at least half of the blocks that today's cull skips, so that a bound that never fires fails."""
import importlib.util
import os

import numpy as np
import pytest

_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")


def _load(name):
    import sys
    if _DIR not in sys.path:
        sys.path.insert(0, _DIR)
    spec = importlib.util.spec_from_file_location(name, os.path.join(_DIR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("ray_bounds_estimate")
V = R.V
f32 = np.float32

SCENES = {
    "room": V.ROOM,
    "tangent_sphere": dict(V.ROOM, spheres=[((0.0, 4.0, 3.0), 1.0)]),
    "box_in_wall": dict(V.ROOM, boxes=[((3.0, 0.5, 4.0), (1.5, 1.5, 1.5))]),
}


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def perpendicular(rng, n):
    """a random unit vector perpendicular to each row of n"""
    v = np.cross(n, rng.normal(size=n.shape))
    return unit(v)


def families(scene, rng):
    """{family: (origins, directions)} in float64; the marches run their float32 roundings"""
    c, r = (np.array(v, float) for v in scene["spheres"][0])
    bc, be = (np.array(v, float) for v in scene["boxes"][0])
    lo, hi = np.array([-1.0, -1.0, -6.0]), np.array([7.0, 7.0, 7.0])
    out = {}
    n = 20000
    out["random"] = (lo + 0.01 + rng.rand(n, 3) * (hi - lo - 0.02), unit(rng.normal(size=(n, 3))))
    n = 4096  # through a point within 1e-3 .. 1e-6 of the sphere's surface, inside and outside, along a tangent there
    nrm = unit(rng.normal(size=(n, 3)))
    off = 10.0 ** rng.uniform(-6, -3, n) * rng.choice([-1.0, 1.0], n)
    T = c + nrm * (r + off)[:, None]
    u = perpendicular(rng, nrm)
    out["tangent"] = (T - u * rng.uniform(0.0, 3.0, (n, 1)), u)
    n = 6144  # along and just off the box's faces (2048), edges (2048) and corners (2048)
    sg = rng.choice([-1.0, 1.0], (n, 3))
    on = sg * be * np.where(rng.rand(n, 3) < 0.5, 1.0, rng.rand(n, 3))  # a point of the box whose coordinates are at the faces or inside
    kind = np.repeat([1, 2, 3], n // 3)
    ax = rng.randint(0, 3, n)
    for k in range(n):  # kind 1: one coordinate on its face; 2: two (an edge); 3: all three (a corner)
        fixed = [(ax[k] + j) % 3 for j in range(kind[k])]
        on[k, fixed] = sg[k, fixed] * be[fixed]
    off = 10.0 ** rng.uniform(-6, -3, (n, 1)) * rng.choice([-1.0, 0.0, 1.0], (n, 1))
    through = bc + on + sg * off
    dirs = rng.normal(size=(n, 3))
    rows = np.arange(n)
    dirs[rows[kind == 1], ax[kind == 1]] = 0.0  # within the face's plane
    edge = kind == 2
    dirs[edge] = 0.0
    dirs[rows[edge], (ax[edge] + 2) % 3] = 1.0  # along the edge
    dirs = unit(dirs)
    out["box_features"] = (through - dirs * rng.uniform(0.0, 3.0, (n, 1)), dirs)
    n = 4096  # leaving the sphere and the box from their surfaces
    nrm = unit(rng.normal(size=(n, 3)))
    d = unit(nrm + 0.9 * rng.normal(size=(n, 3)))
    d = np.where((np.sum(d * nrm, axis=1) < 0)[:, None], -d, d)
    out["leave_sphere"] = (c + nrm * (r + 2e-3), d)
    face = rng.randint(0, 3, n)
    p = (rng.rand(n, 3) * 2 - 1) * be
    s = rng.choice([-1.0, 1.0], n)
    p[np.arange(n), face] = s * (be[face] + 2e-3)
    d = unit(rng.normal(size=(n, 3)))
    flip = np.sign(d[np.arange(n), face]) != s
    d[flip] = -d[flip]
    out["leave_box"] = (bc + p, d)
    n = 1024
    o = (rng.rand(n, 3) * 2 - 1) * 40.0
    o[np.arange(n), rng.randint(0, 3, n)] = rng.choice([-1.0, 1.0], n) * rng.uniform(16.001, 60.0, n)
    out["beyond_lim"] = (o, unit(np.array([3.0, 3.0, 3.0]) - o + rng.normal(size=(n, 3))))
    n = 1024
    o = lo + 0.01 + rng.rand(n, 3) * (hi - lo - 0.02)
    d = unit(rng.normal(size=(n, 3)))
    q = n // 4
    d[:q] *= np.where(rng.rand(q, 1) < 0.5, rng.uniform(0.2, 0.999, (q, 1)), rng.uniform(1.001, 4.0, (q, 1)))
    d[q:2 * q] = 0.0
    d[2 * q:3 * q][np.arange(q), rng.randint(0, 3, q)] = np.inf
    d[3 * q:][np.arange(n - 3 * q), rng.randint(0, 3, n - 3 * q)] = np.nan
    out["bad_directions"] = (o, d)
    return out


OFF = ("beyond_lim", "bad_directions")  # families whose bounds must be off


def march_and_check(sc, lim, o, d, hs, hb, max_steps=192):
    """march_plain per ray in float32 (at most max_steps evaluations: a prefix of the march's positions); the claim at every
    evaluation.  Returns the number of sphere and of box blocks the bounds skip (per lane)."""
    o = o.astype(f32); d = d.astype(f32)
    tmax = sc["max_dist"]
    E = float((lim + tmax) * R.MARGIN)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    c64, r64 = sc["spheres"][0][:3].astype(np.float64), float(sc["spheres"][0][3])
    b64, e64 = sc["boxes"][0][:3].astype(np.float64), sc["boxes"][0][3:].astype(np.float64)
    se = 2.0 * float(e64.sum())
    total = np.zeros(len(o), f32)
    live = np.ones(len(o), bool)
    skipped = [0, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(max_steps):
            idx = np.nonzero(live)[0]
            if not len(idx):
                break
            x = (o[idx] + d[idx] * total[idx, None]).astype(f32)
            c, d2, ds, m, db = R.sdf_parts(sc, x)
            p64 = o64[idx] + d64[idx] * total[idx, None].astype(np.float64)
            ks = hs[idx] > c
            assert np.all(ds[ks] >= c[ks]), "sphere: float32 distance below closest behind the bound"
            ds64 = np.linalg.norm(p64[ks] - c64, axis=1) - r64
            assert np.all(ds64 >= c[ks].astype(np.float64) + 0.5 * E), "sphere: float64 slack %g below E / 2 = %g" % (float((ds64 - c[ks]).min()), 0.5 * E)
            c1 = np.minimum(c, ds).astype(f32)
            kb = hb[idx] > c1
            assert np.all(db[kb] >= c1[kb]), "box: float32 distance below closest behind the bound"
            q64 = np.abs(p64[kb] - b64) - e64
            db64 = np.linalg.norm(np.maximum(q64, 0.0), axis=1) + np.minimum(q64.max(axis=1), 0.0)
            # the ray's own margin E (1 + 2 sum(e) / |q|), |q| its closest-point vector's length: not below E
            assert np.all(db64 >= c1[kb].astype(np.float64) + 0.5 * E), "box: float64 slack %g below E / 2 = %g" % (float((db64 - c1[kb]).min()), 0.5 * E)
            skipped[0] += int(ks.sum()); skipped[1] += int(kb.sum())
            sd = np.minimum(c1, db).astype(f32)
            assert np.array_equal(sd, V.sdf(sc, x), equal_nan=True)  # (the parts are vis_clearance's sdf)
            h = sd < V.EPS
            total[idx[~h]] = total[idx[~h]] + sd[~h]
            live[idx] = ~h & (total[idx] < tmax)
    return skipped, se


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_skipped_block_is_never_below_closest(name):
    sc = V.scene_arrays(SCENES[name])
    thr, lim = V.margins(sc)
    assert thr > 0 and lim == 16.0
    fam = families(SCENES[name], np.random.RandomState(26))
    assert sum(len(o) for o, _ in fam.values()) * len(SCENES) >= 100000
    for key, (o, d) in sorted(fam.items()):
        hs, hb = R.ray_bounds(sc, thr, lim, o, d, sc["max_dist"])
        if key in OFF:
            assert np.all(np.isnan(hs)) and np.all(np.isnan(hb)), key
        else:
            assert np.isfinite(hs).mean() > 0.99, key  # (unit directions inside lim: the bounds are on)
        skipped, _ = march_and_check(sc, lim, o, d, hs, hb)
        print(name, key, len(o), "rays; sphere and box blocks skipped:", skipped)
        if key == "random":
            assert skipped[0] > 10000 and skipped[1] > 10000, skipped


def test_the_bounds_are_off_for_scenes_without_segment_clear():
    bad = dict(V.ROOM, spheres=[((3.0, 4.0, 3.0), -1.0)])
    sc = V.scene_arrays(bad)
    thr, lim = V.margins(sc)
    assert thr == 0
    o, d = families(bad, np.random.RandomState(1))["random"]
    hs, hb = R.ray_bounds(sc, thr, lim, o[:256], d[:256], sc["max_dist"])
    assert np.all(np.isnan(hs)) and np.all(np.isnan(hb))
    sc = V.scene_arrays(V.ROOM)
    thr, lim = V.margins(sc)
    for tmax in (np.inf, np.nan, -1.0):  # a non-finite or negative tmax fails closed: -inf or NaN, never above a finite closest
        hs, hb = R.ray_bounds(sc, thr, lim, o[:256], d[:256], f32(tmax))
        assert not np.any(hs > -np.inf) and not np.any(hb > -np.inf), tmax


def test_the_sphere_bound_fires_where_todays_cull_does():
    """the headline camera's tiles (every 12th along x and y), wavefront by wavefront: the condition of the issue, and the
    claim again at wavefront granularity -- every position at which a block is skipped for the whole tile"""
    sc = V.scene_arrays(V.ROOM)
    thr, lim = V.margins(sc)
    tiles = np.array([(x, y) for y in range(0, 135, 12) for x in range(0, 240, 12)])
    check = []
    c0, c1 = R.frame(sc, thr, lim, 1920, 1080, (2.0, 2.0, 0.0), 0.0, 0.0, tiles, check)
    today = int(c0["sphere_today"].sum() + c1["sphere_today"].sum())
    bound = int(c0["sphere_bound"].sum() + c1["sphere_bound"].sum())
    box_today = int(c0["box_today"].sum() + c1["box_today"].sum())
    box_bound = int(c0["box_bound"].sum() + c1["box_bound"].sum())
    print("sphere blocks skipped per tile: today %.2f, by the bound %.2f; box: today %.2f, by the bound %.2f"
          % (today / len(tiles), bound / len(tiles), box_today / len(tiles), box_bound / len(tiles)))
    assert today > 0 and 2 * bound >= today
    assert box_bound > 0
    for what, x, c, dist in check:
        assert np.all(dist >= c), what
