"""Scenes and probe-visibility segments at the edge of segment_clear's bound (mdh_device.h), for
tests/test_gpu_vis_clearance_device.py (the device's bound and march against the numpy restatement, scripts/vis_clearance.py)
and the host-only checks of tests/test_vis_clearance_bound.py.

A scene is the restatement's description (axis planes as (axis, sign, offset), general planes as (normal, offset)).
Segments are built as the kernels build them -- vd = fl(h / fl(|h|)) in float32 -- and most pass a surface at a distance
g in [EPS - delta, EPS + 3 delta]: tangent to a sphere, parallel to a wall, over a box face, past a box edge or corner, or
starting next to a wall (a probe on a wall).  Edge cases follow: starts inside a primitive, vmax <= 0, long vmax,
endpoints at the coordinate bound lim, NaN and infinities."""
import importlib.util
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "vis_clearance.py")
_spec = importlib.util.spec_from_file_location("vis_clearance", _PATH)
vc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(vc)

f32 = np.float32
EPS = float(vc.EPS)


SCALE_K = {1: (1.0, 0.0), 40: (5.0, 0.0), 300: (2.0, 290.0)}  # scale -> (k, t)


def _affine(k, t):
    """the map x -> k x + t of a unit scene (coordinates in [-1, 7]) to scale ~1 (k 1), ~40 (k 5) or ~300 (k 2, t 290)"""
    return lambda x: tuple(float(k * v + t) for v in x)


def room_scene(rng, scale):
    """the rooms' census: six axis walls, one sphere, one box"""
    k, t = SCALE_K[scale]
    X = _affine(k, t)
    lo, hi = -rng.uniform(0.5, 1.5, 3), 6.0 + rng.uniform(0.0, 1.0, 3)
    lo, hi = k * lo + t, k * hi + t
    planes = [(a, 1, float(-lo[a])) for a in range(3)] + [(a, -1, float(hi[a])) for a in range(3)]
    r = float(rng.choice([0.0, rng.uniform(0.2, 1.2)])) * k
    e = rng.uniform(0.0, 1.5, 3) * k
    e[rng.integers(0, 3)] *= float(rng.integers(0, 2))  # sometimes a zero extent
    return dict(planes=planes, spheres=[(X(rng.uniform(1.0, 5.0, 3)), r)], boxes=[(X(rng.uniform(1.0, 5.0, 3)), tuple(float(v) for v in e))],
                max_dist=20.0 * k + 20.0)


def general_scene(rng, scale):
    """2-6 spheres, 2-4 boxes, tilted planes beside the walls, zero radii and zero extents"""
    d = room_scene(rng, scale)
    k, t = SCALE_K[scale]
    X = _affine(k, t)
    for _ in range(int(rng.integers(1, 3))):
        n = np.abs(rng.normal(size=3)) + 0.2; n /= np.linalg.norm(n)
        c = np.array(X(rng.uniform(-0.5, 0.5, 3)))  # a plane that cuts off a corner of the room
        d["planes"].append((tuple(float(v) for v in n), float(-np.dot(n, c))))
    d["spheres"] = [(X(rng.uniform(0.5, 5.5, 3)), float(rng.choice([0.0, rng.uniform(0.1, 1.0)])) * k) for _ in range(int(rng.integers(2, 7)))]
    ext = rng.uniform(0.0, 1.2, (int(rng.integers(2, 5)), 3)) * k
    ext[0, rng.integers(0, 3)] = 0.0
    d["boxes"] = [(X(rng.uniform(0.5, 5.5, 3)), tuple(float(v) for v in e)) for e in ext]
    return d


def _tangent(rng, nrm):
    """unit vectors perpendicular to the rows of nrm"""
    v = rng.normal(size=nrm.shape)
    v -= nrm * np.einsum("ij,ij->i", v, nrm)[:, None]
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _finish(rng, A64, E64):
    """float32 segments from A to E as the kernels build them: h = E - A, vd = h / |h|, vmax = |h| (or a little less)"""
    A = A64.astype(f32)
    h = (E64.astype(f32) - A).astype(f32)
    dist = np.sqrt(vc.dot(h, h)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        vd = (h / dist[:, None]).astype(f32)
    vmax = np.where(rng.random(len(A)) < 0.7, dist, (dist - vc.MIN_STEP * f32(5)).astype(f32)).astype(f32)
    return A, vd, vmax


def grazing(rng, sc, n, delta, k):
    """n segments, each passing one surface at a distance drawn from [EPS - delta, EPS + 3 delta] (k: the scene's scale)"""
    g = rng.uniform(EPS - delta, EPS + 3 * delta, n)
    L = rng.uniform(0.02, 0.3, (n, 2)) * k
    feat = rng.choice(6, n, p=[0.25, 0.25, 0.15, 0.15, 0.12, 0.08])  # wall, sphere, face, edge, corner, wall start
    P = np.zeros((n, 3)); nrm = np.zeros((n, 3))
    off = sc["off"].astype(np.float64)
    lo, hi = -off[0::2], off[1::2]
    # walls: a point of a wall, its inward normal
    m = (feat == 0) | (feat == 5)
    w = rng.integers(0, 6, m.sum())
    Pw = rng.uniform(lo + 0.7 * k, hi - 0.7 * k, (m.sum(), 3))
    a, neg = w // 2, w % 2
    Pw[np.arange(len(w)), a] = np.where(neg, hi[a], lo[a])
    Nw = np.zeros_like(Pw); Nw[np.arange(len(w)), a] = np.where(neg, -1.0, 1.0)
    P[m], nrm[m] = Pw, Nw
    # spheres: a point of the surface
    m = feat == 1
    if len(sc["spheres"]):
        s = sc["spheres"][rng.integers(0, len(sc["spheres"]), m.sum())].astype(np.float64)
        u = rng.normal(size=(m.sum(), 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        P[m], nrm[m] = s[:, :3] + u * s[:, 3:4], u
    else:
        feat[m] = 0
    # boxes: a point of a face, an edge or a corner, with the outward (bisecting) normal
    m = (feat >= 2) & (feat <= 4)
    b = sc["boxes"][rng.integers(0, len(sc["boxes"]), m.sum())].astype(np.float64)
    sg = rng.choice([-1.0, 1.0], (m.sum(), 3))
    u = rng.uniform(-1.0, 1.0, (m.sum(), 3))
    kind = feat[m] - 1  # axes pinned to the box's surface: 1 face, 2 edge, 3 corner
    pin = np.argsort(rng.random((m.sum(), 3)), axis=1) < kind[:, None]
    u = np.where(pin, sg, u)
    Nb = np.where(pin, sg, 0.0); Nb /= np.linalg.norm(Nb, axis=1, keepdims=True)
    P[m], nrm[m] = b[:, :3] + u * b[:, 3:], Nb
    # the segment: tangent through P + g nrm, or (wall start) from P + g nrm into the room
    Q = P + nrm * g[:, None]
    T = _tangent(rng, nrm)
    A64 = Q - T * L[:, :1]
    E64 = Q + T * L[:, 1:]
    m = feat == 5
    E64[m] = Q[m] + (nrm[m] + 0.7 * T[m]) * L[m, 1:]
    A64[m] = Q[m]
    flip = rng.random(n) < 0.5  # either direction
    A64[flip], E64[flip] = E64[flip].copy(), A64[flip].copy()
    return _finish(rng, A64, E64)


def edge_cases(rng, sc, lim):
    """starts inside primitives, vmax <= 0, long vmax, endpoints at +-lim, NaN and infinities"""
    A, vd, vmax = [], [], []
    def add(a, d, v):
        A.append(np.asarray(a, f32)); vd.append(np.asarray(d, f32)); vmax.append(f32(v))
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=3)).astype(f32)
    for s in sc["spheres"]:
        for v in (0.0, 0.5, 3.0):
            add(s[:3], unit(), v)
    for b in sc["boxes"]:
        for v in (0.0, 0.5, 3.0):
            add(b[:3] + b[3:] * f32(0.5), unit(), v)
    mid = np.where(np.isfinite(sc["off"][0::2]) & np.isfinite(sc["off"][1::2]), (sc["off"][1::2] - sc["off"][0::2]) / 2, 0.0).astype(f32)
    for v in (0.0, -0.0, -1.0, -1e30, 1e-30, 1e4, 1e7, 3e38, np.inf, -np.inf, np.nan):
        add(mid, unit(), v)
    L = f32(lim)
    for x in (L, np.nextafter(L, f32(0)), np.nextafter(L, f32(np.inf)), -L, -np.nextafter(L, f32(np.inf))):
        a = mid.copy(); a[0] = x
        add(a, (0, 1, 0), 0.5)
        add(mid, (1, 0, 0), f32(x - mid[0]))  # B.x = fl(mid.x + (x - mid.x)) lands at or next to x
        add(mid, (-1, 0, 0), f32(x + mid[0]))
    for bad in (np.nan, np.inf, -np.inf):
        for c in range(3):
            a = mid.copy(); a[c] = bad
            add(a, unit(), 1.0)
            d = unit(); d[c] = bad
            add(mid, d, 1.0)
        add(mid, (0, 0, 0), 1.0)
        add(mid, (bad, bad, bad), 0.0)
    return np.array(A, f32), np.array(vd, f32), np.array(vmax, f32)


def segments(rng, sc, n, k):
    """n grazing segments and the edge cases behind them (k: the scene's scale, SCALE_K)"""
    thr, lim = vc.margins(sc)
    delta = float(np.ldexp(1.0 + float(lim), -12))
    A, vd, vmax = grazing(rng, sc, n, delta, k)
    eA, evd, evm = edge_cases(rng, sc, lim)
    return np.concatenate([A, eA]), np.concatenate([vd, evd]), np.concatenate([vmax, evm])


def bands(sc, A, vd, vmax):
    """the exact minimum of each segment (fp64; NaN where the inputs are not finite or vmax <= 0) and its band:
    0 below EPS - delta, 1 in [EPS - delta, EPS + 3 delta], 2 above"""
    thr, lim = vc.margins(sc)
    delta = float(np.ldexp(1.0 + float(lim), -12))
    ok = np.all(np.isfinite(A), axis=1) & np.all(np.isfinite(vd), axis=1) & np.isfinite(vmax) & (vmax > 0) & (vmax < 1e6)
    m = np.full(len(A), np.nan)
    m[ok] = vc.segment_min64(sc, A[ok], vd[ok], vmax[ok])
    band = np.where(m < EPS - delta, 0, np.where(m <= EPS + 3 * delta, 1, 2))
    return m, band, delta
