"""The numpy restatement of segment_clear (scripts/vis_clearance.py): it never clears a segment on which the
float32 march or a dense float32 walk meets an SDF value below EPS, nor one whose exact (fp64) minimum of the SDF lies
below EPS + delta / 2 -- the bound's own rounding is a few 2^-22 lim, far below that margin."""
import importlib.util
import os

import numpy as np
import pytest

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "vis_clearance.py")
_spec = importlib.util.spec_from_file_location("vis_clearance", _PATH)
vc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(vc)

f32 = np.float32


def _scene(rng, scale):
    planes = [(1, 1, 1.0 * scale), (1, -1, 7.0 * scale), (0, 1, 1.0 * scale), (0, -1, 7.0 * scale), (2, 1, 6.0 * scale), (2, -1, 7.0 * scale)]
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    planes.append((tuple(n), float(rng.uniform(2, 4) * scale)))
    spheres = [(tuple(rng.uniform(0, 6, 3) * scale), float(rng.uniform(0.0, 1.0) * scale)) for _ in range(3)]
    ext = rng.uniform(0, 1.2, (3, 3)) * scale
    ext[0, rng.integers(0, 3)] = 0.0  # a zero extent
    boxes = [(tuple(rng.uniform(0, 6, 3) * scale), tuple(e)) for e in ext]
    return vc.scene_arrays(dict(planes=planes, spheres=spheres, boxes=boxes, max_dist=20.0 * scale + 20.0))


def _segments(rng, sc, n, scale):
    """Segments aimed to pass close to the primitives: from random points towards a surface point pushed off by a
    distance of the order of the threshold."""
    A = rng.uniform(-0.5, 6.5, (n, 3)) * scale
    kinds = rng.integers(0, 2, n)
    tgt = np.empty((n, 3))
    for i in range(n):
        if kinds[i] == 0 and len(sc["spheres"]):
            s = sc["spheres"][rng.integers(0, len(sc["spheres"]))]
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            tgt[i] = s[:3] + d * (s[3] + rng.uniform(-0.002, 0.02) * max(1.0, scale))
        else:
            b = sc["boxes"][rng.integers(0, len(sc["boxes"]))]
            corner = np.sign(rng.normal(size=3)) * b[3:]
            tgt[i] = b[:3] + corner * rng.choice([1.0, 1.0, rng.uniform(0, 1)], 3) + rng.uniform(-0.01, 0.01, 3) * max(1.0, scale)
    # the segment passes the target point, which lies somewhere inside it
    d = tgt - A
    L = np.linalg.norm(d, axis=1)
    vd = (d / L[:, None]).astype(f32)
    vmax = (L * rng.uniform(0.5, 2.0, n)).astype(f32)
    return A.astype(f32), vd, vmax


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("scale", [1.0, 40.0, 300.0])
def test_bound_never_clears_a_blocked_segment(seed, scale):
    rng = np.random.default_rng(1000 + seed)
    sc = _scene(rng, scale)
    thr, lim = vc.margins(sc)
    assert thr > 0
    A, vd, vmax = _segments(rng, sc, 600, scale)
    keep = np.all(np.abs(A) <= lim, axis=1)
    clear = vc.segment_clear(sc, thr, lim, A, vd, vmax)
    assert clear.any() and not clear.all()  # the segments straddle the bound
    Ac, vdc, vmc = A[clear], vd[clear], vmax[clear]
    assert (vc.dense_min(sc, Ac, vdc, vmc, samples=1024) >= vc.EPS).all()
    delta = np.ldexp(1.0 + float(lim), -12)
    m64 = vc.segment_min64(sc, Ac, vdc, vmc)
    assert (m64 >= float(vc.EPS) + delta / 2).all(), float(m64.min() - float(vc.EPS) - delta / 2)
    vis, steps, mins = vc.march(sc, Ac, vdc, vmc, vc.sdf(sc, Ac))
    assert vis.all() and (mins >= vc.EPS).all()
    assert keep[clear].all()


def test_bound_fails_closed():
    sc = vc.scene_arrays(vc.ROOM)
    thr, lim = vc.margins(sc)
    A = np.array([[2.0, 2.0, 0.0]] * 4, f32)
    vd = np.array([[0.0, 0.0, 1.0]] * 4, f32)
    vmax = np.array([0.5, np.nan, 0.5, 0.5], f32)
    A[2, 0] = np.nan
    vd[3, 1] = np.inf
    assert vc.segment_clear(sc, thr, lim, A, vd, vmax).tolist() == [True, False, False, False]
    assert not vc.segment_clear(sc, f32(0), lim, A[:1], vd[:1], vmax[:1])[0]  # delta = 0: off
    neg = vc.scene_arrays(dict(vc.ROOM, spheres=[((3.0, 4.0, 3.0), -1.0)]))
    assert vc.margins(neg)[0] == 0
    flat = vc.scene_arrays(dict(vc.ROOM, boxes=[((3.0, 0.0, 4.0), (-0.1, 1.0, 1.0))]))
    assert vc.margins(flat)[0] == 0


def test_headline_room_clears_most_march_steps():
    rng = np.random.default_rng(7)
    sc = vc.scene_arrays(vc.ROOM)
    thr, lim = vc.margins(sc)
    P, N = vc.room_points(rng, 1500)
    A, vd, vmax, _ = vc.visibility_rays(P, N)
    sd0 = vc.sdf(sc, A)
    need = (vmax > 0) & ~(sd0 < vc.EPS) & (sd0 < vmax)
    A, vd, vmax, sd0 = A[need], vd[need], vmax[need], sd0[need]
    clear = vc.segment_clear(sc, thr, lim, A, vd, vmax)
    vis, steps, _ = vc.march(sc, A, vd, vmax, sd0)
    assert not (clear & ~vis).any()
    assert steps[clear].sum() > 0.5 * steps.sum()
    delta = np.ldexp(1.0 + float(lim), -12)
    assert (vc.segment_min64(sc, A[clear], vd[clear], vmax[clear]) >= float(vc.EPS) + delta / 2).all()
