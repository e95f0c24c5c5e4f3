"""The yardstick of the swept-sphere tests, held on the CPU (no device): the chain of tests/sweep_cases.py -- the march of
mdh_spherecast in numpy float32 over the oracle's distances -- is the oracle's own raycast at radius 0, bit for bit, over
the whole scene and over all kinds listed; larger radii give it something to do; and the bounds the analytic cases of
tests/test_gpu_sweeps.py assert follow from the loop, in float64 and in the chain's float32."""
import numpy as np
import pytest

import ray_query_cases as rq
import sweep_cases as sw
import test_gpu_ray_queries as tq
from helpers import same_bits

N = tq.N
SCENES = ("rooms, LDS scan", "partition, Clamp", "partition, Fallback", "mesh, global residency", "open scene")
NO_PARTITION = ("rooms, LDS scan", "mesh, global residency", "open scene")

_scenes = {}


def scene(orc, name):
    if name not in _scenes:
        _scenes[name] = (tq.CASES[name][1](orc),) + tuple(tq.CASES[name][2](N))
    return _scenes[name]


@pytest.mark.parametrize("name", SCENES)
def test_the_chain_at_radius_0_is_the_oracles_raycast(orc, name):
    Ro, org, drs = scene(orc, name)
    want = rq.orc_raycast(orc, Ro, org, drs)
    got = sw.whole_scene_answers(orc, Ro, org, drs, 0.0, None)
    print("%s: %d rounds of the chain, most steps %d" % (name, got["rounds"], got["steps"].max()))
    for k in ("hit", "index", "steps"):
        assert np.array_equal(got[k], want[k]), k
    assert same_bits(got["t"], want["t"])


@pytest.mark.parametrize("name", NO_PARTITION)
def test_the_listed_chain_over_all_kinds_is_the_oracles_raycast(orc, name):
    Ro, org, drs = scene(orc, name)
    want = rq.orc_raycast(orc, Ro, org, drs)
    got = sw.chain(sw.listed(Ro, sw.all_kinds(Ro)), org, drs, 0.0, None)
    for k in ("hit", "steps"):
        assert np.array_equal(got[k], want[k]), k
    assert same_bits(got["t"], want["t"])


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("radius", sw.RADII[1:])
def test_a_radius_gives_the_chain_contacts_at_once_and_later(orc, name, radius):
    Ro, org, drs = scene(orc, name)
    got = sw.whole_scene_answers(orc, Ro, org, drs, radius, None)  # (asserts the scan's distance bits at every hit)
    hit = got["hit"] != 0
    print("%s, radius %g: %d of %d hit, %d at t = 0, most steps %d" % (name, radius, hit.sum(), N, (hit & (got["t"] == 0.0)).sum(), got["steps"].max()))
    assert hit.sum() >= N * 4 // 10 and (hit & (got["t"] == 0.0) & (got["steps"] == 1)).sum() >= 2 and (hit & (got["t"] > 0.0)).any()


def _loop64(D, org, drs, rho, tmax=20.0):
    """the loop in float64, one ray"""
    total, steps = 0.0, 0
    while total < tmax:
        dist = D(org + drs * total) - rho
        steps += 1
        if dist < float(sw.EPS):
            return True, total, steps
        if total + dist == total:
            break
        total += dist
    return False, 0.0, steps


def test_the_analytic_bounds_follow_from_the_loop():
    """a floor alone, a sphere alone: t lies in [gap - EPS, gap] in exact arithmetic -- the loop returns at the first
    dist < EPS and total never overshoots -- which float64 keeps within 1e-12 and the chain's float32 within 4 ulp of the
    start's distance"""
    down = np.array([0.0, -1.0, 0.0])
    for h, rho in sw.DROPS:
        hit, t, steps = _loop64(lambda p: p[1], np.array([0.3, h, -0.2]), down, rho)
        assert hit and h - rho - float(sw.EPS) - 1e-12 <= t <= h - rho + 1e-12, (h, rho, t)
    for R, L, rho in sw.APPROACHES:
        hit, t, steps = _loop64(lambda p: np.sqrt((p * p).sum()) - R, np.array([0.0, 0.0, -L]), np.array([0.0, 0.0, 1.0]), rho)
        assert hit and L - R - rho - float(sw.EPS) - 1e-12 <= t <= L - R - rho + 1e-12, (R, L, rho, t)
    # the chain itself, over the two distances in float32
    org, drs, rho = sw.drop_rays()
    got = sw.chain(lambda p: (p[:, 1],), org, drs, rho)
    for k, (h, r) in enumerate(sw.DROPS):
        lo, hi = sw.analytic_bounds(h - r, h)
        assert got["hit"][k] == 1 and lo <= float(got["t"][k]) <= hi, (h, r, got["t"][k])
    for R, L, r in sw.APPROACHES:
        def D(p, R=R):
            q = p.astype(np.float32)
            return ((np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) - np.float32(R)).astype(np.float32),)
        got = sw.chain(D, np.array([(0.0, 0.0, -L)], np.float32), np.array([(0.0, 0.0, 1.0)], np.float32), r)
        lo, hi = sw.analytic_bounds(L - R - r, L)
        assert got["hit"][0] == 1 and lo <= float(got["t"][0]) <= hi, (R, L, r, got["t"][0])
