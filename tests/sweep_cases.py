"""The yardstick, the scenes and the radii of the swept-sphere tests (tests/test_sweeps_host.py on the CPU,
tests/test_gpu_sweeps.py and tests/sweep_device_checks.py on the device).

The yardstick is a chain, not an oracle export: the march of mdh_spherecast written in numpy float32 -- one separate
product, sum and difference per operation -- whose distance D comes from the oracle in batches over the rays still alive:
ray_query_cases.orc_closest for the whole scene (the partition's lookup, or the scan without one), Eval_Distances_To with
the shaders' division for listed kinds.  tests/test_sweeps_host.py holds the chain itself: at radius 0 it is
orc_probe_raycast, bit for bit."""
import numpy as np

import ray_query_cases as rq
import ref64_cases
from helpers import SEED, SMALL_PROBES
from madarch_amd import _binding as B

EPS, MAX_DIST = rq.EPS, rq.MAX_DIST
RADII = (0.0, 0.05, 0.3)
NO_INSTANCE = np.float32(1.0e10)  # the scan's initial closest


def seeded_radii(n, seed=SEED + 61):
    """a radius per ray: a fifth of them 0, the rest up to 0.4"""
    rng = np.random.RandomState(seed & 0x7FFFFFFF)
    r = rng.uniform(0.0, 0.4, n).astype(np.float32)
    r[rng.rand(n) < 0.2] = 0.0
    return r


def per_ray(v, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (n,)))


def whole_scene(orc, Ro):
    """D of the whole scene: points -> (distance, index) of partitioning_closest_info"""
    return lambda pts: rq.orc_closest(orc, Ro, pts)


def all_kinds(Ro):
    return [p for p, _ in Ro.Scene.Prims_Count]


def listed(Ro, kinds):
    """D of listed kinds: points -> (distance, normal) of Eval_Distances_To with the shaders' division"""
    def D(pts):
        ada = Ro.Get_Option(B.OPT_ADA_EVAL_DIV)
        Ro.Set_Option(B.OPT_ADA_EVAL_DIV, 0)
        try:
            return Ro.Eval_Distances_To(pts, kinds)
        finally:
            Ro.Set_Option(B.OPT_ADA_EVAL_DIV, ada)
    return D


def chain(D, org, drs, radius=0.0, tmax=None):
    """mdh_spherecast's loop for all rays at once, every operation one binary32 operation:
          for (total = 0; total < tmax;) { dist = D (org + dir * total) - radius; ++steps;
                                           if (dist < EPS) hit at t = total; if (total + dist == total) miss; total += dist }
    D (points) -> (distance, ..).  -> {hit, t, steps, position}; t and position 0 on a miss"""
    n = len(org)
    org, drs = np.asarray(org, np.float32), np.asarray(drs, np.float32)
    rho = per_ray(radius, n)
    tmax = per_ray(MAX_DIST if tmax is None else tmax, n)
    total, t = np.zeros(n, np.float32), np.zeros(n, np.float32)
    steps, hit = np.zeros(n, np.int32), np.zeros(n, np.int32)
    alive = total < tmax
    rounds = 0
    while alive.any():
        ix = np.nonzero(alive)[0]
        dist = (np.asarray(D(rq.march_point(org[ix], drs[ix], total[ix]))[0], np.float32) - rho[ix]).astype(np.float32)
        steps[ix] += 1
        h = dist < EPS
        hit[ix[h]] = 1
        t[ix[h]] = total[ix[h]]
        alive[ix[h]] = False
        go, step = ix[~h], dist[~h]
        with np.errstate(invalid="ignore", over="ignore"):
            new = (total[go] + step).astype(np.float32)
            alive[go] = (new != total[go]) & (new < tmax[go])  # (the stall guard, then the loop's test; a NaN ends the loop)
        total[go] = new
        rounds += 1
    on = hit != 0
    return {"hit": hit, "t": t, "steps": steps, "position": np.where(on[:, None], rq.march_point(org, drs, t), np.float32(0.0)), "rounds": rounds}


def whole_scene_answers(orc, Ro, org, drs, radius=0.0, tmax=None):
    """what mdh_spherecast over the whole scene must return, from the oracle alone: the chain over orc_closest, the index of
    orc_closest at the centre of contact, and there the normal of Eval_Distances_To over all kinds -- whose scan is asserted to
    have the march's distance bits at every hit, as ray_query_cases.oracle_answers does (no coincident primitives)"""
    D = whole_scene(orc, Ro)
    want = chain(D, org, drs, radius, tmax)
    on = want["hit"] != 0
    d, i = D(want["position"])
    assert ((d - per_ray(radius, len(org))).astype(np.float32)[on] < EPS).all()
    dist, nrm = listed(Ro, all_kinds(Ro))(want["position"])
    assert np.array_equal(dist[on], d[on])  # (the same arg-min as the lookup's: the normal is the touched primitive's)
    want["index"] = np.where(on, i, -1).astype(np.int32)
    want["normal"] = np.where(on[:, None], nrm, np.float32(0.0))
    return want


# ------------------------------------------------------------------------------------------------ a scene of four kinds
KIND_BASE = {"Sphere": 0, "Plane": 8, "Box": 16, "Triangle": 24}  # the flat index: the sum of the earlier DECLARED counts
SWEPT_SPHERE = ((1.0, 1.0, 5.0), 0.4)  # the scene's second sphere: the ball of the listed tests


def four_kinds(kinds=None, partition=None):
    """all four built-in kinds, no two primitives coincident: the room's six planes and a slanted one, two spheres, two boxes,
    two triangles.  `kinds`: the instances of these kinds alone (the declaration stays, so the flat indices do);
    `partition`: "Clamp" or "Fallback" -- a grid of unit cells that holds the room"""
    prims = [("Plane", n, o, m) for n, o, m in ref64_cases.ROOM_PLANES] + [("Plane", (0.6, 0.8, 0.0), 0.5, 1)] + [
        ("Sphere", (3.0, 4.0, 3.0), 1.0, 3), ("Sphere",) + SWEPT_SPHERE + (3,), ("Box", (3.0, 0.0, 4.0), (1.5, 1.5, 1.5), 4),
        ("Box", (5.5, 5.0, 1.0), (0.3, 0.9, 0.5), 4)] + [("Triangle", a, b, c, 2) for a, b, c in ref64_cases.TRIANGLES[:2]]
    desc = {"kinds": [("Sphere", 8), ("Plane", 8), ("Box", 8), ("Triangle", 8)],
            "prims": [p for p in prims if kinds is None or p[0] in kinds],
            "light_kinds": [("point", 2)], "lights": [("point", (3.0, 6.0, 1.0), (0.9, 0.9, 0.8))],
            "materials": [((0.7, 0.7, 0.7), 0.0, 0.6)] * 5, "max_dist": 20.0, "cam_pos": (2.0, 2.0, 0.0), "cam_m": np.eye(3), "ao_steps": 3,
            "spec_mode": 2, "probes": ref64_cases.probes_of(SMALL_PROBES)}
    if partition is not None:
        desc["partition"] = {"dims": (8, 8, 13), "spacing": (1.0, 1.0, 1.0), "offset": (-1.0, -1.0, -6.0), "index_count": 20, "border": partition}
    return desc


def make_four_kinds(binding, kinds=None, partition=None, residency=None):
    from madarch_amd import renderers
    R = ref64_cases.make_renderer(four_kinds(kinds, partition), 16, 16, binding)
    if residency is not None:
        R.Set_Option(B.OPT_TABLE_RESIDENCY, residency)
    if partition is not None:
        R.Update_Partitioning(Method=renderers.CPU_Fast)
    return R


def kind_types(names):
    return [ref64_cases.KINDS[k][0] for k in names]


def four_kinds_rays(n, seed=SEED + 67):
    """the room's mixture (ray_query_cases.room_rays: the same room, sphere and box) with a few origins inside the small sphere"""
    org, drs = rq.room_rays(n, seed)
    at = np.arange(3, n, 41)
    rng = np.random.RandomState(seed % 991)
    org[at] = (np.asarray(SWEPT_SPHERE[0]) + rng.uniform(-0.2, 0.2, (len(at), 3))).astype(np.float32)
    return org, drs


def listed_answers(orc, Ro, Ro_listed, names, org, drs, radius=0.0, tmax=None):
    """what mdh_spherecast over the listed kinds must return: the chain over Eval_Distances_To (Ro: the whole scene on the
    oracle), the normal of the same call at the centre of contact, and the index of orc_closest there in Ro_listed -- the scene
    built from the listed kinds' instances alone, partition off: its scan runs in scene order, the listed order is another, and
    without coincident primitives the arg-min is the same -- whose flat indices are the whole scene's (the declaration stays)"""
    D = listed(Ro, kind_types(names))
    want = chain(D, org, drs, radius, tmax)
    on = want["hit"] != 0
    dist, nrm = D(want["position"])
    d, i = rq.orc_closest(orc, Ro_listed, want["position"])
    assert np.array_equal(d[on], dist[on])
    want["index"] = np.where(on, i, -1).astype(np.int32)
    want["normal"] = np.where(on[:, None], nrm, np.float32(0.0))
    return want


# ------------------------------------------------------------------------------------------------ the analytic cases
def ulp32(x):
    return float(np.spacing(np.float32(x)))


def analytic_bounds(gap, scale):
    """a sphere that starts `gap` = (distance to the surface) - radius away and moves straight at it: the loop returns at the
    first dist < EPS, and total is a sum of distances that never overshoot -- gap - EPS - 4 ulp (scale) <= t <= gap + 4 ulp (scale)"""
    return gap - float(EPS) - 4.0 * ulp32(scale), gap + 4.0 * ulp32(scale)


def floor_alone():
    return {"kinds": [("Sphere", 2), ("Plane", 2)], "prims": [("Plane", (0.0, 1.0, 0.0), 0.0, 0)],
            "light_kinds": [("point", 2)], "lights": [("point", (3.0, 6.0, 1.0), (0.9, 0.9, 0.8))],
            "materials": [((0.7, 0.7, 0.7), 0.0, 0.6)] * 2, "max_dist": 20.0, "cam_pos": (2.0, 2.0, 0.0), "cam_m": np.eye(3), "ao_steps": 3,
            "spec_mode": 2, "probes": ref64_cases.probes_of(SMALL_PROBES)}


def sphere_alone(radius):
    d = floor_alone()
    d["prims"] = [("Sphere", (0.0, 0.0, 0.0), radius, 0)]
    return d


DROPS = ((1.0, 0.0), (2.5, 0.3), (7.3, 0.05), (0.75, 0.25), (12.0, 1.5))      # (height h, radius rho)
APPROACHES = ((1.0, 5.0, 0.0), (0.5, 3.3, 0.3), (2.0, 9.1, 0.7), (0.25, 1.0, 0.05))  # (the scene's sphere R, distance L, radius rho)


def drop_rays():
    org = np.array([(0.3 * k, h, -0.2 * k) for k, (h, _) in enumerate(DROPS)], np.float32)
    return org, np.tile(np.array([(0.0, -1.0, 0.0)], np.float32), (len(DROPS), 1)), np.array([r for _, r in DROPS], np.float32)
