"""The host side of MDH_OPT_TRIANGLE_BVH through mdh_bvh_build (no renderer, no device): the hierarchy's structure, which
triangles go to the always-evaluated list, and a float64 walk that prunes with the returned margins."""
import numpy as np
import pytest

import bvh_scenes as S
from helpers import SEED, seeded_points
from madarch_amd import meshes

MESHES = {
    "n0": lambda: np.zeros((0, 3, 3), dtype=np.float32),
    "n1": lambda: S.fan(1),
    "n2": lambda: S.fan(2),
    "n5": lambda: S.fan(5),
    "torus200": lambda: meshes.torus(10, 10),
    "torus1000": lambda: meshes.torus(),
    "degenerate": S.degenerate_mesh,
    "coincident": S.coincident_mesh,
}
_built = {}


def built(name):
    if name not in _built:
        tris = MESHES[name]()
        _built[name] = (tris,) + S.bvh_build(tris)
    return _built[name]


def subtree_ranges(nodes):
    """[first, end) of the permutation below every node (depth-first order: a subtree's leaves are contiguous)"""
    first = np.zeros(len(nodes), dtype=np.int64)
    end = np.zeros(len(nodes), dtype=np.int64)
    at = 0
    for i, nd in enumerate(nodes):
        first[i] = at
        if nd["leaf"] >= 0:
            assert nd["leaf"] >> 3 == at
            at += nd["leaf"] & 7
    for i, nd in enumerate(nodes):
        end[i] = first[nd["skip"]] if nd["skip"] < len(nodes) else at
    return first, end


@pytest.mark.parametrize("name", sorted(MESHES))
def test_structure(name):
    tris, nodes, perm, always, delta, rho = built(name)
    n = len(tris)
    assert sorted(np.concatenate((perm, always)).tolist()) == list(range(n))
    assert delta > 0.0 and rho > 0.0
    if len(perm) == 0:
        assert len(nodes) == 0
        return
    assert len(nodes) <= 2 * n and nodes[0]["skip"] == len(nodes)  # the root's skip link ends the walk
    first, end = subtree_ranges(nodes)
    assert end[0] == len(perm)
    covered = np.zeros(len(perm), dtype=np.int64)
    t64 = tris.astype(np.float64)
    for i, nd in enumerate(nodes):
        assert i < nd["skip"] <= len(nodes)  # forward
        if nd["leaf"] >= 0:
            cnt = nd["leaf"] & 7
            assert 1 <= cnt <= 4 and nd["skip"] == i + 1
            covered[first[i]:first[i] + cnt] += 1
        else:
            assert nd["leaf"] == -1 and nd["skip"] > i + 2  # two children at least
        v = t64[perm[first[i]:end[i]]].reshape(-1, 3)
        assert len(v) and (v >= nd["lo"].astype(np.float64)).all() and (v <= nd["hi"].astype(np.float64)).all()
    assert (covered == 1).all()


def test_always_evaluated_list():
    _, _, _, always, _, _ = built("degenerate")
    assert sorted(always.tolist()) == [18, 19]  # the zero-area triangle and the sliver, nothing else
    for name in ("torus200", "torus1000", "n5", "coincident"):
        assert len(built(name)[3]) == 0, name
    bad = S.fan(3)
    bad[1, 2, 0] = np.nan
    bad[2, 0, 1] = np.inf
    assert sorted(S.bvh_build(bad)[2].tolist()) == [1, 2]


@pytest.mark.parametrize("name", ["torus1000", "degenerate", "n5"])
def test_two_builds_give_equal_bytes(name):
    tris = MESHES[name]()
    a, b = S.bvh_build(tris), S.bvh_build(tris.copy())
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3:] == b[3:]


@pytest.mark.parametrize("name", ["torus1000", "torus200", "degenerate", "coincident"])
def test_float64_walk_never_prunes_a_closer_triangle(name):
    """the kernels' walk in numpy over 2 000 seeded points at once: value = the float64 distance, a node is skipped when its
    box is farther than closest (1 + rho) + delta; no skipped subtree may hold a triangle below the running minimum"""
    tris, nodes, perm, always, delta, rho = built(name)
    lo, hi = tris.reshape(-1, 3).min(0) - 1.5, tris.reshape(-1, 3).max(0) + 1.5
    P = seeded_points(2000, lo, hi, SEED).astype(np.float64)
    D = np.concatenate([S.tri_distance64(P[i:i + 250], tris) for i in range(0, len(P), 250)])
    closest = np.full(len(P), 20.0)
    for i in always:
        closest = np.minimum(closest, D[:, i])
    first, end = subtree_ranges(nodes)
    resume = np.zeros(len(P), dtype=np.int64)  # the node a point's walk goes on at
    pruned_nodes = 0
    for i, nd in enumerate(nodes):
        here = resume <= i
        q = np.maximum(np.maximum(nd["lo"].astype(np.float64) - P, P - nd["hi"].astype(np.float64)), 0.0)
        prune = here & (np.sqrt((q * q).sum(1)) > closest * (1.0 + rho) + delta)
        below = D[np.ix_(prune, perm[first[i]:end[i]])]
        assert (below.min(axis=1) >= closest[prune]).all() if below.size else True
        resume[prune] = nd["skip"]
        pruned_nodes += int(prune.sum())
        visit = here & ~prune
        if nd["leaf"] >= 0:
            for j in perm[first[i]:first[i] + (nd["leaf"] & 7)]:
                closest[visit] = np.minimum(closest[visit], D[visit, j])
    assert np.array_equal(closest, np.minimum(D.min(axis=1), 20.0))  # the brute-force minimum
    if name.startswith("torus"):
        assert pruned_nodes > 0  # (a walk that never prunes proves nothing)


def threshold_mesh(rng, n=80):
    """triangles around what the builder admits: the sine of their smallest angle between 2^-7 and 2^-2, edges from
    2^-11 to 30, placed out to +-50"""
    L = 2.0 ** rng.uniform(-11.0, 5.0, n)
    ang = 2.0 ** rng.uniform(-7.0, -2.0, n)
    base = rng.uniform(-1.0, 1.0, (n, 3)) * rng.choice([1.0, 10.0, 50.0], (n, 1))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    far = (u * np.cos(ang)[:, None] + w * np.sin(ang)[:, None]) * (L * rng.uniform(0.3, 1.0, n))[:, None]
    return np.stack((base, base + u * L[:, None], base + far), 1).astype(np.float32)


def probe_points(rng, tris, lim):
    """points that look for the face branch's weak spots: above foot points inside a triangle, above its corners and edges a
    hair outside, from 1e-4 to 10 away; then points all around and far away"""
    P = [rng.uniform(-1.5, 1.5, (300, 3)) * lim, rng.uniform(-1.0, 1.0, (60, 3)) * 1.0e4, rng.uniform(-1.0, 1.0, (20, 3)) * 1.0e6]
    for k in range(0, len(tris), max(1, len(tris) // 24)):
        a, b, c = tris[k].astype(np.float64)
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        foot = rng.dirichlet((1.0, 1.0, 1.0), 24) @ np.stack((a, b, c))
        h = rng.uniform(-1.0, 1.0, (24, 1)) * 10.0 ** rng.uniform(-4.0, 1.0, (24, 1))
        P.append(foot + n * h)
        for corner, other in ((a, b), (b, c), (c, a)):
            out = rng.normal(size=(8, 3)) * 10.0 ** rng.uniform(-7.0, -3.0, (8, 1)) * np.linalg.norm(other - corner)
            P.append(corner + n * h[:8] + out)
            P.append(corner + (other - corner) * rng.uniform(0.0, 1.0, (8, 1)) + n * h[8:16] + out)
    return np.concatenate(P).astype(np.float32)


@pytest.mark.parametrize("trial", range(12))
def test_fp32_value_respects_the_bound_the_margin_rests_on(trial):
    """mdh_device.h's margin argument on the CPU: for every triangle the builder admits to the walk, sd_triangle in fp32
    (bvh_scenes.sd_triangle32, the kernel's operations one by one) is at least D (1 - 2^-19) - 2^-12 lim, D the float64
    distance and lim the largest coordinate -- the inequality the comment derives, from which rho and delta follow.  And the
    kernels' walk in fp32, pruning per point (a wavefront's ballot prunes less), gives the bits of the fp32 scan."""
    rng = np.random.RandomState((SEED + 104729 * trial) & 0x7FFFFFFF)
    tris = S.fuzz_mesh(100 + trial) if trial < 4 else threshold_mesh(rng)
    nodes, perm, always, delta, rho = S.bvh_build(tris)
    assert len(perm) >= len(tris) // 4  # (a mesh the builder rejects wholesale checks nothing)
    lim = float(np.abs(tris[perm]).max())
    P = probe_points(rng, tris[perm], lim)
    d32 = np.concatenate([S.sd_triangle32(tris, P[i:i + 400]) for i in range(0, len(P), 400)])
    D = np.concatenate([S.tri_distance64(P[i:i + 400], tris[perm]) for i in range(0, len(P), 400)])
    got = d32[:, perm].astype(np.float64)
    ok = ~np.isnan(got)  # (a NaN value changes no minimum)
    floor = D * (1.0 - 2.0 ** -19) - 2.0 ** -12 * lim
    worst = float((floor - got)[ok].max() / (2.0 ** -12 * lim))
    print("worst (bound - value) / (2^-12 lim): %.4f" % worst)
    assert (got[ok] >= floor[ok]).all()
    # the walk, fp32 as in bvh_triangles
    f = np.float32
    scan = np.fmin(np.where(np.isnan(d32), f(np.inf), d32).min(axis=1), f(20.0)).astype(f)
    closest = np.full(len(P), 20.0, dtype=f)
    for i in always:
        closest = np.fmin(closest, d32[:, i])
    resume = np.zeros(len(P), dtype=np.int64)
    at = 0
    for i, nd in enumerate(nodes):
        here = resume <= i
        q = np.fmax(np.fmax(nd["lo"] - P, P - nd["hi"]), f(0.0))
        d2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        thr = closest * f(1.0 + rho) + f(delta)
        with np.errstate(over="ignore"):
            need = ~(thr < 0) & ~(d2 > thr * thr)
        resume[here & ~need] = nd["skip"]
        if nd["leaf"] >= 0:
            v = here & need
            for j in perm[at:at + (nd["leaf"] & 7)]:
                closest[v] = np.fmin(closest[v], d32[v, j])
            at += nd["leaf"] & 7
    assert np.array_equal(closest, scan)
