"""MDH_TWIN_FOLDED (shade_structured, mdh_march.h): the claim behind what a sharing wavefront's first corner loop no longer
computes per lane at a corner folded along y or z, restated in numpy float32.

Per lane and cage corner i the loop computes

    q = cage_probe (gp, i);  pw = grid_to_world (q);  hvec = pw - P;  dist = length (hvec);  vd = hvec / dist
    vis = the visibility ray's outcome -- for a corner with i & folded the bit of corner i & ~folded
    angle = (dot (vd, N) + 1) / 2;  weight = angle^2 + 0.2;  weight *= vis;  weight < 0.2: weight *= weight^2 / 0.04

with folded's bit a set where the cell lies outside the probe grid along axis a, so that the clamp of cage_probe names one probe
for both corners along a.  Everything below is the device code operation for operation: float32 after every operation, no
contraction, dot as (x x + y y) + z z, the square root and the divisions correctly rounded.

The test shows, for every value of folded from 0 to 7 (cells at both ends of every grid axis, one and two cells outside, and
inside), that corner i and corner i & ~folded name the same probe and produce the same 32-bit patterns of position, direction,
distance and weight; and that the loop as it is written now -- x-twins from the corner in front (twin_prev), y and z twins from
the four kept weights w_fold[i & 3] and the copied visibility bit -- hands every corner the bits of the loop that computes all
eight corners for itself."""
import itertools

import numpy as np
import pytest

from test_shared_taps_claim import ODD, POW2, Probes, bits, cage_probe, world_to_grid

F = np.float32
CRUSH = F(0.2)


def grid_to_world(pr, q):
    return [q[0].astype(np.float32) * pr.sx, q[1].astype(np.float32) * pr.sy, q[2].astype(np.float32) * pr.sz]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def direction(pr, gp, i, P):
    """cage_probe, grid_to_world, the difference, its length and the normalisation of corner i"""
    q = cage_probe(pr, gp, i)
    pw = grid_to_world(pr, q)
    hvec = [pw[k] - P[k] for k in range(3)]
    dist = np.sqrt(dot(hvec, hvec))
    vd = [h / dist for h in hvec]
    assert all(v.dtype == np.float32 for v in pw + hvec + vd) and dist.dtype == np.float32
    return q, pw, dist, vd


def weight_of(vd, N, vis):
    """render_probes.glsl:26-33 as the loop writes it: the weight before the trilinear factor"""
    angle = (dot(vd, N) + F(1.0)) * F(0.5)
    w = angle * angle + F(0.2)
    w = w * vis
    w = np.where(w < CRUSH, w * (w * w * (F(1.0) / (CRUSH * CRUSH))), w).astype(np.float32)
    return w


def folded_of(pr, gp):
    return (((gp[0] < 0) | (gp[0] >= pr.gx - 1)) * 1 + ((gp[1] < 0) | (gp[1] >= pr.gy - 1)) * 2 + ((gp[2] < 0) | (gp[2] >= pr.gz - 1)) * 4).astype(np.int64)


def cells(pr):
    """per axis: two and one cell below the grid, its first and second cell, one in the middle, its last cell inside, the first
    one on and the first beyond its upper face -- every combination of the three axes, so every folded from 0 to 7"""
    per_axis = [sorted({-2, -1, 0, 1, g // 2, g - 2, g - 1, g}) for g in (pr.gx, pr.gy, pr.gz)]
    return np.array(list(itertools.product(*per_axis)), np.int64)


def wavefronts(pr, seed):
    """one wavefront of 64 points per cell: points inside the cell, one normal, and per-corner march outcomes"""
    rng = np.random.RandomState(seed)
    cell = cells(pr)
    n = len(cell)
    inside = (0.05 + 0.9 * rng.rand(n, 64, 3)).astype(np.float32)
    P = ((cell[:, None, :] + inside) * np.array([pr.sx, pr.sy, pr.sz], np.float32)).astype(np.float32)
    P = [P[..., k] for k in range(3)]
    gp = world_to_grid(pr, P)
    keep = np.all([(gp[k] == cell[:, None, k]).all(axis=1) for k in range(3)], axis=0)  # (a product that rounded into the next cell: no uniform tile)
    assert keep.sum() > 0.9 * n
    free = rng.randn(n, 3).astype(np.float32)
    free = (free / np.sqrt((free * free).sum(axis=1, keepdims=True))).astype(np.float32)
    axes = np.eye(3, dtype=np.float32)[rng.randint(0, 3, n)] * rng.choice([-1.0, 1.0], n).astype(np.float32)[:, None]
    N = np.where((np.arange(n) % 2 == 0)[:, None], axes, free).astype(np.float32)
    N = [np.repeat(N[:, None, k], 64, axis=1) for k in range(3)]
    marched = rng.rand(n, 64, 8) < 0.6  # what a corner's own visibility march would find, per lane
    sel = lambda a: a[keep]
    return [sel(g) for g in gp], [sel(p) for p in P], [sel(c) for c in N], sel(marched), sel(cell)


def literal_loop(pr, gp, P, N, marched):
    """the loop with MDH_REUSE_FOLDED alone: every corner computes its own term; a folded one takes its twin's visibility bit"""
    folded = folded_of(pr, gp)
    vis_bits = np.zeros(gp[0].shape, np.int64)
    out = []
    for i in range(8):
        q, pw, dist, vd = direction(pr, gp, i, P)
        twin_bit = (vis_bits >> (i & ~folded)) & 1
        vis = np.where((i & folded) != 0, twin_bit, marched[..., i].astype(np.int64))
        w = weight_of(vd, N, vis.astype(np.float32))
        vis_bits |= (vis != 0).astype(np.int64) << i
        out.append((q, pw, dist, vd, w))
    return out, vis_bits, folded


@pytest.mark.parametrize("geometry", [POW2, ODD], ids=["pow2", "odd"])
def test_a_folded_corner_is_its_twin_bit_for_bit(geometry):
    pr = Probes(seed=7, **geometry)
    gp, P, N, marched, cell = wavefronts(pr, 23)
    terms, vis_bits, folded = literal_loop(pr, gp, P, N, marched)
    assert set(np.unique(folded)) == set(range(8))  # every combination of folds
    for a, g in enumerate((pr.gx, pr.gy, pr.gz)):  # both ends of every axis, outside and the last cell inside
        assert {-2, -1, 0, g - 2, g - 1, g} <= set(cell[:, a])
    rows = np.arange(folded.shape[0])[:, None], np.arange(64)[None, :]
    for i in range(8):
        b = i & ~folded  # [wavefront][lane]
        for what in range(5):
            mine = terms[i][what]
            for k in range(3) if what in (0, 1, 3) else [None]:
                x = mine[k] if k is not None else mine
                twin = np.stack([(terms[c][what][k] if k is not None else terms[c][what]) for c in range(8)], axis=-1)
                y = twin[rows[0], rows[1], b]
                if what == 0:
                    assert np.array_equal(x, y), (i, "probe")
                else:
                    assert np.array_equal(bits(x), bits(y)), (i, what)
        assert np.array_equal((vis_bits >> i) & 1, (vis_bits >> b) & 1)


@pytest.mark.parametrize("geometry", [POW2, ODD], ids=["pow2", "odd"])
def test_the_loop_with_kept_weights_is_the_literal_loop(geometry):
    """The loop of a sharing wavefront as written: `folds` = the y and z bits of the wavefront's folded (one scalar), corner i
    with i & folds reads w_fold[(folds & 2) ? i & 1 : i & 3] and copies bit i & ~folds; an odd corner folded along x takes the
    corner in front; every corner leaves its weight in w_fold[i & 3]."""
    pr = Probes(seed=9, **geometry)
    gp, P, N, marched, _ = wavefronts(pr, 29)
    terms, want_bits, folded = literal_loop(pr, gp, P, N, marched)
    assert (folded == folded[:, :1]).all()  # (one cell per wavefront)
    folds = folded[:, :1] & 6
    vis_bits = np.zeros(gp[0].shape, np.int64)
    w_fold = [np.zeros(gp[0].shape, np.float32) for _ in range(4)]
    w_keep = np.zeros(gp[0].shape, np.float32)
    computed = np.zeros(8, np.int64)
    for i in range(8):
        _, _, _, vd = direction(pr, gp, i, P)
        twin_fold = np.broadcast_to((i & folds) != 0, vis_bits.shape)
        twin_prev = ~twin_fold & bool(i & 1) & ((folded & 1) != 0)
        vis_own = np.where((i & folded) != 0, (vis_bits >> (i & ~folded)) & 1, marched[..., i].astype(np.int64))  # (the loop's own code, MDH_REUSE_FOLDED)
        w_own = weight_of(vd, N, vis_own.astype(np.float32))
        w_twin = np.where((folds & 2) != 0, w_fold[i & 1], w_fold[i & 3])
        bit_twin = (vis_bits >> (i & ~folds)) & 1
        bit_prev = (vis_bits >> max(i - 1, 0)) & 1
        w = np.where(twin_fold, w_twin, np.where(twin_prev, w_keep, w_own)).astype(np.float32)
        bit = np.where(twin_fold, bit_twin, np.where(twin_prev, bit_prev, (vis_own != 0).astype(np.int64)))
        vis_bits |= bit << i
        assert np.array_equal(bits(w), bits(terms[i][4])), i
        w_keep = w
        w_fold[i & 3] = w
        computed[i] = (~twin_fold & ~twin_prev).sum()
    assert np.array_equal(vis_bits, want_bits)
    assert computed[0] == vis_bits.size and (computed[1:] < vis_bits.size).all() and (computed[1:] > 0).all()  # (both paths ran at every corner)
