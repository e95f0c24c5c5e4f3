"""MDH_INFO_CULL (closest_primitive_info, mdh_device.h) restated in numpy float32: the typed arg-min of a hit point -- the six
folded planes as candidates, then every sphere and every box behind closest_primitive's two wave-ballot culls -- against the scan
in scene order (scenes.adb:631-674: the first of equal distances).  Index and distance must be equal bit for bit.

A culled candidate has d > closest strictly in every lane of its wavefront, so it can neither win nor tie under the candidates'
rule (closer, or as close with a lower flat index); a NaN keeps the sphere needed, and the box's maxNum drops a NaN component in the
cull and in the distance alike.  Wavefronts are 64 consecutive points of
one place (a wall, a face, an edge ...), as an 8x8 tile's hit points are.

Scenes: the room's census, and three built for ties -- a sphere tangent to a wall, a box face in a wall's plane, two boxes
sharing a face -- each with its kinds declared in two orders, so that a tie goes to a plane in one and to a solid in the other.
The test also holds that both culls fired on at least half of the wall points: it cannot pass with dead code."""
import numpy as np
import pytest

f32 = np.float32
MAX_DIST = f32(20.0)
K1 = f32(1.000001)
WALLS = [(1, 1, 1.0), (1, -1, 7.0), (0, 1, 1.0), (0, -1, 7.0), (2, 1, 6.0), (2, -1, 7.0)]  # (axis, sign, offset): sign * x[axis] + offset

SCENES = {
    "room": dict(spheres=[((3.0, 4.0, 3.0), 1.0)], boxes=[((3.0, 0.0, 4.0), (1.5, 1.5, 1.5))]),
    "tangent_sphere": dict(spheres=[((0.0, 4.0, 3.0), 1.0)], boxes=[((3.0, 0.0, 4.0), (1.5, 1.5, 1.5))]),  # touches the wall x = -1
    "box_in_wall": dict(spheres=[((3.0, 4.0, 3.0), 1.0)], boxes=[((3.0, 0.5, 4.0), (1.5, 1.5, 1.5))]),  # its lower face is the floor y = -1
    "twin_boxes": dict(spheres=[((3.0, 4.0, 3.0), 1.0)], boxes=[((2.0, 0.0, 4.0), (1.0, 1.5, 1.5)), ((4.0, 0.0, 4.0), (1.0, 1.5, 1.5))]),  # share x = 3
}
ORDERS = [("plane", "sphere", "box"), ("box", "sphere", "plane")]


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def build(scene, order):
    """Flat indices by declaration order of the kinds, as primitive_info counts them."""
    sp = np.array([list(c) + [r] for c, r in scene["spheres"]], f32).reshape(-1, 4)
    bx = np.array([list(c) + list(e) for c, e in scene["boxes"]], f32).reshape(-1, 6)
    count = dict(plane=len(WALLS), sphere=len(sp), box=len(bx))
    base, at = {}, 0
    for k in order:
        base[k] = at
        at += count[k]
    return dict(spheres=sp, boxes=bx, base=base, order=order)


def d_plane(g, x):
    a, s, o = WALLS[g]
    return (x[:, a] if s > 0 else -x[:, a]) + f32(o)


def d_sphere(s, x):
    v = s[:3] - x
    return np.sqrt(dot(v, v)) - s[3]


def d_box(b, x):
    q = np.abs(b[:3] - x) - b[3:]
    qp = np.fmax(q, f32(0))  # (max_ and min_ are maxNum and minNum: a NaN component is dropped, as on the device)
    return np.sqrt(dot(qp, qp)) + np.fmin(np.fmax(q[:, 0], np.fmax(q[:, 1], q[:, 2])), f32(0))


def scene_order_scan(sc, x):
    """closest_primitive_info's scan in scene order: d < closest takes, so the first of equal distances stays."""
    closest = np.full(len(x), MAX_DIST, f32)
    index = np.full(len(x), -1, np.int64)
    with np.errstate(invalid="ignore"):
        for kind in sc["order"]:
            n = dict(plane=len(WALLS), sphere=len(sc["spheres"]), box=len(sc["boxes"]))[kind]
            for i in range(n):
                d = d_plane(i, x) if kind == "plane" else d_sphere(sc["spheres"][i], x) if kind == "sphere" else d_box(sc["boxes"][i], x)
                take = d < closest
                closest = np.where(take, d, closest)
                index = np.where(take, sc["base"][kind] + i, index)
    return closest, index


def typed_argmin(sc, x, cull, fired):
    """The typed arg-min over wavefronts of 64 points; `fired` [n, 2] is set where the wavefront skipped the spheres / the boxes."""
    n = len(x)
    assert n % 64 == 0
    closest = np.full(n, MAX_DIST, f32)
    best = np.full(n, -1, np.int64)

    def cand(d, i, lanes):
        nonlocal closest, best
        with np.errstate(invalid="ignore"):
            take = lanes & ((d < closest) | ((d == closest) & (best >= 0) & (i < best)))
        closest = np.where(take, d, closest)
        best = np.where(take, i, best)

    everyone = np.ones(n, bool)
    for g in range(6):
        cand(d_plane(g, x), sc["base"]["plane"] + g, everyone)
    wave = lambda need: np.repeat(need.reshape(-1, 64).any(axis=1), 64)  # noqa: E731  (__ballot (need) != 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, s in enumerate(sc["spheres"]):
            lanes = everyone
            if cull:
                tsum = closest + s[3]
                v = s[:3] - x
                lanes = wave(~(tsum < 0) & ~(dot(v, v) > (tsum * tsum) * K1))
                fired[:, 0] &= ~lanes
            cand(d_sphere(s, x), sc["base"]["sphere"] + i, lanes)
        for i, b in enumerate(sc["boxes"]):
            lanes = everyone
            if cull:
                q = np.abs(b[:3] - x) - b[3:]
                m = np.fmax(q[:, 0], np.fmax(q[:, 1], q[:, 2]))  # (maxNum: a NaN component of q is dropped -- such a lane can still cull the box)
                thr = np.where(closest > 0, closest * K1, closest)
                lanes = wave(~(m > thr))
                fired[:, 1] &= ~lanes
            cand(d_box(b, x), sc["base"]["box"] + i, lanes)
    return closest, best


def points(scene, rng):
    """[(place, points)]: every place a multiple of 64 points, so that a wavefront holds one place."""
    out = []
    lo, hi = np.array([-1.0, -1.0, -6.0]), np.array([7.0, 7.0, 7.0])
    for g, (a, s, o) in enumerate(WALLS):  # on the walls: 8x8 patches, as a tile's hit points lie
        for _ in range(6):
            c = lo + rng.random(3) * (hi - lo)
            p = c + (rng.random((64, 3)) - 0.5) * 0.05
            p[:, a] = -s * o
            out.append(("wall", p))
    for c, r in scene["spheres"]:
        for _ in range(4):
            v = rng.normal(size=3); v /= np.linalg.norm(v)
            d = v + (rng.random((64, 3)) - 0.5) * 0.1
            out.append(("sphere", np.array(c) + r * d / np.linalg.norm(d, axis=1, keepdims=True)))
        t = np.array(c) - np.array([r, 0, 0])  # the tangent point's side: exactly on the sphere along -x, and around it
        p = np.tile(t, (64, 1)); p[1:, 1:] += (rng.random((63, 2)) - 0.5) * 1e-3
        out.append(("tangent", p))
    for c, e in scene["boxes"]:
        c, e = np.array(c), np.array(e)
        for ax in range(3):
            for sg in (-1.0, 1.0):
                u = rng.random((64, 3)) * 2 - 1
                u[:, ax] = sg
                out.append(("face", c + u * e))  # faces (the exact face coordinate: distance 0, ties with a coinciding plane or box)
                u2 = u.copy(); u2[:, (ax + 1) % 3] = rng.choice([-1.0, 1.0], 64)
                out.append(("edge", c + u2 * e))
        corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float)
        out.append(("corner", c + np.tile(corners, (8, 1)) * e))
        out.append(("equal", c + np.tile(corners, (8, 1)) * (e + 0.25)))  # outside a corner: equal distances to what mirrors there
    far = lo + 0.001 + rng.random((256, 3)) * 0.01  # deep in a room corner, far from both solids
    out.append(("far", far))
    mid = np.tile((lo + hi) / 2, (64, 1)); mid[:, 0] = 3.0  # exactly between two walls: equal plane distances
    out.append(("equal", mid))
    nan = lo + rng.random((64, 3)) * (hi - lo)
    nan[::7, 1] = np.nan  # a NaN coordinate in some lanes of a wavefront
    out.append(("nan", nan))
    return [(k, p.astype(f32)) for k, p in out]


def bits(a):
    return np.ascontiguousarray(a.astype(f32)).view(np.uint32)


@pytest.mark.parametrize("order", ORDERS, ids=["planes_first", "boxes_first"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_culled_typed_argmin_is_the_scan_in_scene_order(name, order):
    sc = build(SCENES[name], order)
    pts = points(SCENES[name], np.random.default_rng(23))
    x = np.concatenate([p for _, p in pts])
    place = np.concatenate([[k] * len(p) for k, p in pts])
    assert len(x) >= 3000 and len(x) % 64 == 0
    want_d, want_i = scene_order_scan(sc, x)
    fired = np.ones((len(x), 2), bool)
    for cull in (False, True):
        got_d, got_i = typed_argmin(sc, x, cull, fired)
        assert np.array_equal(got_i, want_i), "%d indices differ (cull %d)" % (int((got_i != want_i).sum()), cull)
        assert np.array_equal(bits(got_d), bits(want_d)), "%d distances differ (cull %d)" % (int((bits(got_d) != bits(want_d)).sum()), cull)
    assert (want_i[place != "nan"] >= 0).all()
    wall = place == "wall"
    assert fired[wall, 0].mean() >= 0.5 and fired[wall, 1].mean() >= 0.5, fired[wall].mean(axis=0)
    assert fired[place == "far"].all()  # both culls fire far from the solids
    nan_rows = np.isnan(x).any(axis=1)
    # a NaN lane keeps the sphere (its d2 is NaN and the test fails open); the box's m drops the NaN component, so such a wavefront
    # may cull the box -- sd_box drops the same component, the index and the distance above are the scan's either way
    assert nan_rows.any() and not fired[np.repeat(nan_rows.reshape(-1, 64).any(axis=1), 64), 0].any()
    ties = {"tangent_sphere": "tangent", "box_in_wall": "face", "twin_boxes": "face"}.get(name)
    if ties:  # the scene's tie is met: some point has two primitives at the winning distance
        d_all = [d_plane(g, x) for g in range(6)] + [d_sphere(s, x) for s in sc["spheres"]] + [d_box(b, x) for b in sc["boxes"]]
        with np.errstate(invalid="ignore"):
            assert ((np.stack(d_all) == want_d[None, :]).sum(axis=0)[place == ties] >= 2).any()
