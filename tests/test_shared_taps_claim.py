"""MDH_SHARE_TAPS (shade_structured, mdh_march.h): the claim behind fetching a wavefront's eight irradiance taps once, restated
in numpy float32.

The first point's corner loop computes, per lane and cage corner i,

    q = cage_probe (gp, i);  base = probe_id_to_coord (grid_to_probe_id (q))
    tap = atlas_tap_issue (base + rid_n / probe_count);  tx = atlas_tap_resolve (tap);  s_term = sqrt (tx)
    acc = acc + s_term * weight_i            (i = 0 .. 7, weight_i the lane's own)

with gp = world_to_grid (P) and rid_n the clamped octahedral texel of N.  Where every active lane of a wavefront holds the
same gp and the same bits of N, the lane of rank r computes corner r & 7 once and every lane reads s_term of corner i from
the wavefront's row.  Everything below is the device code operation for operation: float32 after every operation, no
contraction, the RGBA8 decode as fma (k, c_hi, k c_lo), the square root correctly rounded, the texel index as row term +
column term in 32-bit integers.  The test computes a tile's 64 points both ways -- every lane for itself, corner after
corner, from its OWN P and N; and as lane c from the FIRST lane's cell and normal -- and asserts equal bits of every s_term
and of the folded sum, over random cells (folded ones outside the grid included), random axis and free normals, texels
beside the atlas (mirrored repeat) and both kinds of atlas geometry (powers of two, and nothing a power of two).  The tap is
also held against the plain definition: GL_LINEAR with GL_MIRRORED_REPEAT on the 2-D atlas image."""
import numpy as np
import pytest

F = np.float32
I = np.int64
C_HI, C_LO = F(float.fromhex("0x1.010102p-8")), F(float.fromhex("-0x1.fdfdfep-33"))  # 1 / 255 = C_HI + C_LO (u8_unorm)


class Probes:
    """What KProbes holds of the irradiance atlas (mdh_api.hip: probes_of)."""

    def __init__(self, grid, spacing, count, ires, seed):
        self.gx, self.gy, self.gz = grid
        self.sx, self.sy, self.sz = (F(s) for s in spacing)
        self.pcx, self.pcy = count
        assert self.pcx * self.pcy >= self.gx * self.gy * self.gz
        self.ires = ires
        self.irr_lo = F(0.5) / F(ires)
        self.irr_hi = F(1.0) - self.irr_lo
        self.irr_w, self.irr_h = F(self.pcx * ires), F(self.pcy * ires)
        rng = np.random.RandomState(seed)
        # the reference's image, [Y][X] of RGBA8 words, and the library's probe-major store of the same texels
        self.image = rng.randint(0, 1 << 32, size=(self.pcy * ires, self.pcx * ires), dtype=np.uint64).astype(np.uint32)
        self.image[rng.rand(*self.image.shape) < 0.1] = 0  # black texels: sqrt (0)
        Y, X = np.mgrid[0:self.pcy * ires, 0:self.pcx * ires]
        self.store = np.zeros(self.image.size, np.uint32)
        self.store[atlas_index(self, X, Y)] = self.image


def atlas_index(pr, X, Y):
    tx, ty = X // pr.ires, Y // pr.ires
    return ((ty * pr.pcx + tx) * pr.ires + (Y - ty * pr.ires)) * pr.ires + (X - tx * pr.ires)


def u32(x):
    return np.asarray(x, dtype=np.int64) & 0xFFFFFFFF


def atlas_col(pr, X):
    tx = X // pr.ires
    return u32(u32(tx * pr.ires) * pr.ires + (X - tx * pr.ires))


def atlas_row(pr, Y):
    ty = Y // pr.ires
    return u32(u32(u32(ty * pr.pcx) * pr.ires + (Y - ty * pr.ires)) * pr.ires)


def mirror(i, n):
    m = np.mod(i, 2 * n)  # (the general form; the device's shortcuts have its values)
    return np.where(m >= n, 2 * n - 1 - m, m)


def u8_unorm(k):
    k = np.asarray(k).astype(np.float32)
    lo = k * C_LO
    return (k.astype(np.float64) * np.float64(C_HI) + lo.astype(np.float64)).astype(np.float32)  # fma: one rounding (the product is exact in float64)


def texel(word):
    return [u8_unorm(word & 255), u8_unorm((word >> 8) & 255), u8_unorm((word >> 16) & 255)]


def sqrt_cr(x):
    return np.sqrt(x.astype(np.float32))  # IEEE: correctly rounded, as sqrt_unscaled_ and sqrt_ are


def world_to_grid(pr, P):
    return [np.floor(P[k] / s).astype(I) for k, s in enumerate((pr.sx, pr.sy, pr.sz))]


def cage_probe(pr, gp, i):
    return [np.clip(gp[0] + (i & 1), 0, pr.gx - 1), np.clip(gp[1] + ((i >> 1) & 1), 0, pr.gy - 1), np.clip(gp[2] + ((i >> 2) & 1), 0, pr.gz - 1)]


def ray_dir_to_ray_id(N):
    s = F(1.0) / ((np.abs(N[0]) + np.abs(N[1])) + np.abs(N[2]))
    px, py = N[0] * s, N[1] * s
    snz = lambda v: np.where(v >= 0, F(1.0), F(-1.0)).astype(np.float32)
    ox = np.where(N[2] <= 0, (F(1.0) - np.abs(py)) * snz(px), px).astype(np.float32)
    oy = np.where(N[2] <= 0, (F(1.0) - np.abs(px)) * snz(py), py).astype(np.float32)
    return (ox + F(1.0)) * F(0.5), (oy + F(1.0)) * F(0.5)


def clamped_texel_of(pr, N):
    rx, ry = ray_dir_to_ray_id(N)
    return np.fmin(np.fmax(rx, pr.irr_lo), pr.irr_hi), np.fmin(np.fmax(ry, pr.irr_lo), pr.irr_hi)


def tap_coord(pr, gp, i, rid):
    q = cage_probe(pr, gp, np.asarray(i))
    pid = q[2] * pr.gx * pr.gy + q[1] * pr.gx + q[0]
    y = pid // pr.pcx
    x = pid - y * pr.pcx
    bx, by = x.astype(np.float32) / F(pr.pcx), y.astype(np.float32) / F(pr.pcy)
    return bx + rid[0] / F(pr.pcx), by + rid[1] / F(pr.pcy)


def s_term(pr, gp, i, rid, coord=None):
    """atlas_tap_issue, atlas_tap_resolve and the three roots of corner i: a function of the cell, the corner and the texel of N."""
    cx, cy = coord if coord is not None else tap_coord(pr, gp, i, rid)
    W, H = pr.pcx * pr.ires, pr.pcy * pr.ires
    px, py = cx * pr.irr_w - F(0.5), cy * pr.irr_h - F(0.5)
    fx0, fy0 = np.floor(px), np.floor(py)
    fx, fy = px - fx0, py - fy0
    x0, x1, y0, y1 = mirror(fx0.astype(I), W), mirror(fx0.astype(I) + 1, W), mirror(fy0.astype(I), H), mirror(fy0.astype(I) + 1, H)
    c0, c1, r0, r1 = atlas_col(pr, x0), atlas_col(pr, x1), atlas_row(pr, y0), atlas_row(pr, y1)
    idx = [u32(r0 + c0), u32(r0 + c1), u32(r1 + c0), u32(r1 + c1)]
    for k, (X, Y) in zip(idx, ((x0, y0), (x1, y0), (x0, y1), (x1, y1))):
        assert np.array_equal(k, atlas_index(pr, X, Y))  # the sum of a row term and a column term is the index
    a, b, c, d = (texel(pr.store[k].astype(I)) for k in idx)
    w00, w10, w01, w11 = (F(1.0) - fx) * (F(1.0) - fy), fx * (F(1.0) - fy), (F(1.0) - fx) * fy, fx * fy
    out = [sqrt_cr(((a[k] * w00 + b[k] * w10) + c[k] * w01) + d[k] * w11) for k in range(3)]
    assert all(o.dtype == np.float32 for o in out)
    return np.stack(np.broadcast_arrays(*out), axis=-1), (x0, x1, y0, y1, fx, fy)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


POW2 = dict(grid=(8, 8, 8), spacing=(1.0, 1.0, 1.0), count=(32, 16), ires=8)
ODD = dict(grid=(5, 5, 3), spacing=(1.6, 1.9, 2.5), count=(15, 5), ires=6)
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-0.0, 1, 0], [0, -0.0, -1]], np.float32)


def tiles(pr, rng, n):
    """n tiles of 64 points: one cell (up to two cells outside the grid on every side: folded cages) and one normal each."""
    cell = np.stack([rng.randint(-2, g + 1, n) for g in (pr.gx, pr.gy, pr.gz)], axis=1)
    inside = (0.05 + 0.9 * rng.rand(n, 64, 3)).astype(np.float32)
    P = ((cell[:, None, :] + inside) * np.array([pr.sx, pr.sy, pr.sz], np.float32)).astype(np.float32)
    free = rng.randn(n, 3).astype(np.float32)
    free = (free / np.sqrt((free * free).sum(axis=1, keepdims=True))).astype(np.float32)
    N = np.where((np.arange(n) % 2 == 0)[:, None], AXES[rng.randint(0, len(AXES), n)], free).astype(np.float32)
    return cell, P, np.repeat(N[:, None, :], 64, axis=1)


@pytest.mark.parametrize("geometry", [POW2, ODD], ids=["pow2", "odd"])
def test_a_tap_computed_as_lane_c_is_the_lanes_own(geometry):
    pr = Probes(seed=7, **geometry)
    rng = np.random.RandomState(11)
    cell, P, N = tiles(pr, rng, 400)
    n = len(cell)
    # every lane for itself (the loop as it stands): its own P -> gp, its own N -> texel, corner after corner
    gp = world_to_grid(pr, [P[..., k] for k in range(3)])
    keep = np.all([(gp[k] == cell[:, None, k]).all(axis=1) for k in range(3)], axis=0)  # (a product that rounded into the next cell: not a uniform tile)
    assert keep.sum() > 0.9 * n
    rid = clamped_texel_of(pr, [N[..., k] for k in range(3)])
    own = np.stack([s_term(pr, gp, i, rid)[0] for i in range(8)], axis=2)  # [tile][lane][corner][3]
    # the wavefront's pass: rank r takes corner r & 7 from the FIRST lane's cell and normal; ranks 0 .. 7 store
    rank = np.arange(64)
    first_gp = [np.repeat(g[:, :1], 64, axis=1) for g in gp]
    first_rid = clamped_texel_of(pr, [np.repeat(N[:, :1, k], 64, axis=1) for k in range(3)])
    as_lane, _ = s_term(pr, first_gp, rank[None, :] & 7, first_rid)  # [tile][lane][3]
    slots = as_lane[:, :8, :]
    assert np.array_equal(bits(as_lane), bits(np.tile(slots, (1, 8, 1))))  # whichever lane computes corner c: one value
    for i in range(8):
        assert np.array_equal(bits(own[keep][:, :, i, :]), bits(np.repeat(slots[keep][:, i:i + 1, :], 64, axis=1))), i
    # a corner folded onto an earlier one names that one's probe: its slot holds the same triple (twin_prev reuses it)
    folded = ((cell[:, 0] < 0) | (cell[:, 0] >= pr.gx - 1)) * 1 + ((cell[:, 1] < 0) | (cell[:, 1] >= pr.gy - 1)) * 2 + ((cell[:, 2] < 0) | (cell[:, 2] >= pr.gz - 1)) * 4
    assert (folded != 0).sum() >= 20 and (folded == 0).sum() >= 20  # (the generator gave both kinds of cell)
    for i in range(8):
        twin = i & ~folded
        assert np.array_equal(bits(slots[np.arange(n), i]), bits(slots[np.arange(n), twin]))
    # the fold: per-lane weights, order i = 0 .. 7
    w = rng.rand(n, 64, 8).astype(np.float32)
    acc_own = np.zeros((n, 64, 3), np.float32)
    acc_shared = np.zeros((n, 64, 3), np.float32)
    for i in range(8):
        acc_own = acc_own + own[:, :, i, :] * w[:, :, i, None]
        acc_shared = acc_shared + slots[:, None, i, :] * w[:, :, i, None]
    assert np.array_equal(bits(acc_own[keep]), bits(acc_shared[keep]))


def test_what_the_decision_compares_is_what_the_tap_reads():
    """The decision compares gp and the bit patterns of N.  Equal bits of N give equal texels (a function of N alone); a lane
    in the next cell names other probes, so the cell must be compared; and the decision is allowed to refuse more than it must
    (a normal that differs in the sign of a zero may well name the same texel: it is not asked)."""
    pr = Probes(seed=3, **ODD)
    rng = np.random.RandomState(17)
    N = rng.randn(3, 1000).astype(np.float32)
    a, b = clamped_texel_of(pr, list(N)), clamped_texel_of(pr, [n.copy() for n in N])
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert (a[0] >= pr.irr_lo).all() and (a[0] <= pr.irr_hi).all() and (a[1] >= pr.irr_lo).all() and (a[1] <= pr.irr_hi).all()
    rid = (a[0][:1], a[1][:1])
    g0, g1 = [np.array([1]), np.array([1]), np.array([1])], [np.array([2]), np.array([1]), np.array([1])]
    assert not np.array_equal(tap_coord(pr, g0, 0, rid)[0], tap_coord(pr, g1, 0, rid)[0])
    for i in range(8):  # ... while corner i | 1 of a cell is corner i & ~1 of its right-hand neighbour: the same probe
        if i & 1:
            assert np.array_equal(tap_coord(pr, g0, i, rid)[0], tap_coord(pr, g1, i & ~1, rid)[0])


@pytest.mark.parametrize("geometry", [POW2, ODD], ids=["pow2", "odd"])
def test_the_tap_is_gl_linear_with_mirrored_repeat(geometry):
    """Coordinates over the whole image and half a texel beyond every edge: the four texels and their weights are those of
    GL_LINEAR on the 2-D image with GL_MIRRORED_REPEAT, read through the probe-major store."""
    pr = Probes(seed=5, **geometry)
    rng = np.random.RandomState(13)
    W, H = pr.pcx * pr.ires, pr.pcy * pr.ires
    cx = np.concatenate([rng.uniform(-0.6 / W, 1 + 0.6 / W, 4000), [0.0, 1.0, 0.25 / W, 1 - 0.25 / W]]).astype(np.float32)
    cy = np.concatenate([rng.uniform(-0.6 / H, 1 + 0.6 / H, 4000), [1.0, 0.0, 1 - 0.25 / H, 0.25 / H]]).astype(np.float32)
    got, (x0, x1, y0, y1, fx, fy) = s_term(pr, None, None, None, coord=(cx, cy))
    assert (x0 == x1).any() and (y0 == y1).any()  # taps beside the image: both texels are the edge's
    want = []
    for k in range(3):
        t = lambda X, Y: u8_unorm((pr.image[Y, X].astype(I) >> (8 * k)) & 255)
        top = t(x0, y0) * ((F(1.0) - fx) * (F(1.0) - fy)) + t(x1, y0) * (fx * (F(1.0) - fy))
        want.append(np.sqrt((top + t(x0, y1) * ((F(1.0) - fx) * fy)) + t(x1, y1) * (fx * fy)))
    assert np.array_equal(bits(got), bits(np.stack(want, axis=-1)))
    # k / 255 for every byte, correctly rounded
    k = np.arange(256)
    assert np.array_equal(bits(u8_unorm(k)), bits((k / 255.0).astype(np.float32)))
