"""null_light (mdh_device.h, MDH_SKIP_NULL_BRDF): the claim behind skipping the BRDF of a light, restated in numpy float32.

The light loop of compute_direct_lighting (shade_structured, mdh_march.h) computes, per light and shaded point,

    radiance = sample_light (...);  NdotL = max_ (dot (N, L), 0);  cook_torrance (...) -> kD, kS
    B = kD * albedo / PI + kS;  contrib = (B * radiance) * NdotL
    shadows = softshadows (...) if NdotL > EPS and contrib != 0, else 0
    Lo = Lo + contrib * shadows

and null_light says, before cook_torrance, that the last line leaves Lo's bits alone.  Everything below is the device
code operation for operation: float32 after every operation, min_ / max_ as minNum / maxNum (np.fmin / np.fmax), dot as
(x x' + y y') + z z', no contraction.  For every input where the predicate holds the test asserts that B is finite and
that Lo + contrib * shadows has Lo's bits, with the parent's own `shadows`."""
import itertools

import numpy as np
import pytest

F = np.float32
PI = F(3.14159265358)
EPS = F(0.001)
INF = F(np.inf)
NAN = F(np.nan)
TINY = F(2.0 ** -149)


def _f(x):
    return np.asarray(x, dtype=np.float32)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def length(a):
    return np.sqrt(dot(a, a))


def max_(a, b):
    return np.fmax(a, b)


def min_(a, b):
    return np.fmin(a, b)


def mix_(x, y, a):
    return x * (F(1.0) - a) + y * a


def pow5_(x):
    x2 = x * x
    return (x2 * x2) * x


def pow8_(x):
    x2 = x * x
    x4 = x2 * x2
    return x4 * x4


def acos_(x):
    ax = np.abs(x)
    p = F(-0.0012624911)
    for c in (0.0066700901, -0.0170881256, 0.0308918810, -0.0501743046, 0.0889789874, -0.2145988016, 1.5707963050):
        p = p * ax + F(c)
    r = np.sqrt(F(1.0) - ax) * p
    return np.where(x < F(0.0), F(3.14159265358979) - r, r)


def sample_point(lpos, colour, pos):
    d = [lpos[i] - pos[i] for i in range(3)]
    dist = length(d)
    L = [d[i] / dist for i in range(3)]
    den = (dist * dist) * F(0.03)
    return L, dist, [colour[i] / den for i in range(3)]


def sample_spot(lpos, aperture, sdir, colour, pos):
    d = [lpos[i] - pos[i] for i in range(3)]
    dist = length(d)
    L = [d[i] / dist for i in range(3)]
    attenuation = F(1.0) / ((dist * dist) * F(0.03))
    theta = acos_(max_(dot([-L[0], -L[1], -L[2]], sdir), F(0.0)))
    ratio = min_(max_(theta / aperture, F(0.0)), F(1.0))
    visible = F(1.0) - pow8_(ratio)
    a = min_(attenuation, F(1.5))
    return L, dist, [(colour[i] * a) * visible for i in range(3)]


def cook_torrance(N, V, L, NdotL, albedo, metallic, roughness):
    VL = [V[i] + L[i] for i in range(3)]
    ln = length(VL)
    H = [VL[i] / ln for i in range(3)]
    NdotV = max_(dot(N, V), F(0.0))
    F0 = [mix_(F(0.04), albedo[i], metallic) for i in range(3)]
    a = roughness * roughness
    a2 = a * a
    NdotH = max_(dot(N, H), F(0.0))
    NdotH2 = NdotH * NdotH
    denom = NdotH2 * (a2 - F(1.0)) + F(1.0)
    denom = PI * denom * denom
    NDF = a2 / denom
    rr = roughness + F(1.0)
    kk = (rr * rr) / F(8.0)
    ggx2 = NdotV / (NdotV * (F(1.0) - kk) + kk)
    ggx1 = NdotL / (NdotL * (F(1.0) - kk) + kk)
    G = ggx1 * ggx2
    p5 = pow5_(F(1.001) - max_(dot(H, V), F(0.0)))
    Fr = [F0[i] + (F(1.0) - F0[i]) * p5 for i in range(3)]
    ng = NDF * G
    numerator = [Fr[i] * ng for i in range(3)]
    denominator = F(4.0) * NdotV * NdotL
    dm = max_(denominator, F(0.001))
    kD = [(F(1.0) - Fr[i]) * (F(1.0) - metallic) for i in range(3)]
    kS = [min_(numerator[i] / dm, F(1.0)) for i in range(3)]
    return kD, kS


def unit_range(x):
    return (x >= F(0.0)) & (x <= F(1.0))


def null_light(V, L, NdotL, radiance, albedo, metallic, roughness):
    mat = unit_range(albedo[0]) & unit_range(albedo[1]) & unit_range(albedo[2]) & unit_range(metallic) & unit_range(roughness)
    VL = [V[i] + L[i] for i in range(3)]
    s = dot(VL, VL)
    brdf_finite = mat & (dot(V, V) <= F(1.0015)) & (s >= F(1e-30)) & (s <= F(3e38))
    dark = (radiance[0] == F(0.0)) & (radiance[1] == F(0.0)) & (radiance[2] == F(0.0)) & (NdotL <= F(2.0))
    away = ~(NdotL > EPS) & (np.abs(radiance[0]) <= F(1e38)) & (np.abs(radiance[1]) <= F(1e38)) & (np.abs(radiance[2]) <= F(1e38))
    return brdf_finite & (dark | away)


def bits(x):
    return _f(x).view(np.uint32)


def check_claim(N, V, L, NdotL, radiance, albedo, metallic, roughness, Lo, marched_shadows):
    """Asserts the claim on every element where the predicate holds, for both settings of cfg.direct_specular;
    returns the predicate."""
    with np.errstate(all="ignore"):
        null = null_light(V, L, NdotL, radiance, albedo, metallic, roughness)
        kD, kS = cook_torrance(N, V, L, NdotL, albedo, metallic, roughness)
        for direct_specular in (True, False):
            ks = kS if direct_specular else [np.zeros_like(kS[i]) for i in range(3)]
            B = [(kD[i] * albedo[i]) / PI + ks[i] for i in range(3)]
            contrib = [(B[i] * radiance[i]) * NdotL for i in range(3)]
            lit = (contrib[0] != F(0.0)) | (contrib[1] != F(0.0)) | (contrib[2] != F(0.0))
            shadows = np.where((NdotL > EPS) & lit, marched_shadows, F(0.0)).astype(np.float32)
            for i in range(3):
                assert np.isfinite(B[i][null]).all(), "B is not finite under the predicate"
                assert (np.abs(B[i][null]) < F(1.33)).all(), "B leaves the bound the overflow argument uses"
                new = Lo[i] + contrib[i] * shadows
                same = (bits(new) == bits(Lo[i])) | (np.isnan(new) & np.isnan(Lo[i]))
                assert same[null].all(), "Lo changes under the predicate at %d inputs" % (~same[null]).sum()
    return null


def _unit(rng, n):
    v = rng.standard_normal((3, n)).astype(np.float32)
    ln = length(v)
    return [v[i] / ln for i in range(3)]


def _random_inputs(n, seed):
    rng = np.random.RandomState(seed)
    u = lambda lo, hi, *shape: (lo + (hi - lo) * rng.rand(*(shape or (n,)))).astype(np.float32)
    pos = [u(-1.0, 7.0), u(-1.0, 7.0), u(-7.0, 6.0)]
    N = _unit(rng, n)
    V = _unit(rng, n)
    lpos = [u(-1.0, 7.0), u(-1.0, 7.0), u(-7.0, 6.0)]
    colour = [u(0.0, 1.0), u(0.0, 1.0), u(0.0, 1.0)]
    sdir = _unit(rng, n)
    aperture = u(0.2, 1.5)
    albedo = [u(0.0, 1.0), u(0.0, 1.0), u(0.0, 1.0)]
    metallic, roughness = u(0.0, 1.0), u(0.0, 1.0)
    # the corners of the material range, and materials outside it
    for arr in albedo + [metallic, roughness]:
        pick = rng.rand(n)
        arr[pick < 0.05] = F(0.0)
        arr[(pick >= 0.05) & (pick < 0.10)] = F(1.0)
        arr[(pick >= 0.10) & (pick < 0.11)] = TINY
        arr[(pick >= 0.11) & (pick < 0.12)] = F(np.nextafter(F(1.0), F(2.0)))
        arr[(pick >= 0.12) & (pick < 0.13)] = F(2.5)
        arr[(pick >= 0.13) & (pick < 0.135)] = F(-TINY)
    # adversarial geometry: the light at the point or next to it, huge and non-finite colours, V opposite to L, V not a unit vector
    pick = rng.rand(n)
    for i in range(3):
        lpos[i][pick < 0.01] = pos[i][pick < 0.01]
        near = (pick >= 0.01) & (pick < 0.02)
        lpos[i][near] = pos[i][near] + (u(-1e-3, 1e-3) * N[i])[near]
    pick = rng.rand(n)
    scale = np.ones(n, dtype=np.float32)
    scale[pick < 0.02] = F(1e38)
    scale[(pick >= 0.02) & (pick < 0.03)] = F(3.4e38)
    scale[(pick >= 0.03) & (pick < 0.035)] = INF
    scale[(pick >= 0.035) & (pick < 0.04)] = F(-1e30)
    with np.errstate(all="ignore"):
        colour = [colour[i] * scale for i in range(3)]
        spot = rng.rand(n) < 0.5
        Lp, _, rp = sample_point(lpos, colour, pos)
        Ls, _, rs = sample_spot(lpos, aperture, sdir, colour, pos)
        L = [np.where(spot, Ls[i], Lp[i]) for i in range(3)]
        radiance = [np.where(spot, rs[i], rp[i]) for i in range(3)]
        pick = rng.rand(n)
        opp = pick < 0.02
        jitter = np.where(rng.rand(n) < 0.5, F(0.0), u(-1e-20, 1e-20))
        V = [np.where(opp, -L[i] + jitter, V[i]) for i in range(3)]
        vs = np.ones(n, dtype=np.float32)
        vs[(pick >= 0.02) & (pick < 0.03)] = F(1e19)
        vs[(pick >= 0.03) & (pick < 0.04)] = F(1.01)
        vs[(pick >= 0.04) & (pick < 0.05)] = F(1e-20)
        V = [V[i] * vs for i in range(3)]
        NdotL = max_(dot(N, L), F(0.0))
    Lo = [u(0.0, 2.0), u(0.0, 2.0), u(0.0, 2.0)]
    pick = rng.rand(n)
    for i in range(3):
        Lo[i][pick < 0.2] = F(0.0)
        Lo[i][(pick >= 0.2) & (pick < 0.22)] = F(-0.75)  # (a negative colour makes Lo negative; never -0)
        Lo[i][(pick >= 0.22) & (pick < 0.23)] = INF
        Lo[i][(pick >= 0.23) & (pick < 0.24)] = NAN
    return N, V, L, NdotL, radiance, albedo, metallic, roughness, Lo, u(0.0, 1.0)


def test_random_inputs_keep_lo_and_are_not_vacuous():
    n = 1 << 20  # 1 048 576 >= 10^6
    args = _random_inputs(n, 0x4D414441 & 0x7FFFFFFF)
    null = check_claim(*args)
    albedo, metallic, roughness = args[5], args[6], args[7]
    outside = np.zeros(n, dtype=bool)
    for arr in albedo + [metallic, roughness]:
        outside |= ~((arr >= F(0.0)) & (arr <= F(1.0)))
    assert outside.sum() > n // 50 and not null[outside].any()
    assert null.sum() >= n // 10, "only %d of %d inputs satisfy the predicate" % (null.sum(), n)
    # both clauses take part: dark lights in front of the surface, and lit ones behind it
    NdotL, radiance = args[3], args[4]
    dark = (radiance[0] == 0) & (radiance[1] == 0) & (radiance[2] == 0)
    assert (null & dark & (NdotL > EPS)).sum() >= n // 50
    assert (null & ~dark & ~(NdotL > EPS)).sum() >= n // 50


VECS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (0.6, 0.8, 0.0), (0.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.6, np.nan, 0.8),
        (np.inf, 0.0, 0.0), (0.0, -np.inf, 1.0), (np.inf, np.inf, np.inf), (1e19, 0.0, 0.0), (1e-23, 0.0, 0.0), (-0.6, -0.8, 0.0)]
MAT_VALUES = [0.0, 2.0 ** -149, 0.03, 0.75, 1.0]
NDOTL_VALUES = [0.0, 0.001, np.nextafter(F(0.001), F(0.0)), np.nextafter(F(0.001), F(1.0)), 0.5, 1.0, 2.0, np.nextafter(F(2.0), F(3.0)), np.inf]
RADIANCE_VALUES = [0.0, -0.0, 2.0 ** -149, 3e38, np.inf, -3e38, 1e38, np.nextafter(F(1e38), INF), 0.7, np.nan]


def _edge_grid():
    """N x V x L (every V also against L = -V) x NdotL x radiance, as flat arrays; materials are crossed in by the test."""
    triples = [(n, v, l) for n in (VECS[1], VECS[3], VECS[4], VECS[6], VECS[8], VECS[10]) for v in VECS for l in VECS]
    triples += [(n, v, tuple(-c for c in v)) for n in VECS for v in VECS]
    rad = [(r, r, r) for r in RADIANCE_VALUES] + [(0.0, 0.0, 3e38), (0.0, -0.0, 0.0), (2.0 ** -149, 0.0, 0.0), (0.0, np.inf, 0.0), (1e38, -1e38, 0.5)]
    rows = list(itertools.product(range(len(triples)), NDOTL_VALUES, range(len(rad))))
    t = np.array([r[0] for r in rows])
    ndl = _f([r[1] for r in rows])
    ri = np.array([r[2] for r in rows])
    tv = _f(triples)  # [triple, which, component]
    rv = _f(rad)
    N, V, L = ([tv[t, w, c] for c in range(3)] for w in range(3))
    return N, V, L, ndl, [rv[ri, c] for c in range(3)]


def test_edge_grid_keeps_lo():
    N, V, L, NdotL, radiance = _edge_grid()
    n = NdotL.size
    rng = np.random.RandomState(7)
    marched = rng.rand(n).astype(np.float32)
    marched[::3] = F(1.0)
    Lo = [np.where(np.arange(n) % 4 == 0, F(0.0), F(0.3 + 0.1 * i)).astype(np.float32) for i in range(3)]
    hits = 0
    for alb, met, rough in itertools.product(MAT_VALUES, MAT_VALUES, MAT_VALUES):
        albedo = [np.full(n, alb, dtype=np.float32)] * 3
        null = check_claim(N, V, L, NdotL, radiance, albedo, np.full(n, met, dtype=np.float32), np.full(n, rough, dtype=np.float32), Lo, marched)
        hits += int(null.sum())
    mixed = [np.full(n, 1.0, dtype=np.float32), np.full(n, 0.0, dtype=np.float32), np.full(n, 2.0 ** -149, dtype=np.float32)]
    hits += int(check_claim(N, V, L, NdotL, radiance, mixed, np.full(n, 1.0, dtype=np.float32), np.full(n, 0.0, dtype=np.float32), Lo, marched).sum())
    assert hits > 0


def test_light_at_the_point_is_not_null():
    """dist = 0: L is NaN and the radiance colour / 0; the predicate must refuse (s = dot2 (V + L) is NaN)."""
    one = lambda x: _f([x])
    pos = [one(1.0), one(2.0), one(3.0)]
    with np.errstate(all="ignore"):
        for L, dist, radiance in (sample_point(pos, [one(0.9)] * 3, pos), sample_spot(pos, one(0.7), [one(1.0), one(0.0), one(0.0)], [one(0.9)] * 3, pos),
                                  sample_point(pos, [one(0.0)] * 3, pos)):
            assert dist[0] == 0.0 and np.isnan(L[0][0])
            V = [one(0.0), one(0.0), one(1.0)]
            NdotL = max_(dot(V, L), F(0.0))
            assert not null_light(V, L, NdotL, radiance, [one(0.5)] * 3, one(0.5), one(0.5))[0]


@pytest.mark.parametrize("albedo, metallic, roughness", [
    ((0.5, 0.5, 0.5), 0.0, 1.9), ((0.5, 0.5, 0.5), 0.0, 2.5), ((0.5, 0.5, 0.5), 1.5, 0.5), ((np.nan, 0.5, 0.5), 0.0, 0.5),
    ((0.5, 0.5, np.nan), 0.0, 0.5), ((2.0, 0.5, 0.5), 0.0, 0.5), ((0.5, 0.5, 0.5), np.nan, 0.5), ((0.5, 0.5, 0.5), 0.5, np.nan),
    ((0.5, np.nextafter(F(1.0), F(2.0)), 0.5), 0.5, 0.5), ((0.5, 0.5, 0.5), -2.0 ** -149, 0.5), ((0.5, 0.5, 0.5), 0.5, -2.0 ** -149),
    ((0.5, 0.5, 0.5), np.nextafter(F(1.0), F(2.0)), 0.5), ((0.5, 0.5, 0.5), 0.5, np.nextafter(F(1.0), F(2.0))), ((np.inf, 0.5, 0.5), 0.5, 0.5)])
def test_material_outside_the_range_is_never_null(albedo, metallic, roughness):
    N, V, L, NdotL, radiance = _edge_grid()
    n = NdotL.size
    with np.errstate(all="ignore"):
        null = null_light(V, L, NdotL, radiance, [np.full(n, a, dtype=np.float32) for a in albedo], np.full(n, metallic, dtype=np.float32),
                          np.full(n, roughness, dtype=np.float32))
    assert not null.any()


def test_the_narrowing_conditions_are_needed():
    """Why the predicate asks for more than the material range: each of these has a dark light or NdotL = 0, a material
    inside [0, 1], and a B that is not finite or a contrib * 0 that is NaN -- and the predicate refuses each."""
    one = lambda x: _f([x])
    vec = lambda v: [one(c) for c in v]
    mat = ([one(0.5)] * 3, one(0.0), one(0.5))
    zero = vec((0.0, 0.0, 0.0))
    with np.errstate(all="ignore"):
        # V + L so small that its squared length underflows: H.x = +inf, p5 = -inf
        V, L = vec((1e-23, 1e-23, 1e-23)), vec((0.0, 0.0, 0.0))
        kD, _ = cook_torrance(vec((0.0, 1.0, 0.0)), V, L, one(0.0), *mat)
        assert not np.isfinite(kD[0][0]) and not null_light(V, L, one(0.0), zero, *mat)[0]
        # V far from a unit vector: dot (H, V) = 1e19
        V, L = vec((1e19, 0.0, 0.0)), vec((0.0, 1.0, 0.0))
        kD, _ = cook_torrance(vec((0.0, 1.0, 0.0)), V, L, one(0.0), *mat)
        assert not np.isfinite(kD[0][0]) and not null_light(V, L, one(0.0), zero, *mat)[0]
        # a finite radiance that overflows in B * radiance: inf * (NdotL = 0) is NaN
        N, V, L = vec((0.0, 1.0, 0.0)), vec((0.0, 1.0, 0.0)), vec((0.0, 1.0, 0.0))
        rough = ([one(0.5)] * 3, one(0.0), one(2.0 ** -149))  # (a2 = 0 with NdotH = 1: NDF is 0 / 0, kS = min_ (NaN, 1) = 1)
        kD, kS = cook_torrance(N, V, L, one(0.0), *rough)
        B = (kD[0] * F(0.5)) / PI + kS[0]
        assert np.isfinite(B[0]) and B[0] > 1.0
        radiance = vec((3e38, 3e38, 3e38))
        assert np.isnan(((B * radiance[0]) * F(0.0)) * F(0.0))[0]
        assert not null_light(V, L, one(0.0), radiance, *rough)[0]
        assert null_light(V, L, one(0.0), vec((1e38, 1e38, 1e38)), *rough)[0]
