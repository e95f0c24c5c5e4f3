"""What the path-tracing tests share (tests/test_path_trace_host.py on the CPU, tests/test_gpu_path_trace.py and
tests/path_trace_device_checks.py on the device): the numpy restatement of the random numbers (uint32, from the description in
madarch_amd/csrc/mdh_path.h), the float64 restatement of the sampler, the furnace-free plane, a float64 path tracer built on
ref64.Run.raycast, Scene.info and Run.direct, the free rays and their three float64 runs, and the estimator composed from
the public queries one segment at a time."""
import contextlib

import numpy as np

import ray_query_cases as Q
import ref64
import ref64_cases
from helpers import SEED, SMALL_PROBES
from madarch_amd import renderers

SEED_PATHS = 20261020  # the committed seed of the plane (CPU and device) and of the free rays
N_FREE = 257
FREE_BOUNCES = 2
FREE_SAMPLES = (1, 4)
SEEDS = (None, 1, 2)  # shade_rays_cases.SEEDS: the float64 runs as stated and twice jittered
MIN_STEP = np.float32(0.05)
BAD_BITS = 0x7FC00000
PI32, TWO_PI32 = float(np.float32(3.14159265358)), float(np.float32(6.28318530718))  # the header's constants, as binary32 holds them
SKY32 = np.array([0.30, 0.36, 0.60], np.float32)


# ------------------------------------------------------------------------------------------------ the random numbers
def _pcg(v):
    v = np.asarray(v, dtype=np.uint32)
    s = v * np.uint32(747796405) + np.uint32(2891336453)
    w = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
    return (w >> np.uint32(22)) ^ w


def u01(seed, ray_id, sample, bounce, dimension):
    """path_u01 in numpy uint32 (arrays broadcast): exact binary32 values in [0, 1)"""
    with np.errstate(over="ignore"):
        h = _pcg(np.uint32(seed))
        for word in (ray_id, sample, bounce, dimension):
            h = _pcg(h + np.asarray(word, dtype=np.uint32))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def numbers(seed, ids, sample, bounce):
    """(n, 3): the three numbers path_scatter takes for rays `ids` at (sample, bounce)"""
    ids = np.asarray(ids, dtype=np.uint32)
    return np.stack([u01(seed, ids, sample, bounce, q) for q in range(3)], axis=1)


# ------------------------------------------------------------------------------------------------ the sampler in float64
def scatter64(D, N, rough, u):
    """path_scatter as the header describes it, in float64: n = N / |N|; u0 < roughness: cosine-weighted about n through the
    copysign frame; otherwise reflect (D, n) + uniform_vector (u1, u2) * roughness; normalised"""
    D, N, u = np.asarray(D, np.float64), np.asarray(N, np.float64), np.asarray(u, np.float64)
    rough = np.broadcast_to(np.asarray(rough, np.float64), (len(D),))
    with np.errstate(divide="ignore", invalid="ignore"):
        n = N / np.sqrt((N * N).sum(axis=1))[:, None]
        s = np.copysign(1.0, n[:, 2])
        a = -1.0 / (s + n[:, 2])
        b = n[:, 0] * n[:, 1] * a
        t1 = np.stack([1.0 + s * n[:, 0] * n[:, 0] * a, s * b, -s * n[:, 0]], axis=1)
        t2 = np.stack([b, s + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=1)
        phi = TWO_PI32 * u[:, 2]
        cos_d = (t1 * np.cos(phi)[:, None] + t2 * np.sin(phi)[:, None]) * np.sqrt(u[:, 1])[:, None] + n * np.sqrt(1.0 - u[:, 1])[:, None]
        al = PI32 * u[:, 1]
        off = np.stack([np.sin(phi) * np.sin(al), np.cos(phi) * np.sin(al), np.cos(al)], axis=1)
        mir = (D - n * (2.0 * (n * D).sum(axis=1))[:, None]) + off * rough[:, None]
        d = np.where((u[:, 0] < rough)[:, None], cos_d, mir)
        return d / np.sqrt((d * d).sum(axis=1))[:, None]


# ------------------------------------------------------------------------------------------------ the furnace-free plane
PLANE_ALBEDO = (0.8, 0.5, 0.25)
PLANE_RAYS, PLANE_SAMPLES = 64, 1024


def plane_desc():
    """a single floor plane y = -1 of albedo PLANE_ALBEDO and roughness 1 under one light that does not shine"""
    return {"kinds": [("Plane", 2)], "prims": [("Plane", (0.0, 1.0, 0.0), 1.0, 0)], "light_kinds": [("point", 2)],
            "lights": [("point", (0.0, 5.0, 0.0), (0.0, 0.0, 0.0))], "materials": [(PLANE_ALBEDO, 0.0, 1.0)], "max_dist": 20.0,
            "cam_pos": (0.0, 1.0, 0.0), "cam_m": np.eye(3), "ao_steps": 0, "spec_mode": 0, "probes": ref64_cases.probes_of(SMALL_PROBES)}


def plane_rays():
    """64 seeded rays from above the floor, all downwards: each hits the plane well inside max_dist"""
    rng = np.random.RandomState(SEED % 1000 + 61)
    org = np.stack([rng.uniform(-3.0, 3.0, PLANE_RAYS), rng.uniform(0.5, 3.0, PLANE_RAYS), rng.uniform(-3.0, 3.0, PLANE_RAYS)], axis=1).astype(np.float32)
    d = Q.unit_dirs(rng, PLANE_RAYS)
    d[:, 1] = -np.abs(d[:, 1]) - np.float32(0.3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(org), np.ascontiguousarray(d)


def plane_expected():
    """mean and allowed deviation of the estimator's average over S samples, per channel: a (sky_c - 0.7 * 2/3) and
    6 * 0.7 a / sqrt (18 S) + 1e-3 (the cosine-weighted mean of dir.y is 2/3, its variance 1/18)"""
    a = np.asarray(PLANE_ALBEDO, np.float64)
    return a * (ref64.SKY - 0.7 * 2.0 / 3.0), 6.0 * 0.7 * a / np.sqrt(18.0 * PLANE_SAMPLES) + 1e-3


def plane_estimate(drs, id_first=0, samples=PLANE_SAMPLES, seed=SEED_PATHS):
    """the estimator on the plane restated in numpy float64 -- the hit is analytic, nothing is marched: the first segment hits
    the floor (no direct light, mask = a), roughness 1 takes the cosine branch about (0, 1, 0), the second segment leaves the
    scene and adds a * sky (dir).  -> the average over the samples, (rays, 3)"""
    n = len(drs)
    ids = np.arange(n, dtype=np.uint32) + np.uint32(id_first)
    a = np.asarray(PLANE_ALBEDO, np.float64)
    up = np.tile(np.array([[0.0, 1.0, 0.0]]), (n, 1))
    total = np.zeros((n, 3))
    for s in range(samples):
        d = scatter64(drs, up, 1.0, numbers(seed, ids, s, 0))
        total += a[None, :] * (ref64.SKY[None, :] - 0.7 * d[:, 1:2])
    return total / samples


# ------------------------------------------------------------------------------------------------ a float64 path tracer
def trace64(run, org, drs, seed, id_first, sample_first, sample_count, bounces):
    """the estimator of k_path_trace in float64 on ref64's marches and lights: -> the SUM over the samples (n, 3), and `near`:
    some segment's march came near its threshold (Run.raycast) or a triangle's normal took part in the path"""
    sc = run.sc
    n = len(org)
    ids = np.arange(n, dtype=np.uint32) + np.uint32(id_first)
    total, near = np.zeros((n, 3)), np.zeros(n, dtype=bool)
    for s in range(sample_first, sample_first + sample_count):
        O, D = np.asarray(org, np.float64), np.asarray(drs, np.float64)
        mask, rgb = np.ones((n, 3)), np.zeros((n, 3))
        live = np.arange(n)
        for b in range(bounces + 1):
            if not len(live):
                break
            hit, arg, t, P, nr = run.raycast(O, D)
            # (a segment behind a black surface -- the room's floor, ceiling, front and back wall have albedo 0 -- is multiplied
            #  by a mask of exactly 0 in either precision: whatever its march finds, finite, adds 0 to the sum)
            lit = (mask[live] != 0.0).any(axis=1)
            near[live] |= nr & lit
            miss = ~hit
            rgb[live[miss]] += mask[live[miss]] * (ref64.SKY[None, :] - 0.7 * D[miss, 1:2])
            live, P, D, arg = live[hit], P[hit], D[hit], arg[hit]
            if not len(live):
                break
            N, mat = sc.info(arg, P)
            near[live] |= (sc.kind[arg] == 3) & lit[hit]  # triangle_normal_noise (ref64.hold)
            albedo, metallic, rough = sc.m_albedo[mat], sc.m_metallic[mat], sc.m_rough[mat]
            rgb[live] += mask[live] * run.direct(P, N, D, albedo, metallic, rough, True)
            mask[live] = mask[live] * albedo
            if b == bounces:
                break
            nd = scatter64(D, N, rough, numbers(seed, ids[live], s, b))
            ok = np.isfinite(nd).all(axis=1)
            live, O, D = live[ok], (P + N * ref64.MSS * 5.0)[ok], nd[ok]
        total += rgb
    return total, near


ROOM_LIGHTS = (("point", (1.5, 5.5, 4.5), (0.6, 0.5, 0.4)), ref64_cases.SPOT)  # (shade_points_cases: the spot light alone lights few points)


def describe(name):
    return ref64_cases.describe("room", lights=ROOM_LIGHTS) if name == "room" else ref64_cases.describe(name)


def free_rays(name):
    """257 rays of ray_query_cases.room_rays in the "room", of open_rays in the "open" scene"""
    return Q.room_rays(N_FREE) if name == "room" else Q.open_rays(N_FREE, SEED + 59)


def free_runs(name, samples):
    """three float64 runs of the free rays at FREE_BOUNCES bounces and `samples` samples, computed once: dicts of colour (the sum)
    and near"""
    def compute():
        sc = ref64.Scene(describe(name))
        org, drs = free_rays(name)
        runs = []
        for seed in SEEDS:
            c, near = trace64(ref64.Run(sc, seed), org, drs, SEED_PATHS, 0, 0, samples, FREE_BOUNCES)
            runs.append({"colour": c, "near": near})
        return runs
    return ref64_cases.cached(("path_trace", name, samples), compute)


def fragile(runs, samples):
    """hold_values' own count under the tolerances of the sums (ref64's times the samples)"""
    rtol, atol = ref64.COLOUR_RTOL, ref64.COLOUR_ATOL * samples
    bad = np.zeros(len(runs[0]["colour"]), dtype=bool)
    for r in runs:
        bad |= r["near"]
    for a in range(len(runs)):
        for b in range(a + 1, len(runs)):
            ca, cb = runs[a]["colour"], runs[b]["colour"]
            bad |= ~(np.abs(ca - cb) <= 0.5 * (atol + rtol * np.minimum(np.abs(ca), np.abs(cb)))).all(axis=-1)
    return bad


# ------------------------------------------------------------------------------------------------ composed from the public queries
@contextlib.contextmanager
def material_log():
    """the material table a scene builder writes, as the renderer was given it: {id: (albedo float32 (3,), roughness float32)}"""
    table = {}
    set_m, add_m = renderers.Renderer.Set_Material, renderers.Renderer.Add_Material

    def entry(e):
        from madarch_amd import materials
        return np.asarray(e.Get(materials.Albedo).data, dtype=np.float32), np.float32(e.Get(materials.Roughness).data)

    def set_material(self, index, e):
        table[int(index)] = entry(e)
        return set_m(self, index, e)

    def add_material(self, e):
        i = add_m(self, e)
        table[int(i)] = entry(e)
        return i
    renderers.Renderer.Set_Material, renderers.Renderer.Add_Material = set_material, add_material
    try:
        yield table
    finally:
        renderers.Renderer.Set_Material, renderers.Renderer.Add_Material = set_m, add_m


def compose(R, table, org, drs, seed, id_first, sample, bounces):
    """one sample of the estimator from Raycast, Primitive_Material, Shade_Points (mode 2, AO steps 0, linear) and
    Path_Scatter, chained by the host one segment at a time; the sums and products in numpy float32 -> rgb (n, 3), and the
    primary segment's hit, index, t"""
    from madarch_amd import _binding as B
    assert R.Get_Option(B.OPT_AO_STEPS) == 0
    n = len(org)
    f32 = np.float32
    rgb, mask = np.zeros((n, 3), f32), np.ones((n, 3), f32)
    live = np.arange(n)
    O, D = np.ascontiguousarray(org, f32), np.ascontiguousarray(drs, f32)
    first = None
    for b in range(bounces + 1):
        if not len(live):
            break
        rc = R.Raycast(O, D)
        if first is None:
            first = (rc["hit"].copy(), rc["index"].copy(), rc["t"].copy())
        hit = rc["hit"] == 1
        miss = ~hit
        s = D[miss, 1] * f32(0.7)
        rgb[live[miss]] = rgb[live[miss]] + mask[live[miss]] * (SKY32[None, :] - s[:, None])
        live, D = live[hit], np.ascontiguousarray(D[hit])
        if not len(live):
            break
        P, N = np.ascontiguousarray(rc["position"][hit]), np.ascontiguousarray(rc["normal"][hit])
        mat = R.Primitive_Material(rc["index"][hit])
        direct = R.Shade_Points(P, N, D, mat, Mode=2, Tone_Map=False)
        albedo = np.stack([table[int(m)][0] for m in mat])
        rough = np.array([table[int(m)][1] for m in mat], f32)
        rgb[live] = rgb[live] + mask[live] * direct
        mask[live] = mask[live] * albedo
        if b == bounces:
            break
        nd = _scatter_ids(R, D, N, rough, seed, id_first, live, sample, b)
        ok = np.isfinite(nd).all(axis=1)
        O = np.ascontiguousarray((P + (N * MIN_STEP) * f32(5.0))[ok])
        live, D = live[ok], np.ascontiguousarray(nd[ok])
    return (np.zeros((n, 3), f32) + rgb), first


def _scatter_ids(R, D, N, rough, seed, id_first, rows, sample, bounce):
    """Path_Scatter for rays whose ids are no longer consecutive: one call per run of consecutive ids"""
    out = np.zeros((len(rows), 3), np.float32)
    start = 0
    while start < len(rows):
        end = start + 1
        while end < len(rows) and rows[end] == rows[end - 1] + 1:
            end += 1
        out[start:end] = R.Path_Scatter(D[start:end], N[start:end], rough[start:end], Seed=seed, Id_First=id_first + int(rows[start]), Sample=sample, Bounce=bounce)
        start = end
    return out


def ref_plane():
    """plane_estimate over plane_rays under the committed seed, computed once: the CPU test holds it against the analytic mean,
    the device test holds the kernel against both"""
    return ref64_cases.cached(("path_trace_plane",), lambda: plane_estimate(plane_rays()[1]))
