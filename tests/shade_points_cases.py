"""The points, the atlases and the float64 answers that the point-query tests share (tests/test_shade_points_host.py on the
CPU, tests/test_gpu_shade_points.py and tests/shade_points_device_checks.py on the device): 257 free points with seeded
normals, view directions and material ids in the "room" and the "open" scene of ref64_cases, ref64's lighting of those
points composed as Run.pixel_color_probes composes it behind its hit, the five classes of points the irradiance is held
at against the oracle, and the frame's hit points as Camera_Rays -> Raycast -> Primitive_Material hands them over."""
import numpy as np

import ray_query_cases as Q
import ref64
import ref64_cases
import shade_rays_cases as S
from helpers import SEED
from madarch_amd import _binding as B
from madarch_amd import scenes

N_FREE = 257
MODES = (0, 2)
IRRADIANCE = 3  # MDH_POINT_IRRADIANCE
BAD_BITS = 0x7FC00000
ROOM_LIGHTS = (("point", (1.5, 5.5, 4.5), (0.6, 0.5, 0.4)), ref64_cases.SPOT)  # with the spot light alone 5 of 257 points see any direct light


# ---------------------------------------------------------------------------------------- free points against float64
def describe(name):
    return ref64_cases.describe("room", lights=ROOM_LIGHTS) if name == "room" else ref64_cases.describe(name)


def free_points(name, n_materials):
    """positions, normals, view directions, material ids"""
    if name == "room":
        pos = Q.rays_inside(N_FREE, Q.ROOM_LO, Q.ROOM_HI, SEED + 41)[0]
    else:
        pos = Q.open_rays(N_FREE, SEED + 43)[0]
    rng = np.random.RandomState(SEED % 1000 + 47)
    nrm, view = Q.unit_dirs(rng, N_FREE), Q.unit_dirs(rng, N_FREE)
    mat = (rng.randint(0, 1 << 30, N_FREE) % n_materials).astype(np.int32)
    return pos, nrm, view, mat


def shade64(run, P, N, D, mat, mode, spec_mode, ao_steps):
    """the lighting of pixel_color_probes behind its hit (ref64.Run.pixel_color_probes, the block under `if len (rows)`) at
    points that are given: -> colour, the irradiance alone, the direct term alone, fragile flags (the reflection's march
    came near its threshold, or a triangle's normal took part in it).  The run's jitter moves P, N and D as Run.ray moves a
    ray."""
    sc = run.sc
    P, N = run.ray(P, N)
    D, _ = run.ray(D, D)
    albedo, metallic, rough = sc.m_albedo[mat], sc.m_metallic[mat], sc.m_rough[mat]
    direct = run.direct(P, N, D, albedo, metallic, rough, True)
    ao = run.ambient_occlusion(P, N, ao_steps)[:, None]
    flags = np.zeros(len(P), dtype=bool)
    irradiance = run.sample_irradiance(P, N)
    if mode == 2:
        return direct * ao, irradiance, direct, flags
    sdir = D - N * (2.0 * (N * D).sum(axis=1))[:, None]  # reflect, GLSL 4.30 section 8.5
    scol = np.zeros((len(P), 3))
    gate = rough < 0.75
    if spec_mode == 2 and gate.any():
        f = np.zeros(int(gate.sum()), dtype=bool)
        scol[gate] = run.radiance_no_specular(P[gate], N[gate], sdir[gate], f)
        flags[np.nonzero(gate)[0][f]] = True
    kD, kS = run.cook_torrance(N, -D, sdir, albedo, metallic, rough)  # lighting.glsl:42-49
    indirect = kD * irradiance / ref64.PI + kS * scol * np.maximum((N * sdir).sum(axis=1), 0.0)[:, None]
    return ao * (direct + indirect), irradiance, direct, flags


def free_runs(name, mode):
    """three float64 runs over the free points of scene `name`, computed once: dicts of colour, irradiance, direct, near"""
    def compute():
        desc = describe(name)
        irr, rad = S.free_atlases(desc)
        sc = ref64.Scene(desc)
        pos, nrm, view, mat = free_points(name, len(desc["materials"]))
        runs = []
        for seed in S.SEEDS:
            c, i, d, f = shade64(ref64.Run(sc, seed, irr, rad), pos, nrm, view, mat, mode, desc["spec_mode"], desc["ao_steps"])
            runs.append({"colour": c, "irradiance": i, "direct": d, "near": f})
        return runs
    return ref64_cases.cached(("shade_points", name, mode), compute)


def fragile(runs, key="colour"):
    """hold_values' own count, for the CPU test: flagged by a run, or two runs more than half the tolerance apart"""
    bad = np.zeros(len(runs[0][key]), dtype=bool)
    if key == "colour":
        for r in runs:
            bad |= r["near"]
    for a in range(len(runs)):
        for b in range(a + 1, len(runs)):
            ca, cb = runs[a][key], runs[b][key]
            bad |= ~(np.abs(ca - cb) <= 0.5 * (ref64.COLOUR_ATOL + ref64.COLOUR_RTOL * np.minimum(np.abs(ca), np.abs(cb)))).all(axis=-1)
    return bad


# ---------------------------------------------------------------------------------------- the irradiance against the oracle
# name -> the same scene over the oracle's binding (table residency and the triangle BVH are options of the HIP library alone
# and change no bit)
ORACLE_TWINS = {
    "rooms": Q.gi_room,
    "partition, Clamp": lambda b: Q.simple_partition(b, scenes.Clamp),
    "partition, Fallback": lambda b: Q.simple_partition(b, scenes.Fallback),
    "partition, Clamp, global residency": lambda b: Q.simple_partition(b, scenes.Clamp),
    "partition, Fallback, global residency": lambda b: Q.simple_partition(b, scenes.Fallback),
    "mesh, scanned": lambda b: S.mesh(b),
    "mesh, global residency": lambda b: S.mesh(b),
    "mesh, triangle BVH": lambda b: S.mesh(b),
    "open scene": lambda b: Q.described(b, "open")[0],
}
assert list(ORACLE_TWINS) == list(S.FRAME_SCENES)
PROBE_CLEARANCE = 1e-3  # at a probe the shader divides 0 by 0, and the NaN's sign is nobody's contract


def probe_positions(R):
    p = R.Probes
    g = np.stack(np.meshgrid(*[np.arange(d) for d in p.Grid_Dimensions], indexing="ij"), axis=-1).reshape(-1, 3)
    return g * np.asarray(p.Grid_Spacing, dtype=np.float64)


def irradiance_points(R, name, rays, n=N_FREE):
    """257 points of five classes: on surfaces (Raycast over `rays`), free in the air, inside a primitive (Raycast's hits
    pushed 0.3 behind their surface where the scene's solids are that deep, else 0.01: the first visibility step is below
    epsilon either way), outside the probe grid on each side, within 0.3 of a probe -- every one at least PROBE_CLEARANCE
    from every probe.  -> positions, normals, the class of each"""
    rng = np.random.RandomState(SEED % 1000 + 53)
    probes = probe_positions(R)
    lo, hi = probes.min(axis=0), probes.max(axis=0)
    rc = R.Raycast(*rays)
    hit = np.nonzero(rc["hit"] == 1)[0]
    assert len(hit) >= 16, "%s: %d of the rays hit" % (name, len(hit))
    k_surface, k_inside, k_out, k_near = 80, 40, 48, 40
    parts = []
    rows = hit[np.arange(k_surface) % len(hit)]
    parts.append((rc["position"][rows], rc["normal"][rows], 0))
    air = (lo - 0.5 + (hi - lo + 1.0) * rng.rand(n - k_surface - k_inside - k_out - k_near, 3)).astype(np.float32)
    parts.append((air, Q.unit_dirs(rng, len(air)), 1))
    rows = hit[(np.arange(k_inside) * 7 + 3) % len(hit)]
    depth = np.where(np.arange(k_inside) % 2 == 0, 0.3, 0.01)[:, None].astype(np.float32)
    parts.append(((rc["position"][rows] - rc["normal"][rows] * depth).astype(np.float32), Q.unit_dirs(rng, k_inside), 2))
    out = (lo + (hi - lo) * rng.rand(k_out, 3))
    side = np.arange(k_out) % 6
    out[np.arange(k_out), side // 2] = np.where(side % 2 == 0, lo[side // 2] - rng.uniform(0.05, 1.5, k_out), hi[side // 2] + rng.uniform(0.05, 1.5, k_out))
    parts.append((out.astype(np.float32), Q.unit_dirs(rng, k_out), 3))
    near = probes[rng.randint(0, len(probes), k_near)] + Q.unit_dirs(rng, k_near) * rng.uniform(0.01, 0.3, (k_near, 1))
    parts.append((near.astype(np.float32), Q.unit_dirs(rng, k_near), 4))
    pos = np.ascontiguousarray(np.concatenate([p[0] for p in parts]), dtype=np.float32)
    nrm = np.ascontiguousarray(np.concatenate([p[1] for p in parts]), dtype=np.float32)
    cls = np.concatenate([np.full(len(p[0]), p[2]) for p in parts])
    assert len(pos) == n
    # the clearance: a point that came too close to a probe steps 0.01 away from it along x
    d = np.linalg.norm(pos[:, None, :].astype(np.float64) - probes[None], axis=2)
    close = d.min(axis=1) < 10.0 * PROBE_CLEARANCE
    pos[close, 0] += np.float32(0.02)
    d = np.linalg.norm(pos[:, None, :].astype(np.float64) - probes[None], axis=2)
    assert d.min() >= PROBE_CLEARANCE
    return pos, nrm, cls


def scene_rays(name, n=N_FREE):
    if name.startswith("mesh"):
        return Q.mesh_rays(n)
    if name == "open scene":
        return Q.open_rays(n)
    return Q.room_rays(n)


def orc_irradiance(orc, Ro, pos, nrm):
    import ctypes as C
    out = np.zeros((len(pos), 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    orc.lib.orc_probe_sample_irradiance(Ro._h, len(pos), vp(pos), vp(nrm), vp(out))
    return out


def twin_renderers(hip, orc, name, atlas=None):
    """scene `name` over the HIP library and over the oracle at the frame's size, the same seeded atlases written to both"""
    with S.frame_size():
        R, Ro = S.FRAME_SCENES[name](hip), ORACLE_TWINS[name](orc)
    for r in (R, Ro):
        if atlas is not None:
            r.Set_Option(B.OPT_ATLAS_FORMAT, atlas)
        irr, rad = S.seeded_atlases(r)
        r.Write_Texture(B.TEX_IRRADIANCE, irr)
        r.Write_Texture(B.TEX_RADIANCE, rad)
    return R, Ro


# ---------------------------------------------------------------------------------------- the frame, point by point
def frame_points(R, W=S.FRAME_W, H=S.FRAME_H):
    """Camera_Rays -> Raycast -> Primitive_Material: the frame's rays, its hit rows, and what Shade_Points takes for them"""
    org, drs = R.Camera_Rays(W, H)
    rc = R.Raycast(org, drs)
    mat = R.Primitive_Material(rc["index"])
    rows = np.nonzero(rc["hit"] == 1)[0]
    c = np.ascontiguousarray
    return org, drs, rows, (c(rc["position"][rows]), c(rc["normal"][rows]), c(drs[rows]), c(mat[rows])), mat, rc
