"""The scenes, the seeded rays and the oracle's answers of the ray-query tests (tests/test_ray_queries_host.py on the
CPU, tests/test_gpu_ray_queries.py on the device).  Every scene is built through the host API over the binding it is
given; the oracle answers through its probe exports (orc_probe_raycast, orc_probe_softshadow, orc_probe_closest)."""
import ctypes as C

import numpy as np

import ref64
import ref64_cases
from helpers import SEED, SMALL_PROBES
from madarch_amd import _binding as B
from madarch_amd import examples, materials, renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import triangles
from mesh_scenes import parity_mesh

EPS = np.float32(0.001)       # maths.glsl:3
MIN_STEP = np.float32(0.05)   # raymarching.glsl:1
MAX_DIST = np.float32(20.0)   # scenes.ads:51, every scene here keeps it
BATCHES = (1, 63, 64, 65, 257, 1000)  # the partial wavefront, the partial workgroup, four workgroups
ROOM_LO, ROOM_HI = np.array([-0.9, -0.9, -5.9]), np.array([6.9, 6.9, 6.9])  # inside the six planes of the examples' room
MESH_TRIANGLES = 120


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ scenes
def gi_room(binding):
    return examples.global_illumination(16, 16, Probes=SMALL_PROBES, Binding=binding)


def simple_partition(binding, border=scenes.Clamp, residency=None):
    """examples.simple_scene behind its space partition.  Clamp: the example's own grid, which holds the whole room.
    Fallback: a grid of 5 x 5 x 6 unit cells at the origin, which the rays leave on their way through the room -- beyond a
    border that falls back to the scan the example's grid would never be left."""
    saved = scenes.Default_Partitioning_Settings
    try:
        if border == scenes.Fallback:
            scenes.Default_Partitioning_Settings = scenes.Partitioning_Settings(
                Border_Behavior=scenes.Fallback, Grid_Dimensions=(5, 5, 6), Grid_Spacing=(1.0, 1.0, 1.0), Grid_Offset=(0.0, 0.0, 0.0))
        R = examples.simple_scene(16, 16, Probes=SMALL_PROBES, Binding=binding, Partitioning_Method=None)
    finally:
        scenes.Default_Partitioning_Settings = saved
    if residency is not None:
        R.Set_Option(B.OPT_TABLE_RESIDENCY, residency)
    R.Update_Partitioning(Method=renderers.CPU_Fast)
    return R


def small_mesh(binding, residency=None, bvh=None):
    """the first MESH_TRIANGLES triangles of the parity tests' sheet, scanned (no partition); `residency` and `bvh` are options
    of the HIP library alone"""
    scene = scenes.Compile([(triangles.Triangle, MESH_TRIANGLES)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(16, 16, "mesh"), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=binding)
    if residency is not None:
        R.Set_Option(B.OPT_TABLE_RESIDENCY, residency)
    if bvh is not None:
        R.Set_Option(B.OPT_TRIANGLE_BVH, bvh)
    mat = R.Add_Material(materials.Create((0.8, 0.2, 0.1), 0.0, 1.0))
    for a, b, c in mesh_triangles():
        R.Add_Primitive(triangles.Triangle, triangles.Create(a, b, c, mat))
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create((0.0, 1.0, -5.0), (0.9, 0.9, 0.9)))
    return R


def mesh_triangles():
    return (parity_mesh()[:MESH_TRIANGLES] + np.asarray(examples.OBJ_MESH_OFFSET, dtype=np.float32)).astype(np.float32)


def described(binding, name):
    """a scene of ref64_cases ("room": the global_illumination example's, "open": a floor, two spheres and a triangle under
    the sky) -> renderer, description (what ref64.Scene takes)"""
    desc = ref64_cases.describe(name)
    return ref64_cases.make_renderer(desc, 16, 16, binding), desc


# ------------------------------------------------------------------------------------------------- rays
def unit_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def rays_inside(n, lo, hi, seed):
    """origins inside the box lo .. hi, directions uniform on the sphere"""
    rng = np.random.RandomState(seed & 0x7FFFFFFF)
    org = (np.asarray(lo) + (np.asarray(hi) - np.asarray(lo)) * rng.rand(n, 3)).astype(np.float32)
    return org, unit_dirs(rng, n)


def rays_from_inside_primitives(n, seed):
    """origins inside the room's sphere ((3, 4, 3), 1) and inside its box ((3, 0, 4), 1.5): a hit at t = 0 after one step"""
    rng = np.random.RandomState(seed & 0x7FFFFFFF)
    half = n // 2
    in_sphere = np.array([3.0, 4.0, 3.0]) + 0.55 * (2.0 * rng.rand(half, 3) - 1.0)
    in_box = np.array([3.0, 0.3, 4.0]) + np.array([1.3, 1.0, 1.3]) * (2.0 * rng.rand(n - half, 3) - 1.0)
    return np.concatenate((in_sphere, in_box)).astype(np.float32), unit_dirs(rng, n)


def rays_along_wall(n, seed):
    """2 mm in front of the wall x = -1 and parallel to it: steps of two epsilon until something else comes close"""
    rng = np.random.RandomState(seed & 0x7FFFFFFF)
    org = np.stack([np.full(n, -1.0 + 0.002), rng.uniform(-0.5, 6.5, n), rng.uniform(-5.5, 6.5, n)], axis=1).astype(np.float32)
    a = rng.uniform(0.0, 2.0 * np.pi, n)
    return org, np.stack([np.zeros(n), np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def room_rays(n, seed=SEED):
    """the room's mixture, in one order for every batch size: mostly rays from inside the room, a few from inside the sphere
    and the box, a few along a wall"""
    k_in, k_wall = max(1, n // 8), max(1, n // 50) if n >= 8 else 0
    parts = [rays_inside(n - k_in - k_wall, ROOM_LO, ROOM_HI, seed)] if n > k_in + k_wall else []
    parts.append(rays_from_inside_primitives(k_in, seed + 1))
    if k_wall:
        parts.append(rays_along_wall(k_wall, seed + 2))
    org, drs = np.concatenate([p[0] for p in parts])[:n], np.concatenate([p[1] for p in parts])[:n]
    order = np.random.RandomState(seed % 1000).permutation(len(org))
    return np.ascontiguousarray(org[order]), np.ascontiguousarray(drs[order])


def open_rays(n, seed=SEED + 7):
    """the open scene: rays from above the floor in every direction -- most of the upward ones leave the scene"""
    return rays_inside(n, (-1.0, -0.5, 0.0), (6.0, 5.0, 7.0), seed)


def mesh_rays(n, seed=SEED + 11):
    """around the strip of triangles; two rays in three aim at a triangle's centroid"""
    org, drs = rays_inside(n, (-1.5, -0.5, -1.0), (2.0, 2.5, 3.0), seed)
    rng = np.random.RandomState((seed + 1) & 0x7FFFFFFF)
    aim = mesh_triangles().mean(axis=1)[rng.randint(0, MESH_TRIANGLES, n)] - org
    aim = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(np.float32)
    keep = np.arange(n) % 3 == 2
    return org, np.where(keep[:, None], drs, aim)


def seeded_tmax(n, seed, lo=0.3, hi=12.0):
    return np.random.RandomState(seed & 0x7FFFFFFF).uniform(lo, hi, n).astype(np.float32)


def light_rays(n, light, lo, hi, seed):
    """shadow rays as the shaders cast them: from seeded points towards a light, as long as the way to it"""
    rng = np.random.RandomState(seed & 0x7FFFFFFF)
    org = (np.asarray(lo) + (np.asarray(hi) - np.asarray(lo)) * rng.rand(n, 3)).astype(np.float32)
    v = np.asarray(light, dtype=np.float32) - org
    dist = np.sqrt((v * v).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return org, (v / dist[:, None]).astype(np.float32), dist


# ---------------------------------------------------------------------------------------- the oracle's answers
def orc_raycast(orc, R, org, drs):
    n = len(org)
    out = {"hit": np.zeros(n, np.int32), "index": np.zeros(n, np.int32), "t": np.zeros(n, np.float32), "steps": np.zeros(n, np.int32)}
    orc.lib.orc_probe_raycast(R._h, n, _vp(org), _vp(drs), _vp(out["hit"]), _vp(out["index"]), _vp(out["t"]), _vp(out["steps"]))
    return out


def orc_softshadow(orc, R, org, drs, tmax, k):
    out = np.zeros(len(org), np.float32)
    tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (len(org),)))
    orc.lib.orc_probe_softshadow(R._h, len(org), _vp(org), _vp(drs), _vp(tmax), C.c_float(k), _vp(out))
    return out


def orc_closest(orc, R, pts):
    """partitioning_closest_info (the scan without a partition) at pts -> distance, index"""
    n = len(pts)
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    d, i = np.zeros(n, np.float32), np.zeros(n, np.int32)
    orc.lib.orc_probe_closest(R._h, n, _vp(pts), 1 if R.Scene.Partitioning_Config.Enable else 0, _vp(d), _vp(i))
    return d, i


def visibility_from_raycast(rc, tmax):
    """raycast_visibility (raymarching.glsl:39-56) marches raycast's very steps and stops them at tmax <= max_dist: it is
    blocked exactly when raycast hits at a march length below tmax"""
    return 1.0 - ((rc["hit"] != 0) & (rc["t"] < np.asarray(tmax, np.float32))).astype(np.float32)


def march_point(org, drs, t):
    """org + dir * t as the march computes it: one binary32 product and one binary32 sum per coordinate"""
    org, drs, t = np.asarray(org, np.float32), np.asarray(drs, np.float32), np.asarray(t, np.float32)
    return org + drs * t[:, None]


def oracle_answers(orc, Ro, org, drs):
    """what mdh_raycast must return, from the oracle alone: orc_probe_raycast's four, the hit point as the float32 product
    and sum -- checked against the oracle itself: it is the point where the oracle's last evaluation found the hit, so its
    arg-min there is the hit's index at a distance below epsilon -- and the normal of orc_eval_distance_to over all kinds in
    scene order at that point (the scenes here have no coincident primitives); position and normal 0 on a miss"""
    rc = orc_raycast(orc, Ro, org, drs)
    hit = rc["hit"] != 0
    assert ((rc["hit"] == 0) | (rc["hit"] == 1)).all() and (rc["index"][~hit] == -1).all() and (rc["t"][~hit] == 0.0).all()
    pos = march_point(org, drs, rc["t"])
    d, i = orc_closest(orc, Ro, pos)
    assert (d[hit] < EPS).all() and np.array_equal(i[hit], rc["index"][hit])
    # (with the shaders' division: under OPT_ADA_EVAL_DIV, its default, a triangle's distance and normal are those of
    #  Madarch.Values."/", which adds -- not what primitive_info computes)
    ada = Ro.Get_Option(B.OPT_ADA_EVAL_DIV)
    Ro.Set_Option(B.OPT_ADA_EVAL_DIV, 0)
    dist, nrm = Ro.Eval_Distances_To(pos, [p for p, _ in Ro.Scene.Prims_Count])
    Ro.Set_Option(B.OPT_ADA_EVAL_DIV, ada)
    assert np.array_equal(dist[hit], d[hit])  # (the same arg-min as the march's: the normal is the hit primitive's)
    rc["position"] = np.where(hit[:, None], pos, np.float32(0.0))
    rc["normal"] = np.where(hit[:, None], nrm, np.float32(0.0))
    return rc


# ------------------------------------------------------------------- soft shadows with min_dist > 0: float64
SHADOW_KS = (0.5, 64.0)
SHADOW_TMINS = (float(MIN_STEP * np.float32(5.0)), 0.1)
REF64_SEEDS = (None, 1, 2)
SHADOW_CASES = {"room": ((3.5, 5.0, 2.0), (-0.8, -0.8, -5.5), (6.8, 6.8, 6.8)), "open": ((3.0, 6.0, 1.0), (-1.0, -0.5, 0.0), (6.0, 5.0, 7.0))}


def shadow_rays(name, n=192):
    light, lo, hi = SHADOW_CASES[name]
    return light_rays(n, light, lo, hi, SEED + 23)


def shadow_runs(desc, org, drs, tmin, tmax, k):
    """ref64's soft shadows as stated and twice jittered, as hold_values takes them"""
    sc = ref64.Scene(desc)
    key = ("softshadows", desc["cam_pos"], len(desc["prims"]), org.tobytes(), drs.tobytes(), float(tmin), np.asarray(tmax).tobytes(), float(k))
    return ref64_cases.cached(key, lambda: [{"colour": ref64.Run(sc, seed).softshadows(org, drs, tmin, tmax, k)[:, None]} for seed in REF64_SEEDS])


def hold_shadows(name, desc, org, drs, tmin, tmax, k, got):
    """`got` against float64 under the colour tolerance of the frames (ref64.COLOUR_RTOL / COLOUR_ATOL) and FRAGILE_CAP as it
    is.  tests/test_ray_queries_host.py puts the ORACLE's own min_dist = 0 results through this very hold: they pass it, so
    these are the tolerances of the device's min_dist > 0 results too."""
    runs = shadow_runs(desc, org, drs, tmin, tmax, k)
    return ref64.hold_values(name, runs, np.asarray(got, np.float64)[:, None], ref64.COLOUR_RTOL, ref64.COLOUR_ATOL)
