"""The scenes, rays and yardsticks of the in-scattering queries (tests/test_inscatter_host.py on the CPU,
tests/test_gpu_inscatter.py and tests/inscatter_device_checks.py on the device): mdh_inscatter_points, mdh_inscatter_rays.

Three yardsticks, none of them the kernels' own output:
  the frame's textures   a froxel's sample point, rebuilt on the host as froxel_point builds it, must give the froxel texture's
                         bits; a scattering texel's camera ray must give the scattering texture's bits where every tap of the
                         fold falls on a texel centre (equal power-of-two grids and steps);
  the chain              a ray's sum is `step *` the sequential binary32 sum of the points' call with f given, f by repeated
                         binary32 addition, the sample point (dir * f) + org per component -- the association the header states;
  float64                ref64.Scene / Run.sample_light / Run.visibility / hg_phase over the f sequence in binary32, as
                         ref64.scattering_texels takes it, held by ref64.hold_values."""
import numpy as np

import ray_query_cases as rq
import ref64
import ref64_cases as RC
from helpers import SEED, SMALL_PROBES
from madarch_amd import _binding as B
from madarch_amd import materials, renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import triangles

BAD_BITS = 0x7FC00000
TAU32 = np.float32(0.1)  # volumetrics.glsl:12


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, "%s: shape %s, expected %s" % (what, g.shape, w.shape)
    assert np.array_equal(g, w), "%s: %d of %d words differ, first at %s: got %s, expected %s" % (
        what, (g != w).sum(), g.size, np.argwhere(g != w)[0].tolist(), np.asarray(got)[tuple(np.argwhere(g != w)[0])],
        np.asarray(want)[tuple(np.argwhere(g != w)[0])])


# ------------------------------------------------------------------------------------------------ scenes
# the volumes of (a) and (b): power-of-two resolutions and steps, so that every intermediate of froxel_point is exact
VOL_A = (RC.volume((8, 8, 8), 0.5, (8, 8), 0.5), RC.volume((16, 8, 4), 0.25, (8, 8), 0.25))
VOL_B = RC.volume((8, 8, 8), 0.5, (8, 8), 0.5)


def room(binding, vol=None, camera="identity"):
    """vol_scene ("room"): the room with its point light and its spot light; no volumetrics without `vol`"""
    desc = RC.vol_scene("room", camera)
    if vol is not None:
        desc["vol"] = RC.vol_of(vol)
    return RC.make_renderer(desc, 8, 8, binding)


def partition(binding, border, vol=None, residency=0):
    """examples.simple_scene behind its space partition (ray_query_cases.simple_partition) with a volume"""
    saved = scenes.Default_Partitioning_Settings
    try:
        if border == scenes.Fallback:
            scenes.Default_Partitioning_Settings = scenes.Partitioning_Settings(
                Border_Behavior=scenes.Fallback, Grid_Dimensions=(5, 5, 6), Grid_Spacing=(1.0, 1.0, 1.0), Grid_Offset=(0.0, 0.0, 0.0))
        scene = scenes.Compile(All_Primitives=[(RC.KINDS["Sphere"][0], 20), (RC.KINDS["Plane"][0], 10), (RC.KINDS["Box"][0], 20)],
                               All_Lights=[(point_lights.Point_Light, 4)])
    finally:
        scenes.Default_Partitioning_Settings = saved
    R = renderers.Create(windows.Open(8, 8, "inscatter"), scene, Probes=SMALL_PROBES, Volumetrics=vol or renderers.No_Volumetrics, Binding=binding)
    for n, o, m in RC.ROOM_PLANES:
        R.Add_Primitive(RC.KINDS["Plane"][0], RC.KINDS["Plane"][1](n, o, 0))
    for c in RC.SIMPLE_SPHERES:
        R.Add_Primitive(RC.KINDS["Sphere"][0], RC.KINDS["Sphere"][1](c, 0.5, 0))
    for c, s in RC.SIMPLE_BOXES:
        R.Add_Primitive(RC.KINDS["Box"][0], RC.KINDS["Box"][1](c, s, 0))
    R.Set_Material(0, materials.Create((0.5, 0.5, 0.5), 0.0, 0.6))
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create((0.0, 3.0, 0.0), (0.9, 0.9, 0.9)))
    R.Set_Camera_Position((2.0, 2.0, 0.0))
    R.Set_Option(B.OPT_TABLE_RESIDENCY, residency)
    R.Update_Partitioning(Method=renderers.CPU_Fast)
    return R


def mesh(binding, bvh, vol=None):
    """ray_query_cases.small_mesh in global residency, with a volume and the camera in front of the strip"""
    scene = scenes.Compile([(triangles.Triangle, rq.MESH_TRIANGLES)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(8, 8, "inscatter mesh"), scene, Probes=SMALL_PROBES, Volumetrics=vol or renderers.No_Volumetrics, Binding=binding)
    R.Set_Option(B.OPT_TABLE_RESIDENCY, 1)
    R.Set_Option(B.OPT_TRIANGLE_BVH, bvh)
    mat = R.Add_Material(materials.Create((0.8, 0.2, 0.1), 0.0, 1.0))
    for a, b, c in rq.mesh_triangles():
        R.Add_Primitive(triangles.Triangle, triangles.Create(a, b, c, mat))
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create((0.0, 1.0, -5.0), (0.9, 0.9, 0.9)))
    R.Set_Camera_Position((0.25, 1.0, -1.5))
    return R


VARIANTS = {
    "room": lambda b, vol=None: room(b, vol),
    "room, rotated camera": lambda b, vol=None: room(b, vol, "rotated"),
    "partition, Clamp": lambda b, vol=None: partition(b, scenes.Clamp, vol),
    "partition, Fallback": lambda b, vol=None: partition(b, scenes.Fallback, vol),
    "partition, Clamp, global residency": lambda b, vol=None: partition(b, scenes.Clamp, vol, 1),
    "partition, Fallback, global residency": lambda b, vol=None: partition(b, scenes.Fallback, vol, 1),
    "mesh, global residency": lambda b, vol=None: mesh(b, 0, vol),
    "mesh, triangle BVH": lambda b, vol=None: mesh(b, 1, vol),
}
CHAIN_VARIANTS = ("room", "partition, Clamp", "partition, Fallback", "partition, Clamp, global residency", "partition, Fallback, global residency",
                  "mesh, global residency", "mesh, triangle BVH")


# ------------------------------------------------------------------------------------------------ (a), (b): the frame's grids
def froxel_points(R, vol):
    """the sample point and direction of every froxel texel, in the texture's order (vh * vz rows of vw), as froxel_point
    (mdh_kernels.h) forms them: the camera ray through (centre (i, vw), row centre), pos = origin + (dir * slice) * vstep in
    binary32.  Camera_Rays' row r looks through v = -centre (r, vh): the texture's row y is its row vh - 1 - y."""
    vw, vh, vz = vol.Visibility_Resolution
    for n in (vw, vh, vz):
        assert n & (n - 1) == 0, "power-of-two resolutions keep frag_height on the row centre"
    org, drs = R.Camera_Rays(vw, vh)
    org, drs = org.reshape(vh, vw, 3)[::-1], drs.reshape(vh, vw, 3)[::-1]
    vstep = np.float32(vol.Visibility_Step_Size)
    pos = np.stack([org + (drs * np.float32(z)) * vstep for z in range(vz)])  # [slice][y][x]
    dirs = np.broadcast_to(drs, pos.shape)
    assert pos.dtype == np.float32
    return np.ascontiguousarray(pos.reshape(-1, 3)), np.ascontiguousarray(dirs.reshape(-1, 3))


def texel_rays(R, sw, sh):
    """the camera rays of the scattering texture's texels, in the texture's order"""
    org, drs = R.Camera_Rays(sw, sh)
    return np.ascontiguousarray(org.reshape(sh, sw, 3)[::-1].reshape(-1, 3)), np.ascontiguousarray(drs.reshape(sh, sw, 3)[::-1].reshape(-1, 3))


# ------------------------------------------------------------------------------------------------ (c): the chain
CHAIN_STEPS = (0.07, 0.1, 2.0 ** -5)
CHAIN_COUNTS = (0, 1, 63, 64, 65, 128, 129)  # steps per ray: around one and two chunks of 64
CHAIN_BATCHES = (1, 3, 4, 5)                 # a partial workgroup of four rays, a full one, two


def f_sequence(step, count):
    """f_0 .. f_count of the serial loop: repeated binary32 addition"""
    out, f, s = [], np.float32(0.0), np.float32(step)
    for _ in range(count + 1):
        out.append(f)
        f = np.float32(f + s)
    return np.array(out, dtype=np.float32)


def tmax_for(step, count):
    """a length with exactly `count` steps: between f_count-1 and f_count (0 for none)"""
    if count == 0:
        return np.float32(0.0)
    f = f_sequence(step, count)
    t = np.float32((np.float64(f[count - 1]) + np.float64(f[count])) * 0.5)
    assert f[count - 1] < t <= f[count]
    return t


def steps_of(step, length):
    """the loop's turns for a binary32 length, on the host"""
    n, f, s = 0, np.float32(0.0), np.float32(step)
    while f < np.float32(length):
        n += 1
        f = np.float32(f + s)
    return n


def chain_rays(name, n, first):
    """n rays from around the variant's camera into its scene, with step counts CHAIN_COUNTS[first ..] in turn"""
    rng = np.random.RandomState((SEED + 97 * n + first) & 0x7FFFFFFF)
    eye = np.array((0.25, 1.0, -1.5) if "mesh" in name else (2.0, 2.0, 0.0))
    org = (eye + rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.3
    drs = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    counts = [CHAIN_COUNTS[(first + i) % len(CHAIN_COUNTS)] for i in range(n)]
    return org, drs, counts


def sample_points(org, drs, step, counts):
    """every ray's sample points (dir * f) + org per component in binary32, the direction repeated, f, and the ray of each"""
    P, D, F, ray = [], [], [], []
    for i, c in enumerate(counts):
        f = f_sequence(step, c)[:c]
        P.append(drs[i][None, :] * f[:, None] + org[i][None, :])
        D.append(np.broadcast_to(drs[i], (c, 3)))
        F.append(f)
        ray.append(np.full(c, i))
    P = np.concatenate(P).astype(np.float32) if P else np.zeros((0, 3), np.float32)
    return (np.ascontiguousarray(P), np.ascontiguousarray(np.concatenate(D), dtype=np.float32), np.concatenate(F).astype(np.float32), np.concatenate(ray))


def chain_sum(products, ray, n, step):
    """step * the sequential binary32 sum of a ray's products, in step order"""
    out = np.zeros((n, 3), np.float32)
    for i in range(n):
        L = np.zeros(3, np.float32)
        for p in products[ray == i]:
            L = (L + p).astype(np.float32)
        out[i] = L * np.float32(step)
    return out


def chain_expected(R, org, drs, step, counts):
    """what Inscatter_Rays must answer, through Inscatter_Points with f given: rgb, len (the caller's), steps"""
    P, D, F, ray = sample_points(org, drs, step, counts)
    products = R.Inscatter_Points(P, D, F) if len(P) else np.zeros((0, 3), np.float32)
    return chain_sum(products, ray, len(org), step)


# ------------------------------------------------------------------------------------------------ (d): float64
N_FREE = 192
FREE_STEP = 0.07


def free_rays(name):
    """origins: the camera position +- 0.3; directions: normalised normal draws with z -> |z| + 0.3; U: a length uniform in
    (0.5, 6); tmax = max (min (U, d - 0.15), 0) with d the float64 hit distance: the rays end in front of what they see"""
    desc = RC.vol_scene(name)
    rng = np.random.RandomState((SEED + (11 if name == "room" else 13)) & 0x7FFFFFFF)
    org = (np.asarray(desc["cam_pos"]) + rng.uniform(-0.3, 0.3, (N_FREE, 3))).astype(np.float32)
    d = rng.normal(size=(N_FREE, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.3
    drs = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    U = rng.uniform(0.5, 6.0, N_FREE).astype(np.float32)
    run = ref64.Run(ref64.Scene(desc))
    hit, _, _, P, _ = run.raycast(org, drs)
    dist = np.where(hit, np.linalg.norm(P - org.astype(np.float64), axis=1), np.inf)
    tmax = np.maximum(np.minimum(U.astype(np.float64), dist - 0.15), 0.0).astype(np.float32)
    return desc, org, drs, U, tmax


def inscatter64(run, P, D):
    """sample_lights (compute_frustrum_visibility.glsl:8-19) in float64, as ref64.froxel_texels sums it"""
    out = np.zeros((len(P), 3))
    for light in run.sc.lights:
        radiance, L, Ld = run.sample_light(light, P)
        out += radiance * (np.exp(-Ld * ref64.TAU) * run.visibility(P, L, Ld) * ref64.TAU * ref64.hg_phase(L, D))[:, None]
    return out


def free_samples(name):
    """the free rays' sample points: binary32 f_k and points, as the kernel forms them"""
    desc, org, drs, U, tmax = free_rays(name)
    counts = [steps_of(FREE_STEP, t) for t in tmax]
    P, D, F, ray = sample_points(org, drs, FREE_STEP, counts)
    return desc, org, drs, tmax, counts, P, D, F, ray


def free_runs(name):
    """three float64 runs over the free rays -> (runs of the rays' sums, runs of the points' integrand)"""
    def compute():
        desc, org, drs, tmax, counts, P, D, F, ray = free_samples(name)
        sc = ref64.Scene(desc)
        near_pt = sc.closest(P.astype(np.float64))[0] < ref64.NEAR_SURFACE
        ray_runs, point_runs = [], []
        for seed in (None, 0x4D41, 0x4441):
            ins = inscatter64(ref64.Run(sc, seed), P.astype(np.float64), D.astype(np.float64))
            point_runs.append({"colour": ins, "near": near_pt})
            prod = ins * np.exp(-F.astype(np.float64) * ref64.TAU)[:, None]
            L = np.zeros((len(org), 3))
            np.add.at(L, ray, prod)
            near = np.zeros(len(org), dtype=bool)
            np.logical_or.at(near, ray, near_pt)
            ray_runs.append({"colour": L * float(np.float32(FREE_STEP)), "near": near})
        return ray_runs, point_runs
    return RC.cached(("inscatter free", name), compute)


def march_runs(name):
    """three float64 runs of the marched length over the free rays with tmax = U: len = min (|hit - org|, U)"""
    def compute():
        desc, org, drs, U, _ = free_rays(name)
        sc = ref64.Scene(desc)
        runs = []
        for seed in (None, 0x4D41, 0x4441):
            run = ref64.Run(sc, seed)
            hit, _, _, P, near = run.raycast(org, drs)
            d = np.where(hit, np.linalg.norm(P - org.astype(np.float64), axis=1), np.inf)
            runs.append({"len": np.minimum(d, U.astype(np.float64)), "near": near & (d < U + ref64.T_ATOL)})
        return runs
    return RC.cached(("inscatter march", name), compute)


def march_fragile(runs):
    """rays whose march the three runs disagree on, or whose march came within the threshold's margin"""
    bad = np.zeros(len(runs[0]["len"]), dtype=bool)
    for a in range(3):
        bad |= runs[a]["near"]
        for b in range(a + 1, 3):
            bad |= np.abs(runs[a]["len"] - runs[b]["len"]) > 0.5 * ref64.T_ATOL
    return bad
