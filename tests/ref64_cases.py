"""The cases of test_ref64_oracle.py (the oracle) and test_gpu_ref64.py (the HIP library): each is one plain scene
description, built once as a renderer over the binding under test and once as ref64's float64 scene, and held by
ref64.hold.  The float64 results are cached per process, so the two files never compute a case twice in one run."""
import numpy as np

import ref64
from helpers import SEED, SMALL_PROBES
from madarch_amd import _binding as B
from madarch_amd import materials, renderers, scenes, windows
from madarch_amd.lights import point_lights, spot_lights
from madarch_amd.primitives import boxes, planes, spheres, triangles

KINDS = {"Sphere": (spheres.Sphere, spheres.Create), "Plane": (planes.Plane, planes.Create), "Box": (boxes.Box, boxes.Create),
         "Triangle": (triangles.Triangle, triangles.Create)}
LIGHTS = {"point": (point_lights.Point_Light, point_lights.Create), "spot": (spot_lights.Spot_Light, spot_lights.Create)}

ROOM_PLANES = (((0.0, 1.0, 0.0), 1.0, 0), ((0.0, -1.0, 0.0), 7.0, 0), ((1.0, 0.0, 0.0), 1.0, 1), ((-1.0, 0.0, 0.0), 7.0, 2),
               ((0.0, 0.0, 1.0), 6.0, 0), ((0.0, 0.0, -1.0), 7.0, 0))
SPOT = ("spot", (3.5, 5.0, 2.0), (1.0, 0.0, 0.0), 3.1415 / 4.0, (0.9, 0.9, 0.8))


def probes_of(P):
    return {"rres": P.Radiance_Resolution, "ires": P.Irradiance_Resolution, "count": P.Probe_Count, "dims": P.Grid_Dimensions,
            "spacing": P.Grid_Spacing, "settings": P}


def room(second_sphere=False, lights=(SPOT,), probes=SMALL_PROBES, clear_of_probes=False):
    """the global_illumination example's room (examples/global_illumination/main.adb:29-74)"""
    prims = [("Plane", n, o, m) for n, o, m in ROOM_PLANES] + [("Sphere", (3.0, 4.0, 3.0), 1.0, 3), ("Box", (3.0, 0.0, 4.0), (1.5, 1.5, 1.5), 4)]
    if clear_of_probes:
        # The radiance pass's room.  A probe that stands inside a primitive starts its rays on a negative distance and shades
        # ITS OWN POSITION, where sample_irradiance divides 0 by 0 (render_probes.glsl:22-24): the example's room holds two such
        # probes of SMALL_PROBES and seventeen of ODD_PROBES (whose top layer is above the ceiling).  Here the ceiling is
        # at y = 9 and the sphere and the box stand between the probes of both grids; the census is the room's.
        prims = [("Plane", n, 9.0 if n == (0.0, -1.0, 0.0) else o, m) for n, o, m in ROOM_PLANES] + [
            ("Sphere", (2.4, 4.75, 3.75), 1.0, 3), ("Box", (3.0, 1.0, 4.0), (1.5, 0.85, 1.5), 4)]
    if second_sphere:
        prims.append(("Sphere", (0.8, 0.2, 3.2), 0.7, 4))
    kinds = sorted({l[0] for l in lights})
    return {"kinds": [("Sphere", 20), ("Plane", 10), ("Box", 10)], "prims": prims, "light_kinds": [(k, 4) for k in kinds], "lights": list(lights),
            "materials": [((0.0, 0.0, 0.0), 0.0, 0.6), ((1.0, 0.0, 0.0), 0.0, 0.6), ((0.0, 0.0, 1.0), 0.0, 0.6), ((0.1, 0.1, 0.1), 0.9, 0.1),
                          ((0.0, 1.0, 0.0), 0.8, 0.3)],
            "max_dist": 20.0, "cam_pos": (2.0, 2.0, 0.0), "cam_m": np.eye(3), "ao_steps": 3, "spec_mode": 2, "probes": probes_of(probes)}


def open_scene(probes=SMALL_PROBES):
    """a floor, two spheres and a small triangle under the sky (like test_open_scene_with_few_hits_per_wavefront)"""
    return {"kinds": [("Sphere", 4), ("Plane", 2), ("Triangle", 2)],
            "prims": [("Plane", (0.0, 1.0, 0.0), 1.0, 0), ("Sphere", (2.0, 0.5, 4.0), 1.2, 1), ("Sphere", (4.5, 2.5, 3.0), 0.6, 0),
                      ("Triangle", (0.2, 2.6, 4.5), (0.9, 3.4, 4.8), (-0.3, 3.3, 5.0), 2)],
            "light_kinds": [("point", 2)], "lights": [("point", (3.0, 6.0, 1.0), (0.9, 0.9, 0.8))],
            "materials": [((0.7, 0.7, 0.7), 0.0, 0.6), ((0.9, 0.2, 0.1), 0.8, 0.2), ((0.1, 0.3, 0.9), 0.0, 0.9)],
            "max_dist": 20.0, "cam_pos": (2.5, 1.5, -1.0), "cam_m": np.eye(3), "ao_steps": 3, "spec_mode": 2, "probes": probes_of(probes)}


def rotation():
    """a rotation about two axes; the matrix is not symmetric, so its transpose is another camera"""
    a, b = 0.35, -0.2
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    m = (ry @ rx).astype(np.float32)
    assert np.abs(m - m.T).max() > 0.05
    return m


SCENES = {"room": room, "open": open_scene}


def describe(scene, camera="identity", ao=3, spec=2, **kw):
    d = SCENES[scene](**kw)
    if camera == "rotated":
        d["cam_m"] = rotation()
        d["cam_pos"] = (3.0, 2.5, -1.0) if scene == "room" else (3.2, 2.0, -1.5)
    d["ao_steps"], d["spec_mode"] = ao, spec
    return d


def make_renderer(desc, W, H, binding, mode=0, atlas=1):
    """the description through the host API; nothing here is shared with ref64"""
    assert desc["max_dist"] == 20.0  # scenes.ads:51, the default every case keeps
    scene = scenes.Compile([(KINDS[k][0], n) for k, n in desc["kinds"]], [(LIGHTS[k][0], n) for k, n in desc["light_kinds"]],
                           Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(W, H, "ref64"), scene, Probes=desc["probes"]["settings"], Volumetrics=renderers.No_Volumetrics, Binding=binding)
    for i, (a, m, r) in enumerate(desc["materials"]):
        R.Set_Material(i, materials.Create(a, m, r))
    for p in desc["prims"]:
        R.Add_Primitive(KINDS[p[0]][0], KINDS[p[0]][1](*p[1:]))
    # Set_Light (Index, ..) leaves the kind's count AND the total at Index, and the light loop walks the kinds by cumulative
    # counts (madarch-renderers.adb:478-482): after each kind's lights, the last kind is padded with dark lights
    # up to the total, which the walk never reaches
    order = [k for k, _ in desc["light_kinds"]]
    assert [l[0] for l in desc["lights"]] == sorted((l[0] for l in desc["lights"]), key=order.index)
    count = 0
    for kind in order:
        count = 0
        for l in desc["lights"]:
            if l[0] == kind:
                count += 1
                R.Set_Light(count, LIGHTS[kind][0], LIGHTS[kind][1](*l[1:]))
    if count != len(desc["lights"]):
        dark = {"point": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), "spot": ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.5, (0.0, 0.0, 0.0))}[order[-1]]
        R.Set_Light(len(desc["lights"]), LIGHTS[order[-1]][0], LIGHTS[order[-1]][1](*dark))
    R.Set_Camera_Position(desc["cam_pos"])
    R.Set_Camera_Orientation(np.asarray(desc["cam_m"], dtype=np.float32).tolist())
    R.Set_Option(B.OPT_SCREEN_MODE, mode)
    R.Set_Option(B.OPT_ATLAS_FORMAT, atlas)
    R.Set_Option(B.OPT_GBUFFER, 1)
    R.Set_Option(B.OPT_AO_STEPS, desc["ao_steps"])
    R.Set_Option(B.OPT_INDIRECT_SPECULAR, desc["spec_mode"])
    return R


def atlases(desc, seed, levels=None):
    """seeded random atlases; with `levels` every value is a multiple of 1 / levels (exact in the RGB8 format)"""
    p = desc["probes"]
    rng = np.random.RandomState(seed)
    out = []
    for res in (p["ires"], p["rres"]):
        shape = (p["count"][1] * res, p["count"][0] * res, 3)
        a = rng.randint(0, levels + 1, size=shape) / float(levels) if levels else rng.uniform(0.0, 1.0, size=shape)
        out.append(a.astype(np.float32))
    return out  # irradiance, radiance


_cache = {}


def cached(key, compute):
    if key not in _cache:
        _cache[key] = compute()
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- frames
def run_screen(binding, name, scene, W, H, mode, camera="identity", ao=3, spec=2, scene_kw=None, prepare=None, frames=1, burst=0):
    """one screen pass (modes 1 and 2: `frames` whole frames through Render; mode 0: Render_Pass (PASS_SCREEN) alone over
    written atlases, so that the probe feedback does not compound and every tap reads known data) against ref64.screen.
    `burst` whole frames through Render come first and are not waited for: what is read afterwards is ordered behind them."""
    scene_kw = scene_kw or {}
    desc = describe(scene, camera, ao, spec, **scene_kw)
    irr, rad = atlases(desc, SEED % 1000 + 3) if mode == 0 else (None, None)
    key = ("screen", scene, W, H, mode, camera, ao, spec, tuple(sorted(scene_kw.items())))
    runs = cached(key, lambda: ref64.three_runs(lambda seed: ref64.screen(desc, W, H, mode, irr, rad, seed=seed)))
    R = make_renderer(desc, W, H, binding, mode=mode)
    if prepare is not None:
        prepare(R)
    for _ in range(burst):
        R.Render()
    if mode == 0:
        R.Write_Texture(B.TEX_IRRADIANCE, irr)
        R.Write_Texture(B.TEX_RADIANCE, rad)
        R.Render_Pass(B.PASS_SCREEN)
    else:
        for _ in range(frames):
            R.Render()
    fb = R.Read_Framebuffer()
    index, t, _ = R.Read_Gbuffer()
    R.Destroy()
    if mode == 1:
        # 0.5 n + 0.5: a hit displaced by the march tolerance dt on a surface whose smallest radius of curvature is r turns the
        # normal by at most dt / r; planes and boxes (away from the box-normal switch, which the jitter finds) are exact
        radii = [float(p[2]) for p in desc["prims"] if p[0] == "Sphere"]
        tol = 0.5 * ref64.T_ATOL / min(radii) + 4.0 * 2.0 ** -24 if radii else 4.0 * 2.0 ** -24
        return ref64.hold(name, runs, fb, index, t, rtol=0.0, atol=tol)
    return ref64.hold(name, runs, ref64.undo_tone_map(fb), index, t)


def run_radiance(binding, name, probes, atlas, prepare=None):
    """one Render_Pass (PASS_RADIANCE) over written atlases, the whole atlas image, two lights (one a spot light)"""
    lights = (("point", (1.5, 5.5, 4.5), (0.6, 0.5, 0.4)), SPOT)
    desc = room(lights=lights, probes=probes, clear_of_probes=True)
    irr, rad = atlases(desc, SEED % 1000 + 5, levels=255 if atlas == 0 else None)
    key = ("radiance", probes.Probe_Count, atlas)
    runs = cached(key, lambda: ref64.three_runs(lambda seed: ref64.radiance_texels(desc, irr, rad, seed=seed)))
    R = make_renderer(desc, 8, 8, binding, atlas=atlas)
    if prepare is not None:
        prepare(R)
    R.Write_Texture(B.TEX_IRRADIANCE, irr)
    R.Write_Texture(B.TEX_RADIANCE, rad)
    if atlas == 0:
        assert np.array_equal(R.Read_Texture(B.TEX_IRRADIANCE), irr)  # (multiples of 1 / 255 survive the RGB8 format)
    R.Render_Pass(B.PASS_RADIANCE)
    got = R.Read_Texture(B.TEX_RADIANCE)
    R.Destroy()
    if atlas == 0:
        return ref64.hold(name, runs, got, more_atol=0.5 / 255.0, clamp=True)
    return ref64.hold(name, runs, got)


# ---------------------------------------------------------------------------------------- Eval_Distances_To
TRIANGLES = [((0.5, 0.5, 1.0), (2.5, 0.8, 1.2), (1.0, 2.4, 0.6)),          # well shaped
             ((3.0, 3.0, 3.0), (6.5, 3.1, 3.2), (4.7, 3.12, 3.1)),         # long and thin: 3.5 long, 0.07 high
             ((5.0, 0.5, 4.0), (5.9, 1.4, 4.6), (5.45, 0.953, 4.3))]       # nearly degenerate: its third vertex 3 mm off the edge


def distance_scene():
    return {"kinds": [("Sphere", 8), ("Plane", 8), ("Box", 8), ("Triangle", 8)],
            "prims": [("Plane", n, o, m) for n, o, m in ROOM_PLANES] + [("Plane", (0.6, 0.8, 0.0), 0.5, 1)] +
                     [("Sphere", (3.0, 4.0, 3.0), 1.0, 3), ("Sphere", (1.0, 1.0, 5.0), 0.4, 3), ("Box", (3.0, 0.0, 4.0), (1.5, 1.5, 1.5), 4),
                      ("Box", (5.5, 5.0, 1.0), (0.3, 0.9, 0.5), 4)] + [("Triangle", a, b, c, 2) for a, b, c in TRIANGLES],
            "light_kinds": [("point", 2)], "lights": [("point", (3.0, 6.0, 1.0), (0.9, 0.9, 0.8))],
            "materials": [((0.7, 0.7, 0.7), 0.0, 0.6)] * 5, "max_dist": 20.0, "cam_pos": (2.0, 2.0, 0.0), "cam_m": np.eye(3), "ao_steps": 3,
            "spec_mode": 2, "probes": probes_of(SMALL_PROBES)}


def distance_points(n, seed):
    """seeded points through the room, plus points inside the spheres and boxes, near the boxes' edges, and round the
    triangles: over their faces, beyond their edges and beyond their vertices"""
    rng = np.random.RandomState(seed)
    desc = distance_scene()
    pts = [rng.uniform((-0.9, -0.9, -5.9), (6.9, 6.9, 6.9), size=(n // 2, 3))]
    m = max(n // 16, 1)
    for p in desc["prims"]:
        if p[0] == "Sphere":
            d = rng.normal(size=(m, 3))
            pts.append(np.asarray(p[1]) + d / np.linalg.norm(d, axis=1, keepdims=True) * p[2] * rng.uniform(0.05, 1.6, size=(m, 1)))
        elif p[0] == "Box":
            pts.append(np.asarray(p[1]) + np.asarray(p[2]) * rng.uniform(-1.4, 1.4, size=(m, 3)))                 # inside and round it
            e = np.where(rng.uniform(size=(m, 3)) < 0.7, rng.choice([-1.0, 1.0], size=(m, 3)), rng.uniform(-1, 1, size=(m, 3)))
            pts.append(np.asarray(p[1]) + np.asarray(p[2]) * e + rng.normal(size=(m, 3)) * 0.05)                   # edges and corners
            # round the normal's switching surfaces |d_i| = |d_j| - 0.002: on them, 3e-6 to either side (inside hold_distances'
            # band) and 1e-4 to either side (outside it: held)
            r = rng.uniform(0.2, 1.3, size=(m, 3))
            i, j = rng.randint(0, 3, size=m), rng.randint(1, 3, size=m)
            j = (i + j) % 3
            r[np.arange(m), i] = r[np.arange(m), j] - 0.002 + rng.choice([0.0, -3e-6, 3e-6, -1e-4, 1e-4], size=m)
            pts.append(np.asarray(p[1]) + np.asarray(p[2]) * r * rng.choice([-1.0, 1.0], size=(m, 3)))
        elif p[0] == "Triangle":
            a, b, c = (np.asarray(v) for v in p[1:4])
            w = rng.uniform(-0.6, 1.3, size=(2 * m, 3))                                                            # face, edge and vertex regions
            bary = np.stack([w[:, 0], w[:, 1], 1.0 - w[:, 0] - w[:, 1]], axis=1)
            nor = np.cross(b - a, c - a)
            nor /= np.linalg.norm(nor)
            pts.append(bary @ np.stack([a, b, c]) + nor * rng.normal(size=(2 * m, 1)) * 0.4)
    return np.concatenate(pts).astype(np.float32)


KIND_SETS = [("Sphere",), ("Plane",), ("Box",), ("Triangle",), ("Box", "Sphere", "Triangle"), ("Triangle", "Plane", "Box", "Sphere")]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def hold_distances(name, desc, kinds, pts, dist, nrm):
    """Distances to binary32 rounding of the float64 value, normals as well outside the bands stated here.

    Distance: a primitive's distance is computed from differences of coordinates, each rounded once, so its error is
    a few ulps of the LARGEST number that enters it, not of the result: 8 ulp32 of max (|p|, |d|), for every kind, thin and
    nearly degenerate triangles included.
    Normal: 1e-5, except
      * within 1e-5 (relative to the side) of a box's switching surfaces |d_i| = |d_j| - 0.002 (boxes.adb:5,23-26), where the
        two precisions may pick different axes;
      * on a triangle: see ref64.hold's triangle_normal_noise -- a component's error is (the distance's error, twice, plus
        one ulp of the coordinate) / h with h = 1e-6, so only the side of the triangle is held: the normal's dot product with the float64
        normal must be positive, away from the triangle's plane by more than 1e-4."""
    sc = ref64.Scene(desc)
    want_d, want_n, arg = ref64.distance(desc, kinds, pts)
    P = pts.astype(np.float64)
    scale = np.maximum(np.abs(P).max(axis=1), np.abs(want_d))
    tol = 8.0 * ulp32(scale)
    err = np.abs(dist.astype(np.float64) - want_d)
    print("%s: %d points, largest distance error %.3g (%.2f of its tolerance)" % (name, len(pts), err.max(), (err / tol).max()))
    bad = err > tol
    assert not bad.any(), "%s: %d distances off, first %s: got %r, float64 %r (tolerance %.3g)" % (
        name, bad.sum(), pts[bad][0], dist[bad][0], want_d[bad][0], tol[bad][0])
    kind = sc.kind[arg]
    band = np.zeros(len(pts), dtype=bool)
    for k, prim in enumerate(sc.prims):
        if prim[0] == "Box":
            r = np.abs((P - prim[1][0]) / prim[1][1])
            near = np.zeros(len(pts), dtype=bool)
            for i in range(3):
                for j in range(3):
                    if i != j:
                        near |= np.abs(r[:, i] - (r[:, j] - 0.002)) < 1e-5
            band |= near & (arg == k)
    tri = kind == 3
    smooth = ~tri & ~band
    nerr = np.abs(nrm.astype(np.float64) - want_n).max(axis=1)
    print("%s: %d normals held to 1e-5 (largest error %.3g), %d in a box's band, %d on triangles" % (
        name, smooth.sum(), nerr[smooth].max() if smooth.any() else 0.0, band.sum(), tri.sum()))
    assert (nerr[smooth] <= 1e-5).all(), "%s: normal off at %s" % (name, pts[smooth][np.argmax(nerr[smooth])])
    side = tri & (want_d > 1e-4)
    if side.any():
        dots = (nrm.astype(np.float64) * want_n).sum(axis=1)[side]
        print("%s: %d triangle normals, smallest dot product with float64 %.3f" % (name, side.sum(), dots.min()))
        assert (dots > 0.0).all(), "%s: a triangle's normal on the wrong side at %s" % (name, pts[side][np.argmin(dots)])
    return want_d, arg


def run_distance(binding, name, kinds, count=None, seed=SEED % 1000 + 11, prepare=None):
    """`count` None: the whole seeded set (about 5000 points); otherwise that many of them, drawn without replacement"""
    desc = distance_scene()
    pts = distance_points(4000, seed)
    if count is not None:
        pts = pts[np.random.RandomState(seed + 1).permutation(len(pts))[:count]]
        assert len(pts) == count
    R = make_renderer(desc, 8, 8, binding)
    R.Set_Option(B.OPT_ADA_EVAL_DIV, 0)  # the geometric truth is that of the GLSL division (test_values_division_bug_is_reproduced has the other)
    if prepare is not None:
        prepare(R)
    dist, nrm = R.Eval_Distances_To(pts, [KINDS[k][0] for k in kinds])
    R.Destroy()
    assert len(dist) == len(pts)
    return hold_distances(name, desc, kinds, pts, dist, nrm)
