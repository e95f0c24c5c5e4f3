"""The cases of test_ref64_oracle.py and test_ref64_partition_oracle.py (the oracle) and of test_gpu_ref64.py,
test_gpu_ref64_passes.py and test_gpu_ref64_partition.py (the HIP library): each is one plain scene
description, built once as a renderer over the binding under test and once as ref64's float64 scene, and held by
ref64.hold.  The float64 results are cached per process, so the two files never compute a case twice in one run."""
import numpy as np

import ref64
from helpers import ODD_PROBES, SEED, SMALL_PROBES
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


def vol_of(V):
    return {"vres": V.Visibility_Resolution, "vstep": V.Visibility_Step_Size, "sres": V.Scattering_Resolution, "sstep": V.Scattering_Step_Size,
            "settings": V}


def volume(vres=(8, 8, 8), vstep=0.1, sres=(24, 24), sstep=0.1):
    return renderers.Volumetrics_Settings(Visibility_Resolution=vres, Visibility_Step_Size=vstep, Scattering_Resolution=sres, Scattering_Step_Size=sstep)


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
    pt = desc.get("partition")
    partitioning = scenes.Partitioning_Settings(Enable=False) if pt is None else scenes.Partitioning_Settings(
        Enable=True, Index_Count=pt["index_count"], Border_Behavior={"Clamp": scenes.Clamp, "Fallback": scenes.Fallback}[pt["border"]],
        Grid_Dimensions=pt["dims"], Grid_Spacing=pt["spacing"], Grid_Offset=pt["offset"])
    scene = scenes.Compile([(KINDS[k][0], n) for k, n in desc["kinds"]], [(LIGHTS[k][0], n) for k, n in desc["light_kinds"]],
                           Partitioning=partitioning)
    volumetrics = desc["vol"]["settings"] if desc.get("vol") else renderers.No_Volumetrics
    R = renderers.Create(windows.Open(W, H, "ref64"), scene, Probes=desc["probes"]["settings"], Volumetrics=volumetrics, Binding=binding)
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
def scattering_texture(vol, seed):
    """the pin's distribution (test_oracle_pins64.py:230-231): rgb uniform (0, 1), the stored length uniform (0.5, 9)"""
    rng = np.random.RandomState(seed)
    sw, sh = vol.Scattering_Resolution
    scat = rng.uniform(0.0, 1.0, size=(sh, sw, 4)).astype(np.float32)
    scat[..., 3] = rng.uniform(0.5, 9.0, size=(sh, sw))
    return scat


def run_screen(binding, name, scene, W, H, mode, camera="identity", ao=3, spec=2, scene_kw=None, prepare=None, frames=1, burst=0, vol=None):
    """one screen pass (modes 1 and 2: `frames` whole frames through Render; mode 0: Render_Pass (PASS_SCREEN) alone over
    written atlases, so that the probe feedback does not compound and every tap reads known data) against ref64.screen.
    `vol` (mode 0): volumetric settings; the scattering texture is written as well and composed into every pixel.
    `burst` whole frames through Render come first and are not waited for: what is read afterwards is ordered behind them."""
    scene_kw = scene_kw or {}
    desc = describe(scene, camera, ao, spec, **scene_kw)
    irr, rad = atlases(desc, SEED % 1000 + 3) if mode == 0 else (None, None)
    scat = None
    if vol is not None:
        assert mode == 0
        desc["vol"] = vol_of(vol)
        scat = scattering_texture(vol, SEED % 1000 + 13)
    key = ("screen", scene, W, H, mode, camera, ao, spec, tuple(sorted(scene_kw.items())), vol and tuple(vol.Scattering_Resolution))
    runs = cached(key, lambda: ref64.three_runs(lambda seed: ref64.screen(desc, W, H, mode, irr, rad, seed=seed, scattering=scat)))
    R = make_renderer(desc, W, H, binding, mode=mode)
    if prepare is not None:
        prepare(R)
    for _ in range(burst):
        R.Render()
    if mode == 0:
        R.Write_Texture(B.TEX_IRRADIANCE, irr)
        R.Write_Texture(B.TEX_RADIANCE, rad)
        if scat is not None:
            R.Write_Texture(B.TEX_SCATTERING, scat)
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


# ---------------------------------------------------------------------------------------- the irradiance fold
def grid_probes(rres, ires, count=(4, 2), dims=(2, 2, 2), spacing=(2.0, 3.0, 3.0)):
    return renderers.Probe_Settings(Radiance_Resolution=rres, Irradiance_Resolution=ires, Probe_Count=count, Grid_Dimensions=dims, Grid_Spacing=spacing)


# (rres, ires): see tests/test_gpu_ref64_passes.py for what each reaches
IRRADIANCE_SHAPES = [(8, 8), (16, 8), (5, 2), (12, 6), (10, 3), (8, 10), (8, 17), (48, 16)]


def irradiance_probes(rres, ires):
    """eight probes, (4, 2) tiles over a 2 x 2 x 2 grid; (12, 6) is ODD_PROBES, 15 x 5 tiles"""
    return ODD_PROBES if (rres, ires) == (12, 6) else grid_probes(rres, ires)


def tap_ray_ids(probes, dtype):
    """fract (c * probe_count) of every tap of every probe (update_probe_irradiance.glsl:19,26-33, probe_utils.glsl:52-56,80-82),
    each operation once in `dtype`"""
    f = dtype
    rres = probes.Radiance_Resolution
    out = []
    for axis in (0, 1):
        pc = probes.Probe_Count[axis]
        step = f(f(f(1.0) / f(pc)) / f(rres))
        base = (np.arange(pc).astype(f) / f(pc)).astype(f)
        c = (base[:, None] + (np.arange(rres).astype(f) * step).astype(f)[None, :]).astype(f)
        c = np.clip(c, step, f(f(1.0) - step)).astype(f)
        x = (c * f(pc)).astype(f)
        out.append((x - np.floor(x)).astype(np.float64))
    return out


def assert_taps_on_one_side(probes):
    """The input condition of run_irradiance.  A tap sits on a texel CORNER, and the corner of a tile's first texel is the tile's
    border: there fract (c * probe_count) is 0 on one side and nearly 1 on the other, and the two decode to different
    directions.  Which side a tap lands on is decided by one rounding; a setting is held only if float64 and binary32 land
    every tap on the same side (no ray id differs by more than 1e-3)."""
    for a, b in zip(tap_ray_ids(probes, np.float64), tap_ray_ids(probes, np.float32)):
        assert np.abs(a - b).max() <= 1e-3, "a tap of %r lands on the other side of its tile's border in binary32" % (probes.Probe_Count,)


def run_irradiance(binding, name, probes, atlas, hysteresis=0, sparse=False, passes=1):
    """Render_Pass (PASS_IRRADIANCE) over a written radiance atlas, the whole irradiance atlas against ref64.irradiance_texels.
    The input: uniform (0, 1) (RGB8: multiples of 1 / 255, exact in the format), or `sparse` (fp32 only): 15 of 16 texels 0, the
    rest uniform (0, 64) -- a tap taken from the wrong lane, chunk or turn then moves a texel by tens of per cent, not by 1 / ntaps.
    `hysteresis` (per mille): a seeded irradiance atlas is written as the previous frame's.
    `passes` > 1: that many passes on one renderer, each over another atlas (the kernel's scratch is reused); the last is held.

    Tolerance: numerator and denominator are sequential binary32 sums of non-negative terms, each with a relative error of at
    most (ntaps - 1) 2^-24, plus a few ulps per tap for the filter and the decode; whatever the values, non-negative terms
    keep that bound relative to the sum.  The pin's rtol = 2e-4, atol = 1e-6 (test_oracle_pins.py:457) holds at 1024 taps; for
    larger tiles rtol = 4 ntaps 2^-24 (twice the two sums' bound).  RGB8 adds half a step of the format and the clamp to
    [0, 1]; mix () is a convex combination and adds nothing."""
    assert not (sparse and atlas == 0)
    assert_taps_on_one_side(probes)
    desc = room(probes=probes)
    ntaps = probes.Radiance_Resolution ** 2
    rtol = max(2e-4, 4.0 * ntaps * 2.0 ** -24)
    rng = np.random.RandomState(SEED % 1000 + 17)
    P = desc["probes"]
    R = make_renderer(desc, 8, 8, binding, atlas=atlas)
    R.Set_Option(B.OPT_HYSTERESIS_PERMILLE, hysteresis)
    for _ in range(passes):
        irr, rad = atlases(desc, rng.randint(1 << 30), levels=255 if atlas == 0 else None)
        if sparse:
            rad = (rng.uniform(0.0, 64.0, size=rad.shape) * (rng.randint(0, 16, size=rad.shape[:2]) == 0)[..., None]).astype(np.float32)
        R.Write_Texture(B.TEX_RADIANCE, rad)
        if hysteresis:
            R.Write_Texture(B.TEX_IRRADIANCE, irr)
        R.Render_Pass(B.PASS_IRRADIANCE)
        got = R.Read_Texture(B.TEX_IRRADIANCE)
    R.Destroy()
    key = ("irradiance", P["rres"], P["ires"], tuple(P["count"]), atlas, hysteresis, sparse, passes)
    want = cached(key, lambda: ref64.irradiance_texels(desc, rad, irr, hysteresis / 1000.0))
    if atlas == 0:
        return ref64.hold_values(name, [{"colour": want}], got, rtol, 1e-6, more_atol=0.5 / 255.0, clamp=True)
    return ref64.hold_values(name, [{"colour": want}], got, rtol, 1e-6)


def run_mips(binding, name, atlas):
    """MDH_OPT_RADIANCE_MIPS over a written atlas of SMALL_PROBES: every level read back against the float64 box of the level
    below AS READ BACK (level 0: the atlas written), which holds the whole chain by induction and lets the bound be a
    single box's: fp32, (a + b) + (c + d) then * 0.25 is three roundings, at most 1 ulp of the largest input -- held to 2;
    RGB8, half a step of the format (and the fp32 sum's ulp)."""
    desc = room()
    _, rad = atlases(desc, SEED % 1000 + 19, levels=255 if atlas == 0 else None)
    R = make_renderer(desc, 8, 8, binding, atlas=atlas)
    R.Write_Texture(B.TEX_RADIANCE, rad)
    R.Set_Option(B.OPT_RADIANCE_MIPS, 1)
    lods = int(np.log2(desc["probes"]["rres"]))
    below, worst = rad, 0.0
    for l in range(1, lods + 1):
        got = R.Read_Texture(B.TEX_RADIANCE_MIP0 + l)
        want = ref64.radiance_mips(below, 1)[1]
        assert got.shape == want.shape
        b = below.astype(np.float64)
        largest = np.maximum(np.maximum(b[0::2, 0::2], b[0::2, 1::2]), np.maximum(b[1::2, 0::2], b[1::2, 1::2]))
        tol = 2.0 * ulp32(largest) if atlas == 1 else 0.5 / 255.0 + 2.0 * ulp32(largest)
        err = np.abs(got.astype(np.float64) - want) / tol
        worst = max(worst, float(err.max()))
        assert (err <= 1.0).all(), "%s: level %d off at %s" % (name, l, np.argwhere(err > 1.0)[0])
        below = got
    R.Destroy()
    assert below.shape[:2] == (desc["probes"]["count"][1], desc["probes"]["count"][0])  # one texel per probe
    print("%s: %d levels, largest error %.3f of its tolerance" % (name, lods, worst))
    return worst


# ---------------------------------------------------------------------------------------- the volumetric passes
SHAFT = ("point", (5.0, 3.0, 6.0), (0.9, 0.9, 0.9))  # examples/light_shafts/main.adb:59
# a spot light above the camera's frustum that looks down into it (SPOT looks along +x, past every froxel volume here); its
# direction is a unit vector to four digits: the light's code does not normalise it, and neither side does here
DOWN_SPOT = ("spot", (3.5, 5.0, 2.0), (-0.4423, -0.8847, -0.1474), 3.1415 / 4.0, (0.9, 0.9, 0.8))
FROXEL_RTOL, FROXEL_ATOL = 3e-4, 1e-7                # test_oracle_pins64.py:186
SCATTER_RTOL, SCATTER_ATOL = 5e-4, 1e-7              # test_oracle_pins64.py:220


def vol_scene(scene, camera="identity"):
    """the scene with two lights, a point light (the light_shafts example's) and the spot light: the pins only see one point light"""
    d = describe(scene, camera)
    d["light_kinds"], d["lights"] = [("point", 4), ("spot", 4)], [SHAFT if scene == "room" else d["lights"][0], DOWN_SPOT]
    return d


def run_froxels(binding, name, vol, scene="room", camera="identity"):
    """Render_Pass (PASS_VISIBILITY), the whole froxel texture against ref64.froxel_texels; fragile: the three runs and `near`"""
    desc = vol_scene(scene, camera)
    key = ("froxels", scene, camera, vol.Visibility_Resolution, vol.Visibility_Step_Size)
    runs = cached(key, lambda: ref64.three_runs(lambda seed: ref64.froxel_texels(desc, vol_of(vol), seed=seed)))
    desc["vol"] = vol_of(vol)
    R = make_renderer(desc, 8, 8, binding)
    R.Render_Pass(B.PASS_VISIBILITY)
    got = R.Read_Texture(B.TEX_VISIBILITY)
    R.Destroy()
    lit = (runs[0]["colour"].max(axis=-1) > 0.0).mean()
    assert 0.3 < lit, "%s: only %.2f of the froxels are lit" % (name, lit)
    return ref64.hold_values(name, runs, got, FROXEL_RTOL, FROXEL_ATOL)


def run_scattering(binding, name, vol, scene="room", camera="identity", written=True, moved=False):
    """written: a seeded froxel texture (uniform 0 .. 1) is written and Render_Pass (PASS_SCATTERING) runs alone, so that no
    froxel's fragility leaks in.  Otherwise one whole Render () -- the only way to the march fused into the visibility
    pass's launch -- or, `moved`, the pair Render_Pass (PASS_VISIBILITY), Render_Pass (PASS_SCATTERING) after a camera move
    (outside a frame the scattering pass marches its own rays); the scattering texture is then held against
    ref64.scattering_texels over the froxel texture READ BACK from the binding, as the pins isolate passes."""
    desc = vol_scene(scene, camera)
    desc["vol"] = vol_of(vol)
    vw, vh, vz = vol.Visibility_Resolution
    R = make_renderer(desc, 8, 8, binding)
    if written:
        vis = np.random.RandomState(SEED % 1000 + 23).uniform(0.0, 1.0, size=(vh * vz, vw, 3)).astype(np.float32)
        R.Write_Texture(B.TEX_VISIBILITY, vis)
        R.Render_Pass(B.PASS_SCATTERING)
    elif moved:
        R.Render()
        desc["cam_pos"] = tuple(np.asarray(desc["cam_pos"]) + np.array([0.4, -0.3, 0.5]))
        R.Set_Camera_Position(desc["cam_pos"])
        R.Render_Pass(B.PASS_VISIBILITY)
        R.Render_Pass(B.PASS_SCATTERING)
        vis = R.Read_Texture(B.TEX_VISIBILITY)
    else:
        R.Render()
        vis = R.Read_Texture(B.TEX_VISIBILITY)
    got = R.Read_Texture(B.TEX_SCATTERING)
    R.Destroy()
    key = ("scattering", scene, camera, vol.Visibility_Resolution, vol.Visibility_Step_Size, vol.Scattering_Resolution, vol.Scattering_Step_Size, moved)
    # (the marches do not depend on the froxel texture: the three runs' lengths are cached, the fold is over `vis`)
    runs = ref64.three_runs(lambda seed: ref64.scattering_texels(desc, vol_of(vol), vis, seed=seed)) if not written else cached(
        key, lambda: ref64.three_runs(lambda seed: ref64.scattering_texels(desc, vol_of(vol), vis, seed=seed)))
    return ref64.hold_values(name, runs, got[..., :3], SCATTER_RTOL, SCATTER_ATOL, length=got[..., 3])


# the froxel volumes: each reaches one of the three froxel-to-lane layouts (tests/test_gpu_ref64_passes.py)
# (the steps are as deep as the room allows with at most 5 % of the sample points within NEAR_SURFACE of a surface or inside the
#  sphere or the box; about a third of the froxels are in shadow or outside the spot light's cone)
FROXEL_CASES = {"blocks 8x8x8": {"vol": volume((8, 8, 8), 0.4)}, "tiles 24x6x4": {"vol": volume((24, 6, 4), 0.9)},
                "rows 10x7x3": {"vol": volume((10, 7, 3), 1.2)}, "rows 10x7x3 open": {"vol": volume((10, 7, 3), 1.6), "scene": "open"},
                "blocks 8x8x8 rotated": {"vol": volume((8, 8, 8), 0.4), "camera": "rotated"}}
SCATTERING_CASES = {
    "23x21": {"vol": volume((6, 5, 8), 0.5, (23, 21), 0.1)},
    "17x5 ten coarse steps": {"vol": volume((6, 5, 8), 0.5, (17, 5), 0.4)},
    "128 steps": {"vol": volume((6, 5, 16), 0.1, (17, 5), 0.0125)},
    "several chunks": {"vol": volume((6, 5, 16), 0.2, (17, 5), 0.007)},
    "equal steps": {"vol": volume((6, 5, 24), 0.2, (17, 5), 0.2)},
    "frame room": {"vol": volume((8, 8, 8), 0.5, (23, 21), 0.1), "written": False},
    "frame open": {"vol": volume((10, 7, 3), 1.5, (17, 5), 0.1), "scene": "open", "written": False},
    "passes after a move": {"vol": volume((8, 8, 8), 0.5, (23, 21), 0.1), "written": False, "moved": True},
    "frame room rotated": {"vol": volume((8, 8, 8), 0.5, (23, 21), 0.1), "camera": "rotated", "written": False},
}


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


# ---------------------------------------------------------------------------------------- the space partition
SIMPLE_SPHERES = [(x, y, z) for y, z, xs in ((3.5, 2.0, (0.5, 1.5, 2.5, 3.5, 4.5, 5.5)), (0.5, 2.0, (0.5, 1.5, 2.5, 3.5, 4.5, 5.5)),
                                             (3.5, 5.0, (0.5, 1.5, 2.5, 3.5, 4.5, 5.5)), (0.5, 5.0, (0.5, 1.5))) for x in xs]
MORE_SPHERES = [(x, 0.5, 5.0) for x in (2.5, 3.5, 4.5, 5.5)] + [(x, 2.0, 3.5) for x in (0.5, 1.5, 2.5, 3.5, 4.5, 5.5)] + [
    (x, 5.5, 3.5) for x in (0.5, 1.5, 2.5, 3.5)]
SIMPLE_BOXES = [((3.0, 1.0, 2.0), (0.5, 0.5, 0.5)), ((0.0, 1.0, 2.0), (0.3, 0.3, 0.5)), ((3.0, 1.0, 4.0), (0.5, 0.5, 0.5)),
                ((4.0, 2.0, 2.0), (0.5, 0.5, 0.5)), ((2.0, 2.0, 2.0), (0.5, 0.5, 0.5)), ((1.0, 1.0, 6.0), (0.5, 0.5, 0.5)),
                ((3.0, 1.0, 6.0), (0.5, 0.5, 0.5))]
SMALL_TRIANGLES = [((2.8, 2.6, 3.0), (3.2, 2.6, 3.1), (3.0, 3.0, 3.05)), ((1.0, 2.2, 3.5), (1.4, 2.2, 3.6), (1.2, 2.6, 3.5))]


def rows(variant="plain", probes=SMALL_PROBES):
    """The simple_scene example's room (examples/simple_scene/main.adb): its planes, its 20 spheres in rows and the first seven
    of its boxes, under its point light, seen by a rotated camera.  Variants: "34 spheres" of 40 declared (more than 32 of a
    kind, 70 declared primitives: three mask words in the library's bit form), "triangles" (two small ones, declared and
    added), "two radii" (the spheres alternate between 0.5 and 0.2)."""
    assert variant in ("plain", "34 spheres", "triangles", "two radii")
    kinds = [("Sphere", 40 if variant == "34 spheres" else 20), ("Plane", 10), ("Box", 20)]
    centres = SIMPLE_SPHERES + (MORE_SPHERES if variant == "34 spheres" else [])
    prims = [("Plane", n, o, m) for n, o, m in ROOM_PLANES]
    prims += [("Sphere", c, 0.2 if variant == "two radii" and i % 2 else 0.5, 3) for i, c in enumerate(centres)]
    prims += [("Box", c, s, 2) for c, s in SIMPLE_BOXES]
    if variant == "triangles":
        kinds.append(("Triangle", 2))
        prims += [("Triangle", a, b, c, 1) for a, b, c in SMALL_TRIANGLES]
    return {"kinds": kinds, "prims": prims, "light_kinds": [("point", 4)], "lights": [("point", (0.0, 3.0, 0.0), (0.9, 0.9, 0.9))],
            "materials": [((0.0, 0.0, 0.0), 0.0, 0.6), ((1.0, 0.0, 0.0), 0.0, 0.6), ((0.0, 0.0, 1.0), 0.0, 0.6), ((0.1, 0.1, 0.1), 0.9, 0.1)],
            "max_dist": 20.0, "cam_pos": (3.0, 2.5, -0.5), "cam_m": rotation(), "ao_steps": 3, "spec_mode": 2, "probes": probes_of(probes)}


# dims, spacing, offset.  A: inside the room, no power of two anywhere.  B: power-of-two spacing (the library's small form).
# C: odd dims (GPU_Fast visits 6 x 4 x 8 of its cells and writes their records with those sizes).  D: A with more than six
# digits, so that the lookup (six-digit text) and the CPU builders (binary32) read different numbers.  E: simple_scene's own.
# The offsets of A .. D keep the cell centres off the scene's half-integer lattice: over E as it stands, several per cent
# of the cells have a primitive within rounding of the builder's threshold.  F, with the scene "ties", is ON a lattice on purpose:
# its diagonal is 1.5 exactly, every centre and distance is computed without rounding, and in the cells (0, 0, z) the wall's
# distance, 2, EQUALS the floor's 0.5 + the diagonal: `dist < threshold` must leave the wall out.
GRIDS = {"A": ((6, 5, 7), (0.7, 0.6, 0.9), (0.37, 0.21, 0.53)), "B": ((8, 6, 12), (0.5, 0.5, 0.5), (0.37, 0.21, 0.53)),
         "C": ((7, 5, 9), (0.7, 0.6, 0.9), (0.37, 0.21, 0.53)), "D": ((6, 5, 7), (0.7071068, 0.6180340, 0.9), (0.3700004, 0.21, 0.53)),
         "E": ((10, 10, 20), (1.0, 1.0, 1.0), (-1.5, -1.5, -10.0)), "F": ((4, 2, 2), (0.5, 1.0, 1.0), (0.0, 0.0, 0.0))}
METHODS = {"CPU_Best": renderers.CPU_Best, "CPU_Fast": renderers.CPU_Fast, "GPU_Fast": renderers.GPU_Fast}
AMBIGUOUS_CAP = 0.05


def partition_scene(scene, grid, border="Clamp", index_count=20):
    """`scene`: "room" (the radiance pass's, both lights) or a variant of rows"""
    if scene == "room":
        desc = room(lights=(("point", (1.5, 5.5, 4.5), (0.6, 0.5, 0.4)), SPOT), clear_of_probes=True)
    elif scene == "ties":
        desc = rows("plain")
        desc["prims"] = [("Plane", (0.0, 1.0, 0.0), 0.0, 0), ("Plane", (1.0, 0.0, 0.0), 1.75, 1), ("Sphere", (10.0, 10.0, 10.0), 0.5, 3)]
    else:
        desc = rows(scene)
    dims, spacing, offset = GRIDS[grid]
    desc["partition"] = {"dims": dims, "spacing": spacing, "offset": offset, "index_count": index_count, "border": border}
    return desc


def check_table(R, name, key, desc, method, overflow=False, ties=False):
    """the table of renderer R against ref64.partition_build: every unambiguous record exactly, and the warnings"""
    build = cached(("table",) + key, lambda: ref64.partition_build(desc, method))
    got = R.Read_Partitioning()
    share = float(build.ambiguous.mean())
    print("%s: %d records, ambiguous share %.4f (%d), %d overflow, %d warnings" % (
        name, len(got), share, int(build.ambiguous.sum()), int(build.overflow.sum()), build.warnings))
    assert share <= AMBIGUOUS_CAP, "%s: %.4f of the records are ambiguous in float64 alone" % (name, share)
    if overflow:
        assert (build.overflow & ~build.ambiguous).any(), "%s: no unambiguous record overflows" % name
    if ties:
        assert build.ties > 0 and not build.ambiguous.any(), "%s: %d exact ties" % (name, build.ties)
    assert got.shape == build.table.shape
    bad = (got != build.table).any(axis=1) & ~build.ambiguous
    assert not bad.any(), "%s: %d records differ, first %d: got %s, float64 %s" % (
        name, bad.sum(), np.argwhere(bad)[0][0], got[bad][0].tolist(), build.table[bad][0].tolist())
    assert R.Partition_Warnings() == build.warnings, "%s: %d warnings, float64 %d" % (name, R.Partition_Warnings(), build.warnings)
    return got


def run_partition_table(binding, name, scene, grid, method, border="Clamp", index_count=20, overflow=False, prepare=None, ties=False):
    """Update_Partitioning (method) through the binding, the table read back and held by check_table.  `overflow`: the case
    is meant to cut lists (some unambiguous record must).  `ties`: the case is meant to have distances EQUAL to the threshold."""
    desc = partition_scene(scene, grid, border, index_count)
    R = make_renderer(desc, 8, 8, binding)
    if prepare is not None:
        prepare(R)
    R.Update_Partitioning(Method=METHODS[method])
    check_table(R, name, (scene, grid, method, index_count), desc, method, overflow, ties)
    R.Destroy()


def differs(a, b, rtol, atol):
    """per pixel: two float64 frames differ by more than the frame test would let pass"""
    return (a["hit"] != b["hit"]) | (a["index"] != b["index"]) | (np.abs(a["t"] - b["t"]) > ref64.T_ATOL) | ~(
        np.abs(a["colour"] - b["colour"]) <= atol + rtol * np.abs(b["colour"])).all(axis=-1)


def run_partition_screen(binding, name, scene, grid, method, mode, prepare=None, border="Clamp", W=36, H=24, negative=False, variant=None):
    """One screen pass marched through a table (modes 1 and 2: one Render; mode 0: Render_Pass (PASS_SCREEN) over written
    atlases, as run_screen).  First the table the binding builds is held by check_table.  Then the float64 frames are
    computed over the table READ BACK from the binding: the frame test so holds the lookup and the march on every record,
    also where the builders' decision was ambiguous and check_table had to let the record pass.
    Two conditions on the float64 side alone come first: the table must change the frame (more than 10 % of the pixels differ
    from the same frame without the partition -- a grid that covers the scene proves nothing about the lookup), and with
    `negative` some soft-shadow step must have a negative radicand.  (A frame of fewer than 100 pixels cannot show a share of
    10 %; the one-pixel case prints its figure and asserts the rest.)
    `variant` (the literal build only): called with the renderer after the frame, to read which kernel ran."""
    desc = partition_scene(scene, grid, border)
    irr, rad = atlases(desc, SEED % 1000 + 3) if mode == 0 else (None, None)
    R = make_renderer(desc, W, H, binding, mode=mode)
    if prepare is not None:
        prepare(R)
    R.Update_Partitioning(Method=METHODS[method])
    table = check_table(R, name, (scene, grid, method, 20), desc, method)
    with_table = dict(desc, partition=dict(desc["partition"], table=table))
    without = {k: v for k, v in desc.items() if k != "partition"}
    key = ("partition screen", scene, grid, border, W, H, mode, table.tobytes())
    runs = cached(key, lambda: ref64.three_runs(lambda seed: ref64.screen(with_table, W, H, mode, irr, rad, seed=seed)))
    plain = cached(("partition screen", scene, W, H, mode), lambda: ref64.screen(without, W, H, mode, irr, rad))
    tols = (0.0, 1e-4) if mode == 1 else (ref64.COLOUR_RTOL, ref64.COLOUR_ATOL)
    changed = float(differs(runs[0], plain, *tols).mean())
    steps = int(runs[0]["negative"].sum())
    print("%s: the table changes %.3f of the pixels; %d pixels with a negative shadow radicand" % (name, changed, steps))
    if W * H >= 100:
        assert changed > 0.10, "%s: the table changes only %.3f of the pixels" % (name, changed)
    if negative:
        assert steps > 0, "%s: no soft-shadow step has a negative radicand" % name
    if mode == 0:
        R.Write_Texture(B.TEX_IRRADIANCE, irr)
        R.Write_Texture(B.TEX_RADIANCE, rad)
        R.Render_Pass(B.PASS_SCREEN)
    else:
        R.Render()
    fb = R.Read_Framebuffer()
    index, t, _ = R.Read_Gbuffer()
    if variant is not None:
        variant(R)
    R.Destroy()
    if mode == 1:  # (run_screen's bound: the hit displaced by the march tolerance turns a sphere's normal by dt / r)
        radii = [float(p[2]) for p in desc["prims"] if p[0] == "Sphere"]
        return ref64.hold(name, runs, fb, index, t, rtol=0.0, atol=0.5 * ref64.T_ATOL / min(radii) + 4.0 * 2.0 ** -24, table=True)
    return ref64.hold(name, runs, ref64.undo_tone_map(fb), index, t, table=True)


def run_partition_radiance(binding, name, grid, method="CPU_Fast", prepare=None, variant=None):
    """one Render_Pass (PASS_RADIANCE) over written atlases through a table, in the radiance pass's room with both lights:
    run_radiance's rules, the table held and read back as in run_partition_screen, and the same first condition"""
    desc = partition_scene("room", grid)
    irr, rad = atlases(desc, SEED % 1000 + 5)
    R = make_renderer(desc, 8, 8, binding, atlas=1)
    if prepare is not None:
        prepare(R)
    R.Update_Partitioning(Method=METHODS[method])
    table = check_table(R, name, ("room", grid, method, 20), desc, method)
    with_table = dict(desc, partition=dict(desc["partition"], table=table))
    without = {k: v for k, v in desc.items() if k != "partition"}
    runs = cached(("partition radiance", grid, table.tobytes()), lambda: ref64.three_runs(lambda seed: ref64.radiance_texels(with_table, irr, rad, seed=seed)))
    plain = cached(("radiance", SMALL_PROBES.Probe_Count, 1), lambda: ref64.three_runs(lambda seed: ref64.radiance_texels(without, irr, rad, seed=seed)))[0]
    changed = float(differs(runs[0], plain, ref64.COLOUR_RTOL, ref64.COLOUR_ATOL).mean())
    print("%s: the table changes %.3f of the texels" % (name, changed))
    assert changed > 0.10, "%s: the table changes only %.3f of the texels" % (name, changed)
    R.Write_Texture(B.TEX_IRRADIANCE, irr)
    R.Write_Texture(B.TEX_RADIANCE, rad)
    R.Render_Pass(B.PASS_RADIANCE)
    got = R.Read_Texture(B.TEX_RADIANCE)
    if variant is not None:
        variant(R)
    R.Destroy()
    return ref64.hold(name, runs, got, table=True)


# The frames of tests/test_gpu_ref64_partition.py, each named for the kernel variant it is meant to run: `pfk` is what the
# diagnostic build's mdh_diag_variant reports for its pass (MDH_PF_PART 1, _FALLBACK 8, _PSMALL 32, _GTAB 64).  pfk is the
# family pick_kernel chose; for mode 1 it still reads PART | PSMALL on grid B, though the census is dropped there and the
# general partition kernel runs.
PART, FALLBACK, PSMALL, GTAB = 1, 8, 32, 64
PARTITION_FRAMES = {
    "B Clamp mode 0": dict(grid="B", mode=0, pfk=PART | PSMALL),
    "B Clamp mode 2": dict(grid="B", mode=2, pfk=PART | PSMALL),
    "B Clamp mode 1": dict(grid="B", mode=1, pfk=PART | PSMALL),
    "A Clamp mode 2": dict(grid="A", mode=2, pfk=PART),                                  # division by the spacing
    "A Fallback mode 0": dict(grid="A", border="Fallback", mode=0, pfk=PART | FALLBACK),
    "A Fallback mode 2": dict(grid="A", border="Fallback", mode=2, pfk=PART | FALLBACK, negative=True),
    "A Clamp resident": dict(grid="A", mode=2, resident=True, pfk=PART | GTAB),
    "A Fallback resident": dict(grid="A", border="Fallback", mode=2, resident=True, pfk=PART | FALLBACK | GTAB, negative=True),
    "34 spheres": dict(scene="34 spheres", grid="B", mode=2, pfk=PART),                  # the general bits form, three mask words
    # (built on the device: the host builders evaluate a triangle through Madarch.Values, whose "/" on floats adds -- a quirk of
    #  the reference that ref64 does not restate, see test_values_division_bug_is_reproduced)
    "triangles": dict(scene="triangles", grid="B", method="GPU_Fast", mode=2, pfk=PART),
    "two radii": dict(scene="two radii", grid="B", mode=2, pfk=PART | PSMALL),
    "C GPU_Fast": dict(grid="C", method="GPU_Fast", mode=2, pfk=PART),
    "D six digits": dict(grid="D", mode=2, pfk=PART),
    "A Fallback 1x1": dict(grid="A", border="Fallback", mode=2, size=(1, 1), pfk=PART | FALLBACK),
    "A Fallback 61x37": dict(grid="A", border="Fallback", mode=2, size=(61, 37), pfk=PART | FALLBACK, negative=True),
}
PARTITION_RADIANCE = {"A": PART, "B": PART | PSMALL}


def force_residency(R):
    """the scene's table read from device memory (as tests/test_gpu_large_scenes.py forces it)"""
    R.Set_Option(B.OPT_TABLE_RESIDENCY, 1)
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == 1


def run_partition_frame(binding, case, variant=None):
    c = PARTITION_FRAMES[case]
    W, H = c.get("size", (36, 24))
    return run_partition_screen(binding, "partition " + case, c.get("scene", "plain"), c["grid"], c.get("method", "CPU_Fast"), c["mode"],
                                prepare=force_residency if c.get("resident") else None, border=c.get("border", "Clamp"), W=W, H=H,
                                negative=c.get("negative", False), variant=variant)


def render_partition_frame(binding, case):
    """the case's renderer after its one frame, nothing held (for the variant check)"""
    c = PARTITION_FRAMES[case]
    W, H = c.get("size", (36, 24))
    desc = partition_scene(c.get("scene", "plain"), c["grid"], c.get("border", "Clamp"))
    R = make_renderer(desc, W, H, binding, mode=c["mode"])
    if c.get("resident"):
        force_residency(R)
    R.Update_Partitioning(Method=METHODS[c.get("method", "CPU_Fast")])
    if c["mode"] == 0:
        irr, rad = atlases(desc, SEED % 1000 + 3)
        R.Write_Texture(B.TEX_IRRADIANCE, irr)
        R.Write_Texture(B.TEX_RADIANCE, rad)
        R.Render_Pass(B.PASS_SCREEN)
    else:
        R.Render()
    return R


def render_partition_radiance(binding, grid):
    desc = partition_scene("room", grid)
    irr, rad = atlases(desc, SEED % 1000 + 5)
    R = make_renderer(desc, 8, 8, binding, atlas=1)
    R.Update_Partitioning(Method=METHODS["CPU_Fast"])
    R.Write_Texture(B.TEX_IRRADIANCE, irr)
    R.Write_Texture(B.TEX_RADIANCE, rad)
    R.Render_Pass(B.PASS_RADIANCE)
    return R


def run_partition_lookups(binding, name, border, n=4000):
    """partitioning_closest_info at seeded points in a box that overhangs grid A by more than a cell on every side,
    through the oracle's orc_probe_closest, against Scene.lookup over the table read back: the distance to 8 ulp32 of the
    largest number that enters it (hold_distances' bound), the index exactly.  Left out: points within the margin of a cell
    face (ref64.hold, cell_face_margin); the index where the two closest candidates are within the distance's bound of
    each other.  The sample must reach the lookup's three border quirks."""
    import ctypes as C
    desc = partition_scene("plain", "A", border)
    R = make_renderer(desc, 8, 8, binding)
    R.Update_Partitioning(Method=METHODS["CPU_Fast"])
    table = R.Read_Partitioning()
    dims, spacing, offset = (np.array(v) for v in GRIDS["A"])
    lo, hi = offset - 1.7 * spacing, offset + (dims + 1.7) * spacing
    rng = np.random.RandomState(SEED % 1000 + 29)
    pts = rng.uniform(lo, hi, size=(n, 3))
    on = n // 20  # the first twentieth ON a face: one coordinate at offset + j * spacing, which binary32 may put on either side
    axis, j = rng.randint(0, 3, size=on), rng.randint(-1, 9, size=on)
    pts[np.arange(on), axis] = (offset + j[:, None] * spacing)[np.arange(on), axis]
    pts = pts.astype(np.float32)
    dist, index = np.zeros(n, np.float32), np.zeros(n, np.int32)
    binding.lib.orc_probe_closest(R._h, n, pts.ctypes.data_as(C.c_void_p), 1, dist.ctypes.data_as(C.c_void_p), index.ctypes.data_as(C.c_void_p))
    R.Destroy()
    sc = ref64.Scene(dict(desc, partition=dict(desc["partition"], table=table)))
    P = pts.astype(np.float64)
    want_d, arg = sc.lookup(P)
    want_i = np.where(arg >= 0, sc.number[np.maximum(arg, 0)], -1)
    fx = np.floor((P - sc.poff6) / sc.psp6)
    inside = ((fx >= 0) & (fx <= dims)).all(axis=1)
    cell = fx[:, 0] * dims[1] * dims[2] + fx[:, 1] * dims[2] + fx[:, 2]
    back = ~inside if border == "Fallback" else np.zeros(n, dtype=bool)
    reach = inside if border == "Fallback" else np.ones(n, dtype=bool)
    cfx = np.clip(fx, 0, dims)
    ccell = cfx[:, 0] * dims[1] * dims[2] + cfx[:, 1] * dims[2] + cfx[:, 2]
    past, aliased = reach & (ccell >= dims.prod()), reach & (cfx[:, 2] == dims[2]) & (ccell < dims.prod())
    print("%s: %d points, %d outside the grid, %d past the table, %d aliased through fx.z == dims.z, %d fall back, %d near a face" % (
        name, n, int((~((fx >= 0) & (fx < dims)).all(axis=1)).sum()), int(past.sum()), int(aliased.sum()), int(back.sum()), int(sc.face.sum())))
    assert past.sum() > 20 and aliased.sum() > 20 and (border != "Fallback" or back.sum() > 20)
    assert sc.face[:on].all() and sc.face.sum() < on + 5
    assert (want_d[past] == sc.max_dist).all() and (want_i[past] == -1).all()
    held = ~sc.face
    tol = 8.0 * ulp32(np.maximum(np.abs(P).max(axis=1), np.abs(want_d)))
    err = np.abs(dist.astype(np.float64) - want_d)
    print("%s: largest distance error %.2f of its tolerance" % (name, (err / tol)[held].max()))
    bad = held & (err > tol)
    assert not bad.any(), "%s: %d distances off, first at %s: got %r, float64 %r" % (name, bad.sum(), pts[bad][0], dist[bad][0], want_d[bad][0])
    # the arg-min is sure where the runner-up -- the cell's next candidate, or max_dist itself -- is farther off than twice the bound
    D = np.stack([sc.prim_distance(k, P) for k in range(len(sc.prims))], axis=1)
    ranks = np.where(back[:, None], 0, sc.rank[np.where(reach & (ccell < dims.prod()), ccell, dims.prod()).astype(int)])
    D = np.where(ranks < sc.never, D, np.inf)
    D[np.arange(n)[arg >= 0], arg[arg >= 0]] = np.inf
    sure = held & (np.minimum(D.min(axis=1), sc.max_dist) - np.where(arg >= 0, want_d, sc.max_dist) > 2.0 * tol) | (held & (arg < 0) & (D.min(axis=1) - sc.max_dist > 2.0 * tol))
    bad = sure & (index != want_i)
    print("%s: %d indices held" % (name, int(sure.sum())))
    assert sure.sum() > 0.9 * n
    assert not bad.any(), "%s: %d indices differ, first at %s: got %d, float64 %d" % (name, bad.sum(), pts[bad][0], index[bad][0], want_i[bad][0])
