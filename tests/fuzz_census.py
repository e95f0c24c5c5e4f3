"""Random scenes inside and just outside the census variants of run_pass (mdh_api.hip): MDH_PF_ROOM (every plane folded
into the six axis offsets, one sphere, one box, no partition) and MDH_PF_PSMALL (the partition's small form), for
differential testing against the oracle (tests/test_gpu_census_fuzz.py, scripts/fuzz_parity.py --census).

tests/fuzz_scenes.py almost never lands in either census (it always declares a triangle kind, which rules PSMALL out), so
this generator builds a scene DESCRIPTION first -- kinds, primitives, partition -- and `census(desc)` restates the two
predicates of run_pass on it.  Three families of seeds:
    room    the rooms' census: 1-6 axis directions, several planes per direction (offsets one ulp apart: the fold's
            arg-min tie), -0.0 normal components, one sphere and one box placed against walls, through each other,
            around a probe, degenerate or far away; a second act moves both within the census (Set_Primitive);
    psmall  the partition's small form: power-of-two spacings, Clamp borders, no triangle kind, at most 32 of a kind and
            64 declared, builders 0-2, edits and rebuilds in the second act;
    near    a census scene changed in ONE way that sends it to the general kernels."""
import numpy as np

import custom_kinds
from helpers import snapshot
from madarch_amd import _binding as B, materials, renderers, scenes, windows
from madarch_amd.lights import point_lights, spot_lights
from madarch_amd.primitives import boxes, planes, spheres, triangles

F32 = np.float32
ROOM_FIRST, PSMALL_FIRST, NEAR_FIRST = 50000, 60000, 70000  # seed ranges of the three families
KINDS = {"sphere": spheres.Sphere, "plane": planes.Plane, "box": boxes.Box, "triangle": triangles.Triangle, "custom": custom_kinds.My_Sphere}
NEAR = ("two_spheres", "two_boxes", "tilted_plane", "nan_offset", "triangle", "spacing_1_5", "fallback", "kind_33", "user_kind", "declared_65")


def family(seed):
    return "room" if seed < PSMALL_FIRST else ("psmall" if seed < NEAR_FIRST else "near")


def _axis_dir(n, o):
    """commit_scene's fold: exactly one non-zero normal component, +-1, and an offset that is not NaN -> direction 0..5"""
    n = [F32(v) for v in n]
    nz = [c for c in range(3) if n[c] != 0]
    if len(nz) == 1 and abs(n[nz[0]]) == 1 and F32(o) == F32(o):
        return 2 * nz[0] + (1 if n[nz[0]] < 0 else 0)
    return None


def _pow2(s):
    m, e = np.frexp(F32(s))
    return m == 0.5 and -100 < e < 100


def pf_bits(desc):
    """run_pass's pf: bit 0 partition, bit 1 user-defined kinds, bit 3 Fallback border (built-in kinds only)"""
    custom = any(t == "custom" for t, _ in desc["kinds"])
    part = desc["part"]
    return (1 if part else 0) | (2 if custom else 0) | (8 if part and part["border"] != scenes.Clamp and not custom else 0)


def census(desc):
    """The census run_pass picks for the committed scene: "room" (MDH_PF_ROOM), "psmall" (MDH_PF_PSMALL) or None."""
    pf = pf_bits(desc)
    if pf == 0:
        n_axis = sum(_axis_dir(n, o) is not None for n, o in desc["planes"])
        if (n_axis > 0 and n_axis == len(desc["planes"]) and len(desc["spheres"]) == 1 and len(desc["boxes"]) == 1
                and not desc["triangles"]):
            return "room"
        return None
    if pf != 1:
        return None
    seen, declared = set(), 0
    for t, m in desc["kinds"]:
        if m > 32 or (m > 0 and t in seen):
            return None
        if m > 0:
            seen.add(t)
        declared += m
    part = desc["part"]
    if declared > 64 or "triangle" in seen or not all(_pow2(s) for s in part["spacing"]):
        return None
    if int(np.prod(part["dims"])) >= 1 << 24:
        return None
    return "psmall"


def expected_pfk(desc):
    c = census(desc)
    return 16 if c == "room" else (1 | 32 if c == "psmall" else pf_bits(desc))


# ---------------------------------------------------------------------------------------------------- the generator
def _probes(rng):
    """power-of-two atlases (the POW2 variants) or odd ones; at least 4 x 4 x 4 probes"""
    if rng.integers(0, 2):
        dims, count, rres, ires = (4, 4, 4), (8, 8), int(rng.choice([8, 16])), int(rng.choice([4, 8]))
    else:
        dims, count, rres, ires = (5, 4, 4), (10, 8), int(rng.choice([6, 10])), int(rng.choice([5, 6]))
    sp = tuple(float(v) for v in rng.uniform(1.2, 2.0, 3))
    return renderers.Probe_Settings(Radiance_Resolution=rres, Irradiance_Resolution=ires, Probe_Count=count, Grid_Dimensions=dims, Grid_Spacing=sp)


def _walls(rng, lo, hi, full):
    """axis planes of a room [lo, hi]: a non-empty subset of the six directions (all six when `full`), 1-3 planes per
    direction with offsets that tie, differ by one ulp or lie farther out; -0.0 in the normals' zero components"""
    dirs = list(range(6)) if full else sorted(rng.choice(6, int(rng.integers(1, 7)), replace=False).tolist())
    out = []
    for g in dirs:
        a, neg = g // 2, g % 2
        n = [float(rng.choice([0.0, -0.0])) for _ in range(3)]
        n[a] = -1.0 if neg else 1.0
        o = F32(hi[a] if neg else -lo[a])  # the wall at x_a = lo (+) or hi (-)
        out.append((tuple(n), float(o)))
        for _ in range(int(rng.choice([0, 0, 1, 2]))):
            k = int(rng.integers(0, 3))
            o2 = o if k == 0 else (np.nextafter(o, F32(np.inf)) if k == 1 else F32(o + F32(rng.uniform(0.0, 2.0))))
            out.append((tuple(n), float(o2)))
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def _sphere_box(rng, lo, hi, probes):
    """one sphere and one box: against walls, through each other, around a probe, degenerate, far away or anywhere"""
    mid = (lo + hi) / 2
    r = float(rng.uniform(0.3, 1.2))
    e = rng.uniform(0.2, 1.0, 3)
    c_s = rng.uniform(lo + 1.0, hi - 1.0)
    c_b = rng.uniform(lo + 1.0, hi - 1.0)
    how = int(rng.integers(0, 6))
    if how == 0:  # touching walls
        a = int(rng.integers(0, 3))
        c_s[a] = lo[a] + r
        c_b[(a + 1) % 3] = hi[(a + 1) % 3] - e[(a + 1) % 3]
    elif how == 1:  # intersecting each other
        c_b = c_s + rng.uniform(-0.5, 0.5, 3) * r
    elif how == 2:  # around a probe
        s = np.array(probes.Grid_Spacing)
        q = np.array([rng.integers(0, d) for d in probes.Grid_Dimensions]) * s
        c_s = q + rng.uniform(-0.2, 0.2, 3) * r
        c_b = np.array([rng.integers(0, d) for d in probes.Grid_Dimensions]) * s + rng.uniform(-0.1, 0.1, 3)
    elif how == 3:  # zero radius, zero extents
        r = 0.0 if rng.integers(0, 2) else r
        e[rng.choice(3, int(rng.integers(1, 4)), replace=False)] = 0.0
    elif how == 4:  # far from the origin
        c_s = mid + rng.choice([-1, 1], 3) * rng.uniform(100.0, 400.0, 3)
    return (tuple(float(v) for v in c_s), r), (tuple(float(v) for v in c_b), tuple(float(v) for v in e))


def _room_desc(rng, full_walls=False):
    probes = _probes(rng)
    ext = (np.array(probes.Grid_Dimensions) - 1) * np.array(probes.Grid_Spacing)
    lo, hi = -rng.uniform(0.3, 1.5, 3), ext + rng.uniform(0.3, 1.5, 3)
    sph, box = _sphere_box(rng, lo, hi, probes)
    return dict(kinds=[("sphere", int(rng.integers(1, 3))), ("plane", 18), ("box", int(rng.integers(1, 3)))], planes=_walls(rng, lo, hi, full_walls),
                spheres=[sph], boxes=[box], triangles=[], custom=[], part=None, probes=probes, lo=lo, hi=hi)


def _psmall_desc(rng):
    probes = _probes(rng)
    ext = (np.array(probes.Grid_Dimensions) - 1) * np.array(probes.Grid_Spacing)
    lo, hi = -rng.uniform(0.3, 1.5, 3), ext + rng.uniform(0.3, 1.5, 3)
    ms, mp, mb = int(rng.integers(1, 9)), int(rng.integers(6, 11)), int(rng.integers(1, 9))
    sp = tuple(float(v) for v in rng.choice([0.5, 1.0, 2.0, 4.0], 3))
    dims = tuple(int(np.clip(np.ceil((hi[a] - lo[a] + 2.0) / sp[a]) + rng.integers(-2, 3), 1, 24)) for a in range(3))
    part = dict(dims=dims, spacing=sp, offset=tuple(float(v) for v in lo - rng.uniform(0.0, 1.5, 3)), border=scenes.Clamp,
                index_count=int(rng.integers(2, 12)), builder=int(rng.integers(0, 3)))
    walls = _walls(rng, lo, hi, True)[:mp]
    if rng.integers(0, 2) and len(walls) < mp:  # a tilted plane: the partition's census does not mind
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        walls.append((tuple(float(v) for v in n), float(rng.uniform(1.0, 3.0))))
    sph = [(tuple(float(v) for v in rng.uniform(lo, hi)), float(rng.choice([0.0, rng.uniform(0.2, 1.0)]))) for _ in range(int(rng.integers(0, ms + 1)))]
    box = [(tuple(float(v) for v in rng.uniform(lo, hi)), tuple(float(v) for v in rng.uniform(0.0, 1.0, 3))) for _ in range(int(rng.integers(0, mb + 1)))]
    return dict(kinds=[("sphere", ms), ("plane", mp), ("box", mb)], planes=walls, spheres=sph, boxes=box, triangles=[], custom=[],
                part=part, probes=probes, lo=lo, hi=hi)


def describe(seed):
    """the scene description of `seed` and, for near-census seeds, the change that leaves the census"""
    rng = np.random.default_rng(seed)
    fam = family(seed)
    if fam == "room":
        return _room_desc(rng), None
    if fam == "psmall":
        return _psmall_desc(rng), None
    change = NEAR[(seed - NEAR_FIRST) % len(NEAR)]
    if change in ("spacing_1_5", "fallback", "kind_33", "declared_65"):
        d = _psmall_desc(rng)
        if change == "spacing_1_5":
            sp = list(d["part"]["spacing"]); sp[int(rng.integers(0, 3))] = 1.5
            d["part"]["spacing"] = tuple(sp)
        elif change == "fallback":
            d["part"]["border"] = scenes.Fallback
        elif change == "kind_33":
            d["kinds"][0] = ("sphere", 33)
        else:
            d["kinds"] = [("sphere", 32), ("plane", 16), ("box", 17)]
        return d, change
    d = _room_desc(rng, full_walls=True)
    lo, hi = d["lo"], d["hi"]
    if change == "two_spheres":
        d["spheres"].append((tuple(float(v) for v in rng.uniform(lo, hi)), float(rng.uniform(0.2, 0.8))))
        d["kinds"][0] = ("sphere", 2)
    elif change == "two_boxes":
        d["boxes"].append((tuple(float(v) for v in rng.uniform(lo, hi)), tuple(float(v) for v in rng.uniform(0.2, 0.8, 3))))
        d["kinds"][2] = ("box", 2)
    elif change == "tilted_plane":
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        d["planes"].append((tuple(float(v) for v in n), float(rng.uniform(2.0, 4.0))))
    elif change == "nan_offset":
        d["planes"].append(((0.0, 1.0, 0.0), float("nan")))
    elif change == "triangle":
        a = rng.uniform(lo, hi)
        d["kinds"].append(("triangle", 2))
        d["triangles"].append(tuple(tuple(float(v) for v in p) for p in (a, a + rng.uniform(-1.5, 1.5, 3), a + rng.uniform(-1.5, 1.5, 3))))
    elif change == "user_kind":
        d["kinds"].append(("custom", 2))
        d["custom"].append((tuple(float(v) for v in rng.uniform(lo, hi)), float(rng.uniform(0.2, 0.6))))
    return d, change


def _settings(seed):
    """the render settings of a seed, from a generator of their own"""
    rng = np.random.default_rng(seed ^ 0xCE45)
    vol = renderers.No_Volumetrics
    if rng.integers(0, 3) == 0:
        vol = renderers.Volumetrics_Settings(Visibility_Resolution=tuple(int(v) for v in rng.integers(4, 12, 3)), Visibility_Step_Size=float(rng.choice([0.25, 0.4])),
                                             Scattering_Resolution=tuple(int(v) for v in rng.integers(4, 16, 2)), Scattering_Step_Size=float(rng.choice([0.1, 0.3])))
    return dict(mode=int(rng.choice([0, 0, 0, 1, 2])), spec=int(rng.integers(0, 4)), atlas=int(rng.integers(0, 2)), mips=bool(rng.integers(0, 2)),
                overlap=int(rng.integers(0, 3)), vol=vol, W=int(rng.choice([96, 104])), H=int(rng.choice([64, 72])), frames=int(rng.integers(1, 3)))


def _add(R, desc, mat):
    for n, o in desc["planes"]:
        R.Add_Primitive(planes.Plane, planes.Create(n, o, mat()))
    for c, r in desc["spheres"]:
        R.Add_Primitive(spheres.Sphere, spheres.Create(c, r, mat()))
    for c, e in desc["boxes"]:
        R.Add_Primitive(boxes.Box, boxes.Create(c, e, mat()))
    for a, b, c in desc["triangles"]:
        R.Add_Primitive(triangles.Triangle, triangles.Create(a, b, c, mat()))
    for c, r in desc["custom"]:
        R.Add_Primitive(custom_kinds.My_Sphere, custom_kinds.sphere(c, r, mat()))


def create(seed, binding):
    """the renderer of `seed` with its scene added and its settings made, before the first frame: (R, desc, settings)"""
    desc, _ = describe(seed)
    st = _settings(seed)
    rng = np.random.default_rng(seed ^ 0x11A7)
    part = desc["part"]
    ps = (scenes.Partitioning_Settings(Enable=True, Index_Count=part["index_count"], Border_Behavior=part["border"], Grid_Dimensions=part["dims"],
                                       Grid_Spacing=part["spacing"], Grid_Offset=part["offset"]) if part else scenes.Partitioning_Settings(Enable=False))
    scene = scenes.Compile([(KINDS[t], m) for t, m in desc["kinds"]], [(point_lights.Point_Light, 2), (spot_lights.Spot_Light, 1)], Partitioning=ps)
    R = renderers.Create(windows.Open(st["W"], st["H"]), scene, Probes=desc["probes"], Volumetrics=st["vol"], Binding=binding)
    for m in range(3):
        R.Set_Material(m, materials.Create(tuple(rng.uniform(0.0, 1.0, 3)), float(rng.choice([0.0, 0.5, 0.9])), float(rng.choice([0.1, 0.4, 0.8]))))
    mat = lambda: int(rng.integers(0, 3))
    _add(R, desc, mat)
    lo, hi = desc["lo"], desc["hi"]
    inside = lambda: tuple(float(v) for v in rng.uniform(lo + 0.2, hi - 0.2))
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create(inside(), tuple(rng.uniform(0.3, 1.0, 3))))
    if rng.integers(0, 2):
        R.Set_Light(2, point_lights.Point_Light, point_lights.Create(inside(), tuple(rng.uniform(0.1, 0.6, 3))))
    if rng.integers(0, 2):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        R.Set_Light(1, spot_lights.Spot_Light, spot_lights.Create(inside(), tuple(float(v) for v in d), float(rng.uniform(0.3, 1.2)), tuple(rng.uniform(0.3, 1.0, 3))))
    R.Set_Camera_Position(inside())
    a, b = rng.uniform(-3.1, 3.1), rng.uniform(-0.6, 0.6)
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    R.Set_Camera_Orientation((np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])).astype(np.float32).tolist())
    R.Set_Option(B.OPT_SCREEN_MODE, st["mode"])
    R.Set_Option(B.OPT_INDIRECT_SPECULAR, st["spec"])
    R.Set_Option(B.OPT_ATLAS_FORMAT, st["atlas"])
    R.Set_Option(B.OPT_GBUFFER, 1)
    R.Set_Option(B.OPT_FRAME_OVERLAP, st["overlap"])
    R.Set_Option(B.OPT_WINDOW, 1)
    R.Set_Option(B.OPT_JIT, 0)
    if st["mips"] and (R.Probes.Radiance_Resolution & (R.Probes.Radiance_Resolution - 1)) == 0:
        R.Set_Option(B.OPT_RADIANCE_MIPS, 1)
    if part:
        R.Update_Partitioning(part["builder"])
    return R, desc, st


def build(seed, binding):
    """every observable output of the seed's two acts (the keys of fuzz_scenes.compare)"""
    R, desc, st = create(seed, binding)
    rng = np.random.default_rng(seed ^ 0xAC72)
    lo, hi = desc["lo"], desc["hi"]
    out = snapshot(R, st["frames"])
    if desc["part"]:
        out["partition"] = R.Read_Partitioning()
    kinds = [KINDS[t] for t, m in desc["kinds"] if m > 0]
    out["eval_d"], out["eval_n"] = R.Eval_Distances_To(rng.uniform(lo - 0.5, hi + 0.5, (int(rng.integers(8, 40)), 3)).astype(np.float32), kinds)
    # the second act: the sphere and the box move (within the census), the partition is rebuilt, frames in flight
    if desc["spheres"]:
        i = int(rng.integers(1, len(desc["spheres"]) + 1))
        R.Set_Primitive(spheres.Sphere, i, spheres.Create(tuple(float(v) for v in rng.uniform(lo, hi)), float(rng.uniform(0.0, 1.0)), 1))
    if desc["boxes"]:
        i = int(rng.integers(1, len(desc["boxes"]) + 1))
        R.Set_Primitive(boxes.Box, i, boxes.Create(tuple(float(v) for v in rng.uniform(lo, hi)), tuple(float(v) for v in rng.uniform(0.0, 1.0, 3)), 2))
    if desc["part"]:
        R.Update_Partitioning(int(rng.integers(0, 3)))
    for _ in range(int(rng.integers(1, 3))):
        R.Set_Camera_Position(tuple(float(v) for v in rng.uniform(lo + 0.2, hi - 0.2)))
        R.Render()
        R.Swap_Buffers()
    for k, v in snapshot(R, 0).items():
        out["act2_" + k] = v
    out["window"] = R.Front_Buffer()
    R.Destroy()
    return out


def seeds(kind, first=0, count=None):
    """seed numbers of a family ("room", "psmall", "near") from its range"""
    base = {"room": ROOM_FIRST, "psmall": PSMALL_FIRST, "near": NEAR_FIRST}[kind]
    return list(range(base + first, base + first + (count if count is not None else 1000)))
