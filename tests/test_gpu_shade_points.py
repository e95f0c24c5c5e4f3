"""mdh_shade_points and mdh_primitive_material on the device: the irradiance alone against the oracle's
orc_probe_sample_irradiance bit for bit, the frame reproduced point by point from Camera_Rays -> Raycast ->
Primitive_Material (the screen pass and mdh_shade_rays are the yardsticks), free points against the float64 renderer of
tests/ref64.py under the tolerances it keeps, a point's answer independent of its batch, nothing edited and the right
frame waited for, every refusal before a launch.  The device-array call runs in a child process with torch
(tests/shade_points_device_checks.py).
(No point here comes near the bound that stands in for a stall guard: max_dist is 20 and every coordinate below 10.)"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import custom_kinds as ck
import ray_query_cases as rq
import ref64
import shade_points_cases as P
import shade_points_device_checks as checks
import shade_rays_cases as S
from helpers import SEED, SMALL_PROBES
from madarch_amd import _binding as B
from madarch_amd import renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import spheres

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = S.FRAME_W, S.FRAME_H


def same(a, b):
    return np.array_equal(S.bits(a), S.bits(b))


def _status(call):
    try:
        call()
    except B.MadarchError as e:
        return e.status
    return B.MDH_OK


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ------------------------------------------------------------------------------------ 1. the irradiance against the oracle
IRRADIANCE_CASES = [(name, atlas) for name in S.FRAME_SCENES for atlas in ((0, 1) if name == "rooms" else (None,))]


@pytest.mark.parametrize("name,atlas", IRRADIANCE_CASES)
def test_irradiance_against_the_oracle_bit_for_bit(hip, orc, name, atlas):
    R, Ro = P.twin_renderers(hip, orc, name, atlas)
    pos, nrm, cls = P.irradiance_points(R, name, P.scene_rays(name))
    want = P.orc_irradiance(orc, Ro, pos, nrm)
    got = R.Shade_Points(pos, nrm, Mode=P.IRRADIANCE)
    print("%s, atlas %s: %d points, %d of them dark, classes %s" % (name, atlas, len(pos), int((want == 0.0).all(axis=1).sum()), np.bincount(cls).tolist()))
    bad = np.nonzero((S.bits(got) != S.bits(want)).any(axis=1))[0]
    assert len(bad) == 0, "%d points differ, first %d (class %d) at %s: %s against the oracle's %s" % (
        len(bad), bad[0], cls[bad[0]], pos[bad[0]], got[bad[0]], want[bad[0]])
    assert np.isfinite(want).all() and (want > 0.0).any()
    if name == "rooms":  # deep inside a wall, the sphere or the box every probe is occluded: exactly 0
        deep = np.nonzero(cls == 2)[0][::2]
        assert ((want[deep] == 0.0).all(axis=1)).sum() * 2 >= len(deep)
    # view directions and material ids are not read in mode 3: garbage there changes nothing
    junk = R.Shade_Points(pos, nrm, np.full_like(pos, np.nan), np.full(len(pos), -5, np.int32), Mode=P.IRRADIANCE)
    assert same(junk, got)
    R.Destroy()
    Ro.Destroy()


# ------------------------------------------------------------------------------------ 2. the frame, point by point
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("name", list(S.FRAME_SCENES))
def test_the_frame_point_by_point(hip, name, mode):
    R = S.frame_renderer(hip, name, mode)
    org, drs, rows, (pos, nrm, view, mat), all_mat, rc = P.frame_points(R)
    print("%s mode %d: %d of %d rays hit" % (name, mode, len(rows), W * H))
    assert len(rows) > 0 and (all_mat[rows] >= 0).all() and (all_mat[rc["hit"] != 1] == -1).all()
    for spec in (2, 0):
        R.Set_Option(B.OPT_INDIRECT_SPECULAR, spec)
        R.Render_Pass(B.PASS_SCREEN)
        fb = R.Read_Framebuffer().reshape(-1, 3)
        index = R.Read_Gbuffer()[0].reshape(-1)
        assert same(index, rc["index"])
        lin = R.Shade_Rays(org, drs, Mode=mode, Tone_Map=False)["rgb"]
        got = R.Shade_Points(pos, nrm, view, mat, Mode=mode, Tone_Map=False)
        bad = np.nonzero((S.bits(got) != S.bits(lin[rows])).any(axis=1))[0]
        assert len(bad) == 0, "spec %d: %d points differ from their rays, first %d: %s against %s" % (spec, len(bad), bad[0], got[bad[0]], lin[rows][bad[0]])
        got = R.Shade_Points(pos, nrm, view, mat, Mode=mode, Tone_Map=True)
        bad = np.nonzero((S.bits(got) != S.bits(fb[rows])).any(axis=1))[0]
        assert len(bad) == 0, "spec %d: %d points differ from their pixels, first %d: %s against %s" % (spec, len(bad), bad[0], got[bad[0]], fb[rows][bad[0]])
    R.Destroy()


def test_primitive_material_is_the_scenes(hip):
    for name in ("room", "open"):
        R, desc = rq.described(hip, name)
        base, at = {}, 0
        for kind, count in desc["kinds"]:
            base[kind] = at
            at += count
        want = np.full(at + 3, -1, np.int32)
        seen = {}
        for p in desc["prims"]:
            want[base[p[0]] + seen.get(p[0], 0)] = p[-1]
            seen[p[0]] = seen.get(p[0], 0) + 1
        index = np.concatenate([np.arange(at + 3), [-1, -7, 1 << 30]]).astype(np.int32)
        got = R.Primitive_Material(index)
        assert np.array_equal(got[:at + 3], want) and (got[at + 3:] == -1).all(), (name, got.tolist())
        assert R.Primitive_Material(np.zeros((0,), np.int32)).shape == (0,)
        assert R.Primitive_Material(index.reshape(2, -1)[:, :4]).shape == (2, 4)
        R.Destroy()
    # a scene with a user-defined kind: its material is a program's result
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    assert _status(lambda: Rc.Primitive_Material([0])) == B.MDH_E_STATE
    Rc.Destroy()


# ------------------------------------------------------------------------------------ 3. free points against float64
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("name", ["room", "open"])
def test_free_points_against_float64(hip, name, mode):
    """Held by ref64.hold_values under COLOUR_RTOL, COLOUR_ATOL and FRAGILE_CAP as they stand."""
    desc = P.describe(name)
    from ref64_cases import make_renderer
    R = make_renderer(desc, 16, 16, hip)
    irr, rad = S.free_atlases(desc)
    R.Write_Texture(B.TEX_IRRADIANCE, irr)
    R.Write_Texture(B.TEX_RADIANCE, rad)
    pos, nrm, view, mat = P.free_points(name, len(desc["materials"]))
    got = R.Shade_Points(pos, nrm, view, mat, Mode=mode, Tone_Map=False)
    irradiance = R.Shade_Points(pos, nrm, Mode=P.IRRADIANCE)
    R.Destroy()
    runs = P.free_runs(name, mode)
    lit = int((runs[0]["direct"].max(axis=1) > 1e-3).sum())
    print("%s mode %d: %d of %d points see direct light" % (name, mode, lit, len(pos)))
    assert 4 * lit >= len(pos)
    ref64.hold_values("%s, mode %d, %d free points" % (name, mode, len(pos)), runs, got, ref64.COLOUR_RTOL, ref64.COLOUR_ATOL)
    ref64.hold_values("%s, the irradiance of %d free points" % (name, len(pos)), [{"colour": r["irradiance"]} for r in runs], irradiance,
                      ref64.COLOUR_RTOL, ref64.COLOUR_ATOL)


# ------------------------------------------------------------------------------------ 4. a point's answer is its own
@pytest.mark.parametrize("mode", (0, 2, 3))
def test_a_points_answer_is_its_own(hip, mode):
    R = S.frame_renderer(hip, "rooms", 0)
    pos, nrm, _ = P.irradiance_points(R, "rooms", rq.room_rays(257))
    rng = np.random.RandomState(SEED % 1000 + 59)
    view = rq.unit_dirs(rng, 257)
    mat = rng.randint(0, 5, 257).astype(np.int32)
    extra = () if mode == 3 else (view, mat)
    whole = R.Shade_Points(pos, nrm, *extra, Mode=mode)
    perm = rng.permutation(257)
    c = np.ascontiguousarray
    mixed = R.Shade_Points(c(pos[perm]), c(nrm[perm]), *[c(a[perm]) for a in extra], Mode=mode)
    assert same(mixed, whole[perm])
    for n in (1, 63, 64, 65, 257):
        part = R.Shade_Points(pos[:n], nrm[:n], *[a[:n] for a in extra], Mode=mode)
        assert same(part, whole[:n]), n
    assert np.isfinite(whole).all() and (whole != 0.0).any()
    R.Destroy()


def test_the_example_lights_its_ring(hip):
    from madarch_amd import examples
    R = examples.global_illumination(32, 32, Probes=SMALL_PROBES, Binding=hip)
    pos, nrm, rgb = examples.lit_points(R, Count=65, Frames=3)
    assert pos.shape == nrm.shape == rgb.shape == (65, 3)
    assert np.isfinite(rgb).all() and (rgb >= 0.0).all() and (rgb.max(axis=1) > 0.0).sum() > 32  # (the probes light most of the ring)
    R.Destroy()


# ------------------------------------------------------------------------------------ 5. device arrays
@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shade_points") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "shade_points_device_checks.py"), out]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(run.stdout[-6000:])
    print(run.stderr[-3000:])
    assert os.path.exists(out), "the checks' process wrote nothing (exit status %d):\n%s" % (run.returncode, run.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert "__error__" not in got, got["__error__"]
    return got


@pytest.mark.parametrize("name", list(checks.CHECKS))
def test_device_arrays(verdicts, name):
    assert name in verdicts, "the checks' process ended before '%s'" % name
    v = verdicts[name]
    print("%.1f s" % v["seconds"])
    assert v["ok"], v["log"]


# ------------------------------------------------------------------------------------ 6. it edits nothing and waits for the right frame
def _query_points(R):
    """65 points on the room's surfaces with seeded view directions and materials"""
    org, drs = rq.room_rays(65)
    rc = R.Raycast(org, drs)
    assert rc["hit"].all()
    rng = np.random.RandomState(SEED % 1000 + 61)
    return rc["position"], rc["normal"], rq.unit_dirs(rng, 65), rng.randint(0, 5, 65).astype(np.int32)


@pytest.mark.parametrize("screen_replay", [0, 1])
def test_queries_edit_nothing(hip, screen_replay):
    """four frames with a point query between them, four frames without: every frame's pixels are the same, and the radiance
    replay, the probe settle and the screen replay have counted the same passes of each kind"""
    outs = []
    for queries in (True, False):
        R = rq.gi_room(hip)
        R.Set_Option(B.OPT_SCREEN_REPLAY, screen_replay)
        pts = _query_points(R)
        frames = []
        for f in range(4):
            R.Render()
            if queries:
                mode = (0, 2, 3, 0)[f]
                R.Shade_Points(*(pts[:2] if mode == 3 else pts), Mode=mode, Tone_Map=bool(f & 1) and mode != 3)
                R.Primitive_Material(np.arange(8))
            frames.append(R.Read_Framebuffer())
        R.Finish()
        outs.append((frames, R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats()))
        R.Destroy()
    (fb_q, rad_q, settle_q, scr_q), (fb, rad, settle, scr) = outs
    print("radiance replay %s, probe settle %s, screen replay %s" % (rad, settle, scr))
    for f in range(4):
        assert same(fb_q[f], fb[f]), f
    assert rad_q == rad and settle_q == settle and scr_q == scr
    assert sum(rad) >= 1 and (screen_replay == 0 or scr[1] + scr[2] > 0)  # (the counters do count)


def test_a_query_waits_for_the_frames_in_flight(hip):
    """three frames nobody waited for, then a query: the answer of a renderer that called Finish first, and the pixels of a
    screen pass issued at that point"""
    with S.frame_size():
        Ra, Rb = rq.gi_room(hip), rq.gi_room(hip)
    org, drs, rows, pts, _, _ = P.frame_points(Ra)
    for R in (Ra, Rb):
        for _ in range(3):
            R.Render()
    Rb.Finish()
    a = Ra.Shade_Points(*pts, Tone_Map=True)
    b = Rb.Shade_Points(*pts, Tone_Map=True)
    assert same(a, b)
    ia, ib = Ra.Shade_Points(*pts[:2], Mode=P.IRRADIANCE), Rb.Shade_Points(*pts[:2], Mode=P.IRRADIANCE)
    assert same(ia, ib) and (ia > 0.0).any()
    Ra.Render_Pass(B.PASS_SCREEN)
    assert same(a, Ra.Read_Framebuffer().reshape(-1, 3)[rows])
    # ... and frames go on behind the query as they go on without it
    Ra.Render()
    Rb.Render()
    assert same(Ra.Read_Framebuffer(), Rb.Read_Framebuffer())
    Ra.Destroy()
    Rb.Destroy()


def test_refusals_launch_nothing(hip):
    R = rq.gi_room(hip)
    R.Set_Option(B.OPT_TIMING, 1)
    R.Render()
    pos, nrm, view, mat = _query_points(R)
    assert _status(lambda: R.Shade_Points(pos, nrm, view, mat)) == B.MDH_OK
    t_before = R.Ray_Query_Time()
    assert t_before > 0.0
    rgb = np.full((65, 3), -3.0, np.float32)

    def raw(r=R, mode=0, tone=0, n=65, p=pos, nr=nrm, v=view, m=mat, out=rgb):
        return hip.shade_points(r._h, n, vp(p), vp(nr), vp(v), vp(m), mode, tone, vp(out))
    assert raw(mode=1) == B.MDH_E_INVALID and raw(mode=4) == B.MDH_E_INVALID and raw(mode=-1) == B.MDH_E_INVALID
    assert raw(n=-1) == B.MDH_E_INVALID and raw(out=None) == B.MDH_E_INVALID and raw(p=None) == B.MDH_E_INVALID and raw(nr=None) == B.MDH_E_INVALID
    assert raw(v=None) == B.MDH_E_INVALID and raw(m=None) == B.MDH_E_INVALID and raw(mode=2, v=None) == B.MDH_E_INVALID and raw(mode=2, m=None) == B.MDH_E_INVALID
    assert raw(mode=3, tone=1) == B.MDH_E_INVALID
    assert raw(n=0) == B.MDH_OK
    # a bad point refuses the whole batch of host arrays
    for what, (arr, at, value) in {"a NaN": (0, (7, 2), np.nan), "an infinite normal": (1, (64, 0), np.inf), "a position at 2000": (0, (3, 1), 2000.0),
                                   "a normal of 1.5": (1, (40, 0), 1.5), "a view direction of -2": (2, (9, 1), -2.0)}.items():
        arrays = [pos.copy(), nrm.copy(), view.copy()]
        arrays[arr][at] = value
        assert raw(p=arrays[0], nr=arrays[1], v=arrays[2]) == B.MDH_E_INVALID, what
        if arr < 2:
            assert raw(mode=3, p=arrays[0], nr=arrays[1], v=None, m=None) == B.MDH_E_INVALID, what
    for bad_id in (-1, 20, 1 << 20):
        m = mat.copy()
        m[11] = bad_id
        assert raw(m=m) == B.MDH_E_INVALID and raw(mode=2, m=m) == B.MDH_E_INVALID, bad_id
    for spec in (1, 3):
        R.Set_Option(B.OPT_INDIRECT_SPECULAR, spec)
        assert raw() == B.MDH_E_STATE and raw(mode=2) == B.MDH_E_STATE, spec
    R.Set_Option(B.OPT_INDIRECT_SPECULAR, 2)
    assert (rgb == -3.0).all()
    assert R.Ray_Query_Time() == t_before  # (no kernel was timed since: none was launched)
    assert raw(mode=3, v=None, m=None) == B.MDH_OK and np.isfinite(rgb).all()  # mode 3 takes NULL for both
    assert raw() == B.MDH_OK and np.isfinite(rgb).all()
    R.Destroy()
    # a scene with a user-defined kind
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    for mode in (0, 2, 3):
        assert raw(r=Rc, mode=mode) == B.MDH_E_STATE, mode
    Rc.Destroy()
    # a light at x = 5000: beyond the scene's half of the bound
    Rl = rq.small_mesh(hip)
    assert raw(r=Rl) == B.MDH_OK
    Rl.Set_Light(1, point_lights.Point_Light, point_lights.Create((5000.0, 1.0, -5.0), (0.9, 0.9, 0.9)))
    assert raw(r=Rl) == B.MDH_E_STATE and raw(r=Rl, mode=2) == B.MDH_E_STATE
    Rl.Destroy()
