"""mdh_shade_rays and mdh_camera_rays on the device: the frame reproduced ray by ray from its own camera rays (the screen
pass is the yardstick -- the parent's code, held against the oracle elsewhere), free rays against the float64 renderer of
tests/ref64.py under the tolerances it keeps, a ray's answer independent of its batch, nothing edited and the right frame
waited for, every refusal before a launch.  The device-array calls run in a child process with torch
(tests/shade_rays_device_checks.py), like the device-array ray queries.
(No ray here comes near the bound that stands in for a stall guard: max_dist is 20 and every coordinate below 10.)"""
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
import ref64_cases
import shade_rays_cases as S
import shade_rays_device_checks as checks
from helpers import SEED, SMALL_PROBES, SMALL_VOL
from madarch_amd import _binding as B
from madarch_amd import examples, renderers, scenes, windows
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


# ------------------------------------------------------------------------------------ 1. the frame, ray by ray
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("name", list(S.FRAME_SCENES))
def test_the_frame_ray_by_ray(hip, name, mode):
    R = S.frame_renderer(hip, name, mode)
    R.Render_Pass(B.PASS_SCREEN)
    fb = R.Read_Framebuffer().reshape(-1, 3)
    index, t, steps = (a.reshape(-1) for a in R.Read_Gbuffer())
    org, drs = R.Camera_Rays(W, H)
    assert org.shape == drs.shape == (W * H, 3)
    got = R.Shade_Rays(org, drs, Mode=mode, Tone_Map=True)
    print("%s mode %d: %d of %d rays hit" % (name, mode, int((index >= 0).sum()), W * H))
    assert (index >= 0).any()  # (the frame shows the scene)
    assert same(got["index"], index) and same(got["t"], t) and same(got["steps"], steps)
    assert np.array_equal(got["hit"], (index >= 0).astype(np.int32))
    bad = np.nonzero((S.bits(got["rgb"]) != S.bits(fb)).any(axis=1))[0]
    assert len(bad) == 0, "%d pixels differ, first %d: %s against the frame's %s" % (len(bad), bad[0], got["rgb"][bad[0]], fb[bad[0]])
    # k_camera_rays by itself: mdh_raycast over the same rays gives the geometry buffer too
    rc = R.Raycast(org, drs)
    assert same(rc["index"], index) and same(rc["t"], t) and same(rc["steps"], steps)
    # the linear colour is what the tone map was applied to
    lin = R.Shade_Rays(org, drs, Mode=mode, Tone_Map=False)
    assert same(lin["index"], index)
    with np.errstate(invalid="ignore"):
        x = lin["rgb"].astype(np.float64)
        assert np.allclose((x / (x + 1.0)) ** ref64.TONE, fb.astype(np.float64), rtol=1e-4, atol=1e-6, equal_nan=True)
    R.Destroy()


# ------------------------------------------------------------------------------------ 2. free rays against float64
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("name", ["room", "open"])
def test_free_rays_against_float64(hip, name, mode):
    R, desc = rq.described(hip, name)
    irr, rad = S.free_atlases(desc)
    R.Write_Texture(B.TEX_IRRADIANCE, irr)
    R.Write_Texture(B.TEX_RADIANCE, rad)
    org, drs = S.free_rays(name)
    got = R.Shade_Rays(org, drs, Mode=mode, Tone_Map=False)
    R.Destroy()
    ref64.hold("%s, mode %d, %d free rays" % (name, mode, len(org)), S.free_runs(name, mode), got["rgb"], got["index"], got["t"])


# ------------------------------------------------------------------------------------ 3. a ray's answer is its own
@pytest.mark.parametrize("mode", S.MODES)
def test_a_rays_answer_is_its_own(hip, mode):
    R = S.frame_renderer(hip, "rooms", mode)
    org, drs = rq.room_rays(257)
    whole = R.Shade_Rays(org, drs, Mode=mode)
    perm = np.random.RandomState(SEED % 1000 + 5).permutation(257)
    mixed = R.Shade_Rays(np.ascontiguousarray(org[perm]), np.ascontiguousarray(drs[perm]), Mode=mode)
    for k in whole:
        assert same(mixed[k], whole[k][perm]), k
    for n in (1, 63, 64, 65, 257):
        part = R.Shade_Rays(org[:n], drs[:n], Mode=mode)
        for k in whole:
            assert same(part[k][0], whole[k][0]), (k, n)
            assert same(part[k], whole[k][:n]), (k, n)
    assert whole["hit"].all() and np.isfinite(whole["rgb"]).all()
    R.Destroy()


# ------------------------------------------------------------------------------------ 4. host arrays against device arrays
@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shade_rays") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "shade_rays_device_checks.py"), out]
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


def test_bad_rays_refuse_the_host_batch(hip):
    R = S.frame_renderer(hip, "rooms", 0)
    org, drs = rq.room_rays(65)
    rgb = np.full((65, 3), -3.0, np.float32)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)
    for what, (arr, at, value) in {"a NaN": (1, (7, 2), np.nan), "an infinity": (0, (64, 0), np.inf), "an origin at 2000": (0, (3, 1), 2000.0),
                                   "an origin at -2000": (0, (3, 1), -2000.0), "a direction of 3": (1, (40, 0), 3.0)}.items():
        o, d = org.copy(), drs.copy()
        (o, d)[arr][at] = value
        assert hip.shade_rays(R._h, 65, vp(o), vp(d), 0, 0, vp(rgb), None, None, None, None) == B.MDH_E_INVALID, what
    assert (rgb == -3.0).all()
    assert hip.shade_rays(R._h, 65, vp(org), vp(drs), 0, 0, vp(rgb), None, None, None, None) == B.MDH_OK  # (every output but rgb may be null)
    assert np.isfinite(rgb).all()
    R.Destroy()


# ------------------------------------------------------------------------------------ 5. it edits nothing and waits for the right frame
@pytest.mark.parametrize("screen_replay", [0, 1])
def test_queries_edit_nothing(hip, screen_replay):
    """four frames with a query between them, four frames without: every frame's pixels are the same, and the radiance
    replay, the probe settle and the screen replay have counted the same passes of each kind"""
    org, drs = rq.room_rays(65)
    outs = []
    for queries in (True, False):
        R = rq.gi_room(hip)
        R.Set_Option(B.OPT_SCREEN_REPLAY, screen_replay)
        frames = []
        for f in range(4):
            R.Render()
            if queries:
                R.Shade_Rays(org, drs, Mode=(0, 2)[f % 2], Tone_Map=bool(f & 2))
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
    """three frames nobody waited for, then a query: the answer of a renderer that called Finish first, and the framebuffer of
    a screen pass issued at that point over the same camera rays"""
    with S.frame_size():
        Ra, Rb = rq.gi_room(hip), rq.gi_room(hip)
    org, drs = Ra.Camera_Rays(W, H)
    for R in (Ra, Rb):
        for _ in range(3):
            R.Render()
    Rb.Finish()
    a = Ra.Shade_Rays(org, drs, Tone_Map=True)
    b = Rb.Shade_Rays(org, drs, Tone_Map=True)
    for k in a:
        assert same(a[k], b[k]), k
    Ra.Render_Pass(B.PASS_SCREEN)
    assert same(a["rgb"], Ra.Read_Framebuffer().reshape(-1, 3))
    # ... and frames go on behind the query as they go on without it
    Ra.Render()
    Rb.Render()
    assert same(Ra.Read_Framebuffer(), Rb.Read_Framebuffer())
    Ra.Destroy()
    Rb.Destroy()


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(hip):
    org, drs = rq.room_rays(65)
    R, Rref = rq.gi_room(hip), rq.gi_room(hip)
    R.Render()
    Rref.Render()
    assert _status(lambda: R.Shade_Rays(org, drs)) == B.MDH_OK
    rgb = np.full((65, 3), -3.0, np.float32)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    def raw(r, mode=0, n=65, o=org, d=drs, out=rgb):
        return hip.shade_rays(r._h, n, vp(o) if o is not None else None, vp(d) if d is not None else None, mode, 0,
                              vp(out) if out is not None else None, None, None, None, None)
    assert raw(R, mode=1) == B.MDH_E_INVALID and raw(R, mode=3) == B.MDH_E_INVALID and raw(R, mode=-1) == B.MDH_E_INVALID
    assert raw(R, n=-1) == B.MDH_E_INVALID and raw(R, out=None) == B.MDH_E_INVALID and raw(R, o=None) == B.MDH_E_INVALID and raw(R, d=None) == B.MDH_E_INVALID
    assert raw(R, n=0) == B.MDH_OK
    for spec in (1, 3):
        R.Set_Option(B.OPT_INDIRECT_SPECULAR, spec)
        assert raw(R) == B.MDH_E_STATE and raw(R, mode=2) == B.MDH_E_STATE, spec
    R.Set_Option(B.OPT_INDIRECT_SPECULAR, 2)
    assert (rgb == -3.0).all()
    assert raw(R) == B.MDH_OK and np.isfinite(rgb).all()
    # camera rays: a frame needs pixels and arrays
    buf = np.zeros((4, 3), np.float32)
    assert hip.camera_rays(R._h, 0, 2, vp(buf), vp(buf)) == B.MDH_E_INVALID and hip.camera_rays(R._h, 2, -1, vp(buf), vp(buf)) == B.MDH_E_INVALID
    assert hip.camera_rays(R._h, 2, 2, None, vp(buf)) == B.MDH_E_INVALID and hip.camera_rays(R._h, 2, 2, vp(buf), None) == B.MDH_E_INVALID
    # the refused calls changed nothing: the next frame is the frame of a renderer that was asked for the one good query alone
    Rref.Set_Option(B.OPT_INDIRECT_SPECULAR, 1)
    Rref.Set_Option(B.OPT_INDIRECT_SPECULAR, 3)
    Rref.Set_Option(B.OPT_INDIRECT_SPECULAR, 2)
    R.Render()
    Rref.Render()
    assert same(R.Read_Framebuffer(), Rref.Read_Framebuffer())
    assert R.Probe_Settle_Stats() == Rref.Probe_Settle_Stats() and R.Radiance_Replay_Stats() == Rref.Radiance_Replay_Stats()
    R.Destroy()
    Rref.Destroy()
    # a scene with a user-defined kind
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rc.Shade_Rays(org, drs)) == B.MDH_E_STATE and _status(lambda: Rc.Shade_Rays(org, drs, Mode=2)) == B.MDH_E_STATE
    Rc.Destroy()
    # a light at x = 5000: beyond the bound that keeps the shadow marches' parameter below 2^14
    Rl = rq.small_mesh(hip)
    assert _status(lambda: Rl.Shade_Rays(org, drs)) == B.MDH_OK
    Rl.Set_Light(1, point_lights.Point_Light, point_lights.Create((5000.0, 1.0, -5.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rl.Shade_Rays(org, drs)) == B.MDH_E_STATE and _status(lambda: Rl.Shade_Rays(org, drs, Mode=2)) == B.MDH_E_STATE
    Rl.Set_Light(1, point_lights.Point_Light, point_lights.Create((0.0, 1.0, -5.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rl.Shade_Rays(org, drs)) == B.MDH_OK
    Rl.Destroy()
    # max_dist 4096
    scene = scenes.Compile([(spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False), Max_Dist=4096.0)
    Rm = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rm.Add_Primitive(spheres.Sphere, spheres.Create((2.0, 2.0, 2.0), 0.5, 0))
    Rm.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rm.Shade_Rays(org, drs)) == B.MDH_E_STATE and _status(lambda: Rm.Shade_Rays(org, drs, Mode=2)) == B.MDH_E_STATE
    Rm.Destroy()


def test_volumetrics_compose_no_fog(hip):
    """a renderer with volumetrics enabled answers with the bits of one without"""
    outs = []
    org, drs = rq.room_rays(65)
    for vol in (SMALL_VOL, None):
        R = examples.light_shafts(16, 16, Probes=SMALL_PROBES, Volumetrics=vol if vol is not None else renderers.No_Volumetrics, Binding=hip)
        irr, rad = S.seeded_atlases(R)
        R.Write_Texture(B.TEX_IRRADIANCE, irr)
        R.Write_Texture(B.TEX_RADIANCE, rad)
        outs.append(R.Shade_Rays(org, drs, Tone_Map=True))
        R.Destroy()
    for k in outs[0]:
        assert same(outs[0][k], outs[1][k]), k
