"""The path-traced frame on the device.  The un-jittered accumulator against mdh_path_trace over mdh_camera_rays' rays bit for bit --
which holds the tile mapping, the cut tiles and the recorded primary segment at once --, its rays against the numpy
restatement of tests/path_frame_cases.py, the jittered accumulator against the chain of public queries over its own rays, the
resolve against numpy, the pixel program and the window's bytes, every refusal before a launch, the captured camera, and frames
that go on across the calls.  The device-array forms run in a child process with torch (tests/path_frame_device_checks.py).
Frames are 20 x 12: two and a half by one and a half 8 x 8 tiles."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import custom_kinds as ck
import path_frame_cases as PF
import path_frame_device_checks as checks
import path_trace_cases as PT
import ray_query_cases as rq
import shade_rays_cases as S
from helpers import SMALL_PROBES
from madarch_amd import _binding as B
from madarch_amd import renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import spheres
from test_gpu_path_trace import COMPOSED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = PF.W, PF.H
SEED = PF.SEED
assert (W, H) == (S.FRAME_W, S.FRAME_H) == (20, 12)


def same(a, b):
    return np.array_equal(S.bits(a), S.bits(b))


def _status(call):
    try:
        call()
    except B.MadarchError as e:
        return e.status
    return B.MDH_OK


def sums_of(R):
    return R.Path_Frame_Read(Rgb=False, Sums=True)["sums"].reshape(-1, 3)


# ------------------------------------------------------------------------------------ 3. the un-jittered frame = the ray query
@pytest.mark.parametrize("name", COMPOSED + ("partition, Clamp, global residency",))
def test_unjittered_frame_equals_the_ray_query(hip, name):
    R = S.FRAME_SCENES[name](hip)
    if name.endswith("global residency"):
        assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == 1
    org, drs = R.Camera_Rays(W, H)
    want = R.Path_Trace(org, drs, Seed=SEED, Id_First=0, Sample_First=0, Sample_Count=3, Bounces=3)
    print("%s: %d of %d primary rays hit" % (name, int(want["hit"].sum()), W * H))
    assert want["hit"].any() and len(np.unique(S.bits(want["rgb"]), axis=0)) > 4
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=3, Jitter=False)
    R.Path_Frame_Accumulate(1)
    R.Path_Frame_Accumulate(2)
    split = sums_of(R)
    assert R.Path_Frame_Info() == {"width": W, "height": H, "samples": 3, "bounces": 3, "jitter": 0}
    bad = np.nonzero(~((S.bits(split) == S.bits(want["rgb"])) | (np.isnan(split) & np.isnan(want["rgb"]))).all(axis=1))[0]
    assert len(bad) == 0, "%d pixels differ, first %d: %s against the ray query's %s" % (len(bad), bad[0], split[bad[0]], want["rgb"][bad[0]])
    # 1 + 2 against 3 in one call
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=3, Jitter=False)
    R.Path_Frame_Accumulate(3)
    assert PF.same_or_nan(sums_of(R), split)
    R.Destroy()


# ------------------------------------------------------------------------------------ 4. the rays
def test_the_rays(hip):
    R = rq.gi_room(hip)
    rows = PF.cam_rows()
    R.Set_Camera_Position(PF.CAM_POS)
    R.Set_Camera_Orientation(rows.tolist())
    centre = R.Camera_Rays(W, H)
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=False)
    for s in (0, 5):
        org, drs = R.Path_Frame_Rays(s)
        assert same(org, centre[0]) and same(drs, centre[1]), s
    want_o, want_d = PF.frame_rays(W, H, SEED, 0, False, PF.CAM_POS, rows)
    assert same(centre[0], want_o) and same(centre[1], want_d)  # (the restatement restates camera_ray)
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=True)
    seen = []
    for s in (0, 5):
        org, drs = R.Path_Frame_Rays(s)
        want_o, want_d = PF.frame_rays(W, H, SEED, s, True, PF.CAM_POS, rows)
        assert same(org, want_o) and same(drs, want_d), s
        assert (S.bits(drs) != S.bits(centre[1])).any(axis=1).all() and (S.bits(org) != S.bits(centre[0])).any(axis=1).all(), s
        seen.append(drs)
    assert (S.bits(seen[0]) != S.bits(seen[1])).any(axis=1).all()  # (every sample its own point)
    R.Destroy()


# ------------------------------------------------------------------------------------ 5. the jittered frame = the chain
@pytest.mark.parametrize("name", ["rooms", "open scene"])
def test_jittered_frame_equals_the_chain_of_ray_queries(hip, name):
    R = S.FRAME_SCENES[name](hip)
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=True)
    R.Path_Frame_Accumulate(4)
    got = sums_of(R)
    acc = None
    for s in range(4):
        org, drs = R.Path_Frame_Rays(s)
        acc = R.Path_Trace(org, drs, Seed=SEED, Id_First=0, Sample_First=s, Sample_Count=1, Bounces=2, Rgb_Accum=acc)["rgb"]
    bad = np.nonzero(~((S.bits(got) == S.bits(acc)) | (np.isnan(got) & np.isnan(acc))).all(axis=1))[0]
    assert len(bad) == 0, "%d pixels differ, first %d: %s against the chain's %s" % (len(bad), bad[0], got[bad[0]], acc[bad[0]])
    assert np.isfinite(got).all() and (got != 0).any()
    # the resolve: one binary32 division a channel
    rgb = R.Path_Frame_Read()
    assert rgb["samples"] == 4 and rgb["rgb"].shape == (H, W, 3)
    assert same(rgb["rgb"].reshape(-1, 3), (got / np.float32(4)).astype(np.float32))
    # the jitter moves the image: the un-jittered sums differ
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=False)
    R.Path_Frame_Accumulate(4)
    assert not same(sums_of(R), got)
    R.Destroy()


@pytest.mark.parametrize("name", ["rooms", "partition, Fallback", "mesh, scanned"])
def test_zero_bounces_equal_the_pixel_program_in_sample_order(hip, name):
    R = S.frame_renderer(hip, name, 2)
    R.Set_Option(B.OPT_AO_STEPS, 0)  # (occlusion is then exactly 1)
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=0, Jitter=True)
    R.Path_Frame_Accumulate(3)
    got = sums_of(R)
    want = np.zeros((W * H, 3), np.float32)
    hits = 0
    for s in range(3):
        org, drs = R.Path_Frame_Rays(s)
        shaded = R.Shade_Rays(org, drs, Mode=2, Tone_Map=False)
        hits += int(shaded["hit"].sum())
        want = (want + shaded["rgb"]).astype(np.float32)
    print("%s: %d of %d rays hit" % (name, hits, 3 * W * H))
    assert hits > 0
    assert same(got, want)
    R.Destroy()


# ------------------------------------------------------------------------------------ 6. the resolve
@pytest.mark.parametrize("name", ["rooms", "open scene"])
def test_the_resolve_is_the_pixel_program_and_the_windows_bytes(hip, name):
    R = S.frame_renderer(hip, name, 2)
    R.Set_Option(B.OPT_AO_STEPS, 0)
    org, drs = R.Camera_Rays(W, H)
    want = R.Shade_Rays(org, drs, Mode=2, Tone_Map=True)["rgb"]
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=0, Jitter=False)
    R.Path_Frame_Accumulate(1)
    got = R.Path_Frame_Read(Tone_Map=True, Rgb=True, Rgba8=True, Sums=True)
    assert got["samples"] == 1 and got["rgba8"].shape == (H, W, 4) and got["rgba8"].dtype == np.uint8
    assert same(got["rgb"].reshape(-1, 3), want)
    R.Render()
    R.Swap_Buffers()
    front = R.Front_Buffer()
    assert front.shape == (H, W, 4)
    if name == "open scene":  # (the room's direct light alone is black in eight bits from its camera: the sky is not)
        assert len(np.unique(front.reshape(-1, 4), axis=0)) > 4
    assert np.array_equal(got["rgba8"], front)
    # the linear image beside it
    linear = R.Path_Frame_Read(Tone_Map=False)["rgb"]
    assert same(linear, got["sums"])  # (one sample: sum / 1)
    if name == "open scene":
        assert not same(linear, got["rgb"])
    R.Destroy()


def test_a_camera_beyond_the_bound_gives_nan_sums_and_black_bytes(hip):
    R = rq.gi_room(hip)
    R.Set_Camera_Position((2000.0, 2.0, 0.0))
    for jitter in (False, True):
        R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=3, Jitter=jitter)
        R.Path_Frame_Accumulate(2)  # (returns: the lanes' own check, no march)
        R.Path_Frame_Accumulate(1)  # ... and the sums stay so
        got = R.Path_Frame_Read(Tone_Map=True, Rgba8=True, Sums=True)
        assert (got["sums"].view(np.uint32) == PT.BAD_BITS).all(), jitter
        assert np.isnan(got["rgb"]).all()
        assert (got["rgba8"].reshape(-1, 4) == np.array([0, 0, 0, 255], np.uint8)).all()
    R.Destroy()


# ------------------------------------------------------------------------------------ 7. device arrays
@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("path_frame") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "path_frame_device_checks.py"), out]
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


# ------------------------------------------------------------------------------------ 8. refusals and state
def test_refusals_launch_nothing(hip):
    R = rq.gi_room(hip)
    R.Set_Option(B.OPT_TIMING, 1)
    org, drs = rq.room_rays(65)
    R.Path_Trace(org, drs, Seed=SEED, Bounces=1)
    before = R.Ray_Query_Time()
    assert before > 0.0
    h = R._h
    n = C.c_int32(-5)
    buf = np.full((W * H, 3), -3.0, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    # no accumulator open
    assert hip.path_frame_accumulate(h, 1) == B.MDH_E_STATE
    assert hip.path_frame_read(h, 0, p, None, None, C.byref(n)) == B.MDH_E_STATE and hip.path_frame_rays(h, 0, p, p) == B.MDH_E_STATE
    assert R.Path_Frame_Info() == {"width": 0, "height": 0, "samples": 0, "bounces": 0, "jitter": 0}
    # begin
    for args in ((0, H, 1, 3, 1), (W, 0, 1, 3, 1), (-1, H, 1, 3, 1), (8193, 8192, 1, 3, 1), (1 << 30, 1 << 30, 1, 3, 1), (W, H, 1, 7, 1), (W, H, 1, -1, 1), (W, H, 1, 3, 2),
                 (W, H, 1, 3, -1)):
        assert hip.path_frame_begin(h, *args) == B.MDH_E_INVALID, args
    assert R.Path_Frame_Info()["width"] == 0  # (a refused begin opens nothing)
    R.Frame_Begin()
    assert hip.path_frame_begin(h, W, H, 1, 3, 1) == B.MDH_E_STATE
    R.Frame_End()
    R.Finish()
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=3, Jitter=True)
    # read before a sample: there is no 0 / 0 image
    assert hip.path_frame_read(h, 0, p, None, None, C.byref(n)) == B.MDH_E_STATE and n.value == -5
    assert hip.path_frame_accumulate(h, 0) == B.MDH_OK and R.Path_Frame_Info()["samples"] == 0
    assert hip.path_frame_accumulate(h, -1) == B.MDH_E_INVALID
    R.Frame_Begin()
    assert hip.path_frame_accumulate(h, 1) == B.MDH_E_STATE
    R.Frame_End()
    R.Finish()
    assert hip.path_frame_rays(h, -1, p, p) == B.MDH_E_INVALID and hip.path_frame_rays(h, 0, None, p) == B.MDH_E_INVALID and hip.path_frame_rays(h, 0, p, None) == B.MDH_E_INVALID
    assert R.Ray_Query_Time() == before  # nothing was launched
    assert (buf == -3.0).all()
    R.Path_Frame_Accumulate(2)
    R.Ray_Query_Wait()
    assert R.Ray_Query_Time() != before  # (the accumulate kernel is what is timed)
    assert hip.path_frame_accumulate(h, 2 ** 31 - 2) == B.MDH_E_INVALID  # 2 + (2^31 - 2) is beyond 2^31 - 1
    assert hip.path_frame_read(h, 2, p, None, None, None) == B.MDH_E_INVALID and hip.path_frame_read(h, -1, p, None, None, None) == B.MDH_E_INVALID
    assert hip.path_frame_read(h, 0, None, None, None, C.byref(n)) == B.MDH_OK and n.value == 2  # (every output is optional)
    first = sums_of(R)
    # begin again restarts from zero with the new size
    R.Path_Frame_Begin(7, 5, Seed=SEED, Bounces=1, Jitter=False)
    assert R.Path_Frame_Info() == {"width": 7, "height": 5, "samples": 0, "bounces": 1, "jitter": 0}
    R.Path_Frame_Accumulate(1)
    small = R.Path_Frame_Read(Sums=True)
    assert small["sums"].shape == (5, 7, 3) and small["samples"] == 1
    o7, d7 = R.Camera_Rays(7, 5)
    assert PF.same_or_nan(small["sums"].reshape(-1, 3), R.Path_Trace(o7, d7, Seed=SEED, Bounces=1)["rgb"])
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=3, Jitter=True)
    R.Path_Frame_Accumulate(2)
    assert same(sums_of(R), first)
    # end, then read
    R.Path_Frame_End()
    assert hip.path_frame_read(h, 0, p, None, None, None) == B.MDH_E_STATE and hip.path_frame_accumulate(h, 1) == B.MDH_E_STATE
    R.Path_Frame_End()  # (again: nothing to free)
    R.Destroy()
    # a scene with a user-defined kind
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rc.Path_Frame_Begin(W, H)) == B.MDH_E_STATE
    Rc.Destroy()
    # a light at x = 5000: the accumulator that was open refuses the samples
    Rl = rq.small_mesh(hip)
    Rl.Path_Frame_Begin(W, H, Seed=SEED)
    assert _status(lambda: Rl.Path_Frame_Accumulate(1)) == B.MDH_OK
    Rl.Set_Light(1, point_lights.Point_Light, point_lights.Create((5000.0, 1.0, -5.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rl.Path_Frame_Accumulate(1)) == B.MDH_E_STATE and _status(lambda: Rl.Path_Frame_Begin(W, H)) == B.MDH_E_STATE
    assert Rl.Path_Frame_Info()["samples"] == 1
    Rl.Destroy()
    # a max_dist of 2048
    scene = scenes.Compile([(spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False), Max_Dist=2048.0)
    Rm = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rm.Add_Primitive(spheres.Sphere, spheres.Create((2.0, 2.0, 2.0), 0.5, 0))
    Rm.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rm.Path_Frame_Begin(W, H)) == B.MDH_E_STATE
    Rm.Destroy()


def test_the_camera_is_captured_at_begin(hip):
    R, Rref = rq.gi_room(hip), rq.gi_room(hip)
    for r in (R, Rref):
        r.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=True)
        r.Path_Frame_Accumulate(1)
    R.Set_Camera_Position(PF.CAM_POS)
    R.Set_Camera_Orientation(PF.cam_rows().tolist())
    for r in (R, Rref):
        r.Path_Frame_Accumulate(2)
    assert same(sums_of(R), sums_of(Rref))
    assert same(R.Path_Frame_Rays(1)[0], Rref.Path_Frame_Rays(1)[0])
    # ... and the next begin takes the camera as it then stands
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=True)
    R.Path_Frame_Accumulate(3)
    assert not same(sums_of(R), sums_of(Rref))
    R.Destroy()
    Rref.Destroy()


# ------------------------------------------------------------------------------------ 9. nothing edited
@pytest.mark.parametrize("screen_replay", [0, 1])
def test_the_accumulator_edits_nothing(hip, screen_replay):
    """four frames with accumulate and read between them, four frames without: every frame's pixels and the atlases are the same,
    and the radiance replay, the probe settle and the screen replay have counted the same passes of each kind; a raycast, a
    surface mesh and a shaded point in between keep their bits, and so does the accumulator"""
    org, drs = rq.room_rays(65)
    outs = []
    for calls in (True, False):
        R = rq.gi_room(hip)
        R.Set_Option(B.OPT_SCREEN_REPLAY, screen_replay)
        frames, others = [], None
        if calls:
            R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=True)
        for f in range(4):
            R.Render()
            if calls:
                R.Path_Frame_Accumulate((2, 1, 3, 1)[f])
                if f == 1:
                    others = queries(R, org, drs)
                if f % 2 == 1:
                    R.Path_Frame_Read(Tone_Map=True, Rgba8=True)
            frames.append(R.Read_Framebuffer())
        R.Finish()
        atlases = [R.Read_Texture(t) for t in (B.TEX_IRRADIANCE, B.TEX_RADIANCE)]
        if calls:
            sums = sums_of(R)
            assert R.Path_Frame_Info()["samples"] == 7
        else:
            others = queries(R, org, drs)
        outs.append((frames, atlases, R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats(), others))
        R.Destroy()
    (fb_q, at_q, rad_q, settle_q, scr_q, oth_q), (fb, at, rad, settle, scr, oth) = outs
    print("radiance replay %s, probe settle %s, screen replay %s" % (rad, settle, scr))
    for f in range(4):
        assert same(fb_q[f], fb[f]), f
    assert same(at_q[0], at[0]) and same(at_q[1], at[1])
    assert rad_q == rad and settle_q == settle and scr_q == scr
    assert sum(rad) >= 1 and (screen_replay == 0 or scr[1] + scr[2] > 0)  # (the counters do count)
    for k in oth:
        assert same(oth_q[k], oth[k]), k
    # the accumulator kept its bits: seven samples in one call of a renderer that did nothing else
    R = rq.gi_room(hip)
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=True)
    R.Path_Frame_Accumulate(7)
    assert same(sums_of(R), sums)
    R.Destroy()


def queries(R, org, drs):
    """one Raycast, one Surface_Mesh and one Shade_Points: their answers by name.  (The points are shaded in mode 2, which reads
    no atlas: the moment of the call among the frames does not enter.)"""
    rc = R.Raycast(org, drs)
    mesh = R.Surface_Mesh((1.0, -2.0, 1.5), 0.5, (8, 15, 9))
    hit = rc["hit"] == 1
    mats = R.Primitive_Material(rc["index"][hit])
    pts = R.Shade_Points(rc["position"][hit], rc["normal"][hit], drs[hit], mats, Mode=2)
    assert hit.any() and len(mesh["positions"]) > 0
    return {"raycast t": rc["t"], "raycast index": rc["index"], "mesh positions": mesh["positions"], "mesh quads": mesh["quads"], "points": pts}
