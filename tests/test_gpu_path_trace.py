"""mdh_path_trace on the device: zero bounces against the validated pixel program (mode 2 without occlusion), the fused kernel
against the estimator composed from the public queries bit for bit, sums that do not depend on how samples and batches are
split, the furnace-free plane against its analytic mean and its numpy restatement, free rays against the float64 path tracer
of tests/path_trace_cases.py, every refusal before a launch, and frames that go on across the queries.  The device-array call
runs in a child process with torch (tests/path_trace_device_checks.py), like the device-array ray queries.
(No ray here comes near the bound that stands in for a stall guard: max_dist is 20 and every coordinate below 10.)"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import custom_kinds as ck
import path_trace_cases as PT
import path_trace_device_checks as checks
import ray_query_cases as rq
import ref64
import ref64_cases
import shade_points_cases as P
import shade_rays_cases as S
from helpers import SEED, SMALL_PROBES
from madarch_amd import _binding as B
from madarch_amd import renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import spheres

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = S.FRAME_W, S.FRAME_H
SEED_P = PT.SEED_PATHS


def same(a, b):
    return np.array_equal(S.bits(a), S.bits(b))


def _status(call):
    try:
        call()
    except B.MadarchError as e:
        return e.status
    return B.MDH_OK


# ------------------------------------------------------------------------------------ f. zero bounces: the pixel program
@pytest.mark.parametrize("name", list(S.FRAME_SCENES))
def test_zero_bounces_equal_the_pixel_program(hip, name):
    R = S.frame_renderer(hip, name, 2)
    R.Set_Option(B.OPT_AO_STEPS, 0)  # (occlusion is then exactly 1)
    org, drs = R.Camera_Rays(W, H)
    want = R.Shade_Rays(org, drs, Mode=2, Tone_Map=False)
    got = R.Path_Trace(org, drs, Seed=SEED_P, Bounces=0, Sample_Count=1)
    print("%s: %d of %d rays hit" % (name, int(want["hit"].sum()), W * H))
    assert want["hit"].any()
    assert same(got["hit"], want["hit"]) and same(got["index"], want["index"]) and same(got["t"], want["t"])
    assert (got["rgb"] == want["rgb"]).all()  # (as numbers: tolerates a signed zero)
    R.Destroy()


# ------------------------------------------------------------------------------------ g. the fused kernel = the public queries
COMPOSED = ("rooms", "partition, Clamp", "mesh, triangle BVH", "open scene")


@pytest.mark.parametrize("name", COMPOSED)
def test_fused_kernel_equals_the_composition_of_the_public_queries(hip, name):
    with PT.material_log() as table:
        R = S.FRAME_SCENES[name](hip)
    R.Set_Option(B.OPT_AO_STEPS, 0)
    org, drs = P.scene_rays(name, 257)
    id_first, sample = 1000, 3
    want, (hit, index, t) = PT.compose(R, table, org, drs, SEED_P, id_first, sample, 3)
    got = R.Path_Trace(org, drs, Seed=SEED_P, Id_First=id_first, Sample_First=sample, Sample_Count=1, Bounces=3)
    R.Destroy()
    print("%s: %d of 257 primary rays hit, %d colours differ from zero" % (name, int((hit == 1).sum()), int((want != 0).any(axis=1).sum())))
    assert (hit == 1).any() and (want != 0).any()
    assert same(got["hit"], hit) and same(got["index"], index) and same(got["t"], t)
    bad = np.nonzero(~((S.bits(got["rgb"]) == S.bits(want)) | (np.isnan(got["rgb"]) & np.isnan(want))).all(axis=1))[0]
    assert len(bad) == 0, "%d rays differ, first %d: %s against the composition's %s" % (len(bad), bad[0], got["rgb"][bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------ h. accumulation and batches
def test_sums_do_not_depend_on_slices_and_batches(hip):
    R = rq.gi_room(hip)
    org, drs = rq.room_rays(257)
    kw = dict(Seed=SEED_P, Bounces=3)
    whole = R.Path_Trace(org, drs, Sample_First=0, Sample_Count=8, **kw)
    first = R.Path_Trace(org, drs, Sample_First=0, Sample_Count=4, **kw)
    both = R.Path_Trace(org, drs, Sample_First=4, Sample_Count=4, Rgb_Accum=first["rgb"], **kw)
    for k in whole:
        assert same(both[k], whole[k]), k
    assert not same(first["rgb"], whole["rgb"])  # (the samples do add up to something)
    # one sample at a time
    acc = None
    for s in range(8):
        acc = R.Path_Trace(org, drs, Sample_First=s, Sample_Count=1, Rgb_Accum=acc, **kw)["rgb"]
    assert same(acc, whole["rgb"])
    # a batch split in two, the ids moved along
    a = R.Path_Trace(org[:100], drs[:100], Sample_Count=8, **kw)
    b = R.Path_Trace(org[100:], drs[100:], Id_First=100, Sample_Count=8, **kw)
    for k in whole:
        assert same(np.concatenate([a[k], b[k]]), whole[k]), k
    # ... and not moved: other numbers, other sums
    c = R.Path_Trace(org[100:], drs[100:], Id_First=0, Sample_Count=8, **kw)
    assert not same(c["rgb"], whole["rgb"][100:])
    for n in (1, 63, 64, 65, 257):
        part = R.Path_Trace(org[:n], drs[:n], Sample_Count=8, **kw)
        for k in whole:
            assert same(part[k][0], whole[k][0]), (k, n)
            assert same(part[k], whole[k][:n]), (k, n)
    # another seed, other sums; no samples, nothing added and nothing launched
    other = R.Path_Trace(org, drs, Seed=SEED_P + 1, Bounces=3, Sample_Count=8)
    assert not same(other["rgb"], whole["rgb"]) and same(other["t"], whole["t"])
    none = R.Path_Trace(org, drs, Sample_Count=0, Rgb_Accum=whole["rgb"], **kw)
    assert same(none["rgb"], whole["rgb"])
    assert np.isfinite(whole["rgb"]).all()
    R.Destroy()


# ------------------------------------------------------------------------------------ i. the furnace-free plane
def test_plane_on_the_device(hip):
    R = ref64_cases.make_renderer(PT.plane_desc(), 16, 16, hip)
    org, drs = PT.plane_rays()
    S_ = PT.PLANE_SAMPLES
    got = R.Path_Trace(org, drs, Seed=SEED_P, Sample_Count=S_, Bounces=1)
    R.Destroy()
    assert got["hit"].all()
    est = got["rgb"].astype(np.float64) / S_
    mean, dev = PT.plane_expected()
    print("largest deviation from the analytic mean: %.3f of its bound" % (np.abs(est - mean[None, :]) / dev[None, :]).max())
    assert (np.abs(est - mean[None, :]) <= dev[None, :]).all()
    want = PT.ref_plane()
    tol = ref64.COLOUR_ATOL + ref64.COLOUR_RTOL * np.abs(want)
    print("largest error against the numpy restatement: %.3f of its tolerance" % (np.abs(est - want) / tol).max())
    assert (np.abs(est - want) <= tol).all()


# ------------------------------------------------------------------------------------ j. free rays against float64
@pytest.mark.parametrize("samples", PT.FREE_SAMPLES)
@pytest.mark.parametrize("name", ["room", "open"])
def test_free_rays_against_float64(hip, name, samples):
    R = ref64_cases.make_renderer(PT.describe(name), 16, 16, hip)
    org, drs = PT.free_rays(name)
    got = R.Path_Trace(org, drs, Seed=SEED_P, Sample_Count=samples, Bounces=PT.FREE_BOUNCES)
    R.Destroy()
    ref64.hold_values("%s, %d samples, %d free rays" % (name, samples, len(org)), PT.free_runs(name, samples), got["rgb"],
                      ref64.COLOUR_RTOL, ref64.COLOUR_ATOL * samples)


# ------------------------------------------------------------------------------------ k. device arrays and refusals
@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("path_trace") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "path_trace_device_checks.py"), out]
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


def test_refusals_launch_nothing(hip):
    org, drs = rq.room_rays(65)
    R, Rref = rq.gi_room(hip), rq.gi_room(hip)
    R.Render()
    Rref.Render()
    rgb = np.full((65, 3), -3.0, np.float32)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    def raw(r, n=65, o=org, d=drs, out=rgb, s0=0, sc=1, nb=3):
        return hip.path_trace(r._h, n, vp(o) if o is not None else None, vp(d) if d is not None else None, SEED_P, 0, s0, sc, nb,
                              vp(out) if out is not None else None, None, None, None)
    assert raw(R, n=-1) == B.MDH_E_INVALID and raw(R, out=None) == B.MDH_E_INVALID and raw(R, o=None) == B.MDH_E_INVALID and raw(R, d=None) == B.MDH_E_INVALID
    assert raw(R, nb=7) == B.MDH_E_INVALID and raw(R, nb=-1) == B.MDH_E_INVALID
    assert raw(R, s0=-1) == B.MDH_E_INVALID and raw(R, sc=-1) == B.MDH_E_INVALID and raw(R, s0=2 ** 31 - 1, sc=1) == B.MDH_E_INVALID
    for what, (arr, at, value) in {"a NaN": (1, (7, 2), np.nan), "an infinity": (0, (64, 0), np.inf), "an origin at 2000": (0, (3, 1), 2000.0),
                                   "a direction of 3": (1, (40, 0), 3.0), "a zero direction": (1, (12, slice(None)), 0.0)}.items():
        o, d = org.copy(), drs.copy()
        (o, d)[arr][at] = value
        assert raw(R, o=o, d=d) == B.MDH_E_INVALID, what
    assert raw(R, n=0) == B.MDH_OK and raw(R, sc=0) == B.MDH_OK
    # an open frame
    R.Frame_Begin()
    assert raw(R) == B.MDH_E_STATE
    Rref.Frame_Begin()
    for r in (R, Rref):
        r.Frame_End()
        r.Finish()
    assert (rgb == -3.0).all()
    # the options of the pixel program do not enter
    R.Set_Option(B.OPT_INDIRECT_SPECULAR, 1)
    assert raw(R, nb=6) == B.MDH_OK and np.isfinite(rgb).all()
    R.Set_Option(B.OPT_INDIRECT_SPECULAR, 2)
    Rref.Set_Option(B.OPT_INDIRECT_SPECULAR, 1)
    Rref.Set_Option(B.OPT_INDIRECT_SPECULAR, 2)
    # the refused calls changed nothing: the next frame is the frame of a renderer that was asked for nothing
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
    assert _status(lambda: Rc.Path_Trace(org, drs)) == B.MDH_E_STATE
    Rc.Destroy()
    # a light at x = 5000
    Rl = rq.small_mesh(hip)
    assert _status(lambda: Rl.Path_Trace(org, drs)) == B.MDH_OK
    Rl.Set_Light(1, point_lights.Point_Light, point_lights.Create((5000.0, 1.0, -5.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rl.Path_Trace(org, drs)) == B.MDH_E_STATE
    Rl.Destroy()
    # a max_dist of 2048
    scene = scenes.Compile([(spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False), Max_Dist=2048.0)
    Rm = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rm.Add_Primitive(spheres.Sphere, spheres.Create((2.0, 2.0, 2.0), 0.5, 0))
    Rm.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rm.Path_Trace(org, drs)) == B.MDH_E_STATE
    Rm.Destroy()


# ------------------------------------------------------------------------------------ l. nothing else moves
@pytest.mark.parametrize("screen_replay", [0, 1])
def test_queries_edit_nothing(hip, screen_replay):
    """four frames with path queries between them, four frames without: every frame's pixels are the same, and the radiance
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
                R.Path_Trace(org, drs, Seed=SEED + f, Sample_First=f, Sample_Count=2, Bounces=(3, 0, 6, 1)[f])
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
