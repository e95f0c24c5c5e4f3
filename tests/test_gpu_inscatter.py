"""mdh_inscatter_points and mdh_inscatter_rays on the device (tests/inscatter_cases.py has the scenes and the yardsticks):
a. points against the frame's froxel texture, bit for bit, in every scene variant the ray queries run over;
b. rays against the frame's scattering texture, bit for bit, where every tap of the fold falls on a texel centre;
c. the chain: a ray's sum is step * the sequential binary32 sum of the points' call with f given, around one and two chunks;
d. free rays, their sample points and their marched lengths against float64 (ref64.hold_values, the project's tolerances);
e. every refusal before a launch, outputs untouched; a scene without lights; a renderer without volumetrics;
f. nothing is edited, pending edits are seen -- and, with torch tensors as the device memory, the _device forms: the host
   arrays' bits, bad lanes, the order with the caller's stream (tests/inscatter_device_checks.py, run once in a child process
   for the reason tests/test_gpu_ray_streams.py gives; each test of the last block is one check's verdict)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import custom_kinds as ck
import inscatter_cases as IC
import inscatter_device_checks as checks
import ref64
import ref64_cases as RC
from helpers import SMALL_PROBES
from madarch_amd import _binding as B
from madarch_amd import renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import planes, spheres

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ a. points against the froxels
@pytest.mark.parametrize("vol", [0, 1], ids=["8x8x8 step 0.5", "16x8x4 step 0.25"])
@pytest.mark.parametrize("name", list(IC.VARIANTS))
def test_points_have_the_froxel_textures_bits(hip, name, vol):
    V = IC.VOL_A[vol]
    R = IC.VARIANTS[name](hip, V)
    R.Render()
    R.Finish()
    tex = R.Read_Texture(B.TEX_VISIBILITY)
    vw, vh, vz = V.Visibility_Resolution
    assert tex.shape == (vh * vz, vw, 3)
    pos, drs = IC.froxel_points(R, V)
    got = R.Inscatter_Points(pos, drs)
    lit = float((tex.max(axis=-1) > 0.0).mean())
    print("%s: %.2f of the froxels are lit" % (name, lit))
    assert lit > 0.1
    IC.assert_bits(got, tex.reshape(-1, 3), name)
    R.Destroy()


# ------------------------------------------------------------------------------------ b. rays against the scattering texture
@pytest.mark.parametrize("camera", ["identity", "rotated"])
def test_rays_have_the_scattering_textures_bits(hip, camera):
    V = IC.VOL_B
    R = IC.room(hip, V, camera)
    R.Render()
    R.Finish()
    assert np.isfinite(R.Read_Texture(B.TEX_VISIBILITY)).all()  # (a tap that is not finite would break the 0-weighted terms of the filter)
    scat = R.Read_Texture(B.TEX_SCATTERING)
    sw, sh = V.Scattering_Resolution
    assert scat.shape == (sh, sw, 4) and (scat[..., :3].max(axis=-1) > 0.0).mean() > 0.5
    org, drs = IC.texel_rays(R, sw, sh)
    length = np.ascontiguousarray(scat[..., 3].reshape(-1))
    assert (length < 4.0).any() and (length == 4.0).any()  # rays that end on the scene and rays that reach max_depth
    given = R.Inscatter_Rays(org, drs, length, 0.5)
    IC.assert_bits(given["rgb"], scat[..., :3].reshape(-1, 3), "the sum")
    assert np.array_equal(given["steps"], [IC.steps_of(0.5, t) for t in length])
    marched = R.Inscatter_Rays(org, drs, 4.0, 0.5, March=True)
    IC.assert_bits(marched["len"], length, "the marched length")
    IC.assert_bits(marched["rgb"], scat[..., :3].reshape(-1, 3), "the sum over the marched length")
    R.Destroy()


# ------------------------------------------------------------------------------------ c. the chain
# (every variant on a renderer created with No_Volumetrics; the room once more with a volume, which does not enter)
@pytest.mark.parametrize("name,volumetrics", [(name, False) for name in IC.CHAIN_VARIANTS] + [("room", True)])
def test_a_rays_sum_is_the_chain_of_its_points(hip, name, volumetrics):
    R = IC.VARIANTS[name](hip, IC.VOL_B if volumetrics else None)
    assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == (1 if "global residency" in name or "mesh" in name else 0)
    lit = 0
    for step in IC.CHAIN_STEPS:
        first = 0
        for n in IC.CHAIN_BATCHES:
            org, drs, counts = IC.chain_rays(name, n, first)
            first += n
            tmax = np.array([IC.tmax_for(step, c) for c in counts], np.float32)
            want = IC.chain_expected(R, org, drs, step, counts)
            got = R.Inscatter_Rays(org, drs, tmax, step)
            what = "%s, step %g, %d rays of %s steps" % (name, step, n, counts)
            IC.assert_bits(got["rgb"], want, what)
            assert got["steps"].tolist() == counts, what
            IC.assert_bits(got["len"], tmax, what)
            lit += int((want.max(axis=1) > 0.0).sum())
    assert lit > 10, "%s: the rays see no light" % name
    R.Destroy()


# ------------------------------------------------------------------------------------ d. float64
@pytest.mark.parametrize("name", ["room", "open"])
def test_free_rays_against_float64(hip, name):
    desc, org, drs, tmax, counts, P, D, F, ray = IC.free_samples(name)
    ray_runs, point_runs = IC.free_runs(name)
    R = RC.make_renderer(desc, 8, 8, hip)
    got = R.Inscatter_Rays(org, drs, tmax, IC.FREE_STEP)
    assert got["steps"].tolist() == counts
    ref64.hold_values(name + ": rays", ray_runs, got["rgb"], RC.SCATTER_RTOL, RC.SCATTER_ATOL)
    ref64.hold_values(name + ": points", point_runs, R.Inscatter_Points(P, D), RC.FROXEL_RTOL, RC.FROXEL_ATOL)
    # the marched length, with tmax = U
    U = IC.free_rays(name)[3]
    runs = IC.march_runs(name)
    fragile = IC.march_fragile(runs)
    assert fragile.mean() <= ref64.FRAGILE_CAP
    length = R.Inscatter_Rays(org, drs, U, IC.FREE_STEP, March=True)["len"].astype(np.float64)
    err = np.where(fragile, 0.0, np.abs(length - runs[0]["len"]))
    print("%s: marched lengths, fragile share %.4f, largest error %.3g (allowed %.3g)" % (name, fragile.mean(), err.max(), ref64.T_ATOL))
    assert (err <= ref64.T_ATOL).all(), "first at %s" % np.argwhere(err > ref64.T_ATOL)[:1]
    assert (runs[0]["len"] < U).any() and (runs[0]["len"] == U).any()
    R.Destroy()


# ------------------------------------------------------------------------------------ e. refusals
def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _status(call):
    try:
        call()
    except B.MadarchError as e:
        return e.status
    return B.MDH_OK


def test_refusals_launch_nothing(hip):
    n = 9
    R, Rref = IC.room(hip, IC.VOL_B), IC.room(hip, IC.VOL_B)
    org, drs, _ = IC.chain_rays("room", n, 0)
    one = np.ones(n, np.float32)
    rgb, length, steps = np.full((n, 3), -3.0, np.float32), np.full(n, -3.0, np.float32), np.full(n, -3, np.int32)

    def planted(a, at, value):
        b = a.copy()
        b[at] = value
        return b

    def rays(o=org, d=drs, t=one, march=0, step=0.1, count=n, out=rgb):
        return hip.inscatter_rays(R._h, count, vp(o) if o is not None else None, vp(d) if d is not None else None, vp(t) if t is not None else None,
                                  march, step, vp(out) if out is not None else None, vp(length), vp(steps))

    def points(p=org, d=drs, f=None, count=n, out=rgb):
        return hip.inscatter_points(R._h, count, vp(p) if p is not None else None, vp(d) if d is not None else None, vp(f) if f is not None else None,
                                    vp(out) if out is not None else None)
    max_dist = np.float32(20.0)
    calls = [
        ("rays: no origins", lambda: rays(o=None)), ("rays: no directions", lambda: rays(d=None)), ("rays: no lengths", lambda: rays(t=None)),
        ("rays: no colours", lambda: rays(out=None)), ("rays: n < 0", lambda: rays(count=-1)),
        ("rays: march 2", lambda: rays(march=2)), ("rays: march -1", lambda: rays(march=-1)),
        ("rays: step 0", lambda: rays(step=0.0)), ("rays: step < 0", lambda: rays(step=-0.1)), ("rays: step NaN", lambda: rays(step=float("nan"))),
        ("rays: step infinite", lambda: rays(step=float("inf"))),
        ("rays: more than 4096 steps in max_dist", lambda: rays(step=float(np.nextafter(np.float32(20.0 / 4096.0), np.float32(0.0))))),
        ("rays: a NaN origin", lambda: rays(o=planted(org, (3, 0), np.nan))), ("rays: an infinite direction", lambda: rays(d=planted(drs, (8, 2), np.inf))),
        ("rays: a NaN length", lambda: rays(t=planted(one, 2, np.nan))), ("rays: a negative length", lambda: rays(t=planted(one, 0, -0.001))),
        ("rays: an infinite length", lambda: rays(t=planted(one, 5, np.inf))),
        ("rays: a length above max_dist", lambda: rays(t=planted(one, 8, np.nextafter(max_dist, np.float32(np.inf))))),
        ("points: no positions", lambda: points(p=None)), ("points: no directions", lambda: points(d=None)), ("points: no colours", lambda: points(out=None)),
        ("points: n < 0", lambda: points(count=-1)),
        ("points: a NaN position", lambda: points(p=planted(org, (0, 1), np.nan))), ("points: an infinite direction", lambda: points(d=planted(drs, (4, 0), -np.inf))),
        ("points: a NaN f", lambda: points(f=planted(one, 7, np.nan))), ("points: an infinite f", lambda: points(f=planted(one, 7, np.inf))),
    ]
    R.Render()
    Rref.Render()
    for what, call in calls:
        assert call() == B.MDH_E_INVALID, what
    # the edges that are allowed: exactly 4096 steps in max_dist, a length of max_dist and of -0 -- and n = 0 without a launch
    assert rays(count=0) == B.MDH_OK and points(count=0) == B.MDH_OK
    assert (rgb == -3.0).all() and (length == -3.0).all() and (steps == -3).all()
    edge = R.Inscatter_Rays(org[:2], drs[:2], np.array([-0.0, 0.01], np.float32), 20.0 / 4096.0)
    assert edge["steps"].tolist() == [0, 3] and (edge["rgb"][0] == 0.0).all()
    R.Render()
    Rref.Render()
    R.Finish()
    Rref.Finish()
    assert np.array_equal(IC.bits(R.Read_Framebuffer()), IC.bits(Rref.Read_Framebuffer()))
    assert R.Probe_Settle_Stats() == Rref.Probe_Settle_Stats() and R.Radiance_Replay_Stats() == Rref.Radiance_Replay_Stats()
    # a scene with a user-defined kind
    scene = scenes.Compile([(ck.My_Sphere, 2), (spheres.Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    Rc = renderers.Create(windows.Open(16, 16), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    Rc.Add_Primitive(ck.My_Sphere, ck.sphere((2.0, 2.0, 2.0), 0.5, 0))
    Rc.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0, 4.0, 1.0), (0.9, 0.9, 0.9)))
    assert _status(lambda: Rc.Inscatter_Points(org, drs)) == B.MDH_E_STATE
    assert _status(lambda: Rc.Inscatter_Rays(org, drs, 1.0, 0.1)) == B.MDH_E_STATE
    assert hip.inscatter_rays(Rc._h, n, vp(org), vp(drs), vp(one), 0, 0.1, vp(rgb), vp(length), vp(steps)) == B.MDH_E_STATE
    assert (rgb == -3.0).all() and (length == -3.0).all() and (steps == -3).all()
    for r in (R, Rref, Rc):
        r.Destroy()


def test_a_scene_without_lights_answers_zeros(hip):
    scene = scenes.Compile([(planes.Plane, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(8, 8), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    R.Add_Primitive(planes.Plane, planes.Create((0.0, 1.0, 0.0), 1.0, 0))
    org, drs, _ = IC.chain_rays("room", 5, 0)
    assert (IC.bits(R.Inscatter_Points(org, drs)) == 0).all()
    out = R.Inscatter_Rays(org, drs, 3.0, 0.1)
    assert (IC.bits(out["rgb"]) == 0).all() and (out["steps"] == IC.steps_of(0.1, 3.0)).all() and (out["len"] == 3.0).all()
    R.Destroy()


def test_the_ray_queries_clock_times_these_kernels(hip):
    R = IC.room(hip)
    R.Set_Option(B.OPT_TIMING, 1)
    assert R.Ray_Query_Time() == 0.0
    org, drs, _ = IC.chain_rays("room", 5, 0)
    R.Inscatter_Points(org, drs)
    t_points = R.Ray_Query_Time()
    R.Inscatter_Rays(org, drs, 6.45, 0.1)
    t_rays = R.Ray_Query_Time()
    print("kernel times: points %.4f ms, rays %.4f ms" % (t_points, t_rays))
    assert t_points > 0.0 and t_rays > 0.0
    R.Destroy()


# ------------------------------------------------------------------------------------ f. nothing is edited, edits are seen
def test_pending_edits_are_seen_and_nothing_is_edited(hip):
    org, drs, counts = IC.chain_rays("room", 5, 2)
    tmax = np.array([IC.tmax_for(0.1, c) for c in counts], np.float32)
    outs = []
    for queries in (True, False):
        R = IC.room(hip, IC.VOL_B)
        for f in range(3):
            R.Render()  # (not waited for)
            if queries:
                (lambda: R.Inscatter_Points(org, drs), lambda: R.Inscatter_Rays(org, drs, tmax, 0.1), lambda: R.Inscatter_Rays(org, drs, tmax, 0.1, March=True))[f]()
        R.Finish()
        outs.append((R.Read_Framebuffer(), R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats()))
        if queries:
            # a sphere moved in front of the light: the query that follows sees it, with frames in flight
            before = R.Inscatter_Rays(org, drs, tmax, 0.1)["rgb"]
            R.Render()
            R.Set_Primitive(spheres.Sphere, 1, spheres.Create((4.0, 2.6, 4.0), 1.5, 3))
            after = R.Inscatter_Rays(org, drs, tmax, 0.1)
            moved = IC.room(hip)
            moved.Set_Primitive(spheres.Sphere, 1, spheres.Create((4.0, 2.6, 4.0), 1.5, 3))
            assert (IC.bits(after["rgb"]) != IC.bits(before)).any(), "the move does not matter to these rays"
            IC.assert_bits(after["rgb"], moved.Inscatter_Rays(org, drs, tmax, 0.1)["rgb"], "after Set_Primitive")
            moved.Destroy()
        R.Destroy()
    (fb_q, rad_q, settle_q, scr_q), (fb, rad, settle, scr) = outs
    assert np.array_equal(IC.bits(fb_q), IC.bits(fb))
    assert rad_q == rad and settle_q == settle and scr_q == scr


# ------------------------------------------------------------------------------------ the _device forms, in a child process
@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("inscatter") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "inscatter_device_checks.py"), out]
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
