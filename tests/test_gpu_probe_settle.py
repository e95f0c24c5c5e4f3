"""MDH_OPT_PROBE_SETTLE: once a frame's irradiance pass has stored the bits it was given for 16 passes in a row, under
inputs that still hold, frames leave their radiance and irradiance passes out.  Both passes are deterministic in what they
read, so nothing changes: a renderer with the option on (A) and one with it off (B) must agree on the framebuffer, the
geometry buffer and both atlases in every bit after every frame -- on a static scene under all three schedules, across
every kind of edit (after which the very next frame launches its passes again), under a moving camera (which keeps the
passes out), under a light set anew every frame (which never lets them out), with volumetrics, through the three-call
frame, with timing on, beside the screen replay, and under a one-rank communicator (which launches every pass).
mdh_probe_settle_stats shows that passes really were left out: a test that finds none fails."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import SMALL_PROBES, make
from madarch_amd import _binding as B
from madarch_amd import materials
from madarch_amd.lights import spot_lights
from madarch_amd.primitives import spheres

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 32
# global_illumination's default probes settle at pair 6, SMALL_PROBES at 7 (tests/test_probe_settle_oracle.py); the run
# has to be 16 long, and the host may see a pass up to 4 frames late: no frame up to 16 can leave its passes out, and one
# by 32 must
EARLIEST, LATEST = 16, 32


def state(R):
    """Everything the comparison is about, after the frame just rendered."""
    out = [R.Read_Framebuffer()] + list(R.Read_Gbuffer()) + [R.Read_Texture(B.TEX_RADIANCE), R.Read_Texture(B.TEX_IRRADIANCE)]
    if R.Volumetrics.Enabled:
        out += [R.Read_Texture(B.TEX_VISIBILITY), R.Read_Texture(B.TEX_SCATTERING)]
    return out


def assert_same(a, b, what):
    names = ("framebuffer", "gbuffer index", "gbuffer t", "gbuffer steps", "radiance", "irradiance", "visibility", "scattering")
    for name, x, y in zip(names, a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), \
            "%s: %s differs in %d bytes" % (what, name, int((x.view(np.uint8) != y.view(np.uint8)).sum()))


def pair(hip, scene="global_illumination", probes=None, **options):
    """A (the option on: the default) and B (off), otherwise alike."""
    out = []
    for settle in (1, 0):
        R = make(scene, W, H, hip, probes=probes)
        assert R.Get_Option(B.OPT_PROBE_SETTLE) == 1  # the default
        R.Set_Option(B.OPT_PROBE_SETTLE, settle)
        for name, value in options.items():
            R.Set_Option(getattr(B, name), value)
        out.append(R)
    return out


def frames(A, Bm, n, what, before=None, render=None):
    """n frames of both, compared after each; returns A's `skipped` after each frame."""
    seen = []
    for f in range(n):
        for R in (A, Bm):
            if before:
                before(R, f)
            (render or type(R).Render)(R)
        assert_same(state(A), state(Bm), "%s, frame %d" % (what, f + 1))
        seen.append(A.Probe_Settle_Stats()[1])
        assert Bm.Probe_Settle_Stats()[1] == 0
    return seen


def until_skipping(A, Bm, what):
    base = A.Probe_Settle_Stats()[1]
    seen = frames(A, Bm, LATEST, what)
    assert seen[EARLIEST - 1] == base and seen[-1] > base, (base, seen)
    return seen


def launched(R):
    return sum(R.Radiance_Replay_Stats())


def light(f):
    return spot_lights.Create((3.5 + 0.02 * f, 5.0, 2.0 + 0.01 * f), (-1.0, 0.0, 0.0), math.pi / 4.0, (0.9, 0.9, 0.8))


@pytest.mark.parametrize("overlap", [2, 1, 0])
def test_static_scene(hip, overlap):
    A, Bm = pair(hip, OPT_FRAME_OVERLAP=overlap)
    seen = frames(A, Bm, 40, "overlap %d" % overlap)
    assert all(s == 0 for s in seen[:EARLIEST]), seen
    assert seen[LATEST - 1] > 0, seen
    assert seen[-1] - seen[-2] == 2, seen  # both probe passes of a settled frame
    run, skipped, changed = A.Probe_Settle_Stats()
    assert run >= 16 and changed == 0
    assert launched(A) + skipped // 2 == 40 and launched(Bm) == 40
    A.Destroy(), Bm.Destroy()


def zero_irradiance(R):
    R.Write_Texture(B.TEX_IRRADIANCE, np.zeros(R.Texture_Shape(B.TEX_IRRADIANCE), dtype=np.float32))


EDITS = {
    "set_light": [lambda R: R.Set_Light(1, spot_lights.Spot_Light, light(25))],
    "set_material": [lambda R: R.Set_Material(1, materials.Create((0.2, 0.9, 0.1), 0.0, 0.6))],
    "set_primitive": [lambda R: R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.5, 3.0, 3.0), 0.9, 4))],
    "write_texture": [zero_irradiance],
    "atlas_format": [lambda R: R.Set_Option(B.OPT_ATLAS_FORMAT, 1)],
    "hysteresis": [lambda R: R.Set_Option(B.OPT_HYSTERESIS_PERMILLE, 500)],
    "frame_overlap": [lambda R: R.Set_Option(B.OPT_FRAME_OVERLAP, 0), lambda R: R.Set_Option(B.OPT_FRAME_OVERLAP, 2)],
    "render_pass": [lambda R: R.Render_Pass(B.PASS_RADIANCE)],
}


@pytest.mark.parametrize("edit", sorted(EDITS))
def test_edit_resumes_the_passes(hip, edit):
    A, Bm = pair(hip)
    assert A.Get_Option(B.OPT_FRAME_OVERLAP) == 2
    until_skipping(A, Bm, edit)
    for step, change in enumerate(EDITS[edit]):
        if step:  # (frame_overlap: the serial schedule settles by itself before the way back -- the atlases stand, 16 passes do it)
            base = A.Probe_Settle_Stats()[1]
            assert frames(A, Bm, LATEST, "%s, step %d" % (edit, step))[-1] > base
        change(A), change(Bm)
        assert A.Probe_Settle_Stats()[0] == 0  # the run is of inputs that no longer hold
        n_launched, n_skipped = launched(A), A.Probe_Settle_Stats()[1]
        frames(A, Bm, 1, "%s: the frame after the edit" % edit)
        assert launched(A) == n_launched + 1 and A.Probe_Settle_Stats()[1] == n_skipped  # the very next frame launches its passes
    frames(A, Bm, 40, "%s: after the edit" % edit)
    A.Destroy(), Bm.Destroy()


def test_moving_camera_keeps_the_passes_out(hip):
    A, Bm = pair(hip)
    seen = until_skipping(A, Bm, "camera")
    n_launched = launched(A)
    moved = frames(A, Bm, 10, "moving camera", before=lambda R, f: R.Set_Camera_Position((2.0 + 0.05 * f, 2.0, 0.02 * f)))
    assert moved[-1] == seen[-1] + 20 and launched(A) == n_launched
    A.Destroy(), Bm.Destroy()


def test_animated_light_never_settles(hip):
    A, Bm = pair(hip)
    seen = frames(A, Bm, 40, "animated light", before=lambda R, f: R.Set_Light(1, spot_lights.Spot_Light, light(f)))
    assert seen[-1] == 0 and launched(A) == 40
    # ... and neither does a light set to the value it has: comparing by value is not part of this
    seen = frames(A, Bm, 40, "light set to itself", before=lambda R, f: R.Set_Light(1, spot_lights.Spot_Light, light(39)))
    assert seen[-1] == 0 and launched(A) == 80
    A.Destroy(), Bm.Destroy()


def test_light_shafts(hip):
    A, Bm = pair(hip, scene="light_shafts", probes=SMALL_PROBES)
    assert A.Volumetrics.Enabled
    seen = frames(A, Bm, 40, "light_shafts")
    assert seen[EARLIEST - 1] == 0 and seen[-1] > 0, seen
    A.Destroy(), Bm.Destroy()


def test_three_call_frame(hip):
    def three_calls(R):
        R.Frame_Begin()
        R.Frame_Probe_Pass(B.PASS_RADIANCE)
        R.Frame_Probe_Pass(B.PASS_IRRADIANCE)
        R.Frame_End()
    A, Bm = pair(hip)
    C3 = make("global_illumination", W, H, hip)  # the option on, frames through Render
    for f in range(40):
        three_calls(A), Bm.Render(), C3.Render()
        sa = state(A)
        assert_same(sa, state(Bm), "three calls against the option off, frame %d" % (f + 1))
        assert_same(sa, state(C3), "three calls against Render, frame %d" % (f + 1))
        assert A.Probe_Settle_Stats()[1] == C3.Probe_Settle_Stats()[1]
    assert A.Probe_Settle_Stats()[1] > 0 and Bm.Probe_Settle_Stats()[1] == 0
    for R in (A, Bm, C3):
        R.Destroy()


def test_timing_counts_settled_passes(hip):
    A, Bm = pair(hip, OPT_TIMING=1)
    for f in range(60):
        A.Render(), Bm.Render()
        if f % 6 == 5:  # (the slots reach the host as frames finish; nothing here waits for one frame at a time)
            A.Finish()
    assert_same(state(A), state(Bm), "frame 60")
    assert A.Probe_Settle_Stats()[1] > 0
    for R in (A, Bm):
        for p in (B.PASS_RADIANCE, B.PASS_IRRADIANCE, B.PASS_SCREEN):
            ms, n = R.Pass_Time(p)
            assert n == 60 and ms >= 0.0, (p, ms, n)
    A.Destroy(), Bm.Destroy()


def test_beside_the_screen_replay(hip):
    A, Bm = pair(hip)
    A.Set_Option(B.OPT_SCREEN_REPLAY, 1)
    seen = frames(A, Bm, 40, "screen replay")
    assert seen[-1] > 0 and A.Screen_Replay_Stats()[2] > 0
    assert A.Probe_Settle_Stats()[0] >= 16  # (the screen replay's option is no edit of what a probe pass reads)
    A.Destroy(), Bm.Destroy()


COMM_SCRIPT = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
from helpers import make
from madarch_amd import _binding as B
import test_gpu_probe_settle as T
hip = B.hip_binding()
A, Bm = T.pair(hip)
for R in (A, Bm):
    R.Comm_Init(R.Comm_Unique_Id(), 0, 1)
seen = T.frames(A, Bm, 40, "one-rank communicator")
assert seen[-1] == 0 and T.launched(A) == 40, seen
for R in (A, Bm):
    R.Comm_Destroy()
# the communicator gone, the renderer is a single rank again: the count starts from nothing
seen = T.frames(A, Bm, 40, "after the communicator")
assert seen[T.EARLIEST - 1] == 0 and seen[-1] > 0, seen
for R in (A, Bm):
    R.Destroy()
print("SETTLE_COMM_OK")
""" % (ROOT, ROOT)


def test_one_rank_communicator_never_settles():
    out = subprocess.run([sys.executable, "-c", COMM_SCRIPT], capture_output=True, text=True, timeout=300)
    assert "SETTLE_COMM_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
