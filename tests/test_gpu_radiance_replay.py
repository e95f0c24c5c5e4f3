"""MDH_OPT_RADIANCE_REPLAY: while the scene's geometry stands still the radiance pass takes every probe ray's hit, arg-min
primitive, step count, first step and cage visibility from a per-ray record instead of marching them again.  The records
hold what the marches computed, bit for bit, and feed the same operations: a renderer that replays (A) and one that marches
every pass (B, option 0) must agree on the radiance atlas, the irradiance atlas and the framebuffer in every bit after every
frame -- under a moving light, across geometry edits, under both frame schedules, with and without the ray order, on a
rank's slice whose last wavefront is partly empty, and across flips of the option itself.  mdh_radiance_replay_stats shows
that the replaying kernel really ran: a test that finds no replaying pass fails."""
import math

import numpy as np
import pytest

from helpers import ODD_PROBES, make
from madarch_amd import _binding as B
from madarch_amd import examples, renderers
from madarch_amd.lights import point_lights, spot_lights
from madarch_amd.primitives import spheres

pytestmark = pytest.mark.gpu

W, H = 96, 64
# the ray order is active (32 x 16 probes of 32 x 32 texels: 524 288 rays); the default 4 x 3 x 3 probes run no order and
# give a small launch, padded to a group of 64 probes
PROBE_CONFIGS = [pytest.param(examples.GI_8X8X8_PROBES, id="8x8x8"), pytest.param(None, id="default")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def frame(R):
    """One frame and everything the comparison is about."""
    R.Render()
    return (R.Read_Texture(B.TEX_RADIANCE), R.Read_Texture(B.TEX_IRRADIANCE), R.Read_Framebuffer())


def assert_same_frame(a, b, what):
    for name, x, y in zip(("radiance", "irradiance", "framebuffer"), a, b):
        assert np.array_equal(bits(x), bits(y)), "%s: %s differs in %d words" % (what, name, int((bits(x) != bits(y)).sum()))


def gi(hip, probes, replay, **options):
    R = make("global_illumination", W, H, hip, probes=probes)
    assert R.Get_Option(B.OPT_RADIANCE_REPLAY) == 1  # the default
    R.Set_Option(B.OPT_RADIANCE_REPLAY, replay)
    for name, value in options.items():
        R.Set_Option(getattr(B, name), value)
    return R


def light(f):
    return spot_lights.Create((3.5 + 0.2 * f, 5.0, 2.0 + 0.1 * f), (-1.0, 0.0, 0.0), math.pi / 4.0, (0.9, 0.9 - 0.05 * f, 0.8))


def kinds(R, before):
    """'p', 'c' or 'r' for the one radiance pass since `before`: plain, recording, replaying."""
    now = R.Radiance_Replay_Stats()
    d = [n - o for n, o in zip(now, before)]
    assert sum(d) == 1 and min(d) == 0, d
    return "pcr"[d.index(1)]


def run_pair(A, Bm, steps):
    """`steps`: callables (or None) applied to both renderers before each frame.  Returns A's pass kinds, one letter per frame."""
    seq = ""
    for f, edit in enumerate(steps):
        if edit:
            edit(A)
            edit(Bm)
        sa = A.Radiance_Replay_Stats()
        fa, fb = frame(A), frame(Bm)
        assert_same_frame(fa, fb, "frame %d" % f)
        seq += kinds(A, sa)
    return seq


@pytest.mark.parametrize("probes", PROBE_CONFIGS)
def test_standing_scene_moving_light(hip, probes):
    A, Bm = gi(hip, probes, 1), gi(hip, probes, 0)
    seq = run_pair(A, Bm, [lambda R, f=f: R.Set_Light(1, spot_lights.Spot_Light, light(f)) for f in range(6)])
    assert seq == "pcrrrr", seq  # a recording pass, then replaying passes
    assert A.Radiance_Replay_Stats() == (1, 1, 4)
    assert Bm.Radiance_Replay_Stats() == (6, 0, 0)  # none of either


@pytest.mark.parametrize("edit", ["set_primitive", "add_primitive"])
@pytest.mark.parametrize("probes", PROBE_CONFIGS)
def test_edit_ends_replay(hip, probes, edit):
    def change(R):
        if edit == "set_primitive":  # the rooms' sphere, moved by a visible amount
            R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.5, 3.0, 3.0), 0.9, 4))
        else:
            R.Add_Primitive(spheres.Sphere, spheres.Create((1.5, 1.0, 4.5), 0.6, 1))
    A, Bm = gi(hip, probes, 1), gi(hip, probes, 0)
    seq = run_pair(A, Bm, [None, None, None, None, change, None, None, None])
    # the pass after the edit marches, then a new recording pass and replaying passes
    assert seq == "pcrr" + "pcrr", seq
    assert Bm.Radiance_Replay_Stats() == (8, 0, 0)


def test_update_partitioning_keeps_marching(hip):
    """simple_scene runs the space-partition kernels, which only march: equal bits, and
    every pass plain -- before and after Update_Partitioning, which would end a replay if there were one."""
    def scene(replay):
        R = make("simple_scene", W, H, hip)
        R.Set_Option(B.OPT_RADIANCE_REPLAY, replay)
        return R
    A, Bm = scene(1), scene(0)
    seq = run_pair(A, Bm, [None, None, None, lambda R: R.Update_Partitioning(renderers.GPU_Fast), None, None])
    assert seq == "pppppp", seq
    assert A.Radiance_Replay_Stats() == Bm.Radiance_Replay_Stats() == (6, 0, 0)


@pytest.mark.parametrize("probes", PROBE_CONFIGS)
def test_schedules(hip, probes):
    """Frames in flight against the serial schedule, replay on in both, one light edit and one primitive edit -- and both
    against the serial schedule that marches every pass."""
    def drive(overlap, replay=1):
        R = gi(hip, probes, replay, OPT_FRAME_OVERLAP=overlap)
        seen = []
        for f in range(8):
            if f == 3:
                R.Set_Light(1, spot_lights.Spot_Light, light(2))
            if f == 5:
                R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.5, 3.0, 3.0), 0.9, 4))
            seen.append(frame(R))
        return seen, R.Radiance_Replay_Stats()
    R0 = gi(hip, probes, 1)
    default = R0.Get_Option(B.OPT_FRAME_OVERLAP)
    assert default != 0
    (serial, stats_s), (piped, stats_p) = drive(0), drive(default)
    for f, (a, b) in enumerate(zip(serial, piped)):
        assert_same_frame(a, b, "frame %d" % f)
    assert stats_s == stats_p == (2, 2, 4)  # frames 0 and 5 march, 1 and 6 record, the others replay
    marched, stats_m = drive(0, replay=0)
    for f, (a, b) in enumerate(zip(serial, marched)):
        assert_same_frame(a, b, "frame %d against replay 0" % f)
    assert stats_m == (8, 0, 0)


def test_order_and_forced_resort(hip):
    """Replay with the rays in probe order and sorted, and across a resort forced in mid-sequence (setting the option drops
    the stored order: the replaying pass then writes the sort keys from the recorded and the marched step counts)."""
    probes = examples.GI_8X8X8_PROBES
    Bm = gi(hip, probes, 0)
    As = [gi(hip, probes, 1, OPT_RADIANCE_ORDER=0), gi(hip, probes, 1, OPT_RADIANCE_ORDER=1), gi(hip, probes, 1, OPT_RADIANCE_ORDER=1)]
    for f in range(6):
        if f == 4:
            As[2].Set_Option(B.OPT_RADIANCE_ORDER, 1)  # the order is dropped: this pass runs unsorted and sorts again
        for R in As + [Bm]:
            R.Set_Light(1, spot_lights.Spot_Light, light(f))
        want = frame(Bm)
        for i, R in enumerate(As):
            assert_same_frame(frame(R), want, "frame %d, renderer %d" % (f, i))
    for R in As:
        assert R.Radiance_Replay_Stats() == (1, 1, 4)


def test_odd_slice(hip):
    """A rank's slice of 25 probes of 12 x 12 texels: 3 600 rays, the last wavefront partly empty, nothing a power of two."""
    def rank(replay):
        R = make("global_illumination", W, H, hip, probes=ODD_PROBES)
        R.Set_Option(B.OPT_RADIANCE_REPLAY, replay)
        R.Set_Option(B.OPT_WORLD, 3)
        R.Set_Option(B.OPT_RANK, 1)
        return R
    A, Bm = rank(1), rank(0)
    assert A.Probe_Total() == 75
    seq = run_pair(A, Bm, [lambda R, f=f: R.Set_Light(1, spot_lights.Spot_Light, light(f)) for f in range(5)])
    assert seq == "pcrrr", seq


@pytest.mark.parametrize("probes", PROBE_CONFIGS)
def test_option_flip(hip, probes):
    A, Bm = gi(hip, probes, 1), gi(hip, probes, 0)
    off = lambda R: R is A and R.Set_Option(B.OPT_RADIANCE_REPLAY, 0)
    on = lambda R: R is A and R.Set_Option(B.OPT_RADIANCE_REPLAY, 1)
    seq = run_pair(A, Bm, [None, None, None, off, None, on, None, None])
    # off: the records are dropped and the passes march; on again over standing geometry: the first pass records
    assert seq == "pcr" + "pp" + "crr", seq
    assert Bm.Radiance_Replay_Stats() == (8, 0, 0)


def test_light_shafts_replays(hip):
    """The light_shafts workload (the rooms under a point light, volumetric passes beside the probe passes)."""
    def scene(replay):
        R = make("light_shafts", W, H, hip)
        R.Set_Option(B.OPT_RADIANCE_REPLAY, replay)
        return R
    A, Bm = scene(1), scene(0)
    seq = run_pair(A, Bm, [lambda R, f=f: R.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0 + 0.3 * f, 5.0, 2.0), (0.8, 0.8, 0.7)))
                           for f in range(4)])
    assert seq == "pcrr", seq
