"""MDH_OPT_SCREEN_REPLAY: while camera and geometry stand still the screen pass takes every pixel's primary hit, reflection
hit, arg-min primitives, first steps, cage visibility and occlusion term from a 32-byte record per pixel instead of marching
them again.  The records hold what the marches computed, bit for bit, and feed the same operations: a renderer that replays
(A, option 1) and one that marches every pass (B, option 0) must agree on framebuffer, geometry buffer, both atlases and the
window's pixels in every bit after every frame.  mdh_screen_replay_stats shows which kernel ran: a test that expects a
replaying pass and finds none fails."""
import math

import numpy as np
import pytest

import custom_kinds as ck
from bvh_scenes import fan, tri_renderer
from helpers import SMALL_PROBES, SMALL_VOL, make
from madarch_amd import _binding as B
from madarch_amd import examples, materials, renderers, scenes, windows
from madarch_amd.lights import point_lights, spot_lights
from madarch_amd.primitives import planes, spheres
from test_gpu_full_size import tile_mask

pytestmark = pytest.mark.gpu

W, H = 44, 28  # partial tiles on both edges; 24 tiles: MDH_OPT_SCREEN_SPLIT hands each to four wavefronts
GI = examples.GI_8X8X8_PROBES  # power-of-two atlases; None: the reference's default 6 x 6 probes, nothing a power of two
PROBE_CONFIGS = [pytest.param(GI, id="8x8x8"), pytest.param(None, id="default")]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def frame(R, window=False):
    """One frame and everything the comparison is about."""
    R.Render()
    out = [R.Read_Framebuffer(), R.Read_Texture(B.TEX_RADIANCE), R.Read_Texture(B.TEX_IRRADIANCE)]
    if R.Get_Option(B.OPT_GBUFFER):
        out += list(R.Read_Gbuffer())
    if window:
        R.Swap_Buffers()
        out.append(R.Front_Buffer())
    return out


def assert_same_frame(a, b, what):
    assert len(a) == len(b)
    for n, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(bits(x), bits(y)), "%s: output %d differs in %d words" % (what, n, int((bits(x) != bits(y)).sum()))


def gi(hip, replay, w=W, h=H, scene="global_illumination", probes=GI, **options):
    R = make(scene, w, h, hip, probes=probes)
    assert R.Get_Option(B.OPT_SCREEN_REPLAY) == 0  # the default
    R.Set_Option(B.OPT_SCREEN_REPLAY, replay)
    for name, value in options.items():
        R.Set_Option(getattr(B, name), value)
    return R


def light(f):
    return spot_lights.Create((3.5 + 0.2 * f, 5.0, 2.0 + 0.1 * f), (-1.0, 0.0, 0.0), math.pi / 4.0, (0.9, 0.9 - 0.05 * f, 0.8))


def move_light(f):
    return lambda R: R.Set_Light(1, spot_lights.Spot_Light, light(f))


def kind(R, before):
    d = [n - o for n, o in zip(R.Screen_Replay_Stats(), before)]
    assert sum(d) == 1 and min(d) == 0, d
    return "pcr"[d.index(1)]


def run_pair(A, Bm, steps, window=False):
    """`steps`: callables (or None) applied to both renderers before each frame.  Returns A's pass kinds, one letter per frame."""
    seq = ""
    for f, edit in enumerate(steps):
        if edit:
            edit(A)
            edit(Bm)
        sa = A.Screen_Replay_Stats()
        fa, fb = frame(A, window), frame(Bm, window)
        assert_same_frame(fa, fb, "frame %d" % f)
        seq += kind(A, sa)
    return seq


@pytest.mark.parametrize("probes", PROBE_CONFIGS)
def test_standing_scene_moving_light(hip, probes):
    A, Bm = gi(hip, 1, probes=probes), gi(hip, 0, probes=probes)
    seq = run_pair(A, Bm, [move_light(f) for f in range(6)])
    assert seq == "pcrrrr", seq
    assert A.Screen_Replay_Stats() == (1, 1, 4)
    assert Bm.Screen_Replay_Stats() == (6, 0, 0)


ROT = [[math.cos(0.3), 0.0, math.sin(0.3)], [0.0, 1.0, 0.0], [-math.sin(0.3), 0.0, math.cos(0.3)]]
ENDS = {
    "camera_position": lambda R: R.Set_Camera_Position((2.3, 2.1, 0.2)),
    "camera_orientation": lambda R: R.Set_Camera_Orientation(ROT),
    "set_primitive": lambda R: R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.5, 3.0, 3.0), 0.9, 4)),
    "add_primitive": lambda R: R.Add_Primitive(spheres.Sphere, spheres.Create((1.5, 1.0, 4.5), 0.6, 1)),
}


@pytest.mark.parametrize("edit", sorted(ENDS))
def test_edit_ends_replay(hip, edit):
    A, Bm = gi(hip, 1), gi(hip, 0)
    seq = run_pair(A, Bm, [None, None, None, ENDS[edit], None, None])
    assert seq == "pcr" + "pcr", seq


def _write_atlas(R):
    t = R.Read_Texture(B.TEX_IRRADIANCE)
    R.Write_Texture(B.TEX_IRRADIANCE, t * 0.5)


KEEPS = {
    "camera_position_same": lambda R: R.Set_Camera_Position((2.0, 2.0, 0.0)),
    "camera_orientation_same": lambda R: R.Set_Camera_Orientation([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),
    "set_light": move_light(3),
    "set_material": lambda R: R.Set_Material(3, materials.Create((0.7, 0.2, 0.1), 0.5, 0.2)),  # (the sphere's: below the reflection's threshold before and after)
    "add_material": lambda R: R.Add_Material(materials.Create((0.3, 0.3, 0.3), 0.1, 0.9)),
    "write_texture": _write_atlas,
}


@pytest.mark.parametrize("edit", sorted(KEEPS))
def test_edit_keeps_replay(hip, edit):
    A, Bm = gi(hip, 1), gi(hip, 0)
    seq = run_pair(A, Bm, [None, None, None, KEEPS[edit], None])
    assert seq == "pcrrr", seq


def test_material_across_reflection_threshold(hip):
    """A reflection ray is traced where the material's roughness is below 0.75.  The sphere's material turning rough switches
    its reflections off in the replaying kernel as in the marching one (the records stay); turning smooth again needs the
    rays of a reflection that the records -- written while it was rough, in the second run -- do not hold: the replay ends."""
    rough = lambda R: R.Set_Material(3, materials.Create((0.1, 0.1, 0.1), 0.9, 0.9))
    smooth = lambda R: R.Set_Material(3, materials.Create((0.1, 0.1, 0.1), 0.9, 0.1))
    A, Bm = gi(hip, 1), gi(hip, 0)
    assert run_pair(A, Bm, [None, None, None, rough, None, smooth, None, None]) == "pcr" + "rr" + "pcr"
    A, Bm = gi(hip, 1), gi(hip, 0)
    assert run_pair(A, Bm, [rough, None, None, smooth, None, None]) == "pcr" + "pcr"


@pytest.mark.parametrize("overlap", [1, 2])
def test_schedules(hip, overlap):
    """MDH_OPT_FRAME_OVERLAP 1 (screen passes on the main stream, probe passes beside them) and 2 (screen passes alternating
    between two streams) against 0, replay on in all; and 0 against the serial run that marches."""
    def drive(overlap, replay=1):
        R = gi(hip, replay, OPT_FRAME_OVERLAP=overlap)
        seen = []
        for f in range(8):
            if f == 3:
                R.Set_Light(1, spot_lights.Spot_Light, light(2))
            if f == 5:
                R.Set_Camera_Position((2.3, 2.1, 0.2))
            seen.append(frame(R))
        return seen, R.Screen_Replay_Stats()
    (serial, stats_s), (piped, stats_p) = drive(0), drive(overlap)
    for f, (a, b) in enumerate(zip(serial, piped)):
        assert_same_frame(a, b, "frame %d" % f)
    assert stats_s == stats_p == (2, 2, 4)
    marched, stats_m = drive(0, replay=0)
    for f, (a, b) in enumerate(zip(serial, marched)):
        assert_same_frame(a, b, "frame %d against replay 0" % f)
    assert stats_m == (8, 0, 0)


@pytest.mark.parametrize("split", [0, 2560])
def test_split_tiles(hip, split):
    A, Bm = gi(hip, 1, OPT_SCREEN_SPLIT=split), gi(hip, 0, OPT_SCREEN_SPLIT=0)
    assert run_pair(A, Bm, [move_light(f) for f in range(4)]) == "pcrr"


def test_whole_tiles(hip):
    A, Bm = gi(hip, 1, 96, 64), gi(hip, 0, 96, 64)
    assert run_pair(A, Bm, [move_light(f) for f in range(4)]) == "pcrr"


@pytest.mark.parametrize("order", [0, 1])
def test_tile_order_resorted_between_recording_and_replaying(hip, order):
    """512 x 256: 2 048 tiles, the smallest frame that runs a tile order.  Frame 0 is followed by the first sort.  The camera
    moves before frame 6: frame 6 marches, frame 7 records, frame 8 replays and -- the eighth pass since the sort, the camera
    having moved -- leaves the durations that the tiles are sorted by again, so frame 9 replays at other launch places than
    frame 7 recorded at."""
    A, Bm = gi(hip, 1, 512, 256, OPT_SCREEN_ORDER=order), gi(hip, 0, 512, 256, OPT_SCREEN_ORDER=order)
    steps = [None] * 10
    steps[6] = ENDS["camera_position"]
    assert run_pair(A, Bm, steps) == "pcrrrr" + "pcrr"


def test_rank_slice(hip):
    def rank(replay):
        return gi(hip, replay, OPT_WORLD=3, OPT_RANK=1)
    A, Bm, whole = rank(1), rank(0), gi(hip, 0)
    assert run_pair(A, Bm, [move_light(f) for f in range(4)]) == "pcrr"
    whole.Render()
    mine = tile_mask(W, H, 3, 1)
    for a, b in zip(A.Read_Gbuffer(), whole.Read_Gbuffer()):  # (what the records hold of the primary ray, against the whole frame's)
        assert np.array_equal(bits(a)[mine], bits(b)[mine])
    assert not A.Read_Framebuffer()[~mine].any()


@pytest.mark.parametrize("options", [dict(OPT_GBUFFER=0), dict(OPT_GBUFFER=1), dict(OPT_ATLAS_FORMAT=0), dict(OPT_ATLAS_FORMAT=1)],
                         ids=["gbuffer0", "gbuffer1", "atlas0", "atlas1"])
def test_outputs(hip, options):
    A, Bm = gi(hip, 1, **options), gi(hip, 0, **options)
    assert run_pair(A, Bm, [move_light(f) for f in range(4)]) == "pcrr"


@pytest.mark.parametrize("window", [0, 1])
def test_window_pixels(hip, window):
    A, Bm = gi(hip, 1, OPT_WINDOW=window), gi(hip, 0, OPT_WINDOW=window)
    assert run_pair(A, Bm, [move_light(f) for f in range(4)], window=True) == "pcrr"


def test_light_shafts_volumetric_epilogue(hip):
    def scene(replay):
        return gi(hip, replay, scene="light_shafts")  # (helpers.make: the default volumetrics at a reduced froxel size)
    A, Bm = scene(1), scene(0)
    assert A.Volumetrics.Enabled
    steps = [lambda R, f=f: R.Set_Light(1, point_lights.Point_Light, point_lights.Create((3.0 + 0.3 * f, 5.0, 2.0), (0.8, 0.8, 0.7))) for f in range(4)]
    assert run_pair(A, Bm, steps) == "pcrr"


def _custom_scene(hip):
    scene = scenes.Compile([(planes.Plane, 8), (ck.My_Sphere, 2)], [(point_lights.Point_Light, 2)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(W, H), scene, Probes=GI, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    m = R.Add_Material(materials.Create((0.8, 0.2, 0.1), 0.0, 0.4))
    for n, o in examples._ROOM_PLANES:
        R.Add_Primitive(planes.Plane, planes.Create(n, o, m))
    R.Add_Primitive(ck.My_Sphere, ck.sphere((3.0, 3.0, 3.0), 1.0, m))
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create((4.0, 5.0, 2.0), (0.9, 0.9, 0.9)))
    R.Set_Camera_Position((2.0, 2.0, 0.0))
    R.Set_Option(B.OPT_GBUFFER, 1)
    return R


MARCHING = {
    "partition": lambda hip: make("simple_scene", W, H, hip, probes=GI),
    "mode2": lambda hip: make("global_illumination", W, H, hip, mode=2, probes=GI),
    "specular1": lambda hip: gi(hip, 0, OPT_INDIRECT_SPECULAR=1),
    "specular3": lambda hip: gi(hip, 0, OPT_INDIRECT_SPECULAR=3),
    "custom_kind": _custom_scene,
    "triangle_bvh": lambda hip: tri_renderer(hip, fan(12), True, W=W, H=H),
}


@pytest.mark.parametrize("variant", sorted(MARCHING))
def test_variants_that_keep_marching(hip, variant):
    A, Bm = MARCHING[variant](hip), MARCHING[variant](hip)
    A.Set_Option(B.OPT_SCREEN_REPLAY, 1)
    if A.Get_Option(B.OPT_SCREEN_MODE) == 0:
        assert run_pair(A, Bm, [None] * 4) == "pppp"
    else:  # (no atlases to read in mode 2)
        for f in range(4):
            A.Render(); Bm.Render()
            assert np.array_equal(bits(A.Read_Framebuffer()), bits(Bm.Read_Framebuffer()))
            for a, b in zip(A.Read_Gbuffer(), Bm.Read_Gbuffer()):
                assert np.array_equal(bits(a), bits(b))
    assert A.Screen_Replay_Stats() == (4, 0, 0)


@pytest.mark.parametrize("overlap", [1, 2])
def test_frames_in_flight_before_the_first_read(hip, overlap):
    """Nothing is read back, so nothing waits on the host, until every frame is enqueued: a plain pass, the recording pass,
    replaying passes, a camera move, a plain pass, a recording pass that must not overwrite records a replaying pass on the
    other screen stream still reads, and replaying passes that must not read before that recording pass has written.
    1024 x 512 so that a pass is long enough for the next frame's to start beside it.  The last frame against a renderer
    that marches, and the same run read back frame by frame."""
    def drive(replay, read_every_frame):
        R = gi(hip, replay, 1024, 512, OPT_FRAME_OVERLAP=overlap)
        for f in range(9):
            if f == 4:
                R.Set_Camera_Position((2.3, 2.1, 0.2))
            R.Set_Light(1, spot_lights.Spot_Light, light(f))
            R.Render()
            if read_every_frame:
                R.Read_Framebuffer()
        out = [R.Read_Framebuffer(), R.Read_Texture(B.TEX_RADIANCE), R.Read_Texture(B.TEX_IRRADIANCE)] + list(R.Read_Gbuffer())
        return out, R.Screen_Replay_Stats()
    (flight, stats_f), (stepped, stats_s), (marched, stats_m) = drive(1, False), drive(1, True), drive(0, False)
    assert stats_f == stats_s == (2, 2, 5) and stats_m == (9, 0, 0)
    assert_same_frame(flight, marched, "in flight against marching")
    assert_same_frame(flight, stepped, "in flight against read back every frame")


def test_option_flip(hip):
    A, Bm = gi(hip, 1), gi(hip, 0)
    off = lambda R: R is A and R.Set_Option(B.OPT_SCREEN_REPLAY, 0)
    on = lambda R: R is A and R.Set_Option(B.OPT_SCREEN_REPLAY, 1)
    ra = A.Radiance_Replay_Stats()
    seq = run_pair(A, Bm, [None, None, None, off, None, on, None, None])
    assert seq == "pcr" + "pp" + "pcr", seq  # on again: nothing is known of the pass before, so a plain pass, then a recording one
    assert tuple(n - o for n, o in zip(A.Radiance_Replay_Stats(), ra)) == (1, 1, 6)  # the radiance replay runs on, untouched
    assert Bm.Screen_Replay_Stats() == (8, 0, 0)


def test_miss_heavy_view(hip):
    """The room's far wall moved out of reach: the rays through the middle of the frame run past max_dist and miss, the ones
    towards floor, ceiling and side walls hit.  A miss's record holds a miss and replays as one."""
    def scene(replay):
        R = gi(hip, replay)
        R.Set_Primitive(planes.Plane, 6, planes.Create((0.0, 0.0, -1.0), 100.0, 0))
        return R
    A, Bm = scene(1), scene(0)
    assert run_pair(A, Bm, [move_light(f) for f in range(4)]) == "pcrr"
    index = A.Read_Gbuffer()[0]
    assert (index < 0).any() and (index >= 0).any(), "the view should hold misses and hits"
