"""The adaptive path-traced frame on the device, bit for bit.  Its sums, counts, moments, active count and total after every round
against the chain of public queries (tests/path_adaptive_cases.py: Path_Trace over Path_Frame_Rays per sample, the update and the
rule in numpy float32), the anchor to the plain frame, exact zero variance under the sky, the compaction that enters no bit, the
resolve by each pixel's own count, and the contract: refusals before a launch, the captured camera, frames that go on unchanged.
The device-array forms run in a child process with torch (tests/path_adaptive_device_checks.py).  Frames are 20 x 12 -- both
kinds of cut tile, 384 slots: the count runs in two workgroups -- and one of 264 x 256, whose 264 workgroup totals take the
scan across its chunk of 256."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import path_adaptive_cases as PA
import path_adaptive_device_checks as checks
import path_frame_cases as PF
import path_trace_cases as PT
import ray_query_cases as rq
import ref64_cases
import shade_rays_cases as S
from madarch_amd import _binding as B
from test_gpu_path_trace import COMPOSED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = PF.W, PF.H
SEED = PA.SEED
RULE = dict(Min_Samples=PA.MIN_SAMPLES, Max_Samples=PA.MAX_SAMPLES, Floor=PA.FLOOR)


def same(a, b):
    return np.array_equal(S.bits(a), S.bits(b))


def _status(call):
    try:
        call()
    except B.MadarchError as e:
        return e.status
    return B.MDH_OK


def states_equal(a, b):
    return not PA.differences(a, b)


# ------------------------------------------------------------------------------------ 1. the chain
@pytest.mark.parametrize("jitter", [True, False])
@pytest.mark.parametrize("name", COMPOSED + ("partition, Clamp, global residency",))
def test_every_round_equals_the_chain_of_public_queries(hip, name, jitter):
    R = S.FRAME_SCENES[name](hip)
    if name.endswith("global residency"):
        assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == 1
    tolerance = PA.TOLERANCE[name]
    chain = PA.Chain(PA.radiances(R, W, H, SEED, 3, jitter, PA.MAX_SAMPLES), PA.MIN_SAMPLES, PA.MAX_SAMPLES, tolerance, PA.FLOOR)
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=3, Jitter=jitter, Tolerance=tolerance, **RULE)
    taken = 0
    for at, k in enumerate(PA.ROUNDS):
        R.Path_Frame_Accumulate(k)
        chain.round(k)
        taken = min(taken + k, PA.MAX_SAMPLES)
        got, want = PA.device_state(R), chain.state()
        print("%s, jitter %d, round %d: %d active, %d samples" % (name, jitter, at, got["active"], got["total_samples"]))
        assert states_equal(got, want), "round %d: %s" % (at, "; ".join(PA.differences(got, want)))
        assert R.Path_Frame_Info()["samples"] == taken
    count = chain.state()["count"]
    early, full = int((count < PA.MAX_SAMPLES).sum()), int((count == PA.MAX_SAMPLES).sum())
    print("%d pixels retired early, %d reached %d samples" % (early, full, PA.MAX_SAMPLES))
    assert early > 0 and full > 0, "path_adaptive_cases.TOLERANCE[%r] = %g is degenerate: %d pixels retired early, %d reached the maximum" % (name, tolerance, early, full)
    R.Destroy()


# ------------------------------------------------------------------------------------ 2. the anchor to the plain frame
@pytest.mark.parametrize("name", ["rooms", "open scene"])
def test_min_equal_to_max_is_the_plain_frame(hip, name):
    R = S.FRAME_SCENES[name](hip)
    samples = 3
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=2, Jitter=True)
    R.Path_Frame_Accumulate(samples)
    plain = R.Path_Frame_Read(Tone_Map=True, Rgb=True, Rgba8=True, Sums=True)
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=2, Jitter=True, Min_Samples=samples, Max_Samples=samples, Tolerance=0.05, Floor=0.01)
    R.Path_Frame_Accumulate(samples)
    got = R.Path_Frame_Read(Tone_Map=True, Rgb=True, Rgba8=True, Sums=True)
    assert np.isfinite(plain["sums"]).all() and (plain["sums"] != 0).any()
    assert same(got["sums"], plain["sums"]) and same(got["rgb"], plain["rgb"]) and np.array_equal(got["rgba8"], plain["rgba8"]) and got["samples"] == samples
    stats = R.Path_Frame_Stats()
    assert (stats["count"] == samples).all() and stats["active"] == 0 and stats["total_samples"] == samples * W * H
    R.Path_Frame_Accumulate(2)  # (nobody is active: nothing moves)
    assert same(R.Path_Frame_Read(Rgb=False, Sums=True)["sums"], plain["sums"]) and R.Path_Frame_Info()["samples"] == samples
    R.Destroy()


# ------------------------------------------------------------------------------------ 3. zero variance
def test_pixels_of_the_sky_retire_at_min_samples(hip):
    """the floor under the sky of tests/test_gpu_path_trace.py without jitter: a pixel whose primary ray misses sees the same
    sky in every sample, y + y and y y + y y are exact, so its variance is exactly 0 and tolerance 0 retires it at min_samples"""
    R = ref64_cases.make_renderer(PT.plane_desc(), 16, 16, hip)
    org, drs = R.Camera_Rays(W, H)
    miss = R.Raycast(org, drs)["hit"] == 0
    assert miss.any() and (~miss).any()
    chain = PA.Chain(PA.radiances(R, W, H, SEED, 1, False, 6), 2, 6, 0.0, 0.0)
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=1, Jitter=False, Min_Samples=2, Max_Samples=6, Tolerance=0.0, Floor=0.0)
    for k in (2, 1, 3, 2):
        R.Path_Frame_Accumulate(k)
        chain.round(k)
        got, want = PA.device_state(R), chain.state()
        assert states_equal(got, want), "; ".join(PA.differences(got, want))
    count = got["count"]
    print("%d pixels miss; counts of the others: %s" % (int(miss.sum()), np.bincount(count[~miss], minlength=7)))
    assert (count[miss] == 2).all()
    assert (count[~miss] >= 2).all() and (count[~miss] <= 6).all() and (count[~miss] > 2).any()
    R.Destroy()


# ------------------------------------------------------------------------------------ 4. the mapping enters no bit
def rounds_of(R, width, height, bounces, rounds, compact, tolerance, max_samples):
    R.Set_Option(B.OPT_PATH_FRAME_COMPACT, compact)
    assert R.Get_Option(B.OPT_PATH_FRAME_COMPACT) == compact
    R.Path_Frame_Begin_Adaptive(width, height, Seed=SEED, Bounces=bounces, Jitter=True, Min_Samples=2, Max_Samples=max_samples, Tolerance=tolerance, Floor=PA.FLOOR)
    states = []
    for k in rounds:
        R.Path_Frame_Accumulate(k)
        states.append(PA.device_state(R))
    return states


def test_compaction_enters_no_bit(hip):
    R = rq.gi_room(hip)
    assert R.Get_Option(B.OPT_PATH_FRAME_COMPACT) == 0  # the default: the value that won in front of the mesh
    on = rounds_of(R, W, H, 3, PA.ROUNDS, 1, PA.TOLERANCE["rooms"], PA.MAX_SAMPLES)
    off = rounds_of(R, W, H, 3, PA.ROUNDS, 0, PA.TOLERANCE["rooms"], PA.MAX_SAMPLES)
    for at, (a, b) in enumerate(zip(on, off)):
        assert states_equal(a, b), "round %d: %s" % (at, "; ".join(PA.differences(a, b)))
    assert 0 < on[1]["active"] < W * H  # (some lanes did idle without it)
    R.Destroy()


def test_the_large_frame_with_and_without_compaction_and_the_chain(hip):
    """264 x 256: 264 workgroup totals, the scan's second chunk; one bounce, three rounds of 2"""
    w, h = PA.LARGE_W, PA.LARGE_H
    assert (w // 8) * (h // 8) * 64 == 67584 and 67584 // 256 == 264
    R = rq.gi_room(hip)
    tolerance = PA.LARGE_TOLERANCE
    chain = PA.Chain(PA.radiances(R, w, h, SEED, 1, True, PA.LARGE_MAX), 2, PA.LARGE_MAX, tolerance, PA.FLOOR)
    on = rounds_of(R, w, h, 1, PA.LARGE_ROUNDS, 1, tolerance, PA.LARGE_MAX)
    off = rounds_of(R, w, h, 1, PA.LARGE_ROUNDS, 0, tolerance, PA.LARGE_MAX)
    for at, k in enumerate(PA.LARGE_ROUNDS):
        chain.round(k)
        want = chain.state()
        print("round %d: %d of %d pixels active, %d samples" % (at, want["active"], w * h, want["total_samples"]))
        assert states_equal(on[at], want), "round %d, compacted: %s" % (at, "; ".join(PA.differences(on[at], want)))
        assert states_equal(off[at], want), "round %d, in place: %s" % (at, "; ".join(PA.differences(off[at], want)))
    # pixels active behind the 256th workgroup and before it: the carry of the scan's first chunk is in their places
    running = PA.active(on[0]["count"], on[0]["m1"], on[0]["m2"], 2, PA.LARGE_MAX, tolerance, PA.FLOOR).reshape(h, w)
    assert running[:h // 2].any() and running[248:, 8:].any() and not running.all()  # (rows 248 .., columns 8 ..: tiles 1 024 .. 1 055, workgroups 256 .. 263)
    R.Destroy()


# ------------------------------------------------------------------------------------ 5. the resolve
def test_the_resolve_divides_by_the_pixels_own_count(hip):
    R = S.FRAME_SCENES["open scene"](hip)
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=3, Jitter=True, Tolerance=PA.TOLERANCE["open scene"], **RULE)
    for k in PA.ROUNDS:
        R.Path_Frame_Accumulate(k)
    st = PA.device_state(R)
    assert len(np.unique(st["count"])) > 1 and (st["count"] >= PA.MIN_SAMPLES).all()
    want = (st["sums"] / st["count"].astype(np.float32)[:, None]).astype(np.float32)
    got = R.Path_Frame_Read(Tone_Map=False, Rgb=True, Sums=True)
    assert got["samples"] == PA.MAX_SAMPLES and same(got["sums"].reshape(-1, 3), st["sums"])
    assert same(got["rgb"].reshape(-1, 3), want)
    assert not same(got["rgb"].reshape(-1, 3), (st["sums"] / np.float32(PA.MAX_SAMPLES)).astype(np.float32))  # (not the frame's count)
    R.Destroy()


@pytest.mark.parametrize("name", ["rooms", "open scene"])
def test_the_resolve_is_the_pixel_program_and_the_windows_bytes(hip, name):
    """as tests/test_gpu_path_frame.py holds the plain frame's resolve: one sample without jitter and without bounces is the pixel
    program in mode 2, tone-mapped, and its bytes are the window's"""
    R = S.frame_renderer(hip, name, 2)
    R.Set_Option(B.OPT_AO_STEPS, 0)
    org, drs = R.Camera_Rays(W, H)
    want = R.Shade_Rays(org, drs, Mode=2, Tone_Map=True)["rgb"]
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=0, Jitter=False, Min_Samples=1, Max_Samples=1, Tolerance=0.0, Floor=0.0)
    R.Path_Frame_Accumulate(1)
    got = R.Path_Frame_Read(Tone_Map=True, Rgb=True, Rgba8=True, Sums=True)
    assert got["samples"] == 1 and got["rgba8"].shape == (H, W, 4) and got["rgba8"].dtype == np.uint8
    assert same(got["rgb"].reshape(-1, 3), want)
    R.Render()
    R.Swap_Buffers()
    assert np.array_equal(got["rgba8"], R.Front_Buffer())
    assert same(R.Path_Frame_Read(Tone_Map=False)["rgb"], got["sums"])  # (one sample: sum / 1)
    R.Destroy()


def test_a_camera_beyond_the_bound_gives_nan_pixels_that_retire(hip):
    R = rq.gi_room(hip)
    R.Set_Camera_Position((2000.0, 2.0, 0.0))
    for jitter in (False, True):
        R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=3, Jitter=jitter, Tolerance=0.1, **RULE)
        assert R.Path_Frame_Stats()["active"] == W * H  # (before the first round every pixel is below min_samples)
        R.Path_Frame_Accumulate(2)  # (returns: the lanes' own check, no march)
        st = PA.device_state(R)
        assert st["active"] == 0 and st["total_samples"] == 0 and (st["count"] == 0).all(), jitter
        for k in ("sums", "m1", "m2"):
            assert (st[k].view(np.uint32) == PT.BAD_BITS).all(), (jitter, k)
        R.Path_Frame_Accumulate(1)  # ... and stay so
        got = R.Path_Frame_Read(Tone_Map=True, Rgba8=True, Sums=True)
        assert (got["sums"].view(np.uint32) == PT.BAD_BITS).all() and np.isnan(got["rgb"]).all()
        assert (got["rgba8"].reshape(-1, 4) == np.array([0, 0, 0, 255], np.uint8)).all()
    R.Destroy()


# ------------------------------------------------------------------------------------ 6. device arrays
@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("path_adaptive") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "path_adaptive_device_checks.py"), out]
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


# ------------------------------------------------------------------------------------ 7. the contract
def test_refusals_launch_nothing(hip):
    R = rq.gi_room(hip)
    R.Set_Option(B.OPT_TIMING, 1)
    org, drs = rq.room_rays(65)
    R.Path_Trace(org, drs, Seed=SEED, Bounces=1)
    before = R.Ray_Query_Time()
    assert before > 0.0
    h = R._h
    count = np.full(W * H, -3, np.int32)
    mom = np.full((W * H, 2), -3.0, np.float32)
    words = (C.c_int64 * 2)(-5, -5)
    pc, pm = count.ctypes.data_as(C.c_void_p), mom.ctypes.data_as(C.c_void_p)
    pa, pt = C.c_void_p(C.addressof(words)), C.c_void_p(C.addressof(words) + 8)
    # no accumulator open
    assert hip.path_frame_stats(h, pc, pm, pa, pt) == B.MDH_E_STATE
    # begin: what the plain begin refuses, and the rule's parameters
    ok = (W, H, 1, 3, 1, 2, 8, 0.1, 0.01)
    for at, value in ((0, 0), (1, -1), (3, 7), (3, -1), (4, 2), (5, 0), (5, 9), (6, (1 << 24) + 1), (7, -0.5), (7, float("nan")), (7, float("inf")), (8, -1.0), (8, float("nan"))):
        args = list(ok)
        args[at] = value
        assert hip.path_frame_begin_adaptive(h, *args) == B.MDH_E_INVALID, args
    assert hip.path_frame_begin_adaptive(h, 8193, 8192, 1, 3, 1, 2, 8, 0.1, 0.01) == B.MDH_E_INVALID
    assert R.Path_Frame_Info()["width"] == 0  # (a refused begin opens nothing)
    R.Frame_Begin()
    assert hip.path_frame_begin_adaptive(h, *ok) == B.MDH_E_STATE
    R.Frame_End()
    R.Finish()
    # a plain frame has no statistics
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=3, Jitter=True)
    assert hip.path_frame_stats(h, pc, pm, pa, pt) == B.MDH_E_STATE
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=3, Jitter=True, Tolerance=0.1, **RULE)
    assert R.Path_Frame_Info() == {"width": W, "height": H, "samples": 0, "bounces": 3, "jitter": 1}
    buf = np.full((W * H, 3), -3.0, np.float32)
    n = C.c_int32(-5)
    assert hip.path_frame_read(h, 0, buf.ctypes.data_as(C.c_void_p), None, None, C.byref(n)) == B.MDH_E_STATE and n.value == -5  # no round has run
    assert hip.path_frame_accumulate(h, 0) == B.MDH_OK and hip.path_frame_accumulate(h, -1) == B.MDH_E_INVALID
    R.Frame_Begin()
    assert hip.path_frame_accumulate(h, 1) == B.MDH_E_STATE
    R.Frame_End()
    R.Finish()
    assert R.Ray_Query_Time() == before  # nothing was launched
    assert (count == -3).all() and (mom == -3.0).all() and (buf == -3.0).all() and list(words) == [-5, -5]
    # every output of the statistics is optional
    assert hip.path_frame_stats(h, None, None, None, None) == B.MDH_OK
    assert hip.path_frame_stats(h, None, None, pa, None) == B.MDH_OK and list(words) == [W * H, -5]
    assert hip.path_frame_stats(h, pc, None, None, pt) == B.MDH_OK and list(words) == [W * H, 0] and (count == 0).all() and (mom == -3.0).all()
    assert R.Ray_Query_Time() == before  # (the statistics take no timing pair)
    R.Path_Frame_Accumulate(2)
    R.Ray_Query_Wait()
    assert R.Ray_Query_Time() != before  # (the round is what is timed)
    first = PA.device_state(R)
    # a plain begin after an adaptive one gives today's plain frame, and an adaptive one after that starts from zero
    R.Path_Frame_Begin(W, H, Seed=SEED, Bounces=3, Jitter=True)
    R.Path_Frame_Accumulate(2)
    plain = R.Path_Frame_Read(Sums=True)
    Rref = rq.gi_room(hip)
    Rref.Path_Frame_Begin(W, H, Seed=SEED, Bounces=3, Jitter=True)
    Rref.Path_Frame_Accumulate(2)
    want = Rref.Path_Frame_Read(Sums=True)
    assert same(plain["sums"], want["sums"]) and same(plain["rgb"], want["rgb"]) and plain["samples"] == 2
    assert same(plain["sums"].reshape(-1, 3), first["sums"])  # (round one of 2 >= min_samples is the plain frame's two samples)
    assert _status(lambda: R.Path_Frame_Stats()) == B.MDH_E_STATE
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=3, Jitter=True, Tolerance=0.1, **RULE)
    R.Path_Frame_Accumulate(2)
    assert states_equal(PA.device_state(R), first)
    R.Path_Frame_End()
    assert hip.path_frame_stats(h, pc, pm, pa, pt) == B.MDH_E_STATE
    R.Destroy()
    Rref.Destroy()


def test_the_camera_is_captured_at_begin(hip):
    R, Rref = rq.gi_room(hip), rq.gi_room(hip)
    for r in (R, Rref):
        r.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=2, Jitter=True, Tolerance=0.1, **RULE)
        r.Path_Frame_Accumulate(2)
    R.Set_Camera_Position(PF.CAM_POS)
    R.Set_Camera_Orientation(PF.cam_rows().tolist())
    for r in (R, Rref):
        r.Path_Frame_Accumulate(3)
    assert states_equal(PA.device_state(R), PA.device_state(Rref))
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=2, Jitter=True, Tolerance=0.1, **RULE)
    R.Path_Frame_Accumulate(2)
    R.Path_Frame_Accumulate(3)
    assert not same(PA.device_state(R)["sums"], PA.device_state(Rref)["sums"])  # (the next begin takes the camera as it then stands)
    R.Destroy()
    Rref.Destroy()


def test_rounds_edit_nothing(hip):
    """four frames with rounds, statistics and reads between them, four frames without: every frame's pixels and the atlases are the
    same, and the radiance replay, the probe settle and the screen replay have counted the same passes of each kind"""
    outs = []
    for calls in (True, False):
        R = rq.gi_room(hip)
        R.Set_Option(B.OPT_SCREEN_REPLAY, 1)
        frames = []
        if calls:
            R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=2, Jitter=True, Tolerance=0.1, **RULE)
        for f in range(4):
            R.Render()
            if calls:
                R.Path_Frame_Accumulate(PA.ROUNDS[f])
                if f == 1:
                    R.Set_Option(B.OPT_PATH_FRAME_COMPACT, 1)  # (no pass reads it: it ends no settle run)
                    R.Path_Frame_Stats()
                if f % 2 == 1:
                    R.Path_Frame_Read(Tone_Map=True, Rgba8=True)
            frames.append(R.Read_Framebuffer())
        R.Finish()
        atlases = [R.Read_Texture(t) for t in (B.TEX_IRRADIANCE, B.TEX_RADIANCE)]
        state = PA.device_state(R) if calls else None
        outs.append((frames, atlases, R.Radiance_Replay_Stats(), R.Probe_Settle_Stats(), R.Screen_Replay_Stats(), state))
        R.Destroy()
    (fb_q, at_q, rad_q, settle_q, scr_q, state), (fb, at, rad, settle, scr, _) = outs
    print("radiance replay %s, probe settle %s, screen replay %s" % (rad, settle, scr))
    for f in range(4):
        assert same(fb_q[f], fb[f]), f
    assert same(at_q[0], at[0]) and same(at_q[1], at[1])
    assert rad_q == rad and settle_q == settle and scr_q == scr
    assert sum(rad) >= 1 and scr[1] + scr[2] > 0  # (the counters do count)
    # the accumulator kept its bits: the same rounds, compacted, in a renderer that did nothing else
    R = rq.gi_room(hip)
    R.Set_Option(B.OPT_PATH_FRAME_COMPACT, 1)
    R.Path_Frame_Begin_Adaptive(W, H, Seed=SEED, Bounces=2, Jitter=True, Tolerance=0.1, **RULE)
    for k in PA.ROUNDS:
        R.Path_Frame_Accumulate(k)
    assert states_equal(PA.device_state(R), state)
    R.Destroy()
