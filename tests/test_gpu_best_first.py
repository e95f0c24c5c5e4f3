"""MDH_BEST_FIRST (shade_structured, mdh_march.h): the reflection point's best cage probe is searched by decreasing
dot(probe_to_spec, -N) -- every lane sends its best untried candidate through the clearance test and the march, round by round,
and the first visible one is the probe the in-order loop names; a lane without a visible candidate in front takes the in-order
loop (the fallback).  No output may change in any bit: frames of the global_illumination scene are held against the oracle word
for word (image, geometry buffer, both atlases) under the cameras of tests/test_gpu_folded_twins.py and two that force the fallback:

    gap       low beside the box, along its face into the gap between box, floor and wall: reflection points on the floor and the
              box's foot whose front-facing cage probes all lie inside the box;
    low_wall  low at the x wall, looking along it and up: the same behind the box, seen over the floor.

scripts/best_first_estimate.py's model (float32, the kernel's operations) was run on all six at 64x64 before any GPU run --
(reflection points, fallback lanes, tiles with fallback lanes, lanes that win in round two or later):

    gap (4096, 399, 9, 70), low_wall (4096, 192, 8, 10), default (4096, 16, 5, 3), edge (4096, 96, 7, 0),
    corner (4096, 19, 2, 0), floor (4096, 1, 1, 0)

so both new cameras have fallback wavefronts, gap, low_wall and default have fast-path winners behind a blocked candidate, and
the other three have theirs in the first round only.  With the 8x8x8 probes (power-of-two addressing), the reference's default
probes and the tests' small grid; with and without the geometry buffer; at 64x64, 65x9 and 67x13 (full wavefronts, 8 lanes, 1
lane), at 256x256 split over two wavefronts per tile; marching, recording and replaying.  The statistics build renders the
64x64 frames in a child process and reports rounds, winners and fallbacks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_folded_twins as T
from madarch_amd import _binding as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BESTSTATS = os.path.join(ROOT, "madarch_amd", "csrc", "libmadarch_hip_beststats.so")
FALLBACK = {"gap": ((0.77, -0.69, 2.16), -0.44, 0.1), "low_wall": ((6.25, -0.69, 1.55), 1.67, 0.45)}
CAMERAS = dict(T.CAMERAS, **FALLBACK)


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("config", sorted(T.CONFIGS))
def test_frames_are_the_oracles(hip, orc, config, camera):
    cam = CAMERAS[camera]
    T.assert_frames(hip, T.oracle_frames(orc, config, cam, 64, 64), config, cam, 64, 64)


@pytest.mark.parametrize("w,h,split", T.SIZES, ids=["%dx%d%s" % (w, h, "" if s is None else "-split%d" % s) for w, h, s in T.SIZES])
@pytest.mark.parametrize("config", sorted(T.CONFIGS))
def test_partial_and_split_tiles_are_the_oracles(hip, orc, config, w, h, split):
    cam = FALLBACK["gap"]
    T.assert_frames(hip, T.oracle_frames(orc, config, cam, w, h), config, cam, w, h, split)


@pytest.mark.parametrize("camera", sorted(FALLBACK))
@pytest.mark.parametrize("config", sorted(T.CONFIGS))
def test_whole_wavefronts_are_the_oracles(hip, orc, config, camera):
    """64x64 as 64 wavefronts of 64 lanes (a window this small is otherwise split over four wavefronts per tile): the
    benchmark's schedule, where winners of several rounds and fallback lanes share a wavefront."""
    cam = FALLBACK[camera]
    T.assert_frames(hip, T.oracle_frames(orc, config, cam, 64, 64), config, cam, 64, 64, 0)


@pytest.mark.parametrize("gbuffer", [1, 0])
@pytest.mark.parametrize("camera", ["edge", "gap", "low_wall"])
@pytest.mark.parametrize("config", sorted(T.CONFIGS))
def test_recording_and_replaying_frames_are_the_marching_renderers(hip, orc, config, camera, gbuffer):
    """MDH_OPT_SCREEN_REPLAY 1 over four static frames -- plain, recording, replaying, replaying -- against a renderer that
    marches every pass.  The recording kernel writes a best-first winner's bits (1 for the winner and every untried corner, 0
    for a tried and blocked one), the replaying kernel walks them in index order: it must name the same probe."""
    cam = CAMERAS[camera]
    outs, kinds = [], []
    for replay in (1, 0):
        R = T.renderer(hip, config, cam, 64, 64)
        R.Set_Option(B.OPT_GBUFFER, gbuffer)
        R.Set_Option(B.OPT_SCREEN_REPLAY, replay)
        frames = []
        for f in range(4):
            R.Render()
            frames.append([R.Read_Framebuffer(), R.Read_Texture(B.TEX_RADIANCE), R.Read_Texture(B.TEX_IRRADIANCE)] + (list(R.Read_Gbuffer()) if gbuffer else []))
        outs.append(frames)
        kinds.append(R.Screen_Replay_Stats())
        R.Destroy()
    assert kinds[0] == (1, 1, 2) and kinds[1] == (4, 0, 0), kinds
    for f, (a, b) in enumerate(zip(*outs)):
        for n, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(T.bits(x), T.bits(y)), "frame %d, output %d: %d words differ" % (f, n, int((T.bits(x) != T.bits(y)).sum()))
    assert np.array_equal(T.bits(outs[1][1][0]), T.bits(T.oracle_frames(orc, config, cam, 64, 64)["image"]))


STATS_SCRIPT = r"""
import ctypes as C, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import test_gpu_best_first as T
from madarch_amd import _binding as B
hip = B.hip_binding()
assert hasattr(hip.lib, "mdh_diag_best_first"), "not the statistics build"
def take():
    out = (C.c_ulonglong * 4)()
    assert hip.lib.mdh_diag_best_first(out) == 0
    return list(out)
for name in sorted(T.CAMERAS):
    R = T.T.renderer(hip, "8x8x8", T.CAMERAS[name], 64, 64)
    R.Set_Option(B.OPT_GBUFFER, 0)  # (the kernel of the benchmark's frame)
    R.Set_Option(B.OPT_SCREEN_SPLIT, 0)  # (and its wavefronts: one per 8x8 tile, 64 of them)
    R.Render(); R.Render()
    take()
    R.Render_Pass(B.PASS_SCREEN)
    print("BEST", name, *take())
    R.Destroy()
print("BEST_FIRST_DONE")
""" % (ROOT, ROOT)


def test_rounds_winners_and_fallbacks():
    """[wave-rounds of the fast path, lanes that won there, wavefronts that entered the fallback, lanes in it] of one 64x64
    screen pass per camera, unsplit.  Conditions on the inputs, not tolerances: every camera has winners; the frame has 64
    wavefronts, each of which runs at most one first round, so more than 64 rounds are rounds beyond a first one; each fallback
    camera sends wavefronts into the fallback."""
    assert os.path.exists(BESTSTATS), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, MADARCH_HIP_LIBRARY=BESTSTATS)
    out = subprocess.run([sys.executable, "-c", STATS_SCRIPT], capture_output=True, text=True, timeout=300, env=env)
    print(out.stdout[-3000:])
    assert "BEST_FIRST_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    got = {}
    for line in out.stdout.splitlines():
        if line.startswith("BEST "):
            f = line.split()
            got[f[1]] = [int(x) for x in f[2:]]
    assert sorted(got) == sorted(CAMERAS)
    for name, (rounds, winners, fb_waves, fb_lanes) in got.items():
        assert winners > 0, (name, got[name])
        assert winners + fb_lanes == 64 * 64, (name, got[name])  # (a closed room: every pixel has a second point, and it wins or falls back)
        assert fb_lanes >= fb_waves, (name, got[name])
    assert any(v[0] > 64 for v in got.values()), got
    for name in FALLBACK:
        assert got[name][2] > 0, (name, got[name])
