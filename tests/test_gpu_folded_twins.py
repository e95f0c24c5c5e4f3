"""MDH_TWIN_FOLDED (shade_structured, mdh_march.h): in a wavefront that shares its irradiance taps, a corner folded along y or z
takes the weight and the visibility bit of the corner it folds onto instead of computing direction, distance and weight again.
No output may change in any bit: frames of the global_illumination scene are held against the oracle word for word
(image, geometry buffer, both atlases) under cameras that put 8x8 tiles on

    edge     close to the room's upper corner, straight at the z wall: tiles in one cell folded along z alone, along z and x, z and
             y (room edges) and all three (the corner), the same on the ceiling (a y wall) and the x wall beside it, and tiles
             across two cells along x and along y whose cells fold differently;
    floor    down at the floor (a y wall below the grid) and the box's faces below y = 0: one cell, two cells along x and along z,
             three and more cells (today's code);
    corner   at the sphere (one cell, 64 normals: never shares) with the x wall behind it across two cells along z;
    default  the example's own camera: the box, the sphere, every wall across four and more cells;

with the 8x8x8 probes (power-of-two addressing), the reference's default probes and the tests' small grid; with and without the
geometry buffer; at 64x64, 65x9 and 67x13 (full wavefronts, 8 lanes, 1 lane), at 256x256 split over two wavefronts per tile;
marching, recording and replaying.  The counters build renders the same frames in a child process: the work counters are the
parent commit's, and so is the count of sharing wavefronts: non-zero under every camera, zero where the one wavefront sees the
sphere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import SMALL_PROBES, assert_parity, make, snapshot
from madarch_amd import _binding as B
from madarch_amd import examples

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = os.path.join(ROOT, "madarch_amd", "csrc", "libmadarch_hip_counters.so")
CONFIGS = {"8x8x8": examples.GI_8X8X8_PROBES, "default": None, "small": SMALL_PROBES}


def rotation(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])).astype(np.float32)


# position, yaw, pitch
CAMERAS = {"edge": ((6.37, 6.37, 6.7), 0.0, 0.0), "floor": ((2.0, 2.0, 0.0), 0.0, 0.7), "corner": ((4.0, 4.0, 3.0), 0.6, -0.5), "default": ((2.0, 2.0, 0.0), 0.0, 0.0)}
SPHERE = ((3.0, 4.0, 1.7), 0.0, 0.0)  # one 8x8 tile in front of the sphere: sphere pixels in the middle, the wall behind it at the rim
SIZES = [(65, 9, None), (67, 13, None), (256, 256, 2560)]

_oracle = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def renderer(binding, config, camera, w, h):
    R = make("global_illumination", w, h, binding, probes=CONFIGS[config])
    pos, yaw, pitch = CAMERAS[camera] if isinstance(camera, str) else camera
    R.Set_Camera_Position(pos)
    R.Set_Camera_Orientation(rotation(yaw, pitch))
    return R


def oracle_frames(orc, config, camera, w, h):
    """two frames of the oracle, rendered once per configuration, camera and size and left unchanged"""
    key = (config, camera, w, h)
    if key not in _oracle:
        R = renderer(orc, config, camera, w, h)
        _oracle[key] = snapshot(R, 2)
        R.Destroy()
    return _oracle[key]


def assert_frames(hip, want, config, camera, w, h, split=None):
    for gbuffer in (1, 0):
        R = renderer(hip, config, camera, w, h)
        R.Set_Option(B.OPT_GBUFFER, gbuffer)
        if split is not None:
            R.Set_Option(B.OPT_SCREEN_SPLIT, split)
        what = "%s %s %dx%d gbuffer %d" % (config, camera, w, h, gbuffer)
        if gbuffer:
            got = snapshot(R, 2)
            assert_parity(got, want)
            for k in want:
                assert np.array_equal(bits(got[k]), bits(want[k])), "%s: %s differs from the oracle in %d words" % (what, k, int((bits(got[k]) != bits(want[k])).sum()))
        else:  # (another kernel variant; nothing to read back but the image and the atlases)
            R.Render()
            R.Render()
            for k, got in (("image", R.Read_Framebuffer()), ("radiance", R.Read_Texture(B.TEX_RADIANCE)), ("irradiance", R.Read_Texture(B.TEX_IRRADIANCE))):
                assert np.array_equal(bits(got), bits(want[k])), "%s: %s" % (what, k)
        R.Destroy()


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_frames_are_the_oracles(hip, orc, config, camera):
    assert_frames(hip, oracle_frames(orc, config, camera, 64, 64), config, camera, 64, 64)


@pytest.mark.parametrize("w,h,split", SIZES, ids=["%dx%d%s" % (w, h, "" if s is None else "-split%d" % s) for w, h, s in SIZES])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_partial_and_split_tiles_are_the_oracles(hip, orc, config, w, h, split):
    assert_frames(hip, oracle_frames(orc, config, "edge", w, h), config, "edge", w, h, split)


@pytest.mark.parametrize("gbuffer", [1, 0])
@pytest.mark.parametrize("camera", ["edge", "floor"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_recording_and_replaying_frames_are_the_marching_renderers(hip, orc, config, camera, gbuffer):
    """MDH_OPT_SCREEN_REPLAY 1 over four static frames -- plain, recording, replaying, replaying -- against a renderer that
    marches every pass: the three kernels share the corner loop.  The marching renderer's second frame is the oracle's."""
    outs, kinds = [], []
    for replay in (1, 0):
        R = renderer(hip, config, camera, 64, 64)
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
            assert np.array_equal(bits(x), bits(y)), "frame %d, output %d: %d words differ" % (f, n, int((bits(x) != bits(y)).sum()))
    assert np.array_equal(bits(outs[1][1][0]), bits(oracle_frames(orc, config, camera, 64, 64)["image"]))


COUNTERS_SCRIPT = r"""
import ctypes as C, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import test_gpu_folded_twins as T
from madarch_amd import _binding as B
hip = B.hip_binding()
assert hasattr(hip.lib, "mdh_diag_shared_taps") and hasattr(hip.lib, "mdh_diag_work"), "not the counters build"
def count(name):
    out = (C.c_ulonglong * 1)()
    assert getattr(hip.lib, name)(out) == 0
    return int(out[0])
def work(R, p):
    out = (C.c_ulonglong * 4)()
    assert hip.lib.mdh_diag_work(R._h, p, out) == 0
    return list(out)
for name, camera, size in [(k, k, 64) for k in sorted(T.CAMERAS)] + [("sphere", T.SPHERE, 8)]:
    R = T.renderer(hip, "8x8x8", camera, size, size)
    R.Set_Option(B.OPT_GBUFFER, 0)  # (the kernel of the benchmark's frame)
    R.Render(); R.Render()
    count("mdh_diag_shared_taps")
    R.Render_Pass(B.PASS_SCREEN)
    print("COUNTS", name, count("mdh_diag_shared_taps"), "WORK", work(R, B.PASS_SCREEN))
    R.Destroy()
print("FOLDED_TWINS_DONE")
""" % (ROOT, ROOT)

# No part removes a march step or an SDF evaluation, and a folded corner's ray that never took a step is counted as before: the
# work counters of each camera's screen pass -- [rays, march steps, SDF evaluations, arg-min evaluations at hit points] -- are
# those that the counters build of the commit before this change reported for the same frames on an MI355X, and so is the count
# of sharing wavefronts.
PARENT = {  # camera: (sharing wavefront-points, the screen pass's work counters)
    "corner": (49, "WORK [57402, 113059, 129631, 8192]"),
    "default": (48, "WORK [47911, 122032, 148111, 8192]"),
    "edge": (172, "WORK [46230, 95198, 121940, 8192]"),
    "floor": (77, "WORK [52322, 116151, 142192, 8192]"),
    "sphere": (0, "WORK [799, 1920, 2295, 128]"),
}


def test_the_counts_and_the_work_counters():
    assert os.path.exists(COUNTERS), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, MADARCH_HIP_LIBRARY=COUNTERS)
    out = subprocess.run([sys.executable, "-c", COUNTERS_SCRIPT], capture_output=True, text=True, timeout=300, env=env)
    print(out.stdout[-3000:])
    assert "FOLDED_TWINS_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    got = {}
    for line in out.stdout.splitlines():
        if line.startswith("COUNTS "):
            name, one, rest = line.split(None, 3)[1:]
            got[name] = (int(one), rest)
    assert sorted(got) == sorted(PARENT)
    for name, (one, work) in PARENT.items():
        assert got[name] == (one, work), (name, got[name], PARENT[name])
    assert all(PARENT[name][0] > 0 for name in CAMERAS) and PARENT["sphere"][0] == 0  # (every camera has sharing tiles; the sphere's tile never shares)
