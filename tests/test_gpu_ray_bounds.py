"""MDH_RAY_BOUNDS (march_plain, mdh_march.h; ray_bounds and closest_primitive, mdh_device.h): the primary and the reflection march
of the screen pass bound the sphere's and the box's distance once per ray and skip a solid's block wherever the bound exceeds the
running minimum in every live lane.  No output may change in any bit (tests/test_ray_bounds_host.py holds the bound in numpy):
64x64 frames against the oracle word for word -- image, both atlases, and the geometry buffer where the variant carries it --

  * with the 8x8x8 probes (k_screen <ROOM | POW2>) and the reference's default probes (k_screen <ROOM>), with and without the
    geometry buffer, marching, and recording then replaying;
  * under the six cameras of tests/test_gpu_best_first.py and `sphere` and `box` of tests/test_gpu_hit_info.py, and

      graze      (3.0, 5.0005, -2.0) along +z: the central rays graze the sphere's top (centre y 4, radius 1);
      box_edge   along the box's upper front edge (y = 1.5, z = 2.5) from the x wall;
      outside    thirty units behind the z wall, more than lim = 16 from the origin: the bounds are off for every ray;

    and, in the tangent-sphere scene of tests/test_gpu_hit_info.py, its camera along the wall through the gap at the tangent point;
  * under the same cameras, the shipped library's image against the image of the `literal` library, which has the switch off.

Finite cameras only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_folded_twins as T
import test_gpu_hit_info as HI
from helpers import snapshot
from madarch_amd import _binding as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITERAL = os.path.join(ROOT, "madarch_amd", "csrc", "libmadarch_hip_literal.so")
NEW = {"graze": ((3.0, 5.0005, -2.0), 0.0, 0.0), "box_edge": ((-0.5, 1.5, 2.5), float(np.pi / 2), 0.0), "outside": ((3.0, 3.0, -30.0), 0.0, 0.0)}
CAMERAS = dict(HI.CAMERAS, **NEW)
CONFIGS = ["8x8x8", "default"]


@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("config", CONFIGS)
def test_frames_are_the_oracles(hip, orc, config, camera):
    """with and without the geometry buffer (assert_frames renders both)"""
    cam = CAMERAS[camera]
    T.assert_frames(hip, T.oracle_frames(orc, config, cam, 64, 64), config, cam, 64, 64)


@pytest.mark.parametrize("camera", ["graze", "box_edge"])
@pytest.mark.parametrize("config", CONFIGS)
def test_whole_wavefronts_are_the_oracles(hip, orc, config, camera):
    """64x64 as 64 wavefronts of 64 lanes, the benchmark's schedule: a bound skips a block for 64 live lanes at once"""
    cam = CAMERAS[camera]
    T.assert_frames(hip, T.oracle_frames(orc, config, cam, 64, 64), config, cam, 64, 64, 0)


def test_tangent_sphere_scene_is_the_oracles(hip, orc):
    """the sphere touches the x wall: rays along the wall pass the gap, where the bound, the sphere's distance and the planes' meet"""
    Ro = HI.tie_renderer(orc, "tangent_sphere")
    want = snapshot(Ro, 2)
    Ro.Destroy()
    for gbuffer in (1, 0):
        R = HI.tie_renderer(hip, "tangent_sphere")
        R.Set_Option(B.OPT_GBUFFER, gbuffer)
        if gbuffer:
            got = snapshot(R, 2)
        else:
            R.Render(); R.Render()
            got = {"image": R.Read_Framebuffer(), "radiance": R.Read_Texture(B.TEX_RADIANCE), "irradiance": R.Read_Texture(B.TEX_IRRADIANCE)}
        R.Destroy()
        for k in got:
            assert np.array_equal(T.bits(got[k]), T.bits(want[k])), "gbuffer %d: %s differs from the oracle in %d words" % (gbuffer, k, int((T.bits(got[k]) != T.bits(want[k])).sum()))


@pytest.mark.parametrize("gbuffer", [1, 0])
@pytest.mark.parametrize("camera", ["graze", "box_edge", "sphere"])
@pytest.mark.parametrize("config", CONFIGS)
def test_recording_and_replaying_frames_are_the_oracles(hip, orc, config, camera, gbuffer):
    """MDH_OPT_SCREEN_REPLAY 1 over three static frames -- plain, recording, replaying -- against a renderer that marches every
    pass, whose second frame is the oracle's: the recording kernel's marches carry the bounds, the replaying kernel has none"""
    cam = CAMERAS[camera]
    outs, kinds = [], []
    for replay in (1, 0):
        R = T.renderer(hip, config, cam, 64, 64)
        R.Set_Option(B.OPT_GBUFFER, gbuffer)
        R.Set_Option(B.OPT_SCREEN_REPLAY, replay)
        frames = []
        for _ in range(3):
            R.Render()
            frames.append([R.Read_Framebuffer(), R.Read_Texture(B.TEX_RADIANCE), R.Read_Texture(B.TEX_IRRADIANCE)] + (list(R.Read_Gbuffer()) if gbuffer else []))
        outs.append(frames)
        kinds.append(R.Screen_Replay_Stats())
        R.Destroy()
    assert kinds[0] == (1, 1, 1) and kinds[1] == (3, 0, 0), kinds
    for f, (a, b) in enumerate(zip(*outs)):
        for n, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(T.bits(x), T.bits(y)), "frame %d, output %d: %d words differ" % (f, n, int((T.bits(x) != T.bits(y)).sum()))
    assert np.array_equal(T.bits(outs[1][1][0]), T.bits(T.oracle_frames(orc, config, cam, 64, 64)["image"]))


LITERAL_SCRIPT = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import test_gpu_ray_bounds as RB
from madarch_amd import _binding as B
hip = B.hip_binding()
assert hasattr(hip.lib, "mdh_diag_work"), "not a diagnostic build"
out = {}
for name in sorted(RB.CAMERAS):
    R = RB.T.renderer(hip, "8x8x8", RB.CAMERAS[name], 64, 64)
    R.Set_Option(B.OPT_GBUFFER, 0)
    R.Render(); R.Render()
    out[name] = R.Read_Framebuffer()
    R.Destroy()
R = RB.HI.tie_renderer(hip, "tangent_sphere")
R.Set_Option(B.OPT_GBUFFER, 0)
R.Render(); R.Render()
out["tangent_sphere"] = R.Read_Framebuffer()
R.Destroy()
np.savez(sys.argv[1], **out)
print("LITERAL_DONE")
""" % (ROOT, ROOT)


def test_images_are_the_literal_librarys(hip, tmp_path):
    """the literal build (every exact work elimination off, MDH_RAY_BOUNDS among them) renders the same cameras in a child process"""
    assert os.path.exists(LITERAL), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    path = str(tmp_path / "literal.npz")
    env = dict(os.environ, MADARCH_HIP_LIBRARY=LITERAL)
    out = subprocess.run([sys.executable, "-c", LITERAL_SCRIPT, path], capture_output=True, text=True, timeout=300, env=env)
    assert "LITERAL_DONE" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    want = np.load(path)
    for name in sorted(CAMERAS) + ["tangent_sphere"]:
        R = HI.tie_renderer(hip, name) if name == "tangent_sphere" else T.renderer(hip, "8x8x8", CAMERAS[name], 64, 64)
        R.Set_Option(B.OPT_GBUFFER, 0)
        R.Render(); R.Render()
        got = R.Read_Framebuffer()
        R.Destroy()
        assert np.array_equal(T.bits(got), T.bits(want[name])), "%s: %d words differ from the literal library's image" % (name, int((T.bits(got) != T.bits(want[name])).sum()))
