"""MDH_BEST_APPROX (mdh_march.h: best_approx): the first round of the reflection point's best-first probe search ranks the cage
corners by an approximate dot(probe_to_spec, -N) and forms the exact direction for the winner alone; a lane the approximation
cannot decide sends its wavefront through the exact scan.  No output may change in any bit:

  * 64x64 frames word for word against the oracle (image, geometry buffer, both atlases; geometry buffer on and off) under the
    six cameras of tests/test_gpu_best_first.py -- gap, low_wall and default have lanes whose first candidate is blocked: rounds
    after the first, which always scan -- with the 8x8x8 and the default probes, and the frame `tie` below;
  * recording then replaying over three static frames against a renderer that marches every pass;
  * the shipped library's images equal to the `literal` library's (every exact work elimination off);
  * the statistics build (mdh_diag_best_approx) met decided and undecided lanes.

scripts/best_approx_estimate.py's model decides EVERY lane of the six 64x64 cameras under both probe grids (their reflection
points lie on no symmetry plane of a cage), so the undecided path has a frame of its own: `tie`, the default probes
(spacing 2 along x) seen from x = 3 at 65x9.  The middle column's primary rays and their reflections stay in the plane x = 3,
midway between the probes at x = 2 and x = 4, with no normal component across it: the two sides' a are equal bit for bit, in
the model (9 lanes) and on the device whatever v_rsq_f32 returns."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_best_first as BF
from madarch_amd import _binding as B

T = BF.T
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madarch_amd", "csrc")
LITERAL = os.path.join(CSRC, "libmadarch_hip_literal.so")
TIE = ("default", T.SPHERE, 65, 9)
CONFIGS = ("8x8x8", "default")


@pytest.mark.parametrize("camera", sorted(BF.CAMERAS))
@pytest.mark.parametrize("config", CONFIGS)
def test_frames_are_the_oracles(hip, orc, config, camera):
    cam = BF.CAMERAS[camera]
    T.assert_frames(hip, T.oracle_frames(orc, config, cam, 64, 64), config, cam, 64, 64)


@pytest.mark.parametrize("split", [None, 0], ids=["split", "whole"])
def test_the_tie_frame_is_the_oracles(hip, orc, split):
    config, cam, w, h = TIE
    T.assert_frames(hip, T.oracle_frames(orc, config, cam, w, h), config, cam, w, h, split)


@pytest.mark.parametrize("camera", sorted(BF.FALLBACK))
@pytest.mark.parametrize("config", CONFIGS)
def test_whole_wavefronts_are_the_oracles(hip, orc, config, camera):
    """one wavefront per 8x8 tile, the benchmark's schedule: winners of several rounds and fallback lanes share a wavefront"""
    cam = BF.FALLBACK[camera]
    T.assert_frames(hip, T.oracle_frames(orc, config, cam, 64, 64), config, cam, 64, 64, 0)


def frames_of(hip, config, cam, w, h, gbuffer, replay, n=3):
    R = T.renderer(hip, config, cam, w, h)
    R.Set_Option(B.OPT_GBUFFER, gbuffer)
    R.Set_Option(B.OPT_SCREEN_REPLAY, replay)
    frames = []
    for _ in range(n):
        R.Render()
        frames.append([R.Read_Framebuffer(), R.Read_Texture(B.TEX_RADIANCE), R.Read_Texture(B.TEX_IRRADIANCE)] + (list(R.Read_Gbuffer()) if gbuffer else []))
    kinds = R.Screen_Replay_Stats()
    R.Destroy()
    return frames, kinds


@pytest.mark.parametrize("gbuffer", [1, 0])
@pytest.mark.parametrize("frame", ["gap", "low_wall", "tie"])
def test_recording_and_replaying_frames_are_the_marching_renderers(hip, orc, frame, gbuffer):
    """MDH_OPT_SCREEN_REPLAY 1 over three static frames -- plain, recording, replaying -- against a renderer that marches every
    pass: a winner the approximation named records the bits a scanned winner records, and the replaying kernel names its probe."""
    config, cam, w, h = TIE if frame == "tie" else ("8x8x8", BF.FALLBACK[frame], 64, 64)
    (a, ka), (b, kb) = frames_of(hip, config, cam, w, h, gbuffer, 1), frames_of(hip, config, cam, w, h, gbuffer, 0)
    assert ka == (1, 1, 1) and kb == (3, 0, 0), (ka, kb)
    for f, (x, y) in enumerate(zip(a, b)):
        for n, (p, q) in enumerate(zip(x, y)):
            assert np.array_equal(T.bits(p), T.bits(q)), "frame %d, output %d: %d words differ" % (f, n, int((T.bits(p) != T.bits(q)).sum()))
    assert np.array_equal(T.bits(b[1][0]), T.bits(T.oracle_frames(orc, config, cam, w, h)["image"]))


CHILD = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import test_gpu_best_approx as A
from madarch_amd import _binding as B
hip = B.hip_binding()
stats = hasattr(hip.lib, "mdh_diag_best_approx")
def take():
    out = (C.c_ulonglong * 4)()
    assert hip.lib.mdh_diag_best_approx(out) == 0
    return list(out)
images = {}
frames = [(name, "8x8x8", A.BF.CAMERAS[name], 64, 64) for name in sorted(A.BF.CAMERAS)] + [("tie",) + A.TIE]
for name, config, cam, w, h in frames:
    R = A.T.renderer(hip, config, cam, w, h)
    R.Set_Option(B.OPT_GBUFFER, 0)
    R.Set_Option(B.OPT_SCREEN_SPLIT, 0)  # (one wavefront per 8x8 tile)
    R.Render(); R.Render()
    images[name] = R.Read_Framebuffer()
    if stats:
        take()
        R.Render_Pass(B.PASS_SCREEN)
        print("APPROX", name, *take())
    R.Destroy()
np.savez(sys.argv[1], **images)
print("BEST_APPROX_DONE")
""" % (ROOT, ROOT)


def child(library, out):
    env = dict(os.environ, MADARCH_HIP_LIBRARY=library)
    run = subprocess.run([sys.executable, "-c", CHILD, out], capture_output=True, text=True, timeout=300, env=env)
    print(run.stdout[-3000:])
    assert "BEST_APPROX_DONE" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    return run.stdout, np.load(out)


def test_the_literal_librarys_images_and_the_statistics(hip, tmp_path):
    """The seven frames (two rendered, the second kept) from the literal library and from the statistics build, each in a child
    process, against the shipped library's here.  [winners, lanes without a candidate, undecided lanes, wavefronts that scanned
    for them] of one unsplit screen pass per frame -- conditions on the inputs, not tolerances: a closed room, so every pixel
    has a second point and its lane is one of the three; the six cameras have decided lanes; `tie` has undecided ones, and every
    wavefront with one scans."""
    for lib in (LITERAL, BF.BESTSTATS):
        assert os.path.exists(lib), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    _, lit = child(LITERAL, str(tmp_path / "literal.npz"))
    out, st = child(BF.BESTSTATS, str(tmp_path / "stats.npz"))
    for name, config, cam, w, h in [(n, "8x8x8", BF.CAMERAS[n], 64, 64) for n in sorted(BF.CAMERAS)] + [("tie",) + TIE]:
        R = T.renderer(hip, config, cam, w, h)
        R.Set_Option(B.OPT_GBUFFER, 0)
        R.Set_Option(B.OPT_SCREEN_SPLIT, 0)
        R.Render(); R.Render()
        img = R.Read_Framebuffer()
        R.Destroy()
        assert np.array_equal(T.bits(img), T.bits(lit[name])), "%s: %d words differ from the literal library's" % (name, int((T.bits(img) != T.bits(lit[name])).sum()))
        assert np.array_equal(T.bits(img), T.bits(st[name])), name
    got = {}
    for line in out.splitlines():
        if line.startswith("APPROX "):
            f = line.split()
            got[f[1]] = [int(x) for x in f[2:]]
    assert sorted(got) == sorted(list(BF.CAMERAS) + ["tie"])
    for name, (win, none, und, waves) in got.items():
        w, h = (65, 9) if name == "tie" else (64, 64)
        assert win + none + und == w * h, (name, got[name])
        assert win > 0, (name, got[name])
        assert (und > 0) == (waves > 0) and waves <= und, (name, got[name])
    assert got["tie"][2] > 0, got["tie"]
