"""MDH_SHARE_TAPS (shade_structured, mdh_march.h): a wavefront whose active lanes share the cage cell and the bits of the normal
at the first shaded point computes its eight irradiance taps once -- the lane of rank r takes corner r & 7 -- and every lane
reads them from the wavefront's park row.  No output may change in any bit: frames of the global_illumination scene are held
against the oracle word for word (image, geometry buffer, both atlases), at sizes that give uniform tiles, tiles across two
planes or cells, partial tiles with exactly 8, 24 and 1 valid lanes, and tiles split over two and four wavefronts; with the
8x8x8 probes (power-of-two addressing), the reference's default probes (nothing a power of two) and float32 atlases; with and
without the geometry buffer; marching, recording and replaying.  Shade_Points is held against the frame's own pixels (which
are the oracle's) and against batches too small to share.  The count of wavefronts that took the path, and the work counters
beside it, are read from the counters build in a child process (test_gpu_work_counters.py loads the literal build that way)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shade_points_cases as P
from helpers import assert_parity, make, snapshot
from madarch_amd import _binding as B
from madarch_amd import examples

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = os.path.join(ROOT, "madarch_amd", "csrc", "libmadarch_hip_counters.so")
GI = examples.GI_8X8X8_PROBES
CONFIGS = {"8x8x8": (GI, 0), "default": (None, 0), "8x8x8-float32": (GI, 1)}
# 64 x 64: whole tiles, most of them on one plane in one cell; 65 x 9: the right-hand column of tiles has one pixel column --
# 8 valid lanes in the upper tile, the rank-to-corner mapping on a sparse mask, and ONE lane in the lower one (below 8: today's
# code); 67 x 13: three pixel columns -- 24 lanes; 256 x 256: 1024 tiles, which MDH_OPT_SCREEN_SPLIT hands to two wavefronts
# each (limit 2560) or four (limit 4096) with idle upper lanes
SIZES = [(64, 64, None), (65, 9, None), (67, 13, None), (256, 256, 2560), (256, 256, 4096)]

_oracle = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def oracle_frames(orc, config, w, h):
    """two frames of the oracle, rendered once per configuration and size and left unchanged"""
    key = (config, w, h)
    if key not in _oracle:
        probes, atlas = CONFIGS[config]
        R = make("global_illumination", w, h, orc, atlas=atlas, probes=probes)
        _oracle[key] = snapshot(R, 2)
        R.Destroy()
    return _oracle[key]


def assert_words(got, want, what):
    assert_parity(got, want)
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s: %s differs from the oracle in %d words" % (what, k, int((bits(got[k]) != bits(want[k])).sum()))


@pytest.mark.parametrize("w,h,split", SIZES, ids=["%dx%d%s" % (w, h, "" if s is None else "-split%d" % s) for w, h, s in SIZES])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_frames_are_the_oracles(hip, orc, config, w, h, split):
    probes, atlas = CONFIGS[config]
    want = oracle_frames(orc, config, w, h)
    for gbuffer in (1, 0):
        R = make("global_illumination", w, h, hip, atlas=atlas, probes=probes)
        R.Set_Option(B.OPT_GBUFFER, gbuffer)
        if split is not None:
            R.Set_Option(B.OPT_SCREEN_SPLIT, split)
        if gbuffer:
            assert_words(snapshot(R, 2), want, "%s %dx%d" % (config, w, h))
        else:  # (another kernel variant; nothing to read back but the image and the atlases)
            R.Render()
            R.Render()
            for k, got in (("image", R.Read_Framebuffer()), ("radiance", R.Read_Texture(B.TEX_RADIANCE)), ("irradiance", R.Read_Texture(B.TEX_IRRADIANCE))):
                assert np.array_equal(bits(got), bits(want[k])), "%s %dx%d without the geometry buffer: %s" % (config, w, h, k)
        R.Destroy()


@pytest.mark.parametrize("gbuffer", [1, 0])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_recording_and_replaying_frames_are_the_marching_renderers(hip, orc, config, gbuffer):
    """MDH_OPT_SCREEN_REPLAY 1 over four static frames -- plain, recording, replaying, replaying -- against a renderer that
    marches every pass: the three kernels share the corner loop.  The marching renderer's second frame is the oracle's."""
    probes, atlas = CONFIGS[config]
    outs, kinds = [], []
    for replay in (1, 0):
        R = make("global_illumination", 64, 64, hip, atlas=atlas, probes=probes)
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
    assert np.array_equal(bits(outs[1][1][0]), bits(oracle_frames(orc, config, 64, 64)["image"]))


def flip_zero_signs(n, k):
    """normal n with the sign of its zero components set from the bits of k (bit a: component a, where it is a zero)"""
    out = n.copy()
    for a in range(3):
        if out[a] == 0.0 and (k >> a) & 1:
            out[a] = -0.0
    return out


def point_cases(R):
    """a renderer's frame and one pixel of it on an axis-aligned surface: what Shade_Points takes for that point"""
    org, drs, rows, (pos, nrm, view, mat), _, _ = P.frame_points(R, R.Width, R.Height)
    fb = R.Read_Framebuffer().reshape(-1, 3)
    axis = np.nonzero(((nrm == 0.0).sum(axis=1) == 2))[0]
    assert len(axis) > 100
    k = axis[len(axis) // 2]
    return (pos[k], nrm[k], view[k], mat[k]), fb[rows[k]]


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_shade_points_shares_and_refuses(hip, config):
    """64 copies of one point and normal: one wavefront, uniform -- every answer is the pixel's.  5 copies: below 8 lanes,
    today's code -- the same answer.  64 points that differ only in the SIGN of a zero component of the normal must not
    share: each is answered as it is alone (batches of 5 of itself)."""
    probes, atlas = CONFIGS[config]
    R = make("global_illumination", 64, 64, hip, atlas=atlas, probes=probes)
    R.Render()
    R.Render()
    R.Render_Pass(B.PASS_SCREEN)  # (the frame from the atlases as they stand now: what Shade_Points reads)
    (p, n, v, m), pixel = point_cases(R)
    rep = lambda x, k: np.ascontiguousarray(np.repeat(np.asarray(x)[None], k, axis=0))
    for copies in (64, 5, 8, 9):
        got = R.Shade_Points(rep(p, copies), rep(n, copies), rep(v, copies), rep(m, copies).reshape(-1), Mode=0, Tone_Map=True)
        assert np.array_equal(bits(got), bits(rep(pixel, copies))), "%d copies: %s against the pixel's %s" % (copies, got[0], pixel)
    normals = np.stack([flip_zero_signs(n, k) for k in range(64)]).astype(np.float32)
    assert len(np.unique(bits(normals), axis=0)) == 4
    mixed = R.Shade_Points(rep(p, 64), normals, rep(v, 64), rep(m, 64).reshape(-1), Mode=0, Tone_Map=True)
    for k in np.unique(bits(normals), axis=0, return_index=True)[1]:  # the four sign patterns, each alone
        sel = np.nonzero((bits(normals) == bits(normals[k])).all(axis=1))[0]
        alone = R.Shade_Points(rep(p, 5), rep(normals[k], 5), rep(v, 5), rep(m, 5).reshape(-1), Mode=0, Tone_Map=True)
        assert np.array_equal(bits(mixed[sel]), bits(rep(alone[0], len(sel)))), k
    R.Destroy()


COUNTERS_SCRIPT = r"""
import ctypes as C, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import test_gpu_shared_taps as T
from helpers import make
from madarch_amd import _binding as B
from madarch_amd import examples
hip = B.hip_binding()
assert hasattr(hip.lib, "mdh_diag_shared_taps") and hasattr(hip.lib, "mdh_diag_work"), "not the counters build"
def shared():
    out = (C.c_ulonglong * 1)()
    assert hip.lib.mdh_diag_shared_taps(out) == 0
    return int(out[0])
def work(R, p):
    out = (C.c_ulonglong * 4)()
    assert hip.lib.mdh_diag_work(R._h, p, out) == 0
    return list(out)
R = make("global_illumination", 64, 64, hip, probes=examples.GI_8X8X8_PROBES)
R.Set_Option(B.OPT_GBUFFER, 0)  # (the kernel of the benchmark's frame; share_taps_screen, mdh_march.h, leaves the one with the geometry buffer out)
shared()
R.Render(); R.Render()
n_frame = shared()
print("WORK", work(R, B.PASS_SCREEN), work(R, B.PASS_RADIANCE))
R.Render_Pass(B.PASS_SCREEN)
n_pass = shared()
(p, n, v, m), pixel = T.point_cases(R)
rep = lambda x, k: np.ascontiguousarray(np.repeat(np.asarray(x)[None], k, axis=0))
counts = {}
for copies in (5, 7, 8, 64, 130):
    got = R.Shade_Points(rep(p, copies), rep(n, copies), rep(v, copies), rep(m, copies).reshape(-1), Mode=0, Tone_Map=True)
    assert np.array_equal(T.bits(got), T.bits(rep(pixel, copies))), copies
    counts[copies] = shared()
normals = np.stack([T.flip_zero_signs(n, k) for k in range(64)]).astype(np.float32)
R.Shade_Points(rep(p, 64), normals, rep(v, 64), rep(m, 64).reshape(-1), Mode=0, Tone_Map=True)
counts["signs"] = shared()
print("SHARED", n_frame, n_pass, counts)
# two frames of 64 tiles: between one wavefront (a frame of mixed tiles only) and every wavefront of both
assert 0 < n_pass <= 64 and n_frame == 2 * n_pass, (n_frame, n_pass)
assert counts == {5: 0, 7: 0, 8: 1, 64: 1, 130: 2, "signs": 0}, counts  # (130 points: 64 + 64 + 2 lanes)
print("SHARED_TAPS_OK")
""" % (ROOT, ROOT)

# Sharing removes no ray, no march step and no SDF evaluation: the work counters of the frame's second screen and radiance pass
# -- [rays, march steps, SDF evaluations, arg-min evaluations at hit points] -- are those that the counters build of the commit
# before this change reported for the same frame on an MI355X.
PARENT_WORK = "WORK [47911, 122032, 148111, 8192] [573569, 6976428, 7975723, 524288]"  # (screen, radiance)


def test_the_count_and_the_work_counters():
    assert os.path.exists(COUNTERS), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, MADARCH_HIP_LIBRARY=COUNTERS)
    out = subprocess.run([sys.executable, "-c", COUNTERS_SCRIPT], capture_output=True, text=True, timeout=300, env=env)
    print(out.stdout[-2000:])
    assert "SHARED_TAPS_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    work = [line for line in out.stdout.splitlines() if line.startswith("WORK ")][0]
    assert work == PARENT_WORK, (work, PARENT_WORK)
