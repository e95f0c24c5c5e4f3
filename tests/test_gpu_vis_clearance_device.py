"""segment_clear on the device (mdh_device.h: segment_clear_bound) against its numpy restatement (scripts/vis_clearance.py)
and against an exact fp64 minimum of the scene's SDF over each segment.

The diagnostic (literal) build exports mdh_diag_segments: for each segment A + vd [0, vmax] it evaluates the bound and the
unmodified march (raycast_visibility) on the committed scene, with the scan run_pass would pick (the rooms' census or the
general scan) or with the general scan forced.  Per scene, for both scans:
  - H_VCLEAR / H_VCLEAR_LIM equal vis_clearance.margins bit for bit (and thr is 0 where the bound does not apply);
  - the device's clear flag equals the restatement's, segment for segment (this ties the CPU soundness tests to the kernel);
  - every cleared segment marches to vis = 1 and its exact minimum is at least EPS + delta / 2.
On the headline room the device clears segments that carry more than half of the march steps (a bound that is silently
off fails there).  Segments: tests/vis_segments.py, 2^20 per scene, most of them grazing a surface within the bound's
margin."""
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITERAL = os.path.join(ROOT, "madarch_amd", "csrc", "libmadarch_hip_literal.so")

SCRIPT = r"""
import ctypes as C, os, sys, time
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import custom_kinds
import vis_segments as vs
from madarch_amd import _binding as B, renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import boxes, planes, spheres, triangles
vc = vs.vc
hip = B.hip_binding()
lib = hip.lib
assert hasattr(lib, "mdh_diag_segments") and hasattr(lib, "mdh_diag_variant"), "not the literal build"
lib.mdh_diag_segments.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
lib.mdh_diag_variant.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
PROBES = renderers.Probe_Settings(Radiance_Resolution=4, Irradiance_Resolution=4, Probe_Count=(2, 1), Grid_Dimensions=(2, 1, 1), Grid_Spacing=(1.0, 1.0, 1.0))
N = 1 << 20

def renderer(desc, extra=(), part=False):
    kinds = [(spheres.Sphere, max(1, len(desc["spheres"]))), (planes.Plane, max(1, len(desc["planes"]))), (boxes.Box, max(1, len(desc["boxes"])))]
    kinds += [(k, 1) for k, _ in extra]
    scene = scenes.Compile(kinds, [(point_lights.Point_Light, 1)], Partitioning=scenes.Partitioning_Settings(Enable=part), Max_Dist=desc["max_dist"])
    R = renderers.Create(windows.Open(8, 8), scene, Probes=PROBES, Volumetrics=renderers.No_Volumetrics, Binding=hip)
    for p in desc["planes"]:
        if len(p) == 3:
            n = [0.0, 0.0, 0.0]; n[p[0]] = float(p[1])
            R.Add_Primitive(planes.Plane, planes.Create(tuple(n), p[2], 0))
        else:
            R.Add_Primitive(planes.Plane, planes.Create(p[0], p[1], 0))
    for c, r in desc["spheres"]:
        R.Add_Primitive(spheres.Sphere, spheres.Create(c, r, 0))
    for c, e in desc["boxes"]:
        R.Add_Primitive(boxes.Box, boxes.Create(c, e, 0))
    for k, ent in extra:
        R.Add_Primitive(k, ent)
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create((1.0, 2.0, 1.0), (1.0, 1.0, 1.0)))
    return R

def run(R, variant, A, vd, vmax):
    n = len(A)
    A, vd, vmax = (np.ascontiguousarray(x, np.float32) for x in (A, vd, vmax))
    clear, vis, tl = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(2, np.float32)
    rc = lib.mdh_diag_segments(R._h, variant, n, A.ctypes.data, vd.ctypes.data, vmax.ctypes.data, clear.ctypes.data, vis.ctypes.data, tl.ctypes.data)
    return rc, clear.astype(bool), vis, tl

def bits(x):
    return int(np.float32(x).view(np.uint32))

# the bound's switch: thr = 0 for a negative radius, a negative half-size, a triangle declared and added
room = vc.ROOM
for name, desc, extra in (("negative radius", dict(room, spheres=[((3.0, 4.0, 3.0), -1.0)]), ()),
                          ("negative half-size", dict(room, boxes=[((3.0, 0.0, 4.0), (1.5, -0.01, 1.5))]), ()),
                          ("triangle", room, ((triangles.Triangle, triangles.Create((1.0, 1.0, 1.0), (2.0, 1.0, 1.0), (1.0, 2.0, 1.0), 0)),))):
    R = renderer(desc, extra)
    thr, lim = vc.margins(vc.scene_arrays(desc))
    rc, clear, vis, tl = run(R, 0, np.zeros((64, 3)) + 2.0, np.tile([0.0, 0.0, 1.0], (64, 1)), np.full(64, 0.5))
    assert rc == 0 and bits(tl[0]) == 0 and not clear.any() and (vis == 1).all(), (name, rc, tl)
    assert bits(tl[1]) == bits(lim), (name, tl, lim)
    if name != "triangle":
        assert bits(thr) == 0, name
    R.Destroy()
# partitioned scenes and user-defined kinds are refused
for part, extra in ((True, ()), (False, ((custom_kinds.My_Sphere, custom_kinds.sphere((2.0, 2.0, 2.0), 0.5, 0)),))):
    R = renderer(room, extra, part)
    assert run(R, 0, np.zeros((1, 3)), np.ones((1, 3)), np.ones(1))[0] == B.MDH_E_STATE, (part, extra)
    R.Destroy()

# efficacy: the headline room's probe-visibility rays (scripts/vis_clearance.py), device clears against the march's steps
sc = vc.scene_arrays(vc.ROOM)
P, Nn = vc.room_points(np.random.default_rng(7), 1500)
A, vd, vmax, _ = vc.visibility_rays(P, Nn)
sd0 = vc.sdf(sc, A)
need = (vmax > 0) & ~(sd0 < vc.EPS) & (sd0 < vmax)
A, vd, vmax, sd0 = A[need], vd[need], vmax[need], sd0[need]
R = renderer(vc.ROOM)
rc, clear, vis, _ = run(R, 0, A, vd, vmax)
R.Destroy()
mvis, steps, _ = vc.march(sc, A, vd, vmax, sd0)
assert rc == 0
share = steps[clear].sum() / steps.sum()
print("headline room efficacy: %%d of %%d rays cleared, %%.1f %%%% of the march steps (device and restatement marches differ on %%d rays)" %% (
      int(clear.sum()), len(A), 100 * share, int((vis != mvis).sum())))
assert share > 0.5, share

rng = np.random.default_rng(0x5E6C)
SCENES = [("headline room", vc.ROOM, 1, 16), ("room x40", vs.room_scene(rng, 40), 40, 16), ("room x300", vs.room_scene(rng, 300), 300, 16),
          ("room x1", vs.room_scene(rng, 1), 1, 16), ("general x1", vs.general_scene(rng, 1), 1, 0), ("general x40", vs.general_scene(rng, 40), 40, 0),
          ("general x300", vs.general_scene(rng, 300), 300, 0)]
for name, desc, scale, pfk in SCENES:
    t0 = time.time()
    sc = vc.scene_arrays(desc)
    thr, lim = vc.margins(sc)
    assert thr > 0, name
    delta = float(np.ldexp(1.0 + float(lim), -12))
    A, vd, vmax = vs.segments(rng, sc, N, vs.SCALE_K[scale][0])
    want = vc.segment_clear(sc, thr, lim, A, vd, vmax)
    R = renderer(desc)
    fails = []  # (every check of a scene is made and reported, not only the first that fails)
    for variant in (0, 1):
        rc, clear, vis, tl = run(R, variant, A, vd, vmax)
        assert rc == 0, (name, variant, rc)
        if not (bits(tl[0]) == bits(thr) and bits(tl[1]) == bits(lim)):
            fails.append(("thr / lim", variant, tl.tolist(), float(thr), float(lim)))
        bad = np.nonzero(clear != want)[0]
        if len(bad):
            fails.append(("device and restatement disagree", variant, len(bad), [(A[i].tolist(), vd[i].tolist(), float(vmax[i]), bool(clear[i])) for i in bad[:3]]))
        if not (vis[clear] == 1.0).all():
            fails.append(("cleared segments that the march finds blocked", variant, int((vis[clear] != 1.0).sum())))
        pos = clear & (vmax > 0)
        m64 = vc.segment_min64(sc, A[pos], vd[pos], vmax[pos])
        if not (m64 >= vs.EPS + delta / 2).all():
            fails.append(("cleared segments closer than EPS + delta / 2", variant, int((m64 < vs.EPS + delta / 2).sum()), float(m64.min()), vs.EPS + delta / 2))
        if not ((vis[vmax <= 0] == 1.0).all() and np.isin(vis, (0.0, 1.0, -1.0)).all() and (vis[~(vmax <= 4096)] == -1.0).all()):
            fails.append(("march results", variant))
    assert not fails, (name, fails)
    R.Render()
    v = np.zeros(2, np.int32)
    assert lib.mdh_diag_variant(R._h, B.PASS_SCREEN, v.ctypes.data) == 0 and v[0] == pfk, (name, v)
    R.Destroy()
    _, band, _ = vs.bands(sc, A[:1 << 16], vd[:1 << 16], vmax[:1 << 16])
    cnt = np.bincount(band, minlength=3)
    assert cnt[1] > 0.5 * cnt.sum(), (name, cnt)
    print("%%-13s delta %%.4f: %%d segments, cleared %%d, blocked %%d; of 65536 sampled, below / in / above the band [EPS - delta, EPS + 3 delta]: %%s, "
          "cleared among them %%s; closest cleared %%.5f (EPS + delta/2 = %%.5f); %%.1f s" %% (
          name, delta, len(A), int(clear.sum()), int((vis == 0).sum()), cnt.tolist(), np.bincount(band[clear[:1 << 16]], minlength=3).tolist(),
          float(m64.min()) if len(m64) else float('inf'), vs.EPS + delta / 2, time.time() - t0), flush=True)

print("VIS_CLEARANCE_DEVICE_OK")
""" % (ROOT, ROOT)


def test_segment_clear_on_the_device():
    assert os.path.exists(LITERAL), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, MADARCH_HIP_LIBRARY=LITERAL)
    t = time.time()
    out = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, timeout=900, env=env)
    print(out.stdout)
    print("wall time %.1f s" % (time.time() - t))
    assert "VIS_CLEARANCE_DEVICE_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
