"""Ray queries (mdh_raycast, mdh_raycast_visibility, mdh_softshadows) without a device: the exports, the rejections that
need no renderer, the wrappers' shape checks -- and the yardsticks of tests/test_gpu_ray_queries.py, proved here on the CPU:
the visibility the GPU test derives from orc_probe_raycast is ref64's raycast_visibility, and the oracle's own soft
shadows pass the float64 hold under the tolerance the device's min_dist > 0 shadows are held to."""
import ctypes as C

import numpy as np
import pytest

import ray_query_cases as rq
import ref64
from helpers import SEED
from madarch_amd import _binding as B
from madarch_amd import renderers, windows

NAMES = ("mdh_raycast", "mdh_raycast_visibility", "mdh_softshadows", "mdh_ray_query_time")


def test_the_library_exports_the_calls(hip):
    for name in NAMES:
        assert hasattr(hip.lib, name), name
    for name in ("raycast", "raycast_visibility", "softshadows", "ray_query_time"):
        assert name in B.HIP_ONLY_ABI and name not in B.ABI  # (the oracle has no orc_raycast: its probes answer for it)


def test_a_null_renderer_is_invalid(hip):
    three, one = (C.c_float * 3)(1.0, 2.0, 3.0), (C.c_float * 1)(1.0)
    hit = (C.c_int32 * 1)()
    assert hip.raycast(None, 1, three, three, hit, None, None, None, None, None) == B.MDH_E_INVALID
    assert hip.raycast_visibility(None, 1, three, three, one, one) == B.MDH_E_INVALID
    assert hip.softshadows(None, 1, three, three, 0.0, one, 64.0, one) == B.MDH_E_INVALID
    assert hip.raycast(None, 0, None, None, None, None, None, None, None, None) == B.MDH_E_INVALID  # (n = 0 excuses no null renderer)
    assert hip.ray_query_time(None, C.byref(C.c_double())) == B.MDH_E_INVALID


class _NoLibrary:
    """a binding that fails the test when anything is called through it"""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def test_the_wrappers_refuse_mismatched_shapes_before_the_library():
    R = renderers.Renderer(_NoLibrary(), None, windows.Open(4, 4, "none"), None, None, None)
    o, d = np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32)
    for bad_o, bad_d in ((o, d[:4]), (o.reshape(3, 5), d.reshape(3, 5)), (o[0], d[0]), (np.zeros(15, np.float32), np.zeros(15, np.float32))):
        for call in (lambda: R.Raycast(bad_o, bad_d), lambda: R.Raycast_Visibility(bad_o, bad_d, 1.0), lambda: R.Softshadows(bad_o, bad_d, 0.0, 1.0, 64.0)):
            with pytest.raises(ValueError):
                call()
    for tmax in (np.ones(4, np.float32), np.ones((5, 1), np.float32)):
        with pytest.raises(ValueError):
            R.Raycast_Visibility(o, d, tmax)
        with pytest.raises(ValueError):
            R.Softshadows(o, d, 0.0, tmax, 64.0)
    # a scalar length is one length per ray: it passes the checks and reaches the library
    with pytest.raises(AssertionError, match="the library was called"):
        R.Raycast_Visibility(o, d, 2.5)
    R._h = None  # (nothing to destroy)


@pytest.mark.parametrize("name", ["room", "open"])
def test_visibility_from_the_oracles_raycast_is_ref64s_visibility(orc, name):
    """The GPU test's yardstick for tmax < max_dist.  The oracle exports raycast, not raycast_visibility; the two march the same
    steps, so visibility = not (hit and t < tmax).  Here that identity, on the oracle's raycast, against the float64
    raycast_visibility of ref64 written from the shader: every ray whose float64 march stays clear of the epsilon threshold
    (`near`) and of its own end (a hit within T_ATOL of tmax may fall on either side of it) must agree."""
    Ro, desc = rq.described(orc, name)
    n = 600
    org, drs = (rq.rays_inside(n, rq.ROOM_LO, rq.ROOM_HI, SEED + 3) if name == "room" else rq.open_rays(n))
    if name == "room":
        o2, d2 = rq.rays_from_inside_primitives(40, SEED + 4)
        org, drs = np.concatenate((org, o2)), np.concatenate((drs, d2))
    rc = rq.orc_raycast(orc, Ro, org, drs)
    assert 0.05 < (rc["hit"] == 0).mean() if name == "open" else (rc["hit"] == 1).all()
    sc = ref64.Scene(desc)
    seen = set()
    for tmax in (np.full(len(org), rq.MAX_DIST), rq.seeded_tmax(len(org), SEED + 5)):
        got = rq.visibility_from_raycast(rc, tmax)
        hit64, _, t64, _, near = ref64.Run(sc).raycast(org, drs, tmax.astype(np.float64))
        want = 1.0 - hit64.astype(np.float64)
        held = ~near & ~(np.abs(t64 - tmax) <= ref64.T_ATOL) & ~(np.abs(rc["t"].astype(np.float64) - tmax) <= ref64.T_ATOL)
        print("%s: %d of %d rays held, %d visible" % (name, held.sum(), len(held), int(want[held].sum())))
        assert held.mean() > 0.95
        assert np.array_equal(got[held], want[held])
        seen |= set(want[held])
    assert seen == {0.0, 1.0}  # (at max_dist nothing in the closed room is visible; below it both answers occur)


@pytest.mark.parametrize("k", rq.SHADOW_KS)
@pytest.mark.parametrize("name", ["room", "open"])
def test_the_oracles_soft_shadows_pass_the_float64_hold(orc, name, k):
    """The tolerance of the device's min_dist > 0 soft shadows comes from here, not from the kernel: the oracle's own
    min_dist = 0 results through ray_query_cases.hold_shadows -- three float64 runs (seeds None, 1, 2), FRAGILE_CAP as it is,
    COLOUR_RTOL / COLOUR_ATOL.  They hold, so those are the tolerances.  And the same rays at both min_dist > 0 of the GPU test
    stay under the cap in float64 alone (hold_values asserts the fragile share)."""
    Ro, desc = rq.described(orc, name)
    org, drs, tmax = rq.shadow_rays(name)
    got = rq.orc_softshadow(orc, Ro, org, drs, tmax, k)
    # blocked rays, and what the k is there for: the wide penumbra of k = 0.5, the lit rays of k = 64
    assert (got == 0.0).sum() > 5 and (((got > 0.0) & (got < 1.0)).sum() > 20 if k < 1.0 else (got == 1.0).sum() > 5)
    rq.hold_shadows("%s k %g, oracle" % (name, k), desc, org, drs, 0.0, tmax, k, got)
    for tmin in rq.SHADOW_TMINS:
        runs = rq.shadow_runs(desc, org, drs, tmin, tmax, k)
        ref64.hold_values("%s k %g min_dist %g, float64 alone" % (name, k, tmin), runs, runs[0]["colour"], ref64.COLOUR_RTOL, ref64.COLOUR_ATOL)
