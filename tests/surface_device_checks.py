"""The checks of mdh_surface_mesh_device on the device, with torch tensors as the device memory.  They run in a process of
their own, started once by tests/test_gpu_surface_streams.py, for the reason tests/ray_stream_device_checks.py gives: torch has
to be imported BEFORE the library is loaded.  main () is that module's (the same loop, the same JSON object: check -> {ok,
log, seconds}; after a device error nothing more is started).

The yardstick is the host-array call, which tests/test_gpu_surface_mesh.py holds against the restatement over the oracle,
bit for bit; the scenes and grids are that test's."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ray_query_cases as rq  # noqa: E402
import ray_stream_device_checks as rs  # noqa: E402
import sweep_cases as sw  # noqa: E402
import test_gpu_surface_mesh as tm  # noqa: E402
from helpers import same_bits  # noqa: E402
from madarch_amd import _binding as B  # noqa: E402
from madarch_amd.primitives import boxes, spheres  # noqa: E402

PAD, FILL = 8, rs.FILL
SHAPE = (17, 16, 15)
CORNERS = 18 * 17 * 16
CHECKS = {}  # name -> function, in the order they run


def check(name):
    def register(fn):
        CHECKS[name] = fn
        return fn
    return register


def torch():
    return rs.torch


def hip():
    return rs.hip


def tensors(nv, nq, field=True):
    t = torch()
    out = {"positions": rs.filled(3 * (nv + PAD), t.float32), "normals": rs.filled(3 * (nv + PAD), t.float32), "index": rs.filled(nv + PAD, t.int32),
           "quads": rs.filled(4 * (nq + PAD), t.int32), "counts": rs.filled(2 + PAD, t.int32)}
    if field:
        out["field"] = rs.filled(CORNERS + PAD, t.float32)
    return out


def device_mesh(R, grid, out, nv, nq, prims=None, stream=0, address=False):
    """Surface_Mesh_Device into the tensors of `out`, or into their plain addresses"""
    origin, h, iso = grid
    a = {k: (int(v.data_ptr()) if address else v) for k, v in out.items()}
    R.Surface_Mesh_Device(origin, h, SHAPE, a["counts"], iso, prims, nv, nq, a["positions"], a["normals"], a["index"], a["quads"], a.get("field"), Stream=stream)


def assert_host_bits(got, want, nv, nq, what):
    """the first min (found, capacity) entries are the host form's, and nothing behind them is written"""
    found = got["counts"][:2]
    assert tuple(found) == (len(want["positions"]), len(want["quads"])), "%s: counts %s" % (what, found)
    assert (got["counts"][2:] == FILL).all()
    v, q = min(nv, int(found[0])), min(nq, int(found[1]))
    assert same_bits(got["positions"].reshape(-1, 3)[:v], want["positions"][:v]) and (got["positions"][3 * v:] == FILL).all(), what + ": positions"
    assert same_bits(got["normals"].reshape(-1, 3)[:v], want["normals"][:v]) and (got["normals"][3 * v:] == FILL).all(), what + ": normals"
    assert np.array_equal(got["index"][:v], want["index"][:v]) and (got["index"][v:] == FILL).all(), what + ": index"
    assert np.array_equal(got["quads"].reshape(-1, 4)[:q], want["quads"][:q]) and (got["quads"][4 * q:] == FILL).all(), what + ": quads"
    if "field" in got:
        assert same_bits(got["field"][:CORNERS], want["field"].ravel()) and (got["field"][CORNERS:] == FILL).all(), what + ": field"


def to_host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@check("tensors and addresses give the host form's bits")
def host_bits():
    for name in ("rooms, LDS scan", "partition, Fallback, global residency", "mesh, triangle BVH"):
        R = tm.CASES[name][0](hip())
        grid = tm.grids_of(name)[SHAPE]
        for prims in (None,) if "mesh" in name else (None, (spheres.Sphere, boxes.Box)):
            want = R.Surface_Mesh(grid[0], grid[1], SHAPE, grid[2], prims, Field=True)
            nv, nq = len(want["positions"]), len(want["quads"])
            assert nv > 256 and nq >= 30
            for address in (False, True):
                for cv, cq in ((nv, nq), (65, 33), (nv + 5, nq + 5)):
                    out = tensors(cv, cq)
                    device_mesh(R, grid, out, cv, cq, prims, address=address)
                    assert_host_bits(to_host(out), want, cv, cq, "%s, %s, capacities %d and %d" % (name, prims, cv, cq))
            # the pure count, and the quads alone
            t = torch()
            counts = rs.filled(2, t.int32)
            R.Surface_Mesh_Device(grid[0], grid[1], SHAPE, counts, grid[2], prims)
            assert tuple(counts.cpu().numpy()) == (nv, nq)
            quads = rs.filled(4 * nq, t.int32)
            R.Surface_Mesh_Device(grid[0], grid[1], SHAPE, counts, grid[2], prims, Quad_Capacity=nq, Quads=quads)
            assert np.array_equal(quads.cpu().numpy().reshape(-1, 4), want["quads"])
        R.Ray_Query_Wait()


@check("ordered with the caller's stream")
def ordering():
    """work given to the caller's stream behind the call sees the counts and the arrays, no host wait between; the edit in
    front of the call is seen with frames in flight"""
    t = torch()
    name = "rooms, LDS scan"
    R = rq.gi_room(hip())
    grid = tm.grids_of(name)[SHAPE]
    want = R.Surface_Mesh(grid[0], grid[1], SHAPE, grid[2], Field=True)
    nv, nq = len(want["positions"]), len(want["quads"])
    for side in (t.cuda.Stream(), None):  # a stream of torch's own, then the default stream (Stream = 0)
        handle = 0 if side is None else side.cuda_stream
        ballast = t.ones(1 << 24, device="cuda")
        t.cuda.synchronize()
        with t.cuda.stream(side if side is not None else t.cuda.default_stream()):
            for _ in range(8):
                ballast = ballast * 1.0001 + 0.5  # (work in front of the call)
            out = tensors(nv, nq)
            device_mesh(R, grid, out, nv, nq, stream=handle)
            used = {k: (v + 0 if v.dtype == t.int32 else v * 1.0) for k, v in out.items()}  # consumed on the same stream, no host wait between
        if side is not None:
            side.synchronize()
        assert_host_bits(to_host(used), want, nv, nq, "stream %#x" % handle)
        R.Ray_Query_Wait()
    for _ in range(2):
        R.Render()  # (not waited for)
    R.Set_Primitive(spheres.Sphere, 1, spheres.Create((2.8, 3.9, 2.9), 0.8, 3))
    out = tensors(nv, nq)
    device_mesh(R, grid, out, nv, nq)
    moved = R.Surface_Mesh(grid[0], grid[1], SHAPE, grid[2], Field=True)
    assert len(moved["positions"]) != nv
    assert_host_bits(to_host(out), moved, nv, nq, "after Set_Primitive")
    R.Finish()


@check("rejections launch nothing")
def rejections():
    t = torch()
    name = "rooms, LDS scan"
    R = rq.gi_room(hip())
    R.Set_Option(B.OPT_TIMING, 1)
    origin, h, iso = tm.grids_of(name)[SHAPE]
    assert len(R.Surface_Mesh(origin, h, SHAPE, iso)["positions"]) > 65
    ms = R.Ray_Query_Time()
    assert ms > 0.0
    nv, nq = 65, 33
    out = tensors(nv, nq)
    o, c = np.asarray(origin, np.float32), np.asarray(SHAPE, np.int32)

    def p(x):
        return None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)

    def call(**kw):
        a = dict(out)
        a.update(kw)
        return hip().surface_mesh_device(R._h, p(o), h, p(c), iso, None, 0, kw.get("vcap", nv), kw.get("qcap", nq), p(a["positions"]), p(a["normals"]),
                                         p(a["index"]), p(a["quads"]), p(a["field"]), p(a["counts"]), None)
    host_f, host_i = np.full(3 * CORNERS, -3.0, np.float32), np.full(4 * (nq + PAD), -3, np.int32)
    # arrays whose last 40 and last 4 bytes alone lie inside their allocation: 32 MiB get an allocation of their own from torch,
    # exactly as large, once the blocks it kept from the checks before (the 64 MiB of ballast) are given back
    t.cuda.synchronize()
    t.cuda.empty_cache()
    big = t.full((8 << 20,), FILL, dtype=t.float32, device="cuda")
    tail, last = int(big.data_ptr()) + (big.numel() - 10) * 4, int(big.data_ptr()) + (big.numel() - 1) * 4
    calls = [("pageable positions", dict(positions=host_f)), ("pageable normals", dict(normals=host_f)), ("pageable index", dict(index=host_i)),
             ("pageable quads", dict(quads=host_i)), ("pageable field", dict(field=host_f)), ("pageable counts", dict(counts=host_i)),
             ("short positions", dict(positions=tail)), ("short normals", dict(normals=tail)), ("a short index", dict(index=tail)),
             ("short quads", dict(quads=tail)), ("a short field", dict(field=tail)), ("short counts", dict(counts=last)),
             ("no counts", dict(counts=None)), ("a negative capacity", dict(vcap=-1)), ("quads without a capacity", dict(qcap=0))]
    for what, kw in calls:
        assert call(**kw) == B.MDH_E_INVALID, what
        assert R.Ray_Query_Time() == ms, what
    R.Ray_Query_Wait()
    assert all((v == FILL).all() for v in to_host(out).values()) and (big.cpu().numpy() == FILL).all()
    assert (host_f == -3.0).all() and (host_i == -3).all()
    # the error did not stick: a valid call behind them answers
    assert call() == B.MDH_OK
    assert_host_bits(to_host(out), R.Surface_Mesh(origin, h, SHAPE, iso, Field=True), nv, nq, "behind the refusals")


def main(argv):
    """tests/ray_stream_device_checks.py's process, over this module's checks"""
    rs.CHECKS.clear()
    rs.CHECKS.update(CHECKS)
    return rs.main(argv)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
