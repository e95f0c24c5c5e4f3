"""Meshes, scenes and the builder's ctypes view for the tests of MDH_OPT_TRIANGLE_BVH (tests/test_triangle_bvh_build.py on the
CPU, tests/test_gpu_triangle_bvh.py on the device)."""
import ctypes as C

import numpy as np

from helpers import SEED, SMALL_PROBES, SMALL_VOL
from madarch_amd import _binding as B
from madarch_amd import materials, meshes, renderers, scenes, windows
from madarch_amd.lights import point_lights
from madarch_amd.primitives import boxes, planes, spheres, triangles

NODE = np.dtype([("lo", "<f4", 3), ("skip", "<i4"), ("hi", "<f4", 3), ("leaf", "<i4")])
assert NODE.itemsize == 32


def bvh_build(tris):
    """mdh_bvh_build on [n, 3, 3] float32 -> (nodes, walked part of perm, always-evaluated list, delta, rho)"""
    b = B.hip_binding()
    t = np.ascontiguousarray(np.asarray(tris, dtype=np.float32).reshape(-1, 9))
    n = len(t)
    nodes = np.zeros(max(1, 2 * n), dtype=NODE)
    perm = np.full(max(1, n), -1, dtype=np.int32)
    n_nodes = C.c_int32(-1)
    dr = np.zeros(2, dtype=np.float32)
    always = b.bvh_build(t.ctypes.data, n, nodes.ctypes.data, C.byref(n_nodes), perm.ctypes.data, dr.ctypes.data)
    assert always >= 0, always
    return nodes[:n_nodes.value].copy(), perm[:n - always].copy(), perm[n - always:n].copy(), float(dr[0]), float(dr[1])


def tri_distance64(P, T):
    """float64 distance of points P [m, 3] to triangles T [n, 3, 3] -> [m, n]: the closer of the three edges and, where the
    foot point lies inside a triangle of non-zero area, its plane"""
    P = np.asarray(P, dtype=np.float64)[:, None, :]
    T = np.asarray(T, dtype=np.float64)
    a, b, c = T[None, :, 0], T[None, :, 1], T[None, :, 2]

    def seg(u, v):
        d = v - u
        dd = (d * d).sum(-1)
        t = np.where(dd > 0.0, ((P - u) * d).sum(-1) / np.where(dd > 0.0, dd, 1.0), 0.0)
        w = u + d * np.clip(t, 0.0, 1.0)[..., None] - P
        return (w * w).sum(-1)
    best = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    nor = np.cross(b - a, c - a)
    nn = (nor * nor).sum(-1)
    ok = nn > 0.0
    nn1 = np.where(ok, nn, 1.0)
    pa = P - a
    h = (pa * nor).sum(-1)
    # barycentric coordinates of the foot point
    u = (np.cross(b - a, pa) * nor).sum(-1) / nn1
    v = (np.cross(pa, c - a) * nor).sum(-1) / nn1
    inside = ok & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0)
    return np.sqrt(np.where(inside, np.minimum(best, h * h / nn1), best))


def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross32(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), -1)


def sd_triangle32(T, P):
    """mdh_device.h: sd_triangle in numpy float32, operation for operation (every numpy operation on float32 arrays is one
    correctly rounded fp32 operation, the square root included): points P [m, 3] x triangles T [n, 3, 3] -> [m, n]"""
    T, P = np.asarray(T, dtype=np.float32), np.asarray(P, dtype=np.float32)
    a, b, c, p = T[None, :, 0], T[None, :, 1], T[None, :, 2], P[:, None, :]
    v21, v32, v13 = b - a, c - b, a - c
    p1, p2, p3 = p - a, p - b, p - c
    nor = _cross32(v21, v13)
    one, zero = np.float32(1.0), np.float32(0.0)
    with np.errstate(all="ignore"):
        s = (np.sign(_dot32(_cross32(v21, nor), p1)) + np.sign(_dot32(_cross32(v32, nor), p2))) + np.sign(_dot32(_cross32(v13, nor), p3))

        def edge(v, q):
            t = np.fmin(np.fmax(_dot32(v, q) / _dot32(v, v), zero), one)  # (fmax / fmin: a NaN quotient clamps to 0, as minNum / maxNum)
            w = v * t[..., None] - q
            return _dot32(w, w)
        e = np.fmin(np.fmin(edge(v21, p1), edge(v32, p2)), edge(v13, p3))
        face = _dot32(nor, p1) * _dot32(nor, p1) / _dot32(nor, nor)
        return np.sqrt(np.where(s < np.float32(2.0), e, face)).astype(np.float32)


def degenerate_mesh():
    """twenty triangles in front of a camera at the origin: eighteen of a small torus, then a zero-area one (index 18: three
    points on a line) and a sliver whose smallest angle is 1e-4 rad (index 19)"""
    t = meshes.torus(3, 3, R=1.6, r=0.9, axis=2) + np.asarray((0.0, 0.0, 3.0), dtype=np.float32)
    flat = np.asarray([[(-1.0, -1.0, 3.0), (0.0, 0.0, 3.0), (1.0, 1.0, 3.0)]], dtype=np.float32)
    sliver = np.asarray([[(-1.5, 1.0, 3.5), (1.5, 1.0, 3.5), (1.5, 1.0 + 3.0e-4, 3.5)]], dtype=np.float32)
    return np.concatenate((t, flat, sliver)).astype(np.float32)


def coincident_mesh():
    """two coincident triangles (different materials in the scenes) facing a camera at the origin"""
    one = np.asarray([[(-3.0, -2.0, 3.0), (3.0, -2.0, 3.0), (0.0, 3.0, 3.0)]], dtype=np.float32)
    return np.concatenate((one, one))


def fan(n):
    """n triangles around (0, 0, 3), facing a camera at the origin"""
    if n == 1:
        return np.asarray([((-2.5, -1.5, 3.0), (2.5, -1.5, 3.3), (0.0, 2.2, 2.8))], dtype=np.float32)
    out = []
    for i in range(n):
        a0, a1 = 2.0 * np.pi * i / n, 2.0 * np.pi * (i + 0.8) / n
        out.append(((0.0, 0.0, 3.0 + 0.1 * i), (2.5 * np.cos(a0), 2.5 * np.sin(a0), 3.2), (2.5 * np.cos(a1), 2.5 * np.sin(a1), 2.9)))
    return np.asarray(out, dtype=np.float32)


def facing_torus(nu, nv):
    """a torus whose ring faces a camera at the origin"""
    return meshes.torus(nu, nv, R=1.3, r=0.55, axis=2) + np.asarray((0.0, 0.0, 3.0), dtype=np.float32)


def fuzz_mesh(seed):
    """8 - 120 triangles: a cluster in front of a camera at the origin, strays out to +-50, some with edges below 1e-3,
    some sharing vertices with their predecessor"""
    rng = np.random.RandomState((SEED + 7919 * seed) & 0x7FFFFFFF)
    n = int(rng.randint(8, 121))
    out = []
    for i in range(n):
        kind = rng.randint(0, 10) if i >= 2 else 9
        if i < 2:  # two large ones in view, so that every scene is hit
            c = np.array((rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(3.0, 5.0)))
            size = rng.uniform(2.5, 4.0)
        elif kind == 0:  # a stray, anywhere
            c = rng.uniform(-50.0, 50.0, 3)
            size = rng.uniform(0.5, 8.0)
        else:
            z = rng.uniform(2.0, 9.0)
            c = np.array((rng.uniform(-0.5, 0.5) * z, rng.uniform(-0.4, 0.4) * z, z))
            size = rng.uniform(0.3, 2.5)
        v = c + rng.uniform(-1.0, 1.0, (3, 3)) * size
        if kind == 1:  # an edge below 1e-3
            v[1] = v[0] + rng.uniform(-1.0, 1.0, 3) * 4.0e-4
        elif kind == 2:  # nearly a line
            v[2] = v[0] + (v[1] - v[0]) * rng.uniform(0.2, 0.8) + rng.uniform(-1.0, 1.0, 3) * 1.0e-5
        elif kind in (3, 4) and out:  # shares an edge with the triangle before it
            v[0], v[1] = out[-1][1], out[-1][2]
        out.append(np.clip(v, -50.0, 50.0))
    return np.asarray(out, dtype=np.float32)


def tri_renderer(binding, tris, bvh, mats=None, others=False, vol=False, W=64, H=48, camera=(0.0, 0.0, 0.0), spare=0):
    """a scene of triangles without a partition; `others`: two general planes, three spheres and two boxes beside them"""
    tris = np.asarray(tris, dtype=np.float32)
    kinds = [(triangles.Triangle, len(tris) + spare)]
    if others:
        kinds = [(planes.Plane, 4), (spheres.Sphere, 4), (boxes.Box, 3)] + kinds
    scene = scenes.Compile(kinds, [(point_lights.Point_Light, 4)], Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(W, H), scene, Probes=SMALL_PROBES, Volumetrics=SMALL_VOL if vol else renderers.No_Volumetrics, Binding=binding)
    if bvh is not None:
        R.Set_Option(B.OPT_TRIANGLE_BVH, 1 if bvh else 0)
    m = [R.Add_Material(materials.Create(a, me, ro)) for a, me, ro in (((0.8, 0.2, 0.1), 0.0, 1.0), ((0.1, 0.3, 0.9), 0.3, 0.5), ((0.5, 0.5, 0.5), 0.0, 0.8))]
    if others:
        R.Add_Primitive(planes.Plane, planes.Create((0.0, 0.8, -0.6), 4.0, m[2]))
        R.Add_Primitive(planes.Plane, planes.Create((0.6, 0.0, -0.8), 7.0, m[2]))
        for c, rad in (((-1.5, 0.5, 3.5), 0.6), ((1.8, -0.8, 4.0), 0.7), ((0.3, 1.6, 5.0), 0.5)):
            R.Add_Primitive(spheres.Sphere, spheres.Create(c, rad, m[1]))
        for c, s in (((-0.5, -1.5, 4.5), (0.6, 0.4, 0.5)), ((2.0, 1.5, 5.5), (0.5, 0.5, 0.5))):
            R.Add_Primitive(boxes.Box, boxes.Create(c, s, m[1]))
    for i, (a, b, c) in enumerate(tris):
        R.Add_Primitive(triangles.Triangle, triangles.Create(a, b, c, m[0] if mats is None else m[mats[i]]))
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create((0.5, 2.0, -1.0), (0.9, 0.9, 0.9)))
    R.Set_Camera_Position(camera)
    R.Set_Option(B.OPT_GBUFFER, 1)
    return R
