"""Small procedural triangle meshes for scenes of the size of the reference's obj_mesh example
(examples/obj_mesh/main.adb: 1000 triangles).  There is no file loader: the
generators stand in for `Meshes.Obj_Loader.Load_Obj_File` + `Meshes.Iterate_Triangles`.

Every generator returns a float32 array [n, 3, 3]: n triangles of three vertices, in a fixed order.
The arithmetic is float64 numpy on integer grids rounded once to float32, so the same call gives the
same bits everywhere.
"""
import numpy as np


def _quads_to_triangles(P, wrap_u, wrap_v):
    """P[i, j] = vertex (i, j) of a quad grid; two triangles per quad, quads in (i, j) order."""
    nu = P.shape[0] if wrap_u else P.shape[0] - 1
    nv = P.shape[1] if wrap_v else P.shape[1] - 1
    tris = np.empty((nu * nv * 2, 3, 3), dtype=np.float32)
    n = 0
    for i in range(nu):
        i1 = (i + 1) % P.shape[0]
        for j in range(nv):
            j1 = (j + 1) % P.shape[1]
            a, b, c, d = P[i, j], P[i1, j], P[i1, j1], P[i, j1]
            tris[n] = (a, b, c)
            tris[n + 1] = (a, c, d)
            n += 2
    return tris


def torus(nu=25, nv=20, R=0.6, r=0.25, axis=1):
    """A torus of nu x nv quads (2 nu nv triangles: 25 x 20 gives exactly 1000) around the origin:
    ring radius R, tube radius r, `axis` = the coordinate its axis of symmetry runs along."""
    u = 2.0 * np.pi * np.arange(nu, dtype=np.float64) / nu
    v = 2.0 * np.pi * np.arange(nv, dtype=np.float64) / nv
    U, V = np.meshgrid(u, v, indexing="ij")
    ring = R + r * np.cos(V)
    a, b, h = ring * np.cos(U), ring * np.sin(U), r * np.sin(V)
    comps = {0: (h, a, b), 1: (b, h, a), 2: (a, b, h)}[axis]
    P = np.stack(comps, axis=-1).astype(np.float32)
    return _quads_to_triangles(P, True, True)


def sheet(nu=25, nv=20, size=(2.9, 1.9), height=0.35, waves=(1.5, 1.0)):
    """A height field of nu x nv quads (2 nu nv triangles) centred on the origin: x in +-size[0]/2,
    y in +-size[1]/2, z = height * sin (waves[0] pi s) * cos (waves[1] pi t) over the unit square.
    Spread over a whole grid it has no point that hundreds of its triangles are equally far from."""
    s = np.arange(nu + 1, dtype=np.float64) / nu
    t = np.arange(nv + 1, dtype=np.float64) / nv
    S, T = np.meshgrid(s, t, indexing="ij")
    x = (S - 0.5) * size[0]
    y = (T - 0.5) * size[1]
    z = height * np.sin(waves[0] * np.pi * S) * np.cos(waves[1] * np.pi * T)
    P = np.stack((x, y, z), axis=-1).astype(np.float32)
    return _quads_to_triangles(P, False, False)


def degenerate(tris, eps=1e-12):
    """Indices of triangles whose area (in float64) is not above eps."""
    t = np.asarray(tris, dtype=np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return np.nonzero(0.5 * np.sqrt((n * n).sum(axis=1)) <= eps)[0]


def Write_Obj(path, positions, quads, normals=None):
    """A quad mesh as Wavefront OBJ text: positions (V, 3), quads (Q, 4) of vertex ids counted from 0 -- what
    Renderer.Surface_Mesh returns -- and optionally a normal per vertex.  %.9g round-trips a float32."""
    with open(path, "w") as f:
        for p in np.asarray(positions, dtype=np.float32):
            f.write("v %.9g %.9g %.9g\n" % tuple(p))
        if normals is not None:
            for n in np.asarray(normals, dtype=np.float32):
                f.write("vn %.9g %.9g %.9g\n" % tuple(n))
        fmt = "f %d//%d %d//%d %d//%d %d//%d\n" if normals is not None else "f %d %d %d %d\n"
        for q in np.asarray(quads, dtype=np.int64) + 1:
            f.write(fmt % (tuple(np.repeat(q, 2)) if normals is not None else tuple(q)))
