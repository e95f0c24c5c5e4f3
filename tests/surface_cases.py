"""The yardstick of the surface mesher's tests (tests/test_surface_mesh_host.py on the CPU, tests/test_gpu_surface_mesh.py and
tests/surface_device_checks.py on the device): the definition of mdh_surface_mesh (include/madarch_hip.h) restated in
vectorised numpy float32, one astype per operation, over a distance D (points) -> (distances, ..) as sweep_cases.chain takes
it -- sw.whole_scene (orc, Ro) for the whole scene, sw.listed (Ro, kinds) for listed kinds -- and a checker of the quads'
topology.  tests/test_surface_mesh_host.py holds the restatement itself against analytic distances."""
import numpy as np

F = np.float32


def corner_points(origin, h, cells):
    """the grid's corners, x fastest: p = origin + (float) i * h, one product then one sum -> ((cz + 1) (cy + 1) (cx + 1), 3)"""
    origin, h = np.asarray(origin, F), F(h)
    axes = [(origin[c] + (np.arange(cells[c] + 1).astype(F) * h).astype(F)).astype(F) for c in range(3)]
    Z, Y, X = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack((X.ravel(), Y.ravel(), Z.ravel()), axis=1))


def corner_offsets(a, e):
    """edge e = 0 .. 3 along axis a: the two other axes in ascending order take the offsets e & 1 and e >> 1"""
    others = [x for x in range(3) if x != a]
    off = [0, 0, 0]
    off[others[0]], off[others[1]] = e & 1, e >> 1
    return off


def surface_nets(D, origin, h, cells, iso=0.0):
    """-> {field (cz + 1, cy + 1, cx + 1), positions (V, 3), quads (Q, 4), counts, cells (V, 3): each vertex's cell (i, j, k),
    border_crossings: crossing grid edges that emit no quad because a cell round them does not exist}"""
    origin, h, iso = np.asarray(origin, F), F(h), F(iso)
    cx, cy, cz = (int(c) for c in cells)
    nx, ny, nz = cx + 1, cy + 1, cz + 1
    d = np.asarray(D(corner_points(origin, h, cells))[0], F)
    field = (d - iso).astype(F).reshape(nz, ny, nx)
    inside = field < 0.0  # (zero and NaN are outside)
    # the cells' eight corners: bit 0 of c the x offset, bit 1 the y offset, bit 2 the z offset
    corner = lambda a, c: a[(c >> 2) & 1:((c >> 2) & 1) + cz, (c >> 1) & 1:((c >> 1) & 1) + cy, (c & 1):(c & 1) + cx]
    v = [corner(field, c) for c in range(8)]
    ins = [corner(inside, c) for c in range(8)]
    n_in = sum(i.astype(np.int32) for i in ins)
    active = (n_in > 0) & (n_in < 8)
    s = [np.zeros((cz, cy, cx), F) for _ in range(3)]
    m = np.zeros((cz, cy, cx), np.int32)
    with np.errstate(all="ignore"):
        for a in range(3):
            for e in range(4):
                off = corner_offsets(a, e)
                c0 = off[0] | off[1] << 1 | off[2] << 2
                c1 = c0 | 1 << a
                cross = ins[c0] != ins[c1]
                t = (v[c0] / (v[c0] - v[c1]).astype(F)).astype(F)
                for comp in range(3):
                    q = t if comp == a else F(off[comp])
                    s[comp] = np.where(cross, (s[comp] + q).astype(F), s[comp])
                m += cross
        K, J, I = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing="ij")
        pos = []
        for comp, ix in enumerate((I, J, K)):
            u = (s[comp] / m.astype(F)).astype(F)
            pos.append((origin[comp] + ((ix.astype(F) + u).astype(F) * h).astype(F)).astype(F))
    on = active.ravel()  # (cell ids ascend in this order: (k cy + j) cx + i)
    positions = np.stack([p.ravel()[on] for p in pos], axis=1)
    vertex = np.full(cx * cy * cz, -1, np.int64)
    vertex[on] = np.arange(on.sum())
    vertex = vertex.reshape(cz, cy, cx)
    # the quads: a grid edge along a from corner (i, j, k)
    Kc, Jc, Ic = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    coords, ncell = (Ic, Jc, Kc), (cx, cy, cz)
    cornerid = (Kc * ny + Jc) * nx + Ic
    keys, quads, border = [], [], 0
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        along = coords[a] < ncell[a]
        shift = [0, 0, 0]
        shift[a] = 1
        upper = np.zeros_like(inside)
        sl_lo = tuple(slice(0, n - sh) for n, sh in zip((nz, ny, nx), shift[::-1]))
        sl_hi = tuple(slice(sh, n) for n, sh in zip((nz, ny, nx), shift[::-1]))
        upper[sl_lo] = inside[sl_hi]
        crossing = along & (upper != inside)
        interior = (coords[b] >= 1) & (coords[b] <= ncell[b] - 1) & (coords[c] >= 1) & (coords[c] <= ncell[c] - 1)
        border += int((crossing & ~interior).sum())
        emit = np.nonzero((crossing & interior).ravel())[0]
        at = [co.ravel()[emit] for co in coords]
        ids = []
        for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            cell = [x.copy() for x in at]
            cell[b] = cell[b] + ob
            cell[c] = cell[c] + oc
            ids.append(vertex[cell[2], cell[1], cell[0]])
        ids = np.stack(ids, axis=1)
        lower_inside = inside.ravel()[emit]
        quads.append(np.where(lower_inside[:, None], ids, ids[:, ::-1]))
        keys.append(cornerid.ravel()[emit] * 3 + a)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    order = np.argsort(keys, kind="stable")
    quads = quads[order].astype(np.int32)
    assert (quads >= 0).all()  # (a crossing edge's four cells are active)
    where = np.stack([x.ravel()[on] for x in (I, J, K)], axis=1)
    return {"field": field, "positions": positions, "quads": quads, "counts": np.array([len(positions), len(quads)], np.int32),
            "cells": where, "border_crossings": border}


def topology(quads, n_vertices=None):
    """the quads' directed edges -> {closed: every directed edge once and its reverse once, unmatched: the directed edges
    without their reverse (n, 2), repeated: directed edges that occur twice, chi: V - E + F over the vertices the quads use,
    components: connected components, component_chi: V - E + F of each}"""
    quads = np.asarray(quads, np.int64).reshape(-1, 4)
    e = np.concatenate([np.stack((quads[:, n], quads[:, (n + 1) % 4]), axis=1) for n in range(4)])
    big = int(quads.max()) + 1 if len(quads) else 1
    key, rev = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    repeated = int((counts > 1).sum())
    unmatched = e[~np.isin(rev, key)]
    und = np.unique(np.minimum(key, rev))
    used = np.unique(quads)
    # connected components: labels propagated along the edges until they stand still
    label = np.arange(big)
    while True:
        lo = np.minimum(label[e[:, 0]], label[e[:, 1]])
        new = label.copy()
        np.minimum.at(new, e[:, 0], lo)
        np.minimum.at(new, e[:, 1], lo)
        if np.array_equal(new, label):
            break
        label = new
    roots = np.unique(label[used])
    comp_chi = []
    for r in roots:
        fq = label[quads[:, 0]] == r
        eu = np.minimum(key, rev)[np.repeat(fq[None, :], 4, axis=0).ravel()] if len(quads) else und[:0]
        comp_chi.append(int((label[used] == r).sum()) - len(np.unique(eu)) + int(fq.sum()))
    return {"closed": repeated == 0 and len(unmatched) == 0, "unmatched": unmatched, "repeated": repeated,
            "chi": len(used) - len(und) + len(quads), "components": len(roots), "component_chi": comp_chi}


def on_border(cell_ijk, cells):
    """is the cell on the grid's border?"""
    c = np.asarray(cell_ijk)
    return ((c == 0) | (c == np.asarray(cells) - 1)).any(axis=-1)
