#!/usr/bin/env python3
"""segment_clear (mdh_device.h, MDH_VIS_CLEAR) restated in numpy, and what it clears in the headline room.

The bound is evaluated in float32 with the kernel's operations in the kernel's order; the march (raycast_visibility,
raymarching.glsl:39-56) likewise.  Run as a script it samples the exposed surfaces of the global_illumination room
evenly by area, traces every distinct probe-visibility ray of each point (the cage corners that the clamp to the
probe grid does not fold), and reports:
  - the share of the rays that still need a march (behind the immediate outcomes) which the bound clears,
  - the share of the march steps those rays account for,
  - the cases where the bound says "clear" but the march's own fp32 positions or a dense fp32 walk of the segment
    fall below EPS (there must be none).

    python scripts/vis_clearance.py [--points N] [--seed S]
"""
import argparse
import sys

import numpy as np

f32 = np.float32
EPS = f32(0.001)
MIN_STEP = f32(0.05)

# the room of examples.global_illumination / light_shafts: six axis planes as (axis, sign, offset) -- the SDF of
# plane (n, o) is dot(n, x) + o -- one sphere and one box
ROOM = dict(
    planes=[(1, 1, 1.0), (1, -1, 7.0), (0, 1, 1.0), (0, -1, 7.0), (2, 1, 6.0), (2, -1, 7.0)],
    spheres=[((3.0, 4.0, 3.0), 1.0)],
    boxes=[((3.0, 0.0, 4.0), (1.5, 1.5, 1.5))],
    max_dist=20.0,
)
PROBE_SPACING = (0.95, 0.95, 0.9)
PROBE_DIMS = (8, 8, 8)


def scene_arrays(scene):
    """The scene as the kernels hold it: six folded axis offsets (+inf where none), general planes, spheres, boxes."""
    off = np.full(6, np.inf, f32)
    gplanes = []
    for p in scene["planes"]:
        if len(p) == 3:
            a, sgn, o = p
            g = 2 * a + (0 if sgn > 0 else 1)
            off[g] = min(off[g], f32(o))
        else:
            gplanes.append(p)
    gp = np.array([list(n) + [o] for n, o in gplanes], f32).reshape(-1, 4)
    sp = np.array([list(c) + [r] for c, r in scene["spheres"]], f32).reshape(-1, 4)
    bx = np.array([list(c) + list(e) for c, e in scene["boxes"]], f32).reshape(-1, 6)
    return dict(off=off, gplanes=gp, spheres=sp, boxes=bx, max_dist=f32(scene["max_dist"]))


def margins(sc):
    """commit_scene's threshold EPS + delta (0: off) and coordinate bound lim."""
    vals = [v for v in sc["off"] if np.isfinite(v)] + list(sc["gplanes"].ravel()) + list(sc["spheres"].ravel()) + list(sc["boxes"].ravel())
    vals = np.array(vals, f32)
    on = bool(np.all(np.isfinite(vals))) and bool(np.all(sc["spheres"][:, 3] >= 0)) and bool(np.all(sc["boxes"][:, 3:] >= 0))
    M = f32(np.max(np.abs(vals))) if len(vals) else f32(0)
    lim = f32(f32(2) * f32(M + f32(1)))
    thr = f32(f32(0.001) + f32(np.ldexp(np.float32(1) + lim, -12)))
    on = on and np.isfinite(lim) and np.isfinite(thr) and sc["max_dist"] > thr
    return (thr if on else f32(0)), lim


def sdf(sc, x):
    """closest_primitive in float32 (x: [..., 3])."""
    x = x.astype(f32)
    c = np.full(x.shape[:-1], sc["max_dist"], f32)
    o = sc["off"]
    for a in range(3):
        c = np.minimum(c, np.minimum(x[..., a] + o[2 * a], -x[..., a] + o[2 * a + 1]))
    for p in sc["gplanes"]:
        c = np.minimum(c, (x[..., 0] * p[0] + x[..., 1] * p[1]) + x[..., 2] * p[2] + p[3])
    for s in sc["spheres"]:
        d = x - s[:3]
        c = np.minimum(c, np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) - s[3])
    for b in sc["boxes"]:
        q = np.abs(b[:3] - x) - b[3:]
        m = np.maximum(q[..., 0], np.maximum(q[..., 1], q[..., 2]))
        qp = np.maximum(q, f32(0))
        c = np.minimum(c, np.sqrt((qp[..., 0] * qp[..., 0] + qp[..., 1] * qp[..., 1]) + qp[..., 2] * qp[..., 2]) + np.minimum(m, f32(0)))
    return c


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def segment_clear(sc, thr, lim, A, vd, vmax):
    """The kernel's bound, float32, vectorised over rays (A, vd: [n, 3], vmax: [n]).  True = proved unblocked."""
    with np.errstate(invalid="ignore", over="ignore"):
        A = A.astype(f32); vd = vd.astype(f32); vmax = vmax.astype(f32)
        B = A + vd * vmax[:, None]
        ok = np.full(len(A), thr > 0)
        ok &= np.all(np.abs(A) <= lim, axis=1) & np.all(np.abs(B) <= lim, axis=1)
        lo, hi = np.fmin(A, B), np.fmax(A, B)
        o = sc["off"]
        pl = np.fmin(lo[:, 0] + o[0], -hi[:, 0] + o[1])
        pl = np.fmin(pl, np.fmin(lo[:, 1] + o[2], -hi[:, 1] + o[3]))
        pl = np.fmin(pl, np.fmin(lo[:, 2] + o[4], -hi[:, 2] + o[5]))
        for p in sc["gplanes"]:
            pl = np.fmin(pl, np.fmin(dot(A, p[:3]) + p[3], dot(B, p[:3]) + p[3]))
        ok &= pl > thr
        for s in sc["spheres"]:
            w = s[:3] - A
            t = np.fmin(np.fmax(dot(w, vd), f32(0)), vmax)
            q = w - vd * t[:, None]
            rt = s[3] + thr
            ok &= dot(q, q) > rt * rt
        hv = vd * (vmax * f32(0.5))[:, None]
        ah = np.abs(hv)
        for b in sc["boxes"]:
            m = (A + hv) - b[:3]
            e = b[3:] + thr
            am = np.abs(m)
            sep = (am[:, 0] > e[0] + ah[:, 0]) | (am[:, 1] > e[1] + ah[:, 1]) | (am[:, 2] > e[2] + ah[:, 2])
            sep |= np.abs(m[:, 1] * hv[:, 2] - m[:, 2] * hv[:, 1]) > e[1] * ah[:, 2] + e[2] * ah[:, 1]
            sep |= np.abs(m[:, 2] * hv[:, 0] - m[:, 0] * hv[:, 2]) > e[2] * ah[:, 0] + e[0] * ah[:, 2]
            sep |= np.abs(m[:, 0] * hv[:, 1] - m[:, 1] * hv[:, 0]) > e[0] * ah[:, 1] + e[1] * ah[:, 0]
            ok &= sep
    return ok


def march(sc, A, vd, vmax, sd0, max_steps=100000):
    """raycast_visibility in float32 with the shared first step: (vis, steps, minimum SDF value met)."""
    n = len(A)
    total = np.zeros(n, f32)
    vis = np.ones(n, bool)
    steps = np.zeros(n, np.int64)
    mins = np.full(n, np.inf, f32)
    live = total < vmax
    first = True
    for _ in range(max_steps):
        if not live.any():
            break
        idx = np.nonzero(live)[0]
        sd = sd0[idx] if first else sdf(sc, A[idx] + vd[idx] * total[idx, None])
        first = False
        steps[idx] += 1
        mins[idx] = np.minimum(mins[idx], sd)
        blocked = sd < EPS
        vis[idx[blocked]] = False
        total[idx] = total[idx] + sd
        live[idx] = ~blocked & (total[idx] < vmax[idx])
    return vis, steps, mins


def dense_min(sc, A, vd, vmax, samples=2048):
    """The minimum of the SDF over a dense float32 walk of each segment [A, A + vd vmax]."""
    out = np.full(len(A), np.inf, f32)
    ts = np.linspace(0.0, 1.0, samples, dtype=f32)
    for k in range(0, samples, 256):
        t = vmax[:, None] * ts[None, k:k + 256]
        out = np.minimum(out, sdf(sc, A[:, None, :] + vd[:, None, :] * t[..., None]).min(axis=1))
    return out


def segment_min64(sc, A, vd, vmax, iters=64):
    """The minimum of the scene's SDF over each segment A + vd t, 0 <= t <= max(vmax, 0), in float64 with the float32 inputs
    taken as exact: planes at the nearer endpoint, spheres at the exact closest point, boxes by golden-section search (each
    primitive's SDF is convex along a line, so the search meets the minimum to ~0.618^iters of the segment's length)."""
    A = np.asarray(A, np.float64); vd = np.asarray(vd, np.float64)
    T = np.maximum(np.asarray(vmax, np.float64), 0.0)
    B = A + vd * T[:, None]
    out = np.full(len(A), float(sc["max_dist"]))
    o = sc["off"].astype(np.float64)
    for a in range(3):
        out = np.minimum(out, np.minimum(np.minimum(A[:, a], B[:, a]) + o[2 * a], -np.maximum(A[:, a], B[:, a]) + o[2 * a + 1]))
    for p in sc["gplanes"].astype(np.float64):
        out = np.minimum(out, np.minimum(A @ p[:3] + p[3], B @ p[:3] + p[3]))
    vv = np.einsum("ij,ij->i", vd, vd)
    for s in sc["spheres"].astype(np.float64):
        w = s[:3] - A
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.clip(np.where(vv > 0, np.einsum("ij,ij->i", w, vd) / vv, 0.0), 0.0, T)
        out = np.minimum(out, np.linalg.norm(w - vd * t[:, None], axis=1) - s[3])
    for b in sc["boxes"].astype(np.float64):
        def f(t):
            q = np.abs(A + vd * t[:, None] - b[:3]) - b[3:]
            return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)
        g = (np.sqrt(5.0) - 1.0) / 2.0
        lo, hi = np.zeros_like(T), T.copy()
        c, d = hi - g * (hi - lo), lo + g * (hi - lo)
        fc, fd = f(c), f(d)
        best = np.minimum(np.minimum(f(lo), f(hi)), np.minimum(fc, fd))
        for _ in range(iters):
            left = fc < fd  # the minimum lies in [lo, d]
            hi = np.where(left, d, hi); lo = np.where(left, lo, c)
            nc, nd = np.where(left, hi - g * (hi - lo), d), np.where(left, c, lo + g * (hi - lo))
            fn = f(np.where(left, nc, nd))
            fc, fd = np.where(left, fn, fd), np.where(left, fc, fn)
            c, d = nc, nd
            best = np.minimum(best, fn)
        out = np.minimum(out, best)
    return out


def room_points(rng, n):
    """Points of the room's exposed surfaces, evenly by area, with their normals."""
    pts, nrm = [], []
    # the six walls (inside faces)
    walls = [(1, -1.0, (1, 0, 0), 1), (1, 7.0, (1, 0, 0), -1), (0, -1.0, (0, 1, 0), 1), (0, 7.0, (0, 1, 0), -1), (2, -6.0, (0, 0, 1), 1), (2, 7.0, (0, 0, 1), -1)]
    lo, hi = np.array([-1.0, -1.0, -6.0]), np.array([7.0, 7.0, 7.0])
    sphere_c, sphere_r = np.array([3.0, 4.0, 3.0]), 1.0
    box_c, box_e = np.array([3.0, 0.0, 4.0]), np.array([1.5, 1.5, 1.5])
    ext = hi - lo
    areas = []
    for a, v, _, s in walls:
        o = [b for b in range(3) if b != a]
        areas.append(ext[o[0]] * ext[o[1]])
    areas.append(4 * np.pi * sphere_r ** 2)
    areas.append(8 * (box_e[0] * box_e[2] + box_e[0] * box_e[1] + box_e[1] * box_e[2]))
    areas = np.array(areas)
    counts = rng.multinomial(n, areas / areas.sum())
    for (a, v, _, s), c in zip(walls, counts[:6]):
        p = lo + rng.random((c, 3)) * ext
        p[:, a] = v
        nn = np.zeros((c, 3)); nn[:, a] = s
        pts.append(p); nrm.append(nn)
    d = rng.normal(size=(counts[6], 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts.append(sphere_c + sphere_r * d); nrm.append(d)
    c = counts[7]
    face = rng.integers(0, 6, c)
    u = rng.random((c, 3)) * 2 - 1
    ax, sg = face // 2, np.where(face % 2 == 0, 1.0, -1.0)
    u[np.arange(c), ax] = sg
    nn = np.zeros((c, 3)); nn[np.arange(c), ax] = sg
    pts.append(box_c + u * box_e); nrm.append(nn)
    P = np.concatenate(pts); N = np.concatenate(nrm)
    # keep what is inside the room and outside the other solids (the box's bottom, the floor under it are hidden)
    inside = np.all((P >= lo - 1e-9) & (P <= hi + 1e-9), axis=1)
    keep = inside & (np.linalg.norm(P - sphere_c, axis=1) >= sphere_r - 1e-9) & ~np.all(np.abs(P - box_c) < box_e - 1e-9, axis=1)
    keep &= P[:, 1] >= -1.0
    return P[keep].astype(f32), N[keep].astype(f32)


def visibility_rays(P, N, spacing=PROBE_SPACING, dims=PROBE_DIMS):
    """Every distinct probe-visibility ray of each point: (A, vd, vmax, point index)."""
    s = np.array(spacing, f32)
    g = np.array(dims)
    base = np.floor(P / s).astype(np.int64)
    A_all, vd_all, vm_all, own = [], [], [], []
    for i in range(8):
        bits = np.array([(i >> a) & 1 for a in range(3)])
        q = np.clip(base + bits, 0, g - 1)
        A_all.append(q); own.append(np.arange(len(P)))
    q = np.concatenate(A_all); own = np.concatenate(own)
    # distinct probes per point
    key = np.unique(np.concatenate([own[:, None], q], axis=1), axis=0)
    own, q = key[:, 0], key[:, 1:]
    pw = (q.astype(f32) * s).astype(f32)
    Pp, Np = P[own], N[own]
    hvec = (pw - Pp).astype(f32)
    dist = np.sqrt(dot(hvec, hvec)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        vd = (hvec / dist[:, None]).astype(f32)
    vmax = (dist - MIN_STEP * f32(5)).astype(f32)
    A = (Pp + (Np * MIN_STEP) * f32(5)).astype(f32)
    return A, vd, vmax, own


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=5)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(a.seed)
    sc = scene_arrays(ROOM)
    thr, lim = margins(sc)
    P, N = room_points(rng, a.points)
    A, vd, vmax, _ = visibility_rays(P, N)
    sd0 = sdf(sc, A)
    need = (vmax > 0) & ~(sd0 < EPS) & (sd0 < vmax)
    A, vd, vmax, sd0 = A[need], vd[need], vmax[need], sd0[need]
    clear = segment_clear(sc, thr, lim, A, vd, vmax)
    vis, steps, mins = march(sc, A, vd, vmax, sd0)
    dmin = dense_min(sc, A[clear], vd[clear], vmax[clear])
    bad_march = int(np.sum(clear & ~vis)) + int(np.sum(mins[clear] < EPS))
    bad_dense = int(np.sum(dmin < EPS))
    print(f"threshold EPS + delta = {float(thr):.6f}, lim = {float(lim):g}")
    print(f"points {len(P)}, distinct visibility rays that need a march {len(A)}")
    print(f"cleared rays        {clear.sum()} / {len(A)} = {clear.mean():.1%}")
    print(f"their march steps   {steps[clear].sum()} / {steps.sum()} = {steps[clear].sum() / max(1, steps.sum()):.1%}")
    print(f"mean steps: cleared {steps[clear].mean():.2f}, not cleared {steps[~clear].mean() if (~clear).any() else 0:.2f}")
    print(f"blocked rays {int((~vis).sum())}, of them cleared {int((clear & ~vis).sum())}")
    print(f"unsound cases: march {bad_march}, dense walk {bad_dense} (minimum over cleared segments {float(dmin.min()) if len(dmin) else float('inf'):.5f})")
    return 1 if bad_march or bad_dense else 0


if __name__ == "__main__":
    sys.exit(main())
