"""An independent float64 renderer, written from the reference's GLSL and Ada text, and the helper that holds a frame
of the oracle or of the HIP library against it.

It shares no code with oracle/ or madarch_amd/csrc/ and calls neither: plain numpy, vectorised over rays with masks.
Every function cites the text it restates.  Besides the screen and the radiance pass it restates the irradiance fold
(irradiance_texels), the optional mip chain (radiance_mips), the two volumetric passes (froxel_texels,
scattering_texels) and the volumetric composition of a pixel, and the space partition: the lookup every march goes
through (Scene.closest) and the three builders of its table (partition_build).

The scene is a plain description (a dict; every number is rounded to binary32 first, as the scene buffer holds it):

  kinds      [(name, declared count)] in declared order, names of Sphere / Plane / Box / Triangle: the geometry buffer
             numbers a primitive as (sum of the declared counts of the kinds before its own) + its place in its kind
             (madarch-scenes.adb:631-674)
  prims      [("Sphere", centre, radius, mat) | ("Plane", normal, offset, mat) | ("Box", centre, side, mat) |
              ("Triangle", v1, v2, v3, mat)] in the order they are added
  materials  [(albedo, metallic, roughness)]
  lights     [("point", position, colour) | ("spot", position, direction, aperture, colour)] as the light loop meets them
  max_dist, cam_pos, cam_m (cam_m[i][j] = row i, column j), ao_steps, spec_mode (0 or 2),
  probes     dict (rres, ires, count (x, y), dims (x, y, z), spacing (x, y, z))
  vol        (optional) dict (vres (x, y, z), vstep, sres (x, y), sstep): the volumetric settings; with them and a
             scattering texture, a mode-0 pixel is composed with the fog (volumetrics.glsl:34-54)
  partition  (optional) dict (dims (x, y, z), spacing (x, y, z), offset (x, y, z), index_count, border "Clamp" | "Fallback",
             table): the space partition (madarch-scenes.ads:28-41).  `table` is an int array of cells x (kinds +
             index_count): per cell the number of candidates of each kind in declared order, then their places in their
             kinds' arrays, as the host API reads the buffer back.  With the key, every march looks the distance up in
             the table (raymarching.glsl:9,27,41, lighting.glsl:61); the builders need no table.

Where the reference leaves a value undefined, the project's stated choice is taken and named:
marches are cut after 4096 steps (Q3), an irradiance with no weight at all is 0 (Q11), textureLod (.., 1.0) on the
single-level atlas reads level 0 (Q5), the probe pass has no AO and no added specular (Q12); a partition index past
the table reads an empty cell (Q6: the index is clamped to dims, not dims - 1, and is kept so), a cell's candidate
lists are cut at index_count, in the builders and in the walk (Q7); min and max ignore a NaN operand (GLSL leaves it
undefined, DESIGN.md section 5 "Numerics"): the soft shadow's sqrt (dist * dist - y * y) (raymarching.glsl:16) is a
NaN where the partition makes the distance more than double in one step, and that step leaves the shadow as it was;
a record the GPU builder never writes (odd grids) keeps the zeros the buffer is created with.

Conventions of this project's read-back (not of the reference): row 0 of a framebuffer is the top of the window
(v = +1 side), row 0 of a texture is its normalised y of 0.
"""
import contextlib

import numpy as np

EPS = 0.001                   # maths.glsl:3
MSS = 0.05                    # raymarching.glsl:1
PI = 3.14159265358            # maths.glsl:1
SKY = np.array([0.30, 0.36, 0.60])  # render_probes.glsl:287
MAX_STEPS = 4096
JITTER = 2.0 ** -18           # relative jitter of every ray's origin and direction in the two extra runs
EPS_MARGIN = 2.0 ** -20       # times max (1, largest coordinate): see hold, threshold_margin
KIND_NAMES = ("Sphere", "Plane", "Box", "Triangle")
TAU = 0.1                     # volumetrics.glsl:12
NEAR_SURFACE = 0.02           # test_oracle_pins64.py:180: a froxel's sample point this close to a surface (or inside one)


def r32(x):
    """a number as the scene buffer holds it: rounded to binary32, then exact in float64"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def image6(x):
    """a number that travels through the generated GLSL text: Single'Image keeps six significant digits
    (madarch-renderers.adb:119-134), and the compiler reads them back as a binary32 literal"""
    return float(np.float32(float("%.5E" % float(np.float32(x)))))


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _unit(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / _norm(a)[..., None]


# ------------------------------------------------------------------------------------------- geometry
def triangle_closest_point(a, b, c, P):
    """The point of triangle (a, b, c) closest to each row of P, by region tests on the barycentric coordinates (the
    vertex, edge and face regions of the triangle's Voronoi diagram).  This is the geometric statement, NOT the
    shader's (madarch-primitives-triangles.adb:16-48 is held against it)."""
    ab, ac = b - a, c - a
    ap, bp, cp = P - a, P - b, P - c
    d1, d2 = ap @ ab, ap @ ac
    d3, d4 = bp @ ab, bp @ ac
    d5, d6 = cp @ ab, cp @ ac
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    with np.errstate(invalid="ignore", divide="ignore"):
        den = va + vb + vc
        Q = a + ab * (vb / den)[:, None] + ac * (vc / den)[:, None]                 # the face
        m = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)                            # edge v2 v3
        Q[m] = (b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None])[m]
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)                                      # edge v1 v3
        Q[m] = (a + ac * (d2 / (d2 - d6))[:, None])[m]
        Q[(d6 >= 0) & (d5 <= d6)] = c                                              # vertex v3
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)                                      # edge v1 v2
        Q[m] = (a + ab * (d1 / (d1 - d3))[:, None])[m]
    Q[(d3 >= 0) & (d4 <= d3)] = b                                                  # vertex v2
    Q[(d1 <= 0) & (d2 <= 0)] = a                                                   # vertex v1
    return Q


def triangle_distance(a, b, c, P):
    return _norm(P - triangle_closest_point(a, b, c, P))


class Scene:
    """the description compiled into arrays, primitives in the order the generated scan meets them: kind by kind in
    declared order, each kind in the order its entities were added (madarch-scenes.adb:602-674)"""

    def __init__(self, desc, vol=None):
        self.desc = desc
        vol = desc.get("vol") if vol is None else vol
        if vol is not None:  # volumetrics.glsl:1-10 from madarch-renderers.adb:119-134
            self.vres, self.sres = np.array(vol["vres"], dtype=int), np.array(vol["sres"], dtype=int)
            self.vstep, self.sstep = image6(vol["vstep"]), image6(vol["sstep"])
            # visibility_max_depth (volumetrics.glsl:3-4) is a constant of the shader: the product of two binary32 constants
            self.max_depth = float(np.float32(self.vstep) * np.float32(self.vres[2]))
        self.max_dist = float(r32(desc.get("max_dist", 20.0)))
        base, b = {}, 0
        for name, count in desc["kinds"]:
            base[name] = b
            b += count
        self.prims = []  # (kind, params (float64), material, number in the geometry buffer)
        for name, _ in desc["kinds"]:
            i = 0
            for p in desc["prims"]:
                if p[0] == name:
                    self.prims.append((name, [r32(v) for v in p[1:-1]], int(p[-1]), base[name] + i))
                    i += 1
        self.kind = np.array([KIND_NAMES.index(p[0]) for p in self.prims], dtype=int)
        self.mat = np.array([p[2] for p in self.prims], dtype=int)
        self.number = np.array([p[3] for p in self.prims], dtype=int)
        self.materials = [(r32(a), float(r32(m)), float(r32(r))) for a, m, r in desc["materials"]]
        self.m_albedo = np.array([m[0] for m in self.materials]).reshape(-1, 3)
        self.m_metallic = np.array([m[1] for m in self.materials])
        self.m_rough = np.array([m[2] for m in self.materials])
        self.lights = [(l[0],) + tuple(r32(v) for v in l[1:]) for l in desc.get("lights", [])]
        self.cam_pos = r32(desc.get("cam_pos", (0.0, 0.0, 0.0)))
        self.cam_m = r32(desc.get("cam_m", np.eye(3))).reshape(3, 3)
        pr = desc.get("probes")
        if pr is not None:
            self.rres, self.ires = int(pr["rres"]), int(pr["ires"])
            self.pc, self.dims, self.spacing = np.array(pr["count"], dtype=int), np.array(pr["dims"], dtype=int), r32(pr["spacing"])
        # a primitive's kind (place among the declared kinds) and its place in its kind's array; place[k][i] is back again
        declared = [name for name, _ in desc["kinds"]]
        self.kind_ix = np.array([declared.index(p[0]) for p in self.prims], dtype=int)
        self.place = [[j for j, p in enumerate(self.prims) if p[0] == name] for name in declared]
        self.part = desc.get("partition")
        self.face = None
        if self.part is not None:
            pt = self.part
            self.pdims, self.pcount = np.array(pt["dims"], dtype=int), int(pt["index_count"])
            self.cells = int(self.pdims.prod())
            assert pt["border"] in ("Clamp", "Fallback")
            self.pfallback = pt["border"] == "Fallback"
            # the lookup and the GPU builder read offset and spacing from the generated text (Vector3_String,
            # madarch-scenes.adb:807-810,1130-1133); the CPU builders read the settings record, binary32
            # (madarch-renderers.adb:611-618)
            self.psp6, self.poff6 = np.array([image6(v) for v in pt["spacing"]]), np.array([image6(v) for v in pt["offset"]])
            self.psp32, self.poff32 = r32(pt["spacing"]), r32(pt["offset"])
            self.rank = None if pt.get("table") is None else self.walk_order(np.asarray(pt["table"]))

    def walk_order(self, table):
        """A cell's record as the order in which partitioning_closest_info meets the primitives (madarch-scenes.adb:
        971-1015, 1033-1099): `i` runs through indices[] while `size` grows by each kind's count in declared order, so the
        kinds are walked by cumulative counts; indices[] has index_count entries, and the walk ends there (Q7).
        -> rank [cell, place in self.prims]: the step of the walk that meets the primitive, `never` if none does; one
        more row, all `never`: the empty cell that an index past the table reads (Q6)."""
        nk, n = len(self.place), len(self.prims)
        assert table.shape == (self.cells, nk + self.pcount), "the table has shape %s" % (table.shape,)
        self.never = n + self.pcount + 1
        rank = np.full((self.cells + 1, n), self.never, dtype=int)
        for c in range(self.cells):
            i = 0
            for k in range(nk):
                size = i + int(table[c, k])
                while i < size and i < self.pcount:
                    e = int(table[c, nk + i])
                    assert 0 <= e < len(self.place[k]), "cell %d names entity %d of kind %d, which was never added" % (c, e, k)
                    rank[c, self.place[k][e]] = min(rank[c, self.place[k][e]], i)
                    i += 1
                i = size
        return rank

    # dist_to_<Kind> (madarch-scenes.adb:417-455)
    def prim_distance(self, k, P):
        name, v, _, _ = self.prims[k]
        if name == "Sphere":    # madarch-primitives-spheres.ads:13-14
            return _norm(v[0] - P) - v[1]
        if name == "Plane":     # madarch-primitives-planes.ads:13-14
            return P @ v[0] + v[1]
        if name == "Box":       # madarch-primitives-boxes.adb:7-15
            q = np.abs(v[0] - P) - v[1]
            return _norm(np.maximum(q, 0.0)) + np.minimum(q.max(axis=1), 0.0)
        return triangle_distance(v[0], v[1], v[2], P)

    def exact32(self, k, P):
        """Per point: binary32 computes primitive k's distance without a single rounding, in whatever order it adds.  Every
        intermediate result of the float64 evaluation is then a binary32 number; by induction binary32 has the same
        operands at each operation, the true result lies within half a float64 ulp of a binary32 number, and the correctly
        rounded binary32 result is that number (a rounding midpoint is half a binary32 ulp away).  The operations are those of
        prim_distance with dot = (x x' + y y') + z z' and length = sqrt (dot) (DESIGN.md section 5 "Numerics"); abs, min and
        max never round.  Triangles: not claimed."""
        name, v, _, _ = self.prims[k]
        P = np.asarray(P, dtype=np.float64)

        def whole(*xs):
            return np.all([(r32(x) == x).reshape(len(P), -1).all(axis=1) for x in xs], axis=0)

        def length(d):
            sq = d * d
            a = sq[:, 0] + sq[:, 1]
            b = a + sq[:, 2]
            return np.sqrt(b), whole(sq, a, b, np.sqrt(b))
        if name == "Sphere":
            d = v[0] - P
            r, ok = length(d)
            return ok & whole(P, d, r - v[1])
        if name == "Plane":
            pr = P * v[0]
            a = pr[:, 0] + pr[:, 1]
            b = a + pr[:, 2]
            return whole(P, pr, a, b, b + v[1])
        if name == "Box":
            d = v[0] - P
            q = np.abs(d) - v[1]
            r, ok = length(np.maximum(q, 0.0))
            return ok & whole(P, d, q, r + np.minimum(q.max(axis=1), 0.0))
        return np.zeros(len(P), dtype=bool)

    # <Kind>_normal (madarch-scenes.adb:457-495)
    def prim_normal(self, k, P):
        name, v, _, _ = self.prims[k]
        if name == "Sphere":    # madarch-primitives-spheres.ads:16-17
            return _unit(P - v[0])
        if name == "Plane":     # madarch-primitives-planes.ads:16-17
            return np.broadcast_to(v[0], P.shape).copy()
        if name == "Box":       # madarch-primitives-boxes.adb:5,17-41
            e = float(r32(0.002))
            d = (P - v[0]) / v[1]
            r = np.abs(d)
            n = np.stack([(r[:, i] > r[:, (i + 1) % 3] - e) * (r[:, i] > r[:, (i + 2) % 3] - e) * np.sign(d[:, i]) for i in range(3)], axis=1)
            return _unit(n.astype(np.float64))
        # madarch-primitives-triangles.adb:50-56: forward differences of the distance, madarch-exprs-derivatives.adb:12-45
        h = float(r32(0.000001))
        f = triangle_distance(v[0], v[1], v[2], P)
        g = np.stack([triangle_distance(v[0], v[1], v[2], P + np.eye(3)[i] * h) - f for i in range(3)], axis=1)
        return _unit(g)

    def closest(self, P, kinds=None, start=None):
        """what a march calls (raymarching.glsl:9,27,41, lighting.glsl:61): partitioning_closest (_info), which IS the
        full scan when the partition is disabled (madarch-scenes.adb:1256-1262)"""
        if self.part is None or kinds is not None:
            return self.scan(P, kinds, start)
        return self.lookup(P)

    def lookup(self, P):
        """partitioning_closest_info (madarch-scenes.adb:799-837, 960-1118; partitioning_closest, :839-958, is its distance)
        -> distance, place in self.prims (-1: `index` is left untouched); self.face: the point lies within the
        margin of a cell face (see hold, cell_face_margin)"""
        P = np.asarray(P, dtype=np.float64)
        n, dims = len(self.prims), self.pdims
        q = (P - self.poff6) / self.psp6
        self.face = (np.abs(q - np.round(q)) * self.psp6 <= EPS_MARGIN * np.maximum(1.0, np.abs(P).max(axis=1, initial=0.0))[:, None]).any(axis=1)
        fx = np.floor(q)                                         # :807-811
        cfx = np.clip(fx, 0.0, dims.astype(np.float64))          # :814-816: to dims, not dims - 1
        if self.pfallback:                                       # :822-825: `fx != cfx` is true if ANY component differs
            back = (fx != cfx).any(axis=1)
        else:                                                    # :819-820
            fx, back = cfx, np.zeros(len(P), dtype=bool)
        fx = np.where(back[:, None], 0.0, fx)
        index = (fx[:, 0] * float(dims[1] * dims[2]) + fx[:, 1] * float(dims[2]) + fx[:, 2]).astype(np.int64)  # :830-834, int () of a whole number
        index = np.where(index >= self.cells, self.cells, index)  # Q6: past the table, an empty cell
        D = np.stack([self.prim_distance(k, P) for k in range(n)], axis=1) if n else np.zeros((len(P), 0))
        rank = self.rank[index]
        rank[back] = np.arange(n)                                 # the full scan meets the primitives in the order of self.prims
        D = np.where(rank < self.never, D, np.inf)
        best = D.min(axis=1, initial=np.inf)
        arg = np.where(D == best[:, None], rank, self.never).argmin(axis=1) if n else np.zeros(len(P), dtype=int)  # of equal ones, the first met
        take = best < self.max_dist                               # `dist < closest` from max_dist, strictly (:1000,1082,1105)
        return np.where(take, best, self.max_dist), np.where(take, arg, -1)

    def scan(self, P, kinds=None, start=None):
        """closest_primitive_info (madarch-scenes.adb:631-674): the scan starts at max_dist and takes a primitive only
        when it is strictly closer.  -> distance, place in self.prims (-1: nothing closer than the start)"""
        best = np.full(len(P), self.max_dist if start is None else start)
        arg = np.full(len(P), -1, dtype=int)
        for k in range(len(self.prims)):
            if kinds is not None and self.prims[k][0] not in kinds:
                continue
            d = self.prim_distance(k, P)
            m = d < best
            best[m], arg[m] = d[m], k
        return best, arg

    def info(self, arg, P):
        """primitive_info (madarch-scenes.adb:676-729): normal and material id of primitive `arg` at P"""
        n = np.zeros((len(P), 3))
        for k in np.unique(arg[arg >= 0]):
            m = arg == k
            n[m] = self.prim_normal(k, P[m])
        return n, np.where(arg >= 0, self.mat[np.maximum(arg, 0)], 0)


class Run:
    """one rendering: the scene, the atlases it reads and the jitter of its rays (seed None: as stated)"""

    def __init__(self, scene, seed=None, irradiance=None, radiance=None, scattering=None):
        self.sc = scene
        self.scat = None if scattering is None else np.asarray(scattering, dtype=np.float64)
        self.rng = None if seed is None else np.random.RandomState(seed)
        self.irr = None if irradiance is None else np.asarray(irradiance, dtype=np.float64)
        self.rad = None if radiance is None else np.asarray(radiance, dtype=np.float64)
        # which pixel each row of the arrays in hand belongs to, and what the marches behind a pixel report about it:
        # a step near a cell face (cell_face_margin, see hold), a shadow step with a negative radicand
        self.scope = self.px_face = self.px_negative = None

    def pixels(self, n):
        self.scope, self.px_face, self.px_negative = np.arange(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)

    @contextlib.contextmanager
    def rows(self, sel):
        """the arrays in hand are now the rows `sel` (indices or a mask) of the ones before"""
        outer = self.scope
        if outer is not None:
            self.scope = outer[sel]
        try:
            yield
        finally:
            self.scope = outer

    def note(self, face, negative=None):
        if self.scope is not None:
            self.px_face[self.scope[face]] = True
            if negative is not None:
                self.px_negative[self.scope[negative]] = True

    def ray(self, O, D):
        O, D = np.array(O, dtype=np.float64), np.array(D, dtype=np.float64)
        if self.rng is not None:
            O = O * (1.0 + JITTER * self.rng.uniform(-1.0, 1.0, O.shape))
            D = D * (1.0 + JITTER * self.rng.uniform(-1.0, 1.0, D.shape))
        return O, D

    # ------------------------------------------------------------------------------------- marches
    def raycast(self, O, D, tmax=None):
        """raycast / raycast_hit_position (raymarching.glsl:25-51) -> hit, place in Scene.prims, t, position, and `near`:
        a step's distance came within EPS_MARGIN of the threshold `dist < epsilon`, or a step's point within the margin of a
        face of the partition's cells (see hold)"""
        O, D = self.ray(O, D)
        n = len(O)
        tmax = np.broadcast_to(self.sc.max_dist if tmax is None else tmax, (n,))
        t, hit, arg, near = np.zeros(n), np.zeros(n, dtype=bool), np.full(n, -1, dtype=int), np.zeros(n, dtype=bool)
        face = np.zeros(n, dtype=bool)
        live = np.nonzero(t < tmax)[0]
        for _ in range(MAX_STEPS):
            if not len(live):
                break
            X = O[live] + D[live] * t[live, None]
            s, a = self.sc.closest(X)
            h = s < EPS
            near[live] |= np.abs(s - EPS) <= EPS_MARGIN * np.maximum(1.0, np.abs(X).max(axis=1))
            if self.sc.part is not None:
                face[live] |= self.sc.face
            hit[live[h]], arg[live[h]] = True, a[h]
            live, s = live[~h], s[~h]
            t[live] += s
            live = live[t[live] < tmax[live]]
        self.note(face)
        return hit, arg, t, O + D * t[:, None], near | face

    def visibility(self, O, D, tmax):  # raymarching.glsl:53-56
        return 1.0 - self.raycast(O, D, tmax)[0].astype(np.float64)

    def softshadows(self, O, D, tmin, tmax, k):  # raymarching.glsl:4-23
        O, D = self.ray(O, D)
        n = len(O)
        tmax = np.broadcast_to(tmax, (n,))
        res, prev, t = np.ones(n), np.full(n, 1e20), np.full(n, float(tmin))
        face, negative = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        live = np.nonzero(t < tmax)[0]
        for _ in range(MAX_STEPS):
            if not len(live):
                break
            s, _ = self.sc.closest(O[live] + D[live] * t[live, None])
            if self.sc.part is not None:
                face[live] |= self.sc.face
            h = s < EPS
            res[live[h]] = 0.0
            live, s = live[~h], s[~h]
            y = s * s / (2.0 * prev[live])
            # Without a partition the distance is 1-Lipschitz: s <= prev + (the step, prev) = 2 prev, so y <= s and the radicand
            # is not negative -- but for rounding where s = 2 prev (a ray that leaves a plane along its normal): there it is 0,
            # as it always was here.  Through a table the next cell may name other candidates, or a clamped index another cell,
            # and s can exceed 2 prev: the square root is then a NaN, and min ignores a NaN operand (the docstring's stated
            # choices) -- the step leaves res as it was.  So does a division by zero: k e / 0 is +inf, or a NaN where e is 0.
            # `rounding`: s and 2 prev carry 2^-21 c and 2^-20 c (threshold_margin, see hold); within twice their sum the sign
            # of the radicand is not float64's to tell.  Through a table such a step makes the pixel fragile.
            X = O[live] + D[live] * t[live, None]
            rounding = np.abs(s - 2.0 * prev[live]) <= 3.0 * EPS_MARGIN * np.maximum(1.0, np.abs(X).max(axis=1))
            radicand = s * s - y * y
            negative[live] |= (radicand < 0.0) & ~rounding
            if self.sc.part is not None:
                face[live] |= rounding
            with np.errstate(divide="ignore", invalid="ignore"):
                e = np.sqrt(np.where(rounding, np.maximum(radicand, 0.0), radicand))
                den = np.maximum(0.0, t[live] - y)
                q = np.where(rounding & (den == 0.0), np.inf, k * e / den)
            res[live] = np.fmin(res[live], q)
            prev[live] = s
            t[live] += s
            live = live[t[live] < tmax[live]]
        assert self.sc.part is not None or not negative.any(), "a negative shadow radicand without a partition"
        self.note(face, negative)
        return res

    # ------------------------------------------------------------------------------------- lights
    def sample_light(self, light, P):
        """sample_light (madarch-scenes.adb:497-549, 731-764) -> radiance, direction to the light, its distance"""
        v = light[1] - P
        dist = _norm(v)
        L = v / dist[:, None]
        if light[0] == "point":  # madarch-lights-point_lights.ads:20-22
            return light[2] / (dist * dist * 0.03)[:, None], L, dist
        # madarch-lights-spot_lights.adb:5-24
        _, _, ldir, aperture, colour = light
        theta = np.arccos(np.clip(np.maximum(_dot(-L, ldir), 0.0), -1.0, 1.0))
        ratio = np.clip(theta / aperture, 0.0, 1.0)
        return colour * (np.minimum(1.0 / (dist * dist * 0.03), 1.5) * (1.0 - ratio ** 8))[:, None], L, dist

    @staticmethod
    def cook_torrance(N, V, L, albedo, metallic, rough):  # cook_torrance_brdf.glsl:1-52
        H = _unit(V + L)
        NdotV, NdotL = np.maximum(_dot(N, V), 0.0), np.maximum(_dot(N, L), 0.0)
        F0 = 0.04 * (1.0 - metallic)[:, None] + albedo * metallic[:, None]
        a2 = rough ** 4
        NDF = a2 / (PI * (np.maximum(_dot(N, H), 0.0) ** 2 * (a2 - 1.0) + 1.0) ** 2)
        k = (rough + 1.0) ** 2 / 8.0
        G = (NdotV / (NdotV * (1.0 - k) + k)) * (NdotL / (NdotL * (1.0 - k) + k))
        F = F0 + (1.0 - F0) * ((1.001 - np.maximum(_dot(H, V), 0.0)) ** 5)[:, None]
        kS = np.minimum((NDF * G)[:, None] * F / np.maximum(4.0 * NdotV * NdotL, 0.001)[:, None], 1.0)
        return (1.0 - F) * (1.0 - metallic)[:, None], kS

    def direct(self, P, N, Dir, albedo, metallic, rough, specular):  # lighting.glsl:1-40
        Lo = np.zeros((len(P), 3))
        for light in self.sc.lights:
            radiance, L, Ld = self.sample_light(light, P)
            NdotL = np.maximum(_dot(N, L), 0.0)
            kD, kS = self.cook_torrance(N, -Dir, L, albedo, metallic, rough)
            sh = np.zeros(len(P))
            m = NdotL > EPS
            if m.any():
                with self.rows(m):
                    sh[m] = self.softshadows((P + N * MSS * 5.0)[m], L[m], 0.0, Ld[m], 64.0)
            if not specular:
                kS = np.zeros_like(kS)
            Lo += (kD * albedo / PI + kS) * radiance * (NdotL * sh)[:, None]
        return Lo

    def ambient_occlusion(self, P, N, steps):  # lighting.glsl:51-69
        if steps <= 0:
            return np.ones(len(P))
        size = float(r32(0.1))
        total = top = 0.0
        for i in range(steps):
            factor = 1.0 / 2.0 ** i
            total = total + factor * self.sc.closest(P + N * ((i + 1) * size))[0]
            if self.sc.part is not None:
                self.note(self.sc.face)
            top += factor * (i + 1) * size
        return 0.6 + 0.4 * total / top

    # ------------------------------------------------------------------------------------- probes
    def tap(self, atlas, q, res, direction):
        """one filtered texel of probe q's tile along `direction`: grid_position_to_probe_id, probe_id_to_coord,
        the clamp of the ray id to the tile's texel centres (probe_utils.glsl:11-15,46-56; render_probes.glsl:50-61)"""
        sc = self.sc
        pid = q[:, 2] * sc.dims[0] * sc.dims[1] + q[:, 1] * sc.dims[0] + q[:, 0]
        base = np.stack([pid % sc.pc[0], pid // sc.pc[0]], axis=1) / sc.pc
        rid = np.clip(oct_encode(direction), 0.5 / res, 1.0 - 0.5 / res)
        c = base + rid / sc.pc
        return bilinear(atlas, c[:, 0], c[:, 1])

    def cage(self, P):
        g = np.floor(P / self.sc.spacing).astype(int)  # probe_utils.glsl:42-44
        for i in range(8):
            off = np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1])
            yield off, np.clip(g + off, 0, self.sc.dims - 1), g

    def sample_irradiance(self, P, N):  # render_probes.glsl:6-69
        sc = self.sc
        acc, total = np.zeros((len(P), 3)), np.zeros(len(P))
        for off, q, g in self.cage(P):
            alpha = P / sc.spacing - g
            to = q * sc.spacing - P  # probe_utils.glsl:38-40
            dist = _norm(to)
            dp = to / dist[:, None]
            w = ((_dot(dp, N) + 1.0) * 0.5) ** 2 + 0.2
            w = w * self.visibility(P + N * MSS * 5.0, dp, dist - MSS * 5.0)
            w = np.where(w < 0.2, w * w * w * (1.0 / (0.2 * 0.2)), w)
            w = w * np.where(off == 1, alpha, 1.0 - alpha).prod(axis=1)
            acc += np.sqrt(self.tap(self.irr, q, sc.ires, N)) * w[:, None]
            total += w
        with np.errstate(invalid="ignore", divide="ignore"):
            out = (acc / total[:, None]) ** 2
        out[total == 0.0] = 0.0
        return out

    def radiance_no_specular(self, P, N, Dir, flags):  # render_probes.glsl:138-209 (M_ADD_INDIRECT_SPECULAR = 1)
        sc = self.sc
        out = np.zeros((len(P), 3))
        hit, arg, _, S, near = self.raycast(P + N * MSS * 5.0, Dir)
        flags |= near
        if not hit.any():
            return out
        rows = np.nonzero(hit)[0]
        S, arg, Dir = S[hit], arg[hit], Dir[hit]
        sn, smat = sc.info(arg, S)
        flags[rows[sc.kind[arg] == 3]] = True
        best = np.full(len(S), -2.0)
        bq, bdir = np.zeros((len(S), 3), dtype=int), np.zeros((len(S), 3))
        with self.rows(rows):
            for _, q, _ in self.cage(S):
                to = S - q * sc.spacing
                dist = _norm(to)
                to = to / dist[:, None]
                w = _dot(to, -sn) * self.visibility(S + sn * MSS * 5.0, -to, dist - MSS * 5.0)
                m = w > best
                best[m], bq[m], bdir[m] = w[m], q[m], to[m]
            zero = np.zeros((len(S), 3))
            out[rows] = self.tap(self.rad, bq, sc.rres, bdir) + self.direct(S, sn, Dir, zero, sc.m_metallic[smat], sc.m_rough[smat], True)
        return out

    def render_volumetrics(self, colour, O, P, hit, frag):
        """volumetrics.glsl:34-54: of the 3 x 3 scattering texels round the fragment (x outer, y inner), the first whose stored
        length is strictly closer to this pixel's than every one before, starting from max_dist; a miss has len = max_dist
        (SURVEY.md Q13).  -> colour, and `near`: another candidate's |a - len| is within 2 T_ATOL of the best one's, so that
        the pick is a coin toss between precisions -- unless the two carry the same fog (within half COLOUR_ATOL): at the
        texture's edge the mirrored repeat makes two offsets read the same texels, and then the pick does not show"""
        sc = self.sc
        tc = (frag + 1.0) * 0.5
        length = np.where(hit, _norm(P - O), sc.max_dist)
        rgb, a = self.scat[..., :3], np.repeat(self.scat[..., 3:], 3, axis=2)
        dists, fogs = [], []
        for x in (-1, 0, 1):
            for y in (-1, 0, 1):
                cx, cy = tc[:, 0] + x / sc.sres[0], tc[:, 1] + y / sc.sres[1]
                dists.append(np.abs(bilinear(a, cx, cy)[:, 0] - length))
                fogs.append(bilinear(rgb, cx, cy))
        dists, fogs = np.stack(dists, axis=1), np.stack(fogs, axis=1)
        best = np.argmin(dists, axis=1)  # (the first of equal ones, as `dist < closest` keeps it)
        rows = np.arange(len(O))
        closest, fog = dists[rows, best], fogs[rows, best]
        fog[~(closest < sc.max_dist)] = 0.0  # (no candidate closer than max_dist: fog_L is undefined; no case comes near)
        rival = (dists - closest[:, None] < 2.0 * T_ATOL) & (np.abs(fogs - fog[:, None, :]).max(axis=2) > 0.5 * COLOUR_ATOL)
        return colour * np.exp(-length * TAU)[:, None] + fog, rival.any(axis=1)

    def pixel_color_probes(self, O, D, mode, specular, indirect_specular, ao_steps, frag=None):
        """render_probes.glsl:246-291.  mode 0 is the reference's; 1 and 2 are this project's BASELINE configs 1 and 2:
        0.5 n + 0.5, and direct light times the ambient occlusion.  -> dict of hit, index, t, pos, normal, colour,
        near (the primary march came near the threshold or a cell face), tri (near, or the march behind the specular term
        did, or a triangle's normal took part, or a shadow, occlusion or visibility step came near a cell face: see hold),
        negative (a soft-shadow step of the pixel had a negative radicand)"""
        sc = self.sc
        n = len(O)
        self.pixels(n)
        hit, arg, t, P, near = self.raycast(O, D)
        O, D = np.asarray(O, dtype=np.float64), np.asarray(D, dtype=np.float64)
        colour = SKY - (D[:, 1] * 0.7)[:, None]
        normal = np.zeros((n, 3))
        tri = near.copy()
        rows = np.nonzero(hit)[0]
        self.scope = rows  # (everything behind the hit is computed for these pixels)
        if len(rows):
            Ph, Dh, ah = P[rows], D[rows], arg[rows]
            N, mat = sc.info(ah, Ph)
            normal[rows] = N
            flags = sc.kind[ah] == 3
            albedo, metallic, rough = sc.m_albedo[mat], sc.m_metallic[mat], sc.m_rough[mat]
            if mode == 1:
                c = 0.5 * N + 0.5
            else:
                direct = self.direct(Ph, N, Dh, albedo, metallic, rough, specular)
                if mode == 2:
                    c = direct * self.ambient_occlusion(Ph, N, ao_steps)[:, None]
                else:
                    irradiance = self.sample_irradiance(Ph, N)
                    sdir = Dh - N * (2.0 * _dot(N, Dh))[:, None]  # reflect, GLSL 4.30 section 8.5
                    scol = np.zeros((len(rows), 3))
                    gate = rough < 0.75
                    if indirect_specular == 2 and gate.any():
                        f = np.zeros(int(gate.sum()), dtype=bool)
                        with self.rows(gate):
                            scol[gate] = self.radiance_no_specular(Ph[gate], N[gate], sdir[gate], f)
                        flags[np.nonzero(gate)[0][f]] = True
                    elif indirect_specular not in (0, 2):
                        raise NotImplementedError("indirect-specular modes 1 and 3 are restated in test_oracle_pins64.py")
                    kD, kS = self.cook_torrance(N, -Dh, sdir, albedo, metallic, rough)  # lighting.glsl:42-49
                    indirect = kD * irradiance / PI + kS * scol * np.maximum(_dot(N, sdir), 0.0)[:, None]
                    c = self.ambient_occlusion(Ph, N, ao_steps)[:, None] * (direct + indirect)
            colour[rows] = c
            tri[rows] |= flags
        tri |= self.px_face  # (a shadow, occlusion or visibility step near a cell face: fragile for its colour)
        negative, self.scope = self.px_negative, None
        if frag is not None and self.scat is not None and mode == 0:  # render_probes.glsl:289 (M_RENDER_VOLUMETRICS)
            colour, coin = self.render_volumetrics(colour, O, P, hit, frag)
            tri = tri | coin  # (fragile for its colour only, like a triangle's normal)
        index = np.where(hit, sc.number[np.maximum(arg, 0)], -1)
        return {"hit": hit, "index": index, "t": np.where(hit, t, 0.0), "pos": P, "normal": normal, "colour": colour, "tri": tri, "near": near,
                "negative": negative}


# ------------------------------------------------------------------------------------------- maps and filters
def oct_encode(v):  # probe_utils.glsl:58-70, 89-92
    p = v[:, :2] / np.abs(v).sum(axis=1)[:, None]
    fold = (1.0 - np.abs(p[:, ::-1])) * np.where(p >= 0.0, 1.0, -1.0)
    return (np.where((v[:, 2] <= 0.0)[:, None], fold, p) + 1.0) * 0.5


def oct_decode(ray_id):  # probe_utils.glsl:72-87
    e = ray_id * 2.0 - 1.0
    z = 1.0 - np.abs(e[:, 0]) - np.abs(e[:, 1])
    fold = (1.0 - np.abs(e[:, ::-1])) * np.where(e >= 0.0, 1.0, -1.0)
    return _unit(np.concatenate([np.where((z < 0.0)[:, None], fold, e), z[:, None]], axis=1))


def bilinear(img, cx, cy):
    """GL_LINEAR with GL_MIRRORED_REPEAT, one level (madarch-render_passes.adb:111-116)"""
    H, W = img.shape[:2]
    px, py = cx * W - 0.5, cy * H - 0.5
    x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
    fx, fy = (px - x0)[:, None], (py - y0)[:, None]

    def mirror(i, n):
        m = np.mod(i, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m)
    xa, xb, ya, yb = mirror(x0, W), mirror(x0 + 1, W), mirror(y0, H), mirror(y0 + 1, H)
    return (img[ya, xa] * (1 - fx) + img[ya, xb] * fx) * (1 - fy) + (img[yb, xa] * (1 - fx) + img[yb, xb] * fx) * fy


# ------------------------------------------------------------------------------------------- the passes
def camera(sc, u, v):
    """draw_screen.glsl:20-24: the matrix acts on the direction AND on the fragment's position"""
    frag = np.stack([u, v, np.zeros_like(u)], axis=1)
    d = _unit(frag - np.array([0.0, 0.0, -1.5]))
    return frag @ sc.cam_m.T + sc.cam_pos, d @ sc.cam_m.T


def centres(W, H):
    """the centres of a W x H image's texels in [-1, 1], row by row (a pass's `pos.xy`)"""
    j, i = np.mgrid[0:H, 0:W]
    return (2.0 * i.ravel() + 1.0) / W - 1.0, (2.0 * j.ravel() + 1.0) / H - 1.0


def camera_rays(sc, W, H):
    u, v = centres(W, H)
    return camera(sc, u, -v)  # row 0 is the top of the window


def _shape(out, H, W):
    return {k: v.reshape((H, W) + v.shape[1:]) for k, v in out.items()}


def primary(desc, W, H, seed=None):
    """per pixel: hit, index in the geometry buffer's numbering, t, pos, normal"""
    sc = Scene(desc)
    run = Run(sc, seed)
    O, D = camera_rays(sc, W, H)
    hit, arg, t, P, near = run.raycast(O, D)
    N, _ = sc.info(arg, P)
    return _shape({"near": near, "hit": hit, "index": np.where(hit, sc.number[np.maximum(arg, 0)], -1), "t": np.where(hit, t, 0.0), "pos": P, "normal": N}, H, W)


def screen(desc, W, H, mode, irradiance_atlas=None, radiance_atlas=None, seed=None, scattering=None):
    """the LINEAR colour per pixel (before draw_screen.glsl:29) with the primary hit behind it; the screen shader's
    defines are those of madarch-renderers.adb:136-143 with ao_steps and spec_mode from the description.  With volumetric
    settings in the description and a `scattering` texture, the fog is composed in (volumetrics.glsl:34-54)."""
    sc = Scene(desc)
    run = Run(sc, seed, irradiance_atlas, radiance_atlas, scattering if desc.get("vol") else None)
    O, D = camera_rays(sc, W, H)
    u, v = centres(W, H)
    return _shape(run.pixel_color_probes(O, D, mode, True, desc.get("spec_mode", 2), desc.get("ao_steps", 3), frag=np.stack([u, -v], axis=1)), H, W)


def radiance_texels(desc, irradiance_atlas, radiance_atlas=None, seed=None):
    """the radiance atlas after one radiance pass (compute_probe_radiance.glsl:16-27): a texel's centre decides its
    probe (coord_to_probe_id, probe_id_to_grid_position, grid_position_to_world_position: probe_utils.glsl:19-40) and
    its ray (coord_to_ray_id, ray_id_to_ray_dir: :80-87); the probe pass's defines are M_COMPUTE_DIRECT_SPECULAR 0 and
    M_COMPUTE_INDIRECT_SPECULAR 0 (madarch-renderers.adb:115-117), no AO, no added specular (undefined: Q12)"""
    sc = Scene(desc)
    run = Run(sc, seed, irradiance_atlas, radiance_atlas)
    W, H = sc.pc[0] * sc.rres, sc.pc[1] * sc.rres
    j, i = np.mgrid[0:H, 0:W]
    nc = np.stack([(i.ravel() + 0.5) / W, (j.ravel() + 0.5) / H], axis=1)
    tile = (nc * sc.pc).astype(int)
    pid = tile[:, 1] * sc.pc[0] + tile[:, 0]
    xy = sc.dims[0] * sc.dims[1]
    gz = pid // xy
    gy = (pid - gz * xy) // sc.dims[0]
    gx = pid - gz * xy - gy * sc.dims[0]
    world = np.stack([gx, gy, gz], axis=1) * sc.spacing
    ray_id = nc * sc.pc - np.floor(nc * sc.pc)
    return _shape(run.pixel_color_probes(world, oct_decode(ray_id), 0, False, 0, 0), H, W)


def irradiance_texels(desc, radiance_atlas, previous=None, hysteresis=0.0):
    """the whole irradiance atlas after one irradiance pass (update_probe_irradiance.glsl:8-43 with probe_utils.glsl): a
    texel's centre decides its probe (coord_to_probe_id :19-25, probe_id_to_coord :52-56) and its direction
    (coord_to_ray_id, ray_id_to_ray_dir :80-87); the taps sit at the CORNERS of the probe's radiance texels, clamped to
    [step, 1 - step] (:19,26-31), each filtered bilinearly and weighted by max (dot, 0) with the direction of where it sits
    (:32-38); summed in the shader's y, x order and divided by the total weight (:42).
    hysteresis h > 0 (not in the reference; the library's irradiance_blend): GLSL mix (fresh, previous, h)."""
    sc = Scene(desc)
    rad = np.asarray(radiance_atlas, dtype=np.float64)
    W, H = sc.pc[0] * sc.ires, sc.pc[1] * sc.ires
    u, v = centres(W, H)
    nc = (np.stack([u, v], axis=1) + 1.0) * 0.5
    tile = np.floor(nc * sc.pc)
    irr_dir = oct_decode(nc * sc.pc - tile)
    rad_coord = tile / sc.pc
    step = 1.0 / sc.pc / sc.rres
    acc, total = np.zeros((len(nc), 3)), np.zeros(len(nc))
    for y in range(sc.rres):
        for x in range(sc.rres):
            c = np.clip(rad_coord + np.array([x, y]) * step, step, 1.0 - step)
            w = np.maximum(_dot(irr_dir, oct_decode(c * sc.pc - np.floor(c * sc.pc))), 0.0)
            acc += bilinear(rad, c[:, 0], c[:, 1]) * w[:, None]
            total += w
    out = (acc / total[:, None]).reshape(H, W, 3)
    if hysteresis > 0.0:
        h = float(r32(hysteresis))
        out = out * (1.0 - h) + np.asarray(previous, dtype=np.float64) * h  # GLSL 4.30 section 8.3, mix
    return out


def radiance_mips(atlas, lods):
    """MDH_OPT_RADIANCE_MIPS (not in the reference): levels 0 .. lods of the atlas image, each the 2 x 2 box of the one
    below; with lods = log2 (radiance resolution) the last has one texel per probe"""
    levels = [np.asarray(atlas, dtype=np.float64)]
    for _ in range(lods):
        a = levels[-1]
        assert a.shape[0] % 2 == 0 and a.shape[1] % 2 == 0
        levels.append((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]) / 4.0)
    return levels


def hg_phase(a, b):  # volumetrics.glsl:21-30
    return (1.0 - TAU * TAU) / (4.0 * PI * (1.0 + TAU * TAU - 2.0 * TAU * _dot(a, b)) ** 1.5)


def froxel_texels(desc, vol, seed=None):
    """the froxel texture after one visibility pass (compute_frustrum_visibility.glsl:8-42): texel (x, y) of the
    (vw, vh * vz) image is slice floor (y / vh), its sample point the camera ray through (x, fract height) advanced by
    slice * step (:28-39); there, over all lights in the light loop's order, exp (-L_dist tau) * raycast_visibility * radiance *
    tau * henvey_greenstein_phase (L, dir) (:8-19).  -> colour, and `near`: the sample point lies within NEAR_SURFACE of a surface
    or inside a primitive, where the visibility ray is blocked at once in one precision only."""
    sc = Scene(desc, vol)
    run = Run(sc, seed)
    vw, vh, vz = (int(n) for n in sc.vres)
    px, py = centres(vw, vh * vz)
    tex_height = (py + 1.0) * 0.5 * vz
    depth = np.floor(tex_height)
    O, D = camera(sc, px, (tex_height - depth) * 2.0 - 1.0)
    P = O + D * (depth * sc.vstep)[:, None]
    out = np.zeros((len(P), 3))
    for light in sc.lights:
        radiance, L, Ld = run.sample_light(light, P)
        out += radiance * (np.exp(-Ld * TAU) * run.visibility(P, L, Ld) * TAU * hg_phase(L, D))[:, None]
    return _shape({"colour": out, "near": sc.closest(P)[0] < NEAR_SURFACE}, vh * vz, vw)


def scattering_texels(desc, vol, froxels, seed=None):
    """the scattering texture after one scattering pass (accumulate_scattering.glsl:9-48) over the froxel texture given:
    len = min (|hit - origin|, max_depth), a miss keeping the far point (:18-21); L = step_s * sum over f = 0, step_s, .. < len of
    bilinear (froxels, (nx, (ny + floor (f / step_v)) / vz)) * exp (-f tau) (:9-15,22-27), GL_LINEAR with mirrored repeat.
    The sequence f_k and floor (f_k / step_v) are the shader's DISCRETE decisions and are taken in binary32
    (test_oracle_pins64.py, test_scattering_texels_against_float64); so is f_k < len where len is the cap, a binary32
    constant of the shader.  -> colour (L), len, and `near`: len comes from the march and some f_k lies within T_ATOL
    of it, so that the march's last ulp decides the number of steps."""
    sc = Scene(desc, vol)
    run = Run(sc, seed)
    sw, sh = (int(n) for n in sc.sres)
    vz = int(sc.vres[2])
    u, v = centres(sw, sh)
    O, D = camera(sc, u, v)
    hit, _, _, P, _ = run.raycast(O, D)
    d = np.where(hit, _norm(P - O), np.inf)
    length = np.minimum(d, sc.max_depth)
    F, f, s = [], np.float32(0.0), np.float32(sc.sstep)
    while float(f) <= sc.max_depth + float(s):
        F.append(f)
        f = np.float32(f + s)
    marched = d < sc.max_depth + T_ATOL
    near = marched & (np.abs(np.array(F, dtype=np.float64)[None, :] - length[:, None]) <= T_ATOL).any(axis=1)
    vis = np.asarray(froxels, dtype=np.float64)
    nx, ny = 0.5 * (u + 1.0), 0.5 * (v + 1.0)
    L = np.zeros((len(O), 3))
    for f in F:
        m = float(f) < length
        if not m.any():
            break
        rel = float(np.floor(f / np.float32(sc.vstep)))  # (binary32: sample_visibility :10)
        L[m] += bilinear(vis, nx[m], (ny[m] + rel) / vz) * np.exp(-float(f) * TAU)
    return _shape({"colour": L * sc.sstep, "len": length, "near": near}, sh, sw)


def distance(desc, kinds, points):
    """Eval_Distance_To (madarch-renderers.adb:499-526): the kinds in the order given, each kind's entities in the order
    they were added, a primitive taken when strictly closer, from 1.0e10; the normal is that primitive's.
    -> distance, normal, place of the primitive in Scene.prims (for the bands of the caller)"""
    sc = Scene(desc)
    P = r32(points).reshape(-1, 3)
    best, arg = np.full(len(P), 1.0e10), np.full(len(P), -1, dtype=int)
    for name in kinds:
        for k, prim in enumerate(sc.prims):
            if prim[0] == name:
                d = sc.prim_distance(k, P)
                m = d < best
                best[m], arg[m] = d[m], k
    return best, sc.info(arg, P)[0], arg


# ------------------------------------------------------------------------------------------- the partition's builders
def length32(v):
    """Math_Utils.Length of a binary32 vector in binary32: sqrt ((x x + y y) + z z), every operation rounded once
    (DESIGN.md section 5 "Numerics")"""
    x, y, z = (np.float32(c) for c in v)
    return float(np.sqrt(np.float32(np.float32(x * x + y * y) + z * z)))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def decision_margin(*operands):
    """How close the two sides of a builder's comparison `a < b` may come before binary32 and float64 may decide it
    differently: 8 ulp32 of the largest number that enters either side (the bound the distances themselves are held
    to).  Each side is a primitive's distance to a point whose coordinates were rounded once: the differences of
    coordinates carry half an ulp of the larger operand each, their norm less than one and a half, its square root and
    the radius or offset taken off half an ulp each -- less than 3 ulp of the largest operand per distance; a threshold
    closest + diagonal adds the rounding of its sum.  Two sides: less than 3 + 3 + 1/2 + (the sample point's own
    rounding, 1) < 8 ulp."""
    return 8.0 * ulp32(np.max([np.abs(o) for o in np.broadcast_arrays(*operands)], axis=0))


class PartitionBuild:
    """table: cells x (kinds + index_count) ints as the lookup reads them.  ambiguous: per RECORD of the table, a
    decision behind it came within decision_margin.  overflow: per record, a list was cut.  warnings: the cuts, one
    per kind and cell (madarch-renderers.adb:593-598 prints one each).  ties: comparisons with the threshold whose two sides are
    EQUAL and that float64 may still decide (both sides exact in binary32): `dist < threshold` leaves such a primitive out."""

    def __init__(self, table, ambiguous, overflow, warnings, ties):
        self.table, self.ambiguous, self.overflow, self.warnings, self.ties = table, ambiguous, overflow, warnings, ties


def partition_build(desc, method):
    """Update_Partitioning (madarch-renderers.adb:757-775) in float64, method "CPU_Best" | "CPU_Fast" | "GPU_Fast".

    CPU (Update_Partitioning_CPU, :551-755), per cell (X, Y, Z) of the whole grid, its record at X dy dz + Y dz + Z (:567-570):
    the settings record's binary32 spacing and offset; grid_pos = (X, Y, Z) * spacing + offset, centre = grid_pos + spacing *
    0.5 (:611-618); closest from 1.0e10 over all entities (:620-632); the precandidates are the entities with dist < closest +
    cell_diag, cell_diag the binary32 length of the spacing (:615,653-667), kind by kind in the scene's order (the
    reference iterates a hashed map; the project takes the declared order).  CPU_Fast takes them all (:725-732).  CPU_Best
    (:669-723): 27 sample points grid_pos + (0, 1/2, 1) * spacing, x outermost; each accepts the precandidate strictly
    closest to it, the first of equal ones, from 1.0e10; an entity joins its kind's list when it is first accepted.

    GPU (Update_Partitioning_GPU :539-549, compute_scene_partitioning.glsl:5-21, partitioning_compute_grid_cell
    madarch-scenes.adb:1120-1187): dims / 2 groups of 2 x 2 x 2 invocations, so only the cells below 2 * (dims / 2) are
    visited, and grid_size -- the size the record's index is computed with -- is that EVEN size: on an odd grid a record is
    not written where the lookup reads its cell.  centre = (cell + 0.5) * spacing + offset with the six-digit text of both;
    the threshold is closest_primitive (centre), which starts from max_dist, + the six-digit text of the binary32 length of the
    spacing; an entity is listed when dist < threshold, kinds in declared order.  Records never written keep the zeros
    the buffer is created with (the docstring's stated choices).

    Writing (:577-607, Q7): kinds in declared order share indices[]; a kind's list is cut so that the record never holds
    more than index_count entries, the count written is the cut one, and every cut counts as one warning."""
    sc = Scene(dict(desc, partition=dict(desc["partition"], table=None)))
    nk, n, dims, count = len(sc.place), len(sc.prims), sc.pdims, sc.pcount
    table = np.zeros((sc.cells, nk + count), dtype=np.int64)
    ambiguous, overflow = np.zeros(sc.cells, dtype=bool), np.zeros(sc.cells, dtype=bool)
    warnings = 0
    diag32 = length32(sc.psp32)
    if method == "GPU_Fast":
        size = 2 * (dims // 2)
        spacing, offset, start, diag = sc.psp6, sc.poff6, sc.max_dist, image6(diag32)
    else:
        assert method in ("CPU_Best", "CPU_Fast")
        size = dims
        spacing, offset, start, diag = sc.psp32, sc.poff32, 1.0e10, diag32
    X, Y, Z = (a.ravel() for a in np.meshgrid(np.arange(size[0]), np.arange(size[1]), np.arange(size[2]), indexing="ij"))
    cell = np.stack([X, Y, Z], axis=1).astype(np.float64)
    record = X * size[1] * size[2] + Y * size[2] + Z
    if method == "GPU_Fast":
        centre = (cell + 0.5) * spacing + offset
        grid_pos = None
    else:
        grid_pos = cell * spacing + offset
        centre = grid_pos + spacing * 0.5
    D = np.stack([sc.prim_distance(k, centre) for k in range(n)], axis=1)                     # visited cells x primitives
    threshold = np.minimum(start, D.min(axis=1)) + diag
    pre = D < threshold[:, None]
    margin = decision_margin(D, threshold[:, None], np.abs(centre).max(axis=1)[:, None])
    close = np.abs(D - threshold[:, None]) <= margin
    # A comparison that close is still float64's to decide where binary32 computes both sides without a single rounding
    # (Scene.exact32): the centre through its products and sums, the closest primitive's distance, its sum with the
    # diagonal, and the candidate's distance.  Binary32 then compares the very numbers compared here -- an exact tie included,
    # which `<` leaves out.  (A grid on the lattice its scene sits on, with a whole diagonal, has such ties.)
    def whole(*xs):
        return np.all([(r32(x) == x).reshape(len(cell), -1).all(axis=1) for x in xs], axis=0)
    exact = np.stack([sc.exact32(k, centre) for k in range(n)], axis=1) if n else np.zeros((len(cell), 0), dtype=bool)
    steps = whole((cell + 0.5) * spacing, centre) if grid_pos is None else whole(cell * spacing, grid_pos, np.broadcast_to(spacing * 0.5, cell.shape), centre)
    nearest = D.argmin(axis=1) if n else np.zeros(len(cell), dtype=int)
    sure = steps & whole(threshold) & ((D.min(axis=1) >= start) | exact[np.arange(len(cell)), nearest])
    decided = close & exact & sure[:, None]
    ties = int((decided & (D == threshold[:, None])).sum())
    unsure = (close & ~decided).any(axis=1)
    if method == "CPU_Best":
        S = np.array([[sx, sy, sz] for sx in range(3) for sy in range(3) for sz in range(3)]) / 2.0   # (Cmp - One) / (Res - One)
        pts = (grid_pos[:, None, :] + S[None, :, :] * spacing).reshape(-1, 3)
        DS = np.stack([sc.prim_distance(k, pts) for k in range(n)], axis=1).reshape(len(cell), 27, n)
        DS = np.where(pre[:, None, :], DS, np.inf)
        first = DS.argmin(axis=2)                                                             # the first of equal ones
        best = DS.min(axis=2)
        m = decision_margin(best, np.abs(pts).max(axis=1).reshape(len(cell), 27))
        rival = (DS - best[:, :, None] <= m[:, :, None]) & (np.arange(n)[None, None, :] != first[:, :, None])
        # A rival is no coin toss where BOTH distances are computed without any rounding (Scene.exact32): binary32 then has the
        # very numbers compared here, ties included, and `<` keeps the first met -- as argmin does.  simple_scene's own grid puts
        # its sample points on the half-integer lattice its primitives sit on: half of its cells have such exact ties.
        exact = np.stack([sc.exact32(k, pts) for k in range(n)], axis=1).reshape(len(cell), 27, n)
        rival &= ~(exact & np.take_along_axis(exact, first[:, :, None], axis=2))
        # Nor where the rival is the winner's MIRROR IMAGE in the sample point: the same kind with the same size, and
        # |centre - point| the same in every component (exact in float64: differences of binary32 numbers), at a point that is
        # itself a binary32 number.  Binary32 then performs the same operations on the same magnitudes for both (a rounded
        # difference only changes sign with its operands' order) and gets the same bits, whatever they are.  So it does with x
        # and y exchanged: length adds (x x + y y) first, and a + b is b + a.
        binary32 = (r32(pts) == pts).all(axis=1).reshape(len(cell), 27)
        away, extent = np.full((n, len(pts), 3), np.nan), np.full((n, 3), np.nan)
        for j, (kind, v, _, _) in enumerate(sc.prims):
            if kind in ("Sphere", "Box"):
                away[j], extent[j] = np.abs(v[0] - pts), v[1]
        away = away.reshape(n, len(cell), 27, 3)
        for j in range(n):
            c, s = np.nonzero(rival[:, :, j])
            w = first[c, s]
            same = [(extent[w][:, o] == extent[j]).all(axis=1) & (away[w, c, s][:, o] == away[j, c, s]).all(axis=1) for o in ([0, 1, 2], [1, 0, 2])]
            mirror = binary32[c, s] & (sc.kind_ix[w] == sc.kind_ix[j]) & (same[0] | same[1])
            rival[c[mirror], s[mirror], j] = False
        unsure |= rival.any(axis=(1, 2))
    for c in range(len(cell)):
        if method == "CPU_Best":
            order = list(dict.fromkeys(int(j) for j in first[c])) if pre[c].any() else []    # in the order of first acceptance
        else:
            order = [int(j) for j in np.nonzero(pre[c])[0]]
        written = 0
        for k in range(nk):
            mine = [int(np.nonzero(np.array(sc.place[k]) == j)[0][0]) for j in order if sc.kind_ix[j] == k]
            if written + len(mine) > count:
                warnings += 1
                overflow[record[c]] = True
                mine = mine[:count - written]
            table[record[c], k] = len(mine)
            table[record[c], nk + written:nk + written + len(mine)] = mine
            written += len(mine)
        ambiguous[record[c]] = unsure[c]
    return PartitionBuild(table, ambiguous, overflow, warnings, ties)


def partition_table(desc, method):
    """-> the table and the mask of its ambiguous records"""
    b = partition_build(desc, method)
    return b.table, b.ambiguous


# ------------------------------------------------------------------------------------------- holding a frame
COLOUR_RTOL, COLOUR_ATOL = 3e-3, 3e-4   # test_oracle_pins64.py:369,409
T_ATOL = 2e-4                            # test_oracle_pins64.py:220
FRAGILE_CAP = 0.05
TONE = float(np.float32(0.4545))


def three_runs(render):
    """`render (seed)` as stated and twice jittered, with fixed seeds"""
    return [render(None), render(0x4D41), render(0x4441)]


def undo_tone_map(fb):
    """the inverse of draw_screen.glsl:29 in float64; a NaN (a negative colour's power) stays NaN"""
    y = np.asarray(fb, dtype=np.float64) ** (1.0 / TONE)
    with np.errstate(divide="ignore", invalid="ignore"):
        return y / (1.0 - y)


def fragile(runs, rtol=COLOUR_RTOL, atol=COLOUR_ATOL, colour=True, march=False):
    """A pixel is fragile if, between any two of the three float64 runs, its hit / miss or primitive index differs, or
    its linear colour differs by more than half the colour tolerance -- or if a triangle's normal took part in it
    (triangle_normal_noise below).  `march`: or its march length differs by more than half T_ATOL (grazing_rays below).
    Nothing the code under test returns takes part."""
    bad = np.zeros(runs[0]["hit"].shape, dtype=bool)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        bad |= (runs[a]["hit"] != runs[b]["hit"]) | (runs[a]["index"] != runs[b]["index"]) | runs[a]["near"] | runs[b]["near"]
        if march:
            bad |= np.abs(runs[a]["t"] - runs[b]["t"]) > 0.5 * T_ATOL
        if colour:
            ca, cb = runs[a]["colour"], runs[b]["colour"]
            bad |= ~(np.abs(ca - cb) <= 0.5 * (atol + rtol * np.minimum(np.abs(ca), np.abs(cb)))).all(axis=-1)
    if colour:
        for r in runs:
            bad |= r["tri"]
    return bad


def hold(name, runs, colour=None, index=None, t=None, rtol=COLOUR_RTOL, atol=COLOUR_ATOL, more_atol=0.0, clamp=False, cap=FRAGILE_CAP,
         table=False):
    """Hold a frame of the code under test (`colour` LINEAR, `index`, `t`) against the float64 runs: at most `cap` of
    the pixels may be fragile, every other pixel must agree -- there is no share that may fail.

    triangle_normal_noise: a triangle's normal is a forward difference with h = 1e-6 (madarch-exprs-derivatives.adb:16)
    of a distance computed in binary32 at a point whose coordinates are of order 1 -- h is four ulps of such a
    coordinate and ten ulps of the distance, so each component of the binary32 normal carries an error of tens of
    per cent; that is the reference's own behaviour.  The float64 difference has no such noise, so the
    jitter cannot show it: a pixel whose colour uses a triangle's normal is counted fragile FOR ITS COLOUR (its hit,
    index and t are held like any other pixel's).

    threshold_margin: a march ends at the first step whose distance is below epsilon = 0.001 (raymarching.glsl:29).  The
    distances of a march towards a plane are a geometric sequence s0 q^k, which a RELATIVE jitter of the ray only scales:
    it moves s_k by parts in 10^5 of itself.  The binary32 march, though, computes s_k from coordinates of the size of the
    room: the point carries two ulps of its largest coordinate c, the distance two more -- 4 * 2^-23 c = 2^-21 c, some 3e-6
    for c = 7, parts in 10^3 of epsilon.  So a step within 2^-20 max (1, c) of epsilon (twice that bound) may end the
    march in one precision and not in the other, and the hit moves by a whole step of 0.001 (five times the tolerance
    on t): the float64 march reports such steps (`near`) and the pixel is fragile.  Marches of visibility and shadow rays
    are not counted: a ray that passes the threshold a step later is blocked all the same.

    cell_face_margin: through the space partition the distance at a point depends on the cell the point falls in, floor ((x -
    offset) / spacing), and jumps at a cell's faces.  The jitter finds most rays whose steps cross a face between the
    precisions; for the others the same bound is derived: the binary32 point carries two ulps of its largest coordinate c,
    the subtraction of the offset and the division one more each -- 4 * 2^-23 c = 2^-21 c in world units -- so a step whose
    point lies within 2^-20 max (1, c) (twice that) of a face, |q - round (q)| * spacing with q = (x - offset) / spacing,
    may fall into the neighbouring cell in one precision only.  A primary ray with such a step is fragile like one
    near the threshold (`near`); a shadow, occlusion or visibility step of that kind makes the pixel fragile for its colour.

    grazing_rays (`table`: the frame was marched through a table): a cell lists the primitives near it and not the walls
    behind them, and past the table a cell is empty.  A ray that grazes a primitive, say at 0.004, and sees nothing else
    from then on doubles its step from that primitive until a wall's cell takes over: the rounding of its closest approach
    (parts in 10^7 of the room) grows with the steps, measured by a factor of 370 to 2.7e-4 in t on a pixel whose index and
    colour agree.  Without a partition the walls bound every step and no case shows it.  The jitter does show it (it moves
    the approach by parts in 10^5): with `table` a pixel whose march length differs by more than half T_ATOL between two
    runs is fragile, as hold_values treats a texture's `len`."""
    ref = runs[0]
    geo = fragile(runs, colour=False, march=table)
    col = fragile(runs, rtol, atol, colour=colour is not None, march=table)
    share = float(col.mean())
    print("%s: fragile share %.4f (%d of %d)" % (name, share, int(col.sum()), col.size))
    assert share <= cap, "%s: %.4f of the inputs are fragile in float64 alone" % (name, share)
    if index is not None:
        bad = (np.asarray(index) != ref["index"]) & ~geo
        assert not bad.any(), "%s: %d primitive indices differ, first at %s" % (name, bad.sum(), np.argwhere(bad)[0])
    if t is not None:
        bad = (np.abs(np.asarray(t, dtype=np.float64) - ref["t"]) > T_ATOL) & ~geo
        assert not bad.any(), "%s: %d march lengths differ, first at %s" % (name, bad.sum(), np.argwhere(bad)[0])
    if colour is not None:
        got, want = np.asarray(colour, dtype=np.float64), ref["colour"]
        if clamp:
            want = np.clip(want, 0.0, 1.0)
        ok = np.abs(got - want) <= atol + more_atol + rtol * np.abs(want)
        # the tone map of a NEGATIVE colour is a NaN, and only a miss pixel's sky has one (render_probes.glsl:287); a NaN
        # anywhere else, on however dark a pixel, is an error.  Through a table (`table`) a hit pixel can have one too: a cell
        # that does not list a wall lets the march step THROUGH it (grazing_rays) and end behind it, on a negative distance;
        # the occlusion's samples (lighting.glsl:61) are negative there, and so is the float64 colour.
        ok |= np.isnan(got) & (want < 0.0) & (~ref["hit"][..., None] | table)
        bad = ~ok.all(axis=-1) & ~col
        with np.errstate(invalid="ignore"):
            ratio = np.where(ok, np.abs(got - want) / (atol + more_atol + rtol * np.abs(want)), np.inf).max(axis=-1)
        print("%s: largest error %.3f of its tolerance" % (name, float(np.where(col, 0.0, np.nan_to_num(ratio, nan=0.0, posinf=np.inf)).max())))
        if bad.any():
            where = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s: %d of %d pixels outside the tolerance, first at %s: got %s, float64 %s, index %d" % (
                name, bad.sum(), bad.size, where, got[where], want[where], ref["index"][where]))
    return share


def hold_values(name, runs, got, rtol, atol, more_atol=0.0, clamp=False, length=None, cap=FRAGILE_CAP):
    """hold's sibling for a texture that has no hit and no index (an atlas, the froxel and the scattering texture): `runs`
    are dicts of `colour` and, where the pass has them, `near` and `len`.  A texel is fragile if a run flags it `near` or
    if, between any two runs, its colour differs by more than half the tolerance or its len by more than half T_ATOL; at
    most `cap` of the texels may be, every other one must agree: the colour within atol + more_atol + rtol |float64|,
    `length` (the fourth component of the texture under test) within T_ATOL.  Prints the fragile share and the largest
    error of a held texel as a fraction of its tolerance, and returns both."""
    ref = runs[0]
    bad = np.zeros(ref["colour"].shape[:-1], dtype=bool)
    for r in runs:
        if "near" in r:
            bad |= r["near"]
    for a in range(len(runs)):
        for b in range(a + 1, len(runs)):
            ca, cb = runs[a]["colour"], runs[b]["colour"]
            bad |= ~(np.abs(ca - cb) <= 0.5 * (atol + rtol * np.minimum(np.abs(ca), np.abs(cb)))).all(axis=-1)
            if "len" in ref:
                bad |= np.abs(runs[a]["len"] - runs[b]["len"]) > 0.5 * T_ATOL
    share = float(bad.mean())
    want = np.clip(ref["colour"], 0.0, 1.0) if clamp else ref["colour"]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %s, float64 %s" % (name, got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got - want) / (atol + more_atol + rtol * np.abs(want))
    ratio = np.where(np.isfinite(got), ratio, np.inf).max(axis=-1)
    if length is not None:
        lr = np.abs(np.asarray(length, dtype=np.float64) - ref["len"]) / T_ATOL
        ratio = np.maximum(ratio, np.where(np.isfinite(lr), lr, np.inf))
    worst = float(np.where(bad, 0.0, ratio).max())
    print("%s: fragile share %.4f (%d of %d), largest error %.3f of its tolerance" % (name, share, int(bad.sum()), bad.size, worst))
    assert share <= cap, "%s: %.4f of the inputs are fragile in float64 alone" % (name, share)
    off = (ratio > 1.0) & ~bad
    if off.any():
        where = tuple(np.argwhere(off)[0])
        raise AssertionError("%s: %d of %d texels outside the tolerance (largest error %.3g of it), first at %s: got %s, float64 %s" % (
            name, off.sum(), off.size, worst, where, got[where], want[where]))
    return share, worst
