"""An independent float64 renderer, written from the reference's GLSL and Ada text, and the helper that holds a frame
of the oracle or of the HIP library against it.

It shares no code with oracle/ or madarch_amd/csrc/ and calls neither: plain numpy, vectorised over rays with masks.
Every function cites the text it restates.  Besides the screen and the radiance pass it restates the irradiance fold
(irradiance_texels), the optional mip chain (radiance_mips), the two volumetric passes (froxel_texels,
scattering_texels) and the volumetric composition of a pixel.  There is no space partition here.

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

Where the reference leaves a value undefined, the project's stated choice is taken and named:
marches are cut after 4096 steps (Q3), an irradiance with no weight at all is 0 (Q11), textureLod (.., 1.0) on the
single-level atlas reads level 0 (Q5), the probe pass has no AO and no added specular (Q12).

Conventions of this project's read-back (not of the reference): row 0 of a framebuffer is the top of the window
(v = +1 side), row 0 of a texture is its normalised y of 0.
"""
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

    def ray(self, O, D):
        O, D = np.array(O, dtype=np.float64), np.array(D, dtype=np.float64)
        if self.rng is not None:
            O = O * (1.0 + JITTER * self.rng.uniform(-1.0, 1.0, O.shape))
            D = D * (1.0 + JITTER * self.rng.uniform(-1.0, 1.0, D.shape))
        return O, D

    # ------------------------------------------------------------------------------------- marches
    def raycast(self, O, D, tmax=None):
        """raycast / raycast_hit_position (raymarching.glsl:25-51) -> hit, place in Scene.prims, t, position, and `near`:
        a step's distance came within EPS_MARGIN of the threshold `dist < epsilon` (see hold)"""
        O, D = self.ray(O, D)
        n = len(O)
        tmax = np.broadcast_to(self.sc.max_dist if tmax is None else tmax, (n,))
        t, hit, arg, near = np.zeros(n), np.zeros(n, dtype=bool), np.full(n, -1, dtype=int), np.zeros(n, dtype=bool)
        live = np.nonzero(t < tmax)[0]
        for _ in range(MAX_STEPS):
            if not len(live):
                break
            X = O[live] + D[live] * t[live, None]
            s, a = self.sc.closest(X)
            h = s < EPS
            near[live] |= np.abs(s - EPS) <= EPS_MARGIN * np.maximum(1.0, np.abs(X).max(axis=1))
            hit[live[h]], arg[live[h]] = True, a[h]
            live, s = live[~h], s[~h]
            t[live] += s
            live = live[t[live] < tmax[live]]
        return hit, arg, t, O + D * t[:, None], near

    def visibility(self, O, D, tmax):  # raymarching.glsl:53-56
        return 1.0 - self.raycast(O, D, tmax)[0].astype(np.float64)

    def softshadows(self, O, D, tmin, tmax, k):  # raymarching.glsl:4-23
        O, D = self.ray(O, D)
        n = len(O)
        tmax = np.broadcast_to(tmax, (n,))
        res, prev, t = np.ones(n), np.full(n, 1e20), np.full(n, float(tmin))
        live = np.nonzero(t < tmax)[0]
        for _ in range(MAX_STEPS):
            if not len(live):
                break
            s, _ = self.sc.closest(O[live] + D[live] * t[live, None])
            h = s < EPS
            res[live[h]] = 0.0
            live, s = live[~h], s[~h]
            y = s * s / (2.0 * prev[live])
            e = np.sqrt(np.maximum(s * s - y * y, 0.0))
            den = np.maximum(0.0, t[live] - y)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(den > 0.0, k * e / den, np.inf)  # (a division by zero gives +inf: res unchanged)
            res[live] = np.minimum(res[live], q)
            prev[live] = s
            t[live] += s
            live = live[t[live] < tmax[live]]
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
        near (the primary march came near the threshold), tri (near, or the march behind the specular term did, or a
        triangle's normal took part: see hold)"""
        sc = self.sc
        n = len(O)
        hit, arg, t, P, near = self.raycast(O, D)
        O, D = np.asarray(O, dtype=np.float64), np.asarray(D, dtype=np.float64)
        colour = SKY - (D[:, 1] * 0.7)[:, None]
        normal = np.zeros((n, 3))
        tri = near.copy()
        rows = np.nonzero(hit)[0]
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
                        scol[gate] = self.radiance_no_specular(Ph[gate], N[gate], sdir[gate], f)
                        flags[np.nonzero(gate)[0][f]] = True
                    elif indirect_specular not in (0, 2):
                        raise NotImplementedError("indirect-specular modes 1 and 3 are restated in test_oracle_pins64.py")
                    kD, kS = self.cook_torrance(N, -Dh, sdir, albedo, metallic, rough)  # lighting.glsl:42-49
                    indirect = kD * irradiance / PI + kS * scol * np.maximum(_dot(N, sdir), 0.0)[:, None]
                    c = self.ambient_occlusion(Ph, N, ao_steps)[:, None] * (direct + indirect)
            colour[rows] = c
            tri[rows] |= flags
        if frag is not None and self.scat is not None and mode == 0:  # render_probes.glsl:289 (M_RENDER_VOLUMETRICS)
            colour, coin = self.render_volumetrics(colour, O, P, hit, frag)
            tri = tri | coin  # (fragile for its colour only, like a triangle's normal)
        index = np.where(hit, sc.number[np.maximum(arg, 0)], -1)
        return {"hit": hit, "index": index, "t": np.where(hit, t, 0.0), "pos": P, "normal": normal, "colour": colour, "tri": tri, "near": near}


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


def fragile(runs, rtol=COLOUR_RTOL, atol=COLOUR_ATOL, colour=True):
    """A pixel is fragile if, between any two of the three float64 runs, its hit / miss or primitive index differs, or
    its linear colour differs by more than half the colour tolerance -- or if a triangle's normal took part in it
    (triangle_normal_noise below).  Nothing the code under test returns takes part."""
    bad = np.zeros(runs[0]["hit"].shape, dtype=bool)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        bad |= (runs[a]["hit"] != runs[b]["hit"]) | (runs[a]["index"] != runs[b]["index"]) | runs[a]["near"] | runs[b]["near"]
        if colour:
            ca, cb = runs[a]["colour"], runs[b]["colour"]
            bad |= ~(np.abs(ca - cb) <= 0.5 * (atol + rtol * np.minimum(np.abs(ca), np.abs(cb)))).all(axis=-1)
    if colour:
        for r in runs:
            bad |= r["tri"]
    return bad


def hold(name, runs, colour=None, index=None, t=None, rtol=COLOUR_RTOL, atol=COLOUR_ATOL, more_atol=0.0, clamp=False, cap=FRAGILE_CAP):
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
    are not counted: a ray that passes the threshold a step later is blocked all the same."""
    ref = runs[0]
    geo = fragile(runs, colour=False)
    col = fragile(runs, rtol, atol, colour=colour is not None)
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
        # anywhere else, on however dark a pixel, is an error
        ok |= np.isnan(got) & (want < 0.0) & ~ref["hit"][..., None]
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
