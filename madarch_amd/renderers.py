"""Host mirror of Madarch.Renderers (reference madarch/madarch-renderers.ads:21-97).

Same operations, names and argument meaning as the Ada package; the body calls
the C ABI of include/madarch_hip.h where the reference's body calls OpenGL.
Ada exceptions become `MadarchError` (status in `.status`).  Everything past
`Update_Partitioning` below is what the headless build adds in place of the
window: frame read-back, DDGI state access, per-pass control and timing.
"""
import ctypes as C

import numpy as np

from . import _binding as B
from . import gpu_types, materials, scenes

CPU_Best, CPU_Fast, GPU_Fast = 0, 1, 2  # Partitioning_Update_Method, renderers.ads:93


class Probe_Settings:  # renderers.ads:23-29
    def __init__(self, Radiance_Resolution=32, Irradiance_Resolution=8, Probe_Count=(6, 6),
                 Grid_Dimensions=(4, 3, 3), Grid_Spacing=(2.0, 3.0, 3.0)):
        self.Radiance_Resolution = Radiance_Resolution
        self.Irradiance_Resolution = Irradiance_Resolution
        self.Probe_Count = tuple(Probe_Count)
        self.Grid_Dimensions = tuple(Grid_Dimensions)
        self.Grid_Spacing = tuple(Grid_Spacing)


class Volumetrics_Settings:  # renderers.ads:33-41
    def __init__(self, Enabled=True, Visibility_Resolution=(100, 100, 100), Visibility_Step_Size=0.1,
                 Scattering_Resolution=(250, 250), Scattering_Step_Size=0.1):
        self.Enabled = bool(Enabled)
        self.Visibility_Resolution = tuple(Visibility_Resolution)
        self.Visibility_Step_Size = Visibility_Step_Size
        self.Scattering_Resolution = tuple(Scattering_Resolution)
        self.Scattering_Step_Size = Scattering_Step_Size


Default_Probe_Settings = Probe_Settings()
Default_Volumetrics_Settings = Volumetrics_Settings()
No_Volumetrics = Volumetrics_Settings(Enabled=False)  # renderers.ads:142-143


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


class Renderer:
    def __init__(self, binding, handle, window, scene, probes, volumetrics):
        self._b, self._h = binding, handle
        self.Window, self.Scene, self.Probes, self.Volumetrics = window, scene, probes, volumetrics
        self.Width, self.Height = window.Width, window.Height

    # ---- the reference's operations ------------------------------------------------
    def Render(self):  # renderers.adb:302-321
        self._b.check(self._b.render(self._h))

    def Set_Material(self, Index, Entity):  # renderers.adb:349-367
        alb = np.asarray(Entity.Get(materials.Albedo).data, dtype=np.float32)
        self._b.check(self._b.set_material(
            self._h, int(Index), alb.ctypes.data_as(C.POINTER(C.c_float)),
            float(Entity.Get(materials.Metallic).data), float(Entity.Get(materials.Roughness).data)))

    def Add_Material(self, Entity):  # renderers.adb:369-377
        alb = np.asarray(Entity.Get(materials.Albedo).data, dtype=np.float32)
        out = C.c_int32(-1)
        self._b.check(self._b.add_material(
            self._h, alb.ctypes.data_as(C.POINTER(C.c_float)),
            float(Entity.Get(materials.Metallic).data), float(Entity.Get(materials.Roughness).data),
            C.byref(out)))
        return out.value

    def Set_Primitive(self, Prim, Index, Entity):  # renderers.adb:379-398
        blob = gpu_types.entity_blob(self.Scene._prim_struct[Prim], Entity)
        self._b.check(self._b.set_primitive(self._h, self.Scene.prim_kind_index(Prim), int(Index),
                                            blob, len(blob)))

    def Add_Primitive(self, Prim, Entity):  # renderers.adb:435-456
        blob = gpu_types.entity_blob(self.Scene._prim_struct[Prim], Entity)
        out = C.c_int32(0)
        self._b.check(self._b.add_primitive(self._h, self.Scene.prim_kind_index(Prim), blob, len(blob),
                                            C.byref(out)))
        return out.value

    def Set_Light(self, Index, Lit, Entity):  # renderers.adb:458-483
        blob = gpu_types.entity_blob(self.Scene._light_struct[Lit], Entity)
        self._b.check(self._b.set_light(self._h, int(Index), self.Scene.light_kind_index(Lit), blob,
                                        len(blob)))

    def Set_Camera_Position(self, Position):  # renderers.adb:485-490
        p = np.asarray(Position, dtype=np.float32).reshape(3)
        self._b.check(self._b.set_camera_position(self._h, p.ctypes.data_as(C.POINTER(C.c_float))))

    def Set_Camera_Orientation(self, Orientation):  # renderers.adb:492-497
        """Orientation[i][j] = row i, column j of the 3x3 matrix; sent column-major."""
        m = np.asarray(Orientation, dtype=np.float32).reshape(3, 3)
        cm = np.ascontiguousarray(m.T).reshape(9)
        self._b.check(self._b.set_camera_orientation(self._h, cm.ctypes.data_as(C.POINTER(C.c_float))))

    def Eval_Distance_To(self, Position, Prims):  # renderers.adb:499-526 -> (distance, normal)
        d, n = self.Eval_Distances_To(np.asarray(Position, dtype=np.float32).reshape(1, 3), Prims)
        return float(d[0]), n[0]

    def Update_Partitioning(self, Method=GPU_Fast):  # renderers.adb:757-775
        self._b.check(self._b.update_partitioning(self._h, int(Method)))

    # ---- headless additions -------------------------------------------------------
    def Eval_Distances_To(self, Positions, Prims):
        pts = np.ascontiguousarray(Positions, dtype=np.float32).reshape(-1, 3)
        kinds = np.asarray([self.Scene.prim_kind_index(p) for p in Prims], dtype=np.int32)
        dist = np.empty(len(pts), dtype=np.float32)
        nrm = np.empty((len(pts), 3), dtype=np.float32)
        self._b.check(self._b.eval_distance_to(self._h, len(pts), _fp(pts), _fp(kinds), len(kinds),
                                               _fp(nrm), _fp(dist)))
        return dist, nrm

    # ---- ray queries (raymarching.glsl:4-56), batched on the device beside the frames in flight; they edit nothing
    @staticmethod
    def _rays(Origins, Directions, Max_Dists=None):
        """(n, 3) origins and directions, and a length per ray (a scalar is broadcast): ValueError before any library call"""
        org = np.ascontiguousarray(Origins, dtype=np.float32)
        drs = np.ascontiguousarray(Directions, dtype=np.float32)
        if org.ndim != 2 or org.shape[1] != 3 or drs.shape != org.shape:
            raise ValueError("origins and directions are (n, 3) arrays of one shape, not %s and %s" % (org.shape, drs.shape))
        if Max_Dists is None:
            return org, drs, None
        tmax = np.asarray(Max_Dists, dtype=np.float32)
        if tmax.ndim == 0:
            tmax = np.full(len(org), tmax, dtype=np.float32)
        if tmax.shape != (len(org),):
            raise ValueError("one length per ray: %s for %d rays" % (tmax.shape, len(org)))
        return org, drs, np.ascontiguousarray(tmax)

    def Raycast(self, Origins, Directions):
        """raycast up to the scene's max_dist: {hit, index, t, steps, position, normal} (index as in Read_Gbuffer, -1 = miss)"""
        org, drs, _ = self._rays(Origins, Directions)
        n = len(org)
        out = {"hit": np.zeros(n, np.int32), "index": np.zeros(n, np.int32), "t": np.zeros(n, np.float32),
               "steps": np.zeros(n, np.int32), "position": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32)}
        self._b.check(self._b.raycast(self._h, n, _fp(org), _fp(drs), _fp(out["hit"]), _fp(out["index"]), _fp(out["t"]),
                                      _fp(out["steps"]), _fp(out["position"]), _fp(out["normal"])))
        return out

    def Raycast_Visibility(self, Origins, Directions, Max_Dists):
        """raycast_visibility: 1.0 where the ray reaches its Max_Dists (a scalar is broadcast) without a hit, else 0.0"""
        org, drs, tmax = self._rays(Origins, Directions, Max_Dists)
        vis = np.zeros(len(org), np.float32)
        self._b.check(self._b.raycast_visibility(self._h, len(org), _fp(org), _fp(drs), _fp(tmax), _fp(vis)))
        return vis

    def Softshadows(self, Origins, Directions, Min_Dist, Max_Dists, K):
        """softshadows with the shader's min_dist, max_dist (per ray; a scalar is broadcast) and k"""
        org, drs, tmax = self._rays(Origins, Directions, Max_Dists)
        out = np.zeros(len(org), np.float32)
        self._b.check(self._b.softshadows(self._h, len(org), _fp(org), _fp(drs), float(Min_Dist), _fp(tmax), float(K), _fp(out)))
        return out

    def Ray_Query_Time(self):
        """OPT_TIMING: the kernel time of the last ray query in milliseconds (HIP events on the query stream)"""
        ms = C.c_double(0.0)
        self._b.check(self._b.ray_query_time(self._h, C.byref(ms)))
        return ms.value

    # ---- the same queries for arrays on the device: asynchronous, ordered with a stream of the caller's.  An array is an
    # integer address or any object with data_ptr () -- a torch tensor, which this package never imports
    @staticmethod
    def _device_array(Array, What, Values, Kind, Optional=False):
        """the address of at least `Values` float32 ("float32") or int32 ("int32") values on the device; what the object tells
        about itself (is_cuda, is_contiguous, numel, dtype) is checked: ValueError before any library call"""
        if Array is None:
            if Optional:
                return None
            raise ValueError("%s: an array is required" % What)
        if isinstance(Array, (int, np.integer)):
            return C.c_void_p(int(Array))
        if not hasattr(Array, "data_ptr"):
            raise ValueError("%s: an integer address or an object with data_ptr (), not %s" % (What, type(Array).__name__))
        if hasattr(Array, "is_cuda") and not Array.is_cuda:
            raise ValueError("%s: not on the device" % What)
        if hasattr(Array, "is_contiguous") and not Array.is_contiguous():
            raise ValueError("%s: not contiguous" % What)
        if hasattr(Array, "dtype") and str(Array.dtype).rsplit(".", 1)[-1] != Kind:
            raise ValueError("%s: %s, not %s" % (What, Array.dtype, Kind))
        if hasattr(Array, "numel") and Array.numel() < Values:
            raise ValueError("%s: %d values, %d needed" % (What, Array.numel(), Values))
        return C.c_void_p(int(Array.data_ptr()))

    @staticmethod
    def _ray_count(Origins, N):
        if N is None:
            if not hasattr(Origins, "numel"):
                raise ValueError("N: the number of rays is required with plain addresses")
            N = Origins.numel() // 3
        if int(N) < 0:
            raise ValueError("N: %d rays" % N)
        return int(N)

    def Raycast_Device(self, Origins, Directions, Hit, Index=None, T=None, Steps=None, Position=None, Normal=None, Stream=0, N=None):
        """Raycast for N rays (default: what Origins holds) in device memory, enqueued behind what `Stream` (an integer
        hipStream_t, 0 = the default stream) holds; work given to Stream afterwards sees the answers.  Every output but Hit
        may be None.  A ray that is not finite is not marched: hit = -1, index = -1, the rest 0."""
        n = self._ray_count(Origins, N)
        dev = self._device_array
        args = [dev(Origins, "Origins", 3 * n, "float32"), dev(Directions, "Directions", 3 * n, "float32"), dev(Hit, "Hit", n, "int32"),
                dev(Index, "Index", n, "int32", True), dev(T, "T", n, "float32", True), dev(Steps, "Steps", n, "int32", True),
                dev(Position, "Position", 3 * n, "float32", True), dev(Normal, "Normal", 3 * n, "float32", True)]
        self._b.check(self._b.raycast_device(self._h, n, *args, C.c_void_p(int(Stream))))

    def Raycast_Visibility_Device(self, Origins, Directions, Max_Dists, Visibility, Stream=0, N=None):
        """Raycast_Visibility likewise, one length per ray; NaN for a ray that is not finite or longer than max_dist"""
        n = self._ray_count(Origins, N)
        dev = self._device_array
        args = [dev(Origins, "Origins", 3 * n, "float32"), dev(Directions, "Directions", 3 * n, "float32"),
                dev(Max_Dists, "Max_Dists", n, "float32"), dev(Visibility, "Visibility", n, "float32")]
        self._b.check(self._b.raycast_visibility_device(self._h, n, *args, C.c_void_p(int(Stream))))

    def Softshadows_Device(self, Origins, Directions, Min_Dist, Max_Dists, K, Out, Stream=0, N=None):
        """Softshadows likewise"""
        n = self._ray_count(Origins, N)
        dev = self._device_array
        org, drs = dev(Origins, "Origins", 3 * n, "float32"), dev(Directions, "Directions", 3 * n, "float32")
        tmax, out = dev(Max_Dists, "Max_Dists", n, "float32"), dev(Out, "Out", n, "float32")
        self._b.check(self._b.softshadows_device(self._h, n, org, drs, float(Min_Dist), tmax, float(K), out, C.c_void_p(int(Stream))))

    def Ray_Query_Wait(self):
        """blocks until every device query enqueued so far has ended"""
        self._b.check(self._b.ray_query_wait(self._h))

    # ---- swept spheres and contacts, for a host that owns moving bodies.  Prims = None: the scene as every pass sees it;
    # a tuple of kinds: the exact minimum over those kinds' instances, in the order given (always the shaders' division)
    def _kinds(self, Prims):
        if Prims is None:
            return None, 0
        kinds = np.asarray([self.Scene.prim_kind_index(p) for p in Prims], dtype=np.int32)
        if len(kinds) == 0:
            raise ValueError("Prims: None for the whole scene, or at least one kind")
        return kinds, len(kinds)

    @staticmethod
    def _per_item(Values, n, What):
        """None, or one float32 per ray or centre (a scalar is broadcast): ValueError before any library call"""
        if Values is None:
            return None
        v = np.asarray(Values, dtype=np.float32)
        if v.ndim == 0:
            v = np.full(n, v, dtype=np.float32)
        if v.shape != (n,):
            raise ValueError("%s: one value per ray or centre: %s for %d" % (What, v.shape, n))
        return np.ascontiguousarray(v)

    def Spherecast(self, Origins, Directions, Radii=None, Max_Dists=None, Prims=None):
        """a sphere of radius Radii (None: 0) swept with its centre along every ray up to Max_Dists (None: the scene's
        max_dist): {hit, index, t, steps, position, normal} -- position is the centre at contact, normal the touched
        primitive's normal at that centre"""
        org, drs, tmax = self._rays(Origins, Directions, Max_Dists)
        n = len(org)
        rad = self._per_item(Radii, n, "Radii")
        kinds, nk = self._kinds(Prims)
        out = {"hit": np.zeros(n, np.int32), "index": np.zeros(n, np.int32), "t": np.zeros(n, np.float32),
               "steps": np.zeros(n, np.int32), "position": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32)}
        self._b.check(self._b.spherecast(self._h, n, _fp(org), _fp(drs), None if rad is None else _fp(rad), None if tmax is None else _fp(tmax),
                                         None if kinds is None else _fp(kinds), nk, _fp(out["hit"]), _fp(out["index"]), _fp(out["t"]),
                                         _fp(out["steps"]), _fp(out["position"]), _fp(out["normal"])))
        return out

    def Contacts(self, Centres, Radii=None, Prims=None):
        """one evaluation at every centre: {dist, index, normal}, dist = the scene's distance minus the radius (negative
        where the sphere penetrates), index the closest primitive (-1: none exists), normal its normal at the centre"""
        pts = np.ascontiguousarray(Centres, dtype=np.float32)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("centres are an (n, 3) array, not %s" % (pts.shape,))
        n = len(pts)
        rad = self._per_item(Radii, n, "Radii")
        kinds, nk = self._kinds(Prims)
        out = {"dist": np.zeros(n, np.float32), "index": np.zeros(n, np.int32), "normal": np.zeros((n, 3), np.float32)}
        self._b.check(self._b.contacts(self._h, n, _fp(pts), None if rad is None else _fp(rad), None if kinds is None else _fp(kinds), nk,
                                       _fp(out["dist"]), _fp(out["index"]), _fp(out["normal"])))
        return out

    def Spherecast_Device(self, Origins, Directions, Hit, Radii=None, Max_Dists=None, Prims=None, Index=None, T=None, Steps=None,
                          Position=None, Normal=None, Stream=0, N=None):
        """Spherecast for N rays in device memory under Raycast_Device's contract; Radii and Max_Dists are device arrays or
        None.  A ray, radius or length the host-array call would refuse is not marched: hit = -1, index = -1, the rest 0."""
        n = self._ray_count(Origins, N)
        dev = self._device_array
        kinds, nk = self._kinds(Prims)
        args = [dev(Origins, "Origins", 3 * n, "float32"), dev(Directions, "Directions", 3 * n, "float32"),
                dev(Radii, "Radii", n, "float32", True), dev(Max_Dists, "Max_Dists", n, "float32", True),
                None if kinds is None else _fp(kinds), nk, dev(Hit, "Hit", n, "int32"),
                dev(Index, "Index", n, "int32", True), dev(T, "T", n, "float32", True), dev(Steps, "Steps", n, "int32", True),
                dev(Position, "Position", 3 * n, "float32", True), dev(Normal, "Normal", 3 * n, "float32", True)]
        self._b.check(self._b.spherecast_device(self._h, n, *args, C.c_void_p(int(Stream))))

    def Contacts_Device(self, Centres, Dist, Radii=None, Prims=None, Index=None, Normal=None, Stream=0, N=None):
        """Contacts likewise; a centre or radius the host-array call would refuse is answered with dist = NaN, index = -1"""
        n = self._ray_count(Centres, N)
        dev = self._device_array
        kinds, nk = self._kinds(Prims)
        args = [dev(Centres, "Centres", 3 * n, "float32"), dev(Radii, "Radii", n, "float32", True), None if kinds is None else _fp(kinds), nk,
                dev(Dist, "Dist", n, "float32"), dev(Index, "Index", n, "int32", True), dev(Normal, "Normal", 3 * n, "float32", True)]
        self._b.check(self._b.contacts_device(self._h, n, *args, C.c_void_p(int(Stream))))

    # ---- the scene's surface as a mesh: surface nets over a regular grid (madarch_hip.h: mdh_surface_mesh has the definition).
    # Prims as for Contacts: None, the whole scene, or a tuple of kinds -- (Sphere, Box) meshes the objects without the walls
    @staticmethod
    def _grid(Origin, Spacing, Cells):
        origin = np.ascontiguousarray(Origin, dtype=np.float32)
        cells = np.ascontiguousarray(Cells, dtype=np.int32)
        if origin.shape != (3,) or cells.shape != (3,):
            raise ValueError("a grid has an origin of 3 floats and 3 cell counts, not %s and %s" % (origin.shape, cells.shape))
        return origin, float(Spacing), cells

    def Surface_Mesh(self, Origin, Spacing, Cells, Iso=0.0, Prims=None, Normals=True, Index=True, Field=False):
        """the level set D = Iso over the grid of Cells cubic cells of side Spacing from Origin: {positions (V, 3), quads
        (Q, 4) of vertex ids, normals (V, 3), index (V), field (cz + 1, cy + 1, cx + 1) corner values minus Iso} -- the last
        three where asked for.  Counts first, allocates, and calls again."""
        origin, h, cells = self._grid(Origin, Spacing, Cells)
        kinds, nk = self._kinds(Prims)
        grid = (_fp(origin), h, _fp(cells), float(Iso), None if kinds is None else _fp(kinds), nk)
        counts = np.zeros(2, np.int32)
        self._b.check(self._b.surface_mesh(self._h, *grid, 0, 0, None, None, None, None, None, _fp(counts)))
        nv, nq = int(counts[0]), int(counts[1])
        out = {"positions": np.zeros((nv, 3), np.float32), "quads": np.zeros((nq, 4), np.int32)}
        if Normals:
            out["normals"] = np.zeros((nv, 3), np.float32)
        if Index:
            out["index"] = np.zeros(nv, np.int32)
        if Field:
            out["field"] = np.zeros((int(cells[2]) + 1, int(cells[1]) + 1, int(cells[0]) + 1), np.float32)

        def ptr(key, n):
            return _fp(out[key]) if key in out and n > 0 else None
        self._b.check(self._b.surface_mesh(self._h, *grid, nv, nq, ptr("positions", nv), ptr("normals", nv), ptr("index", nv), ptr("quads", nq),
                                           ptr("field", 1), _fp(counts)))
        if (int(counts[0]), int(counts[1])) != (nv, nq):
            raise RuntimeError("the scene changed between the count and the fill")
        return out

    def Surface_Mesh_Device(self, Origin, Spacing, Cells, Counts, Iso=0.0, Prims=None, Vertex_Capacity=0, Quad_Capacity=0, Positions=None, Normals=None,
                            Index=None, Quads=None, Field=None, Stream=0):
        """the same mesh into device memory under Raycast_Device's contract: tensors or addresses with their capacities, Counts
        (2 int32 on the device) = the vertices and quads found, whatever the capacities; nothing waits"""
        origin, h, cells = self._grid(Origin, Spacing, Cells)
        kinds, nk = self._kinds(Prims)
        nv, nq = int(Vertex_Capacity), int(Quad_Capacity)
        corners = int(np.prod(cells.astype(np.int64) + 1))
        dev = self._device_array
        args = [dev(Positions, "Positions", 3 * nv, "float32", True), dev(Normals, "Normals", 3 * nv, "float32", True), dev(Index, "Index", nv, "int32", True),
                dev(Quads, "Quads", 4 * nq, "int32", True), dev(Field, "Field", corners, "float32", True), dev(Counts, "Counts", 2, "int32")]
        self._b.check(self._b.surface_mesh_device(self._h, _fp(origin), h, _fp(cells), float(Iso), None if kinds is None else _fp(kinds), nk, nv, nq, *args,
                                                  C.c_void_p(int(Stream))))

    # ---- what a ray sees: the frame's pixel program (pixel_color_probes, render_probes.glsl:246-291) along rays of the host's
    @staticmethod
    def _shade_mode(Mode):
        if int(Mode) not in (0, 2):
            raise ValueError("Mode: rays are shaded in mode 0 or 2, not %s (the normal of mode 1 is Raycast's)" % (Mode,))
        return int(Mode)

    def Shade_Rays(self, Origins, Directions, Mode=0, Tone_Map=False):
        """the colour along every ray: {rgb, hit, index, t, steps}.  Mode 0 is the renderer's fixed mode (direct light, the
        probes' irradiance, the reflection's radiance tap, occlusion; OPT_AO_STEPS and OPT_INDIRECT_SPECULAR as they are set),
        mode 2 direct light times occlusion.  Linear colour, or with Tone_Map the bits the framebuffer would hold; a miss is
        the sky along the ray.  No fog, whatever the volumetric settings.  index, t, steps as in Read_Gbuffer."""
        mode = self._shade_mode(Mode)
        org, drs, _ = self._rays(Origins, Directions)
        n = len(org)
        out = {"rgb": np.zeros((n, 3), np.float32), "hit": np.zeros(n, np.int32), "index": np.zeros(n, np.int32),
               "t": np.zeros(n, np.float32), "steps": np.zeros(n, np.int32)}
        self._b.check(self._b.shade_rays(self._h, n, _fp(org), _fp(drs), mode, 1 if Tone_Map else 0, _fp(out["rgb"]), _fp(out["hit"]),
                                         _fp(out["index"]), _fp(out["t"]), _fp(out["steps"])))
        return out

    def Shade_Rays_Device(self, Origins, Directions, Rgb, Hit=None, Index=None, T=None, Steps=None, Mode=0, Tone_Map=False, Stream=0, N=None):
        """Shade_Rays for N rays (default: what Origins holds) in device memory, asynchronous and ordered with `Stream` as
        Raycast_Device is.  Every output but Rgb may be None.  A ray that is not finite, starts beyond 1024 along an axis or has a
        direction component beyond 2 is not shaded: NaN in all three colours, hit = -1, index = -1, t = 0, steps = 0."""
        mode = self._shade_mode(Mode)
        n = self._ray_count(Origins, N)
        dev = self._device_array
        args = [dev(Origins, "Origins", 3 * n, "float32"), dev(Directions, "Directions", 3 * n, "float32")]
        outs = [dev(Rgb, "Rgb", 3 * n, "float32"), dev(Hit, "Hit", n, "int32", True), dev(Index, "Index", n, "int32", True),
                dev(T, "T", n, "float32", True), dev(Steps, "Steps", n, "int32", True)]
        self._b.check(self._b.shade_rays_device(self._h, n, *args, mode, 1 if Tone_Map else 0, *outs, C.c_void_p(int(Stream))))

    @staticmethod
    def _frame_size(Width, Height):
        if int(Width) <= 0 or int(Height) <= 0:
            raise ValueError("a frame of %s x %s pixels" % (Width, Height))
        return int(Width), int(Height)

    def Camera_Rays(self, Width, Height):
        """(origins, directions), each (Width * Height, 3): the rays of a Width x Height frame of the current camera, rows top
        first, computed on the device by the screen pass's own functions -- the frame's rays to the bit"""
        w, h = self._frame_size(Width, Height)
        org = np.zeros((w * h, 3), np.float32)
        drs = np.zeros((w * h, 3), np.float32)
        self._b.check(self._b.camera_rays(self._h, w, h, _fp(org), _fp(drs)))
        return org, drs

    def Camera_Rays_Device(self, Width, Height, Origins, Directions, Stream=0):
        """Camera_Rays into device memory, enqueued on `Stream`"""
        w, h = self._frame_size(Width, Height)
        dev = self._device_array
        org, drs = dev(Origins, "Origins", 3 * w * h, "float32"), dev(Directions, "Directions", 3 * w * h, "float32")
        self._b.check(self._b.camera_rays_device(self._h, w, h, org, drs, C.c_void_p(int(Stream))))

    # ---- what light arrives at a point the host owns: pixel_color_probes from the hit on (render_probes.glsl:253-285)
    POINT_IRRADIANCE = 3

    @staticmethod
    def _point_mode(Mode, Tone_Map):
        if int(Mode) not in (0, 2, 3):
            raise ValueError("Mode: points are shaded in mode 0, 2 or 3 (the irradiance alone), not %s" % (Mode,))
        if int(Mode) == 3 and Tone_Map:
            raise ValueError("Tone_Map: the irradiance of mode 3 is not tone-mapped")
        return int(Mode)

    def Shade_Points(self, Positions, Normals, View_Dirs=None, Material_Ids=None, Mode=0, Tone_Map=False):
        """(n, 3) colours: the light at every point.  Positions and Normals are used as given; View_Dirs is the direction each
        point is seen ALONG (from the eye to the point), Material_Ids the ids Add_Material returned.  Mode 0 is the renderer's
        fixed mode from the hit on (direct light, the probes' irradiance, the reflection's radiance tap, occlusion), mode 2
        direct light times occlusion, mode 3 sample_irradiance alone (View_Dirs and Material_Ids may be None, no tone map).
        No fog.  Points beyond 1024, normals or view directions with a component beyond 1 and unknown materials are refused."""
        mode = self._point_mode(Mode, Tone_Map)
        pos = np.ascontiguousarray(Positions, dtype=np.float32)
        nrm = np.ascontiguousarray(Normals, dtype=np.float32)
        if pos.ndim != 2 or pos.shape[1] != 3 or nrm.shape != pos.shape:
            raise ValueError("positions and normals are (n, 3) arrays of one shape, not %s and %s" % (pos.shape, nrm.shape))
        n = len(pos)
        view = mat = None
        if mode != 3:
            if View_Dirs is None or Material_Ids is None:
                raise ValueError("modes 0 and 2 need View_Dirs and Material_Ids")
            view = np.ascontiguousarray(View_Dirs, dtype=np.float32)
            mat = np.ascontiguousarray(Material_Ids, dtype=np.int32)
            if view.shape != pos.shape or mat.shape != (n,):
                raise ValueError("one view direction and one material id per point: %s and %s for %d points" % (view.shape, mat.shape, n))
        rgb = np.zeros((n, 3), np.float32)
        self._b.check(self._b.shade_points(self._h, n, _fp(pos), _fp(nrm), _fp(view) if view is not None else None,
                                           _fp(mat) if mat is not None else None, mode, 1 if Tone_Map else 0, _fp(rgb)))
        return rgb

    def Shade_Points_Device(self, Positions, Normals, View_Dirs, Material_Ids, Rgb, Mode=0, Tone_Map=False, Stream=0, N=None):
        """Shade_Points for N points (default: what Positions holds) in device memory, asynchronous and ordered with `Stream`
        as Shade_Rays_Device is.  View_Dirs and Material_Ids may be None in mode 3.  A point that is not shaded (see
        Shade_Points) is answered with NaN in all three colours."""
        mode = self._point_mode(Mode, Tone_Map)
        n = self._ray_count(Positions, N)
        dev = self._device_array
        args = [dev(Positions, "Positions", 3 * n, "float32"), dev(Normals, "Normals", 3 * n, "float32"),
                dev(View_Dirs, "View_Dirs", 3 * n, "float32", mode == 3), dev(Material_Ids, "Material_Ids", n, "int32", mode == 3)]
        rgb = dev(Rgb, "Rgb", 3 * n, "float32")
        self._b.check(self._b.shade_points_device(self._h, n, *args, mode, 1 if Tone_Map else 0, rgb, C.c_void_p(int(Stream))))

    def Primitive_Material(self, Index):
        """the material id of every primitive index (the numbering of Read_Gbuffer and Raycast), -1 for -1 and for an index no
        primitive has: a lookup on the host, which feeds Raycast's hits to Shade_Points"""
        idx = np.ascontiguousarray(Index, dtype=np.int32)
        out = np.full(idx.shape, -1, np.int32)
        flat = np.ascontiguousarray(idx.reshape(-1))
        res = np.zeros(len(flat), np.int32)
        self._b.check(self._b.primitive_material(self._h, len(flat), _fp(flat), _fp(res)))
        out.reshape(-1)[:] = res
        return out

    # ---- ground truth for the probes: a path tracer along rays of the host's (the reference's render_path.glsl made to run)
    MAX_BOUNCES = 6

    @staticmethod
    def _path_args(Seed, Id_First, Sample_First, Sample_Count, Bounces):
        """ValueError before any library call"""
        if not 0 <= int(Bounces) <= Renderer.MAX_BOUNCES:
            raise ValueError("Bounces: paths take 0 to %d bounces, not %s" % (Renderer.MAX_BOUNCES, Bounces))
        if int(Sample_First) < 0 or int(Sample_Count) < 0 or int(Sample_First) + int(Sample_Count) > 2 ** 31 - 1:
            raise ValueError("samples %s .. + %s: both at least 0, their sum below 2^31" % (Sample_First, Sample_Count))
        for what, v in (("Seed", Seed), ("Id_First", Id_First)):
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError("%s: a 32-bit unsigned word, not %s" % (what, v))
        return int(Seed), int(Id_First), int(Sample_First), int(Sample_Count), int(Bounces)

    def Path_Trace(self, Origins, Directions, Seed=0, Id_First=0, Sample_First=0, Sample_Count=1, Bounces=3, Rgb_Accum=None):
        """{rgb, hit, index, t}: rgb is Rgb_Accum (zeros when None; never modified) plus the sum of samples Sample_First ..
        Sample_First + Sample_Count - 1 of the path tracer along every ray -- direct light at every hit, the masked sky at a
        miss, up to Bounces bounces; linear, to be divided by the number of samples.  Ray i has id Id_First + i and its random
        numbers depend on (Seed, id, sample, bounce) alone; a run of samples split over calls has the bits of one call.  hit,
        index and t describe the primary segment.  No fog, no atlas, no occlusion."""
        seed, id0, s0, sc, nb = self._path_args(Seed, Id_First, Sample_First, Sample_Count, Bounces)
        org, drs, _ = self._rays(Origins, Directions)
        n = len(org)
        if Rgb_Accum is None:
            rgb = np.zeros((n, 3), np.float32)
        else:
            rgb = np.array(Rgb_Accum, dtype=np.float32, order="C")
            if rgb.shape != (n, 3):
                raise ValueError("Rgb_Accum: one colour per ray, not %s for %d rays" % (rgb.shape, n))
        out = {"rgb": rgb, "hit": np.zeros(n, np.int32), "index": np.full(n, -1, np.int32), "t": np.zeros(n, np.float32)}
        self._b.check(self._b.path_trace(self._h, n, _fp(org), _fp(drs), seed, id0, s0, sc, nb, _fp(rgb), _fp(out["hit"]),
                                         _fp(out["index"]), _fp(out["t"])))
        return out

    def Path_Trace_Device(self, Origins, Directions, Rgb_Accum, Hit=None, Index=None, T=None, Seed=0, Id_First=0, Sample_First=0,
                          Sample_Count=1, Bounces=3, Stream=0, N=None):
        """Path_Trace for N rays (default: what Origins holds) in device memory, asynchronous and ordered with `Stream` as
        Shade_Rays_Device is; the samples are added to Rgb_Accum in place, which stays on the device from call to call.  A ray
        that is not finite, starts beyond 1024 or has a direction component beyond 2 is not traced: NaN in all three colours,
        hit = -1, index = -1, t = 0."""
        seed, id0, s0, sc, nb = self._path_args(Seed, Id_First, Sample_First, Sample_Count, Bounces)
        n = self._ray_count(Origins, N)
        dev = self._device_array
        args = [dev(Origins, "Origins", 3 * n, "float32"), dev(Directions, "Directions", 3 * n, "float32")]
        outs = [dev(Rgb_Accum, "Rgb_Accum", 3 * n, "float32"), dev(Hit, "Hit", n, "int32", True), dev(Index, "Index", n, "int32", True),
                dev(T, "T", n, "float32", True)]
        self._b.check(self._b.path_trace_device(self._h, n, *args, seed, id0, s0, sc, nb, *outs, C.c_void_p(int(Stream))))

    @staticmethod
    def Path_Scatter(Directions, Normals, Roughness, Seed=0, Id_First=0, Sample=0, Bounce=0, Binding=None):
        """(n, 3) directions: where the path of ray Id_First + i goes behind bounce `Bounce` of sample `Sample`, having arrived
        along Directions[i] at a surface with Normals[i] (any length but 0) and Roughness[i] (a scalar is broadcast).  The
        sampler of Path_Trace by itself, on the host, the same bits: no launch and no renderer."""
        b = Binding or B.hip_binding()
        drs = np.ascontiguousarray(Directions, dtype=np.float32)
        nrm = np.ascontiguousarray(Normals, dtype=np.float32)
        if drs.ndim != 2 or drs.shape[1] != 3 or nrm.shape != drs.shape:
            raise ValueError("directions and normals are (n, 3) arrays of one shape, not %s and %s" % (drs.shape, nrm.shape))
        n = len(drs)
        rough = np.asarray(Roughness, dtype=np.float32)
        if rough.ndim == 0:
            rough = np.full(n, rough, dtype=np.float32)
        if rough.shape != (n,):
            raise ValueError("one roughness per direction: %s for %d" % (rough.shape, n))
        rough = np.ascontiguousarray(rough)
        if int(Sample) < 0 or int(Bounce) < 0:
            raise ValueError("sample %s, bounce %s: both at least 0" % (Sample, Bounce))
        for what, v in (("Seed", Seed), ("Id_First", Id_First)):
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError("%s: a 32-bit unsigned word, not %s" % (what, v))
        out = np.zeros((n, 3), np.float32)
        b.check(b.path_scatter(n, _fp(drs), _fp(nrm), _fp(rough), int(Seed), int(Id_First), int(Sample), int(Bounce), _fp(out)))
        return out

    # ---- a path-traced frame: Path_Trace's estimator over the pixels of a frame of the camera, the sums kept on the device
    @staticmethod
    def _path_frame_args(Width, Height, Seed, Bounces, Jitter):
        """ValueError before any library call"""
        w, h = Renderer._frame_size(Width, Height)
        if w * h > B.PATH_FRAME_MAX_PIXELS:
            raise ValueError("a path-traced frame has at most 2^26 pixels, not %d x %d" % (w, h))
        if not 0 <= int(Bounces) <= Renderer.MAX_BOUNCES:
            raise ValueError("Bounces: paths take 0 to %d bounces, not %s" % (Renderer.MAX_BOUNCES, Bounces))
        if not 0 <= int(Seed) < 2 ** 32:
            raise ValueError("Seed: a 32-bit unsigned word, not %s" % (Seed,))
        return w, h, int(Seed), int(Bounces), Renderer._flag(Jitter, "Jitter")

    @staticmethod
    def _flag(Value, What):
        if isinstance(Value, (bool, np.bool_)) or (isinstance(Value, (int, np.integer)) and int(Value) in (0, 1)):
            return int(Value)
        raise ValueError("%s: True or False (0 or 1), not %r" % (What, Value))

    def Path_Frame_Begin(self, Width, Height, Seed=0, Bounces=3, Jitter=True):
        """opens, or restarts from zero, the renderer's accumulator of Width x Height pixels (any size, not the window's; at most
        2^26 pixels): three float32 sums a pixel on the device.  The camera is captured as it stands, and Seed, Bounces and
        Jitter are fixed.  Pixel (i, j), row 0 at the top, has the ray id j * Width + i; with Jitter every sample's ray goes
        through its own point of the pixel's footprint, without it through the centre: Camera_Rays' rays to the bit."""
        w, h, seed, nb, jit = self._path_frame_args(Width, Height, Seed, Bounces, Jitter)
        self._b.check(self._b.path_frame_begin(self._h, w, h, seed, nb, jit))

    @staticmethod
    def _path_rule_args(Min_Samples, Max_Samples, Tolerance, Floor):
        """ValueError before any library call"""
        lo, hi = int(Min_Samples), int(Max_Samples)
        if not 1 <= lo <= hi <= B.PATH_MAX_SAMPLES:
            raise ValueError("1 <= Min_Samples <= Max_Samples <= 2^24, not %s and %s" % (Min_Samples, Max_Samples))
        tol, floor = float(Tolerance), float(Floor)
        for what, v in (("Tolerance", tol), ("Floor", floor)):
            if not (np.isfinite(v) and 0.0 <= v <= float(np.finfo(np.float32).max)):
                raise ValueError("%s: finite and at least 0, not %s" % (what, v))
        return lo, hi, tol, floor

    def Path_Frame_Begin_Adaptive(self, Width, Height, Seed=0, Bounces=3, Jitter=True, Min_Samples=4, Max_Samples=64, Tolerance=0.05, Floor=0.01):
        """Path_Frame_Begin for an ADAPTIVE accumulator: beside its sums a pixel holds the count n of its samples and the moments
        m1, m2 of y = (r + g) + b.  Path_Frame_Accumulate (k) is then one round: every pixel still active under the rule
        takes min (k, Max_Samples - n) more samples; a pixel is active while n < Max_Samples and (n < Min_Samples or the
        variance of its mean exceeds (Tolerance * (mean + Floor))^2), evaluated at round boundaries only -- two rounds of 2
        are not one round of 4.  A pixel's k-th sample has sample index k.  A stopping rule on a biased variance estimate:
        the image is not claimed to be unbiased, Min_Samples is the caller's guard."""
        w, h, seed, nb, jit = self._path_frame_args(Width, Height, Seed, Bounces, Jitter)
        lo, hi, tol, floor = self._path_rule_args(Min_Samples, Max_Samples, Tolerance, Floor)
        self._b.check(self._b.path_frame_begin_adaptive(self._h, w, h, seed, nb, jit, lo, hi, tol, floor))

    def Path_Frame_Stats(self, Count=True, Moments=True):
        """{count (H, W) int32, moments (H, W, 2) float32 = (m1, m2), active, total_samples} of the adaptive accumulator: active is
        the number of pixels the rule keeps running now, total_samples the sum of the counts.  Waits for the device."""
        info = self.Path_Frame_Info()
        w, h = info["width"], info["height"]
        out = {}
        if Count:
            out["count"] = np.zeros((h, w), np.int32)
        if Moments:
            out["moments"] = np.zeros((h, w, 2), np.float32)
        active, total = C.c_int64(0), C.c_int64(0)
        ptr = [_fp(out[k]) if k in out and out[k].size else None for k in ("count", "moments")]
        self._b.check(self._b.path_frame_stats(self._h, ptr[0], ptr[1], C.cast(C.byref(active), C.c_void_p), C.cast(C.byref(total), C.c_void_p)))
        out["active"], out["total_samples"] = active.value, total.value
        return out

    def Path_Frame_Stats_Device(self, Width, Height, Count=None, Moments=None, Active=None, Total_Samples=None, Stream=0):
        """Path_Frame_Stats into device memory, asynchronous and ordered with `Stream`; Width and Height are the accumulator's.
        Count holds one int32 a pixel, Moments two float32, Active and Total_Samples one int64 each; each may be None."""
        w, h = self._frame_size(Width, Height)
        dev = self._device_array
        args = [dev(Count, "Count", w * h, "int32", True), dev(Moments, "Moments", 2 * w * h, "float32", True), dev(Active, "Active", 1, "int64", True),
                dev(Total_Samples, "Total_Samples", 1, "int64", True)]
        self._b.check(self._b.path_frame_stats_device(self._h, *args, C.c_void_p(int(Stream))))

    @staticmethod
    def Path_Pixel_Active(Count, M1, M2, Min_Samples, Max_Samples, Tolerance, Floor, Binding=None):
        """(n,) bool: the stopping rule of an adaptive frame for the states (Count[q], M1[q], M2[q]), on the host, the function
        the lanes call -- no launch and no renderer"""
        lo, hi, tol, floor = Renderer._path_rule_args(Min_Samples, Max_Samples, Tolerance, Floor)
        count = np.ascontiguousarray(Count, dtype=np.int32)
        m1, m2 = np.ascontiguousarray(M1, dtype=np.float32), np.ascontiguousarray(M2, dtype=np.float32)
        if count.ndim != 1 or m1.shape != count.shape or m2.shape != count.shape:
            raise ValueError("Count, M1 and M2 are (n,) arrays of one length, not %s, %s and %s" % (count.shape, m1.shape, m2.shape))
        b = Binding or B.hip_binding()
        n = len(count)
        out = np.zeros(n, np.uint8)
        b.check(b.path_pixel_active(n, _fp(count) if n else None, _fp(m1) if n else None, _fp(m2) if n else None, lo, hi, tol, floor, _fp(out) if n else None))
        return out.astype(bool)

    def Path_Frame_Accumulate(self, Sample_Count=1):
        """adds the next Sample_Count samples to every pixel and returns without waiting for the device.  The scene is the one
        committed at the call; nothing is edited.  Restarting after an edit (Path_Frame_Begin again) is the caller's business.
        Under OPT_TIMING Ray_Query_Time gives the kernel's time.  On an adaptive accumulator (Path_Frame_Begin_Adaptive) it is
        one round: the pixels the rule keeps running take up to Sample_Count samples, and the resolve divides by each pixel's own
        count."""
        if int(Sample_Count) < 0 or int(Sample_Count) > 2 ** 31 - 1:
            raise ValueError("Sample_Count: %s samples" % (Sample_Count,))
        self._b.check(self._b.path_frame_accumulate(self._h, int(Sample_Count)))

    def Path_Frame_Info(self):
        """{width, height, samples, bounces, jitter} of the accumulator; all 0 while none is open"""
        v = [C.c_int32(0) for _ in range(5)]
        self._b.check(self._b.path_frame_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("width", "height", "samples", "bounces", "jitter"), (x.value for x in v)))

    def Path_Frame_Read(self, Tone_Map=False, Rgb=True, Rgba8=False, Sums=False):
        """the resolve, on the device: {rgb (H, W, 3) float32 = sums / samples, with Tone_Map draw_screen.glsl:29 applied as
        Shade_Rays applies it; rgba8 (H, W, 4) uint8 = that colour as the window's pixels hold it; sums (H, W, 3) the raw sums;
        samples}, rows top first; only what was asked for is computed and copied.  On an adaptive accumulator rgb = sums / the
        pixel's own count (Path_Frame_Stats), and samples is the largest count a pixel can hold."""
        tm = self._flag(Tone_Map, "Tone_Map")
        info = self.Path_Frame_Info()
        w, h = info["width"], info["height"]
        out = {}
        if Rgb:
            out["rgb"] = np.zeros((h, w, 3), np.float32)
        if Rgba8:
            out["rgba8"] = np.zeros((h, w, 4), np.uint8)
        if Sums:
            out["sums"] = np.zeros((h, w, 3), np.float32)
        n = C.c_int32(0)
        ptr = [_fp(out[k]) if k in out and out[k].size else None for k in ("rgb", "rgba8", "sums")]
        self._b.check(self._b.path_frame_read(self._h, tm, ptr[0], ptr[1], ptr[2], C.byref(n)))
        out["samples"] = n.value
        return out

    def Path_Frame_Read_Device(self, Width, Height, Rgb=None, Rgba8=None, Sums=None, Tone_Map=False, Stream=0):
        """Path_Frame_Read into device memory, asynchronous and ordered with `Stream` as Shade_Rays_Device is; Width and Height
        are the accumulator's (what the arrays are checked against here).  Rgb and Sums hold 3 float32 a pixel, Rgba8 one
        int32 (the four bytes) a pixel; each may be None.  Returns the number of samples."""
        tm = self._flag(Tone_Map, "Tone_Map")
        w, h = self._frame_size(Width, Height)
        dev = self._device_array
        args = [dev(Rgb, "Rgb", 3 * w * h, "float32", True), dev(Rgba8, "Rgba8", w * h, "int32", True), dev(Sums, "Sums", 3 * w * h, "float32", True)]
        n = C.c_int32(0)
        self._b.check(self._b.path_frame_read_device(self._h, tm, *args, C.byref(n), C.c_void_p(int(Stream))))
        return n.value

    @staticmethod
    def _sample(Sample):
        if not 0 <= int(Sample) <= 2 ** 31 - 1:
            raise ValueError("Sample: %s" % (Sample,))
        return int(Sample)

    def Path_Frame_Rays(self, Sample=0):
        """(origins, directions), each (Width * Height, 3): the rays the accumulator gives its pixels for sample `Sample`,
        computed on the device by the functions the accumulating kernel calls"""
        s = self._sample(Sample)
        info = self.Path_Frame_Info()
        n = info["width"] * info["height"]
        org = np.zeros((n, 3), np.float32)
        drs = np.zeros((n, 3), np.float32)
        self._b.check(self._b.path_frame_rays(self._h, s, _fp(org) if n else None, _fp(drs) if n else None))
        return org, drs

    def Path_Frame_Rays_Device(self, Width, Height, Origins, Directions, Sample=0, Stream=0):
        """Path_Frame_Rays into device memory, enqueued on `Stream`; Width and Height are the accumulator's"""
        s = self._sample(Sample)
        w, h = self._frame_size(Width, Height)
        dev = self._device_array
        org, drs = dev(Origins, "Origins", 3 * w * h, "float32"), dev(Directions, "Directions", 3 * w * h, "float32")
        self._b.check(self._b.path_frame_rays_device(self._h, s, org, drs, C.c_void_p(int(Stream))))

    def Path_Frame_End(self):
        """frees the accumulator (Destroy does too)"""
        self._b.check(self._b.path_frame_end(self._h))

    @staticmethod
    def Path_Pixel_Uv(Width, Height, Seed=0, Id_First=0, N=None, Sample=0, Jitter=True, Binding=None):
        """(N, 2) screen positions (u, v) of the pixels with ids Id_First .. Id_First + N - 1 (default: to the frame's end) of a
        Width x Height frame for sample `Sample`: the jitter of Path_Frame_Accumulate by itself, on the host, the same bits --
        no launch and no renderer"""
        w, h, seed, _, jit = Renderer._path_frame_args(Width, Height, Seed, 0, Jitter)
        s = Renderer._sample(Sample)
        if not 0 <= int(Id_First) <= w * h:
            raise ValueError("Id_First: a pixel of the frame, not %s" % (Id_First,))
        n = w * h - int(Id_First) if N is None else int(N)
        if n < 0 or int(Id_First) + n > w * h:
            raise ValueError("N: %s pixels from %s on in a frame of %d" % (N, Id_First, w * h))
        b = Binding or B.hip_binding()
        uv = np.zeros((n, 2), np.float32)
        b.check(b.path_pixel_uv(w, h, seed, int(Id_First), n, s, jit, _fp(uv) if n else None))
        return uv

    # ---- the lights' fog at points and along rays of the host's (compute_frustrum_visibility.glsl:8-19,
    # accumulate_scattering.glsl:17-28), without the froxel grid or the camera it is bound to; ray-query plumbing, nothing edited
    INSCATTER_MAX_STEPS = 4096

    @staticmethod
    def _inscatter_step(March, Step):
        """ValueError before any library call (max_dist / Step <= INSCATTER_MAX_STEPS is the library's check: it knows max_dist)"""
        if isinstance(March, (bool, np.bool_)):
            March = int(March)
        if not isinstance(March, (int, np.integer)) or int(March) not in (0, 1):
            raise ValueError("March: 0 or 1, not %r" % (March,))
        step = float(Step)
        if not np.isfinite(step) or not step > 0.0:
            raise ValueError("Step: finite and above 0, not %r" % (Step,))
        return int(March), step

    def Inscatter_Points(self, Positions, Directions, F=None):
        """(n, 3) colours: sample_lights (position, direction) of the visibility pass -- what reaches each point from every
        light through the fog, times tau and the phase function towards `direction`, used as given.  With F (one distance
        per point; a scalar is broadcast) each colour is multiplied by exp (-F tau): the scattering pass's product."""
        pos, drs, f = self._rays(Positions, Directions, F)
        rgb = np.zeros((len(pos), 3), np.float32)
        self._b.check(self._b.inscatter_points(self._h, len(pos), _fp(pos), _fp(drs), _fp(f) if f is not None else None, _fp(rgb)))
        return rgb

    def Inscatter_Rays(self, Origins, Directions, Max_Dists, Step, March=False):
        """{rgb, len, steps}: the in-scattered light along every ray -- L = 0; for (f = 0; f < len; f += Step) L = L +
        inscatter ((dir * f) + org, dir) * exp (-f tau); rgb = L * Step, in fp32 and in this order.  len is Max_Dists (per ray;
        a scalar is broadcast; within 0 .. max_dist), or with March the distance to what the ray hits where that is shorter.
        steps counts the loop's turns.  Independent of the renderer's volumetric settings."""
        march, step = self._inscatter_step(March, Step)
        org, drs, tmax = self._rays(Origins, Directions, Max_Dists)
        if tmax is None:
            raise ValueError("Max_Dists: a length per ray is required")
        n = len(org)
        out = {"rgb": np.zeros((n, 3), np.float32), "len": np.zeros(n, np.float32), "steps": np.zeros(n, np.int32)}
        self._b.check(self._b.inscatter_rays(self._h, n, _fp(org), _fp(drs), _fp(tmax), march, step, _fp(out["rgb"]), _fp(out["len"]),
                                             _fp(out["steps"])))
        return out

    def Inscatter_Points_Device(self, Positions, Directions, Rgb, F=None, Stream=0, N=None):
        """Inscatter_Points for N points (default: what Positions holds) in device memory, asynchronous and ordered with
        `Stream` as Raycast_Device is.  F may be None.  A point with a component that is not finite gets NaN in all three colours."""
        n = self._ray_count(Positions, N)
        dev = self._device_array
        args = [dev(Positions, "Positions", 3 * n, "float32"), dev(Directions, "Directions", 3 * n, "float32"),
                dev(F, "F", n, "float32", True), dev(Rgb, "Rgb", 3 * n, "float32")]
        self._b.check(self._b.inscatter_points_device(self._h, n, *args, C.c_void_p(int(Stream))))

    def Inscatter_Rays_Device(self, Origins, Directions, Max_Dists, Step, Rgb, Len=None, Steps=None, March=False, Stream=0, N=None):
        """Inscatter_Rays likewise, one length per ray in device memory; Len and Steps may be None.  A ray that is not finite, or
        whose length is not finite, negative or beyond max_dist, is not marched: NaN in rgb and len, -1 steps."""
        march, step = self._inscatter_step(March, Step)
        n = self._ray_count(Origins, N)
        dev = self._device_array
        args = [dev(Origins, "Origins", 3 * n, "float32"), dev(Directions, "Directions", 3 * n, "float32"),
                dev(Max_Dists, "Max_Dists", n, "float32")]
        outs = [dev(Rgb, "Rgb", 3 * n, "float32"), dev(Len, "Len", n, "float32", True), dev(Steps, "Steps", n, "int32", True)]
        self._b.check(self._b.inscatter_rays_device(self._h, n, *args, march, step, *outs, C.c_void_p(int(Stream))))

    def Render_Pass(self, Pass):
        self._b.check(self._b.render_pass(self._h, int(Pass)))

    # Render in three steps, for the sharded runs that exchange atlas slices between the passes
    def Frame_Begin(self):
        self._b.check(self._b.frame_begin(self._h))

    def Frame_Probe_Pass(self, Pass):
        self._b.check(self._b.frame_probe_pass(self._h, int(Pass)))

    def Frame_Exchange(self, Tex):
        """all-gather of the ranks' slices of an atlas, inside the library (needs Comm_Init; nothing without)"""
        self._b.check(self._b.frame_exchange(self._h, int(Tex)))

    def Frame_End(self):
        self._b.check(self._b.frame_end(self._h))

    # ---- one frame on N GPUs, one process per GPU: the communicator lives inside the library (RCCL)
    def Comm_Unique_Id(self):
        """rank 0: the 128 bytes every rank hands to Comm_Init"""
        buf = (C.c_uint8 * B.COMM_ID_BYTES)()
        self._b.check(self._b.comm_unique_id(buf))
        return bytes(buf)

    def Comm_Init(self, Id, Rank, World):
        """collective: from here on Render of every rank is one frame of the sharded schedule"""
        if len(Id) != B.COMM_ID_BYTES:
            raise ValueError("a communicator id is %d bytes" % B.COMM_ID_BYTES)
        buf = (C.c_uint8 * B.COMM_ID_BYTES).from_buffer_copy(Id)
        self._b.check(self._b.comm_init(self._h, buf, int(Rank), int(World)))

    def Comm_Available(self):
        """can this process load librccl at all?  (what a rank other than 0 asks before the collective join)"""
        self._b.check(self._b.comm_available())

    def Peer_Export(self):
        """this rank's interprocess handles (radiance atlases, events, a shared-memory block): 512 bytes for every rank"""
        buf = (C.c_uint8 * B.PEER_BLOB_BYTES)()
        self._b.check(self._b.peer_export(self._h, buf))
        return bytes(buf)

    def Peer_Init(self, Blobs, Rank, World):
        """every rank, with all ranks' Peer_Export blobs in rank order: Render is then the sharded frame, its exchange
        being device-to-device copies out of the peers' atlases (Comm_Destroy leaves)"""
        Blobs = b"".join(Blobs) if not isinstance(Blobs, (bytes, bytearray)) else bytes(Blobs)
        if len(Blobs) != B.PEER_BLOB_BYTES * int(World):
            raise ValueError("one %d-byte blob per rank" % B.PEER_BLOB_BYTES)
        buf = (C.c_uint8 * len(Blobs)).from_buffer_copy(Blobs)
        self._b.check(self._b.peer_init(self._h, buf, int(Rank), int(World)))

    def Comm_Destroy(self):
        self._b.check(self._b.comm_destroy(self._h))

    def Comm_Abort(self):
        self._b.check(self._b.comm_abort(self._h))

    def Comm_Barrier(self):
        self._b.check(self._b.comm_barrier(self._h))

    def Comm_Max(self, Value):
        v = C.c_double(float(Value))
        self._b.check(self._b.comm_max_f64(self._h, C.byref(v)))
        return v.value

    def Comm_Reduce_Framebuffer(self, Root=0):
        self._b.check(self._b.comm_reduce_framebuffer(self._h, int(Root)))

    def Finish(self):
        self._b.check(self._b.finish(self._h))

    def Set_Option(self, Option, Value):
        self._b.check(self._b.set_option(self._h, int(Option), int(Value)))

    def Get_Option(self, Option):
        v = C.c_int32(0)
        self._b.check(self._b.get_option(self._h, int(Option), C.byref(v)))
        return v.value

    def Read_Framebuffer(self):
        out = np.empty((self.Height, self.Width, 3), dtype=np.float32)
        self._b.check(self._b.read_framebuffer(self._h, _fp(out)))
        return out

    def Swap_Buffers(self):
        """Glfw.Windows.Context.Swap_Buffers at the end of Render (madarch-renderers.adb:320): the last
        frame becomes the window's RGBA8 pixels, converted on the device and copied to pinned host
        memory behind the frame; returns without waiting, frames stay in flight."""
        self._b.check(self._b.swap_buffers(self._h))

    def Front_Buffer(self, copy=True):
        """The pixels of the most recent Swap_Buffers: (H, W, 4) uint8, R G B A, row 0 = top.  Waits for
        that swap only.  copy=False returns a view of the renderer's buffer, valid until the second
        next Swap_Buffers."""
        ptr, n = C.c_void_p(), C.c_int64()
        self._b.check(self._b.front_buffer(self._h, C.byref(ptr), C.byref(n)))
        buf = (C.c_uint8 * (self.Height * self.Width * 4)).from_address(ptr.value)
        img = np.frombuffer(buf, dtype=np.uint8).reshape(self.Height, self.Width, 4)
        return img.copy() if copy else img

    def Read_Gbuffer(self):
        idx = np.empty((self.Height, self.Width), dtype=np.int32)
        t = np.empty((self.Height, self.Width), dtype=np.float32)
        steps = np.empty((self.Height, self.Width), dtype=np.int32)
        self._b.check(self._b.read_gbuffer(self._h, _fp(idx), _fp(t), _fp(steps)))
        return idx, t, steps

    def Texture_Shape(self, Tex):
        w, h, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._b.check(self._b.read_texture(self._h, int(Tex), None, C.byref(w), C.byref(h), C.byref(c)))
        return h.value, w.value, c.value

    def Read_Texture(self, Tex):
        shape = self.Texture_Shape(Tex)
        out = np.empty(shape, dtype=np.float32)
        w, h, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._b.check(self._b.read_texture(self._h, int(Tex), _fp(out), C.byref(w), C.byref(h), C.byref(c)))
        return out

    def Write_Texture(self, Tex, Data):
        a = np.ascontiguousarray(Data, dtype=np.float32)
        self._b.check(self._b.write_texture(self._h, int(Tex), _fp(a), a.shape[1], a.shape[0], a.shape[2]))

    def Probe_Total(self):
        return self.Probes.Probe_Count[0] * self.Probes.Probe_Count[1]

    def Read_Atlas_Slice(self, Tex, Probe_Begin, N_Probes):
        res = self.Probes.Radiance_Resolution if Tex == B.TEX_RADIANCE else self.Probes.Irradiance_Resolution
        out = np.empty((N_Probes, res, res, 3), dtype=np.float32)
        self._b.check(self._b.read_atlas_slice(self._h, int(Tex), int(Probe_Begin), int(N_Probes), _fp(out)))
        return out

    def Write_Atlas_Slice(self, Tex, Probe_Begin, Data):
        a = np.ascontiguousarray(Data, dtype=np.float32)
        self._b.check(self._b.write_atlas_slice(self._h, int(Tex), int(Probe_Begin), a.shape[0], _fp(a)))

    def Pass_Time(self, Pass):
        ms, n = C.c_double(0.0), C.c_int64(0)
        self._b.check(self._b.pass_time(self._h, int(Pass), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def Radiance_Replay_Stats(self):
        """OPT_RADIANCE_REPLAY: radiance passes since creation that (marched, marched and recorded, replayed)."""
        v = [C.c_int64(0) for _ in range(3)]
        self._b.check(self._b.radiance_replay_stats(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def Probe_Settle_Stats(self):
        """OPT_PROBE_SETTLE: (run of unchanged irradiance passes under the present inputs, probe passes not launched
        since creation, texels the newest observed pass changed)."""
        v = [C.c_int64(0) for _ in range(3)]
        self._b.check(self._b.probe_settle_stats(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def Screen_Replay_Stats(self):
        """OPT_SCREEN_REPLAY: screen passes since creation that (marched, marched and recorded, replayed)."""
        v = [C.c_int64(0) for _ in range(3)]
        self._b.check(self._b.screen_replay_stats(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def Reset_Pass_Times(self):
        self._b.check(self._b.reset_pass_times(self._h))

    def Scene_Layout(self, Is_Light, Kind_Ix):
        v = [C.c_int32() for _ in range(4)]
        self._b.check(self._b.scene_layout(self._h, int(Is_Light), int(Kind_Ix), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)  # count offset, array offset, stride, element size

    def Scene_Buffer_Size(self):
        s, t = C.c_int32(), C.c_int32()
        self._b.check(self._b.scene_buffer_size(self._h, C.byref(s), C.byref(t)))
        return s.value, t.value

    def Read_Scene_Buffer(self):
        n, _ = self.Scene_Buffer_Size()
        out = np.empty(n, dtype=np.uint8)
        self._b.check(self._b.read_scene_buffer(self._h, _fp(out), n))
        return out

    def Read_Partitioning(self):
        p = self.Scene.Partitioning_Config
        cells = p.Grid_Dimensions[0] * p.Grid_Dimensions[1] * p.Grid_Dimensions[2]
        width = len(self.Scene.Prims_Count) + p.Index_Count
        out = np.empty((cells, width), dtype=np.int32)
        self._b.check(self._b.read_partitioning(self._h, _fp(out), out.size))
        return out

    def Partition_Warnings(self):
        return self._b.partition_warnings(self._h)

    def Destroy(self):
        if self._h is not None:
            self._b.destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.Destroy()
        except Exception:
            pass


def Create(Window, Scene, Probes=None, Volumetrics=None, Device=0, Binding=None):
    """Renderers.Create (madarch-renderers.adb:91-300).  `Binding` defaults to the
    HIP library; there is no CPU implementation in this package."""
    b = Binding if Binding is not None else B.hip_binding()
    Probes = Probes if Probes is not None else Default_Probe_Settings
    Volumetrics = Volumetrics if Volumetrics is not None else Default_Volumetrics_Settings
    desc, keep = Scene._desc()
    ps = B.mdh_probe_settings()
    ps.radiance_resolution = Probes.Radiance_Resolution
    ps.irradiance_resolution = Probes.Irradiance_Resolution
    ps.probe_count = (C.c_int32 * 2)(*Probes.Probe_Count)
    ps.grid_dimensions = (C.c_int32 * 3)(*Probes.Grid_Dimensions)
    ps.grid_spacing = (C.c_float * 3)(*Probes.Grid_Spacing)
    vs = B.mdh_volumetrics()
    vs.enabled = 1 if Volumetrics.Enabled else 0
    vs.visibility_resolution = (C.c_int32 * 3)(*Volumetrics.Visibility_Resolution)
    vs.visibility_step_size = Volumetrics.Visibility_Step_Size
    vs.scattering_resolution = (C.c_int32 * 2)(*Volumetrics.Scattering_Resolution)
    vs.scattering_step_size = Volumetrics.Scattering_Step_Size
    handle = C.c_void_p()
    b.check(b.create(Window.Width, Window.Height, C.byref(desc), C.byref(ps), C.byref(vs), int(Device),
                     C.byref(handle)))
    del keep
    return Renderer(b, handle, Window, Scene, Probes, Volumetrics)
