"""The three benchmark scenes of BASELINE.json and the reference's mesh example, written as the
reference's example programs write them (same data, same call order), minus the window loop.

  simple_scene        -- reference examples/simple_scene/main.adb:28-122
  global_illumination -- reference examples/global_illumination/main.adb:29-74,149-161
  light_shafts        -- reference examples/light_shafts/main.adb:29-59,140-155
  obj_mesh            -- reference examples/obj_mesh/main.adb:30-75,139-169 (a procedural mesh for suzanne.obj)

Each returns the Renderer after the last call the example makes before its
first `Renderers.Render`.  `Binding=None` is the HIP library.
"""
import numpy as np

from . import _binding, lights, materials, meshes, primitives, renderers, scenes, windows
from .lights import point_lights, spot_lights
from .primitives import boxes, planes, spheres, triangles

# BASELINE config 3: DDGI 8x8x8 probe grid = 512 probes as a 32x16 atlas; the grid
# has no offset (glsl/probe_utils.glsl:38-40), this spacing keeps it in the room
# 
GI_8X8X8_PROBES = renderers.Probe_Settings(Probe_Count=(32, 16), Grid_Dimensions=(8, 8, 8),
                                           Grid_Spacing=(0.95, 0.95, 0.9))

_ROOM_PLANES = (((0.0, 1.0, 0.0), 1.0), ((0.0, -1.0, 0.0), 7.0), ((1.0, 0.0, 0.0), 1.0),
                ((-1.0, 0.0, 0.0), 7.0), ((0.0, 0.0, 1.0), 6.0), ((0.0, 0.0, -1.0), 7.0))


def simple_scene(Width=1000, Height=1000, Probes=None, Binding=None, Device=0,
                 Partitioning_Method=renderers.CPU_Best):
    Scene = scenes.Compile(
        All_Primitives=[(spheres.Sphere, 20), (planes.Plane, 10), (boxes.Box, 20)],
        All_Lights=[(point_lights.Point_Light, 4)])
    Window = windows.Open(Width, Height, "Simple_Scene")
    R = renderers.Create(Window, Scene, Probes=Probes, Volumetrics=renderers.No_Volumetrics,
                         Device=Device, Binding=Binding)
    Point_Light_Instance = point_lights.Create((0.0, 3.0, 0.0), (0.9, 0.9, 0.9))
    plane_mats = (0, 0, 1, 2, 0, 0)
    Planes = [planes.Create(n, o, m) for (n, o), m in zip(_ROOM_PLANES, plane_mats)]
    Spheres = [spheres.Create((x, y, z), 0.5, 3) for (y, z, xs) in (
        (3.5, 2.0, (0.5, 1.5, 2.5, 3.5, 4.5, 5.5)), (0.5, 2.0, (0.5, 1.5, 2.5, 3.5, 4.5, 5.5)),
        (3.5, 5.0, (0.5, 1.5, 2.5, 3.5, 4.5, 5.5)), (0.5, 5.0, (0.5, 1.5))) for x in xs]
    Boxes = [boxes.Create(c, s, 2) for c, s in (
        ((3.0, 1.0, 2.0), (0.5, 0.5, 0.5)), ((0.0, 1.0, 2.0), (0.3, 0.3, 0.5)),
        ((3.0, 1.0, 4.0), (0.5, 0.5, 0.5)), ((4.0, 2.0, 2.0), (0.5, 0.5, 0.5)),
        ((2.0, 2.0, 2.0), (0.5, 0.5, 0.5)), ((1.0, 1.0, 6.0), (0.5, 0.5, 0.5)),
        ((3.0, 1.0, 6.0), (0.5, 0.5, 0.5)), ((3.0, 1.0, -2.0), (0.5, 0.5, 0.5)),
        ((1.0, 1.0, -2.0), (0.3, 0.3, 0.5)), ((3.0, 1.0, -4.0), (0.5, 0.5, 0.5)),
        ((4.0, 2.0, -2.0), (0.5, 0.5, 0.5)), ((2.0, 2.0, -2.0), (0.5, 0.5, 0.5)),
        ((1.0, 1.0, -6.0), (0.5, 0.5, 0.5)), ((3.0, 1.0, -6.0), (0.5, 0.5, 0.5)))]
    for Plane in Planes:
        R.Add_Primitive(planes.Plane, Plane)
    for Sphere in Spheres:
        R.Add_Primitive(spheres.Sphere, Sphere)
    for Box in Boxes:
        R.Add_Primitive(boxes.Box, Box)
    R.Set_Material(0, materials.Create((0.0, 0.0, 0.0), 0.0, 0.6))
    R.Set_Material(1, materials.Create((1.0, 0.0, 0.0), 0.0, 0.6))
    R.Set_Material(2, materials.Create((0.0, 0.0, 1.0), 0.0, 0.6))
    R.Set_Material(3, materials.Create((0.1, 0.1, 0.1), 0.9, 0.1))
    R.Set_Light(1, point_lights.Point_Light, Point_Light_Instance)
    R.Set_Camera_Position((2.0, 2.0, 0.0))
    if Partitioning_Method is not None:
        R.Update_Partitioning(Method=Partitioning_Method)
    return R


def global_illumination(Width=1000, Height=1000, Probes=None, Binding=None, Device=0):
    Scene = scenes.Compile(
        All_Primitives=[(spheres.Sphere, 20), (planes.Plane, 10), (boxes.Box, 10)],
        All_Lights=[(spot_lights.Spot_Light, 4)],
        Partitioning=scenes.Partitioning_Settings(Enable=False))
    Window = windows.Open(Width, Height, "Global_Illumination")
    R = renderers.Create(Window, Scene, Probes=Probes, Volumetrics=renderers.No_Volumetrics,
                         Device=Device, Binding=Binding)
    Spot_Light_Instance = spot_lights.Create((3.5, 5.0, 2.0), (1.0, 0.0, 0.0), 3.1415 / 4.0,
                                             (0.9, 0.9, 0.8))
    Wall_Mat_1 = R.Add_Material(materials.Create((0.0, 0.0, 0.0), 0.0, 0.6))
    Wall_Mat_2 = R.Add_Material(materials.Create((1.0, 0.0, 0.0), 0.0, 0.6))
    Wall_Mat_3 = R.Add_Material(materials.Create((0.0, 0.0, 1.0), 0.0, 0.6))
    Sphere_Mat = R.Add_Material(materials.Create((0.1, 0.1, 0.1), 0.9, 0.1))
    Box_Mat = R.Add_Material(materials.Create((0.0, 1.0, 0.0), 0.8, 0.3))
    plane_mats = (Wall_Mat_1, Wall_Mat_1, Wall_Mat_2, Wall_Mat_3, Wall_Mat_1, Wall_Mat_1)
    for (n, o), m in zip(_ROOM_PLANES, plane_mats):
        R.Add_Primitive(planes.Plane, planes.Create(n, o, m))
    R.Add_Primitive(spheres.Sphere, spheres.Create((3.0, 4.0, 3.0), 1.0, Sphere_Mat))
    R.Add_Primitive(boxes.Box, boxes.Create((3.0, 0.0, 4.0), (1.5, 1.5, 1.5), Box_Mat))
    R.Set_Camera_Position((2.0, 2.0, 0.0))  # Move_Camera with a zero offset, main.adb:80-85
    R.Set_Light(1, spot_lights.Spot_Light, Spot_Light_Instance)
    return R


def light_shafts(Width=1000, Height=1000, Probes=None, Volumetrics=None, Binding=None, Device=0):
    Scene = scenes.Compile(
        All_Primitives=[(spheres.Sphere, 20), (planes.Plane, 10), (boxes.Box, 10)],
        All_Lights=[(point_lights.Point_Light, 4)],
        Partitioning=scenes.Partitioning_Settings(Enable=False))
    Window = windows.Open(Width, Height, "Light_Shafts")
    R = renderers.Create(Window, Scene, Probes=Probes, Volumetrics=Volumetrics, Device=Device,
                         Binding=Binding)
    Point_Light_Instance = point_lights.Create((5.0, 3.0, 6.0), (0.9, 0.9, 0.9))
    plane_mats = (0, 0, 1, 2, 0, 0)
    for (n, o), m in zip(_ROOM_PLANES, plane_mats):
        R.Add_Primitive(planes.Plane, planes.Create(n, o, m))
    R.Add_Primitive(spheres.Sphere, spheres.Create((3.0, 4.0, 3.0), 1.0, 3))
    R.Add_Primitive(boxes.Box, boxes.Create((3.0, 0.0, 4.0), (1.5, 1.5, 1.5), 2))
    R.Set_Material(0, materials.Create((0.0, 0.0, 0.0), 0.0, 1.0))
    R.Set_Material(1, materials.Create((1.0, 0.0, 0.0), 0.0, 1.0))
    R.Set_Material(2, materials.Create((0.0, 1.0, 0.0), 0.0, 1.0))
    R.Set_Material(3, materials.Create((0.0, 0.0, 1.0), 0.0, 1.0))
    R.Set_Camera_Position((2.0, 2.0, 0.0))
    R.Set_Light(1, point_lights.Point_Light, Point_Light_Instance)
    return R


OBJ_MESH_TRIANGLES = 1000  # main.adb:46
OBJ_MESH_OFFSET = (1.5, 1.0, 1.0)  # Suzanne_Offset, main.adb:139-140


def obj_mesh(Width=1000, Height=1000, Probes=None, Binding=None, Device=0,
             Partitioning_Method=renderers.GPU_Fast, Mesh=None, Index_Count=150, Triangle_BVH=False):
    """examples/obj_mesh/main.adb: 1000 triangles behind a 30 x 20 x 20 partition of 0.1 cells, one point
    light, the default probes (the example declares probe settings and does not pass them).  `Mesh`
    ([n, 3, 3] vertex triples about the origin, n <= 1000) stands for media/suzanne.obj -- there is no
    loader; the default is meshes.torus (25, 20): exactly 1000 triangles.  The scene's table is larger
    than a workgroup's LDS: the HIP library reads its geometry from device memory (OPT_TABLE_RESIDENCY).
    `Triangle_BVH` (HIP library only): the same mesh with `Partitioning => (Enable => False)` and
    OPT_TRIANGLE_BVH on -- the exact scan over all 1000 triangles, walked through a bounding-volume hierarchy."""
    Partitioning_Settings = scenes.Partitioning_Settings(
        Enable=not Triangle_BVH, Index_Count=Index_Count, Border_Behavior=scenes.Clamp, Grid_Dimensions=(30, 20, 20),
        Grid_Spacing=(0.1, 0.1, 0.1), Grid_Offset=(0.0, 0.0, 0.0))
    Scene = scenes.Compile(
        All_Primitives=[(triangles.Triangle, OBJ_MESH_TRIANGLES)],
        All_Lights=[(point_lights.Point_Light, 4)],
        Partitioning=Partitioning_Settings)
    Window = windows.Open(Width, Height, "Obj_Mesh")
    R = renderers.Create(Window, Scene, Probes=Probes, Volumetrics=renderers.No_Volumetrics,
                         Device=Device, Binding=Binding)
    if Triangle_BVH:
        R.Set_Option(_binding.OPT_TRIANGLE_BVH, 1)
    Point_Light_Instance = point_lights.Create((0.0, 1.0, -5.0), (0.9, 0.9, 0.9))
    Mesh_Mat = R.Add_Material(materials.Create((0.8, 0.2, 0.1), 0.0, 1.0))
    if Mesh is None:
        Mesh = meshes.torus(25, 20)
    Offset = np.asarray(OBJ_MESH_OFFSET, dtype=np.float32)
    for A, B, C in np.asarray(Mesh, dtype=np.float32):  # Add_Triangle, main.adb:142-153
        R.Add_Primitive(triangles.Triangle, triangles.Create(A + Offset, B + Offset, C + Offset, Mesh_Mat))
    if Partitioning_Method is not None and not Triangle_BVH:
        R.Update_Partitioning(Method=Partitioning_Method)
    R.Set_Light(1, point_lights.Point_Light, Point_Light_Instance)
    R.Set_Camera_Position((0.0, 1.0, -5.0))  # Move_Camera with a zero offset, main.adb:70-75,133
    return R


class Ball_Game:
    """examples/ball_game/main.adb: the global_illumination room with the default space partition, balls
    thrown from the camera that bounce off planes and boxes.  The physics step is the reference's: per
    ball one Eval_Distance_To against (Plane, Box) -- the CPU expression evaluator there, the batched device
    query here -- then Set_Primitive; every frame rebuilds the partition (Update_Partitioning) and renders.
    The interactive parts (keys, mouse) are the methods Throw_Ball / Move_Camera.
    Swept = True replaces the point test, which a ball whose step is longer than an obstacle is thick passes through, by ONE
    Spherecast for all balls: the first contact of each moving sphere with the planes and boxes."""

    Ball_Radius = np.float32(0.2)
    Gravity = np.array([0.0, -9.81, 0.0], dtype=np.float32)

    def __init__(self, Width=1000, Height=1000, Probes=None, Binding=None, Device=0, Swept=False):
        self.Swept = bool(Swept)
        self.Scene = scenes.Compile(  # main.adb:30-35: the default partitioning settings (enabled)
            All_Primitives=[(spheres.Sphere, 20), (planes.Plane, 10), (boxes.Box, 10)],
            All_Lights=[(spot_lights.Spot_Light, 4)])
        R = self.R = renderers.Create(windows.Open(Width, Height, "Ball_Game"), self.Scene, Probes=Probes,
                                      Volumetrics=renderers.No_Volumetrics, Device=Device, Binding=Binding)
        mats = [R.Add_Material(materials.Create(a, m, r)) for a, m, r in (
            ((0.0, 0.0, 0.0), 0.0, 1.0), ((1.0, 0.0, 0.0), 0.0, 1.0), ((0.0, 0.0, 1.0), 0.0, 1.0),
            ((0.1, 0.1, 0.1), 0.9, 0.1), ((0.0, 1.0, 0.0), 0.8, 0.3))]
        self.Box_Mat = mats[4]
        for (n, o), m in zip(_ROOM_PLANES, (mats[0], mats[0], mats[1], mats[2], mats[0], mats[0])):
            R.Add_Primitive(planes.Plane, planes.Create(n, o, m))
        R.Add_Primitive(spheres.Sphere, spheres.Create((3.0, 4.0, 3.0), 1.0, mats[3]))
        R.Add_Primitive(boxes.Box, boxes.Create((3.0, 0.0, 4.0), (1.5, 1.5, 1.5), mats[4]))
        R.Set_Light(1, spot_lights.Spot_Light, spot_lights.Create((3.5, 6.0, 2.0), (0.0, -1.0, 0.0), 3.1415 / 2.0, (1.0, 1.0, 1.0)))
        self.Camera_Position = np.array([2.0, 2.0, 0.0], dtype=np.float32)
        self.Camera_Orientation = np.eye(3, dtype=np.float32)
        R.Set_Camera_Position(self.Camera_Position)
        self.Ball_Bodies = []  # [index, position, velocity]

    def Move_Camera(self, Offset):  # main.adb:110-115
        self.Camera_Position = (self.Camera_Position + self.Camera_Orientation @ np.asarray(Offset, dtype=np.float32)).astype(np.float32)
        self.R.Set_Camera_Position(self.Camera_Position)

    def Throw_Ball(self):  # main.adb:98-108
        vel = (self.Camera_Orientation @ np.array([0.0, 0.0, 1.0], dtype=np.float32) * np.float32(10.0)).astype(np.float32)
        self.R.Add_Primitive(spheres.Sphere, spheres.Create(self.Camera_Position, self.Ball_Radius, self.Box_Mat))
        self.Ball_Bodies.append([len(self.Ball_Bodies) + 2, self.Camera_Position.copy(), vel])

    def Step_Physics(self, Dt=0.01):  # main.adb:196-228
        """One Eval_Distance_To per ball in the reference; the balls do not see each other (the query
        is against planes and boxes only), so all of them go to the device in ONE batched query."""
        if not self.Ball_Bodies:
            return
        Dt = np.float32(Dt)
        new_vel = [(b[2] + self.Gravity * Dt).astype(np.float32) for b in self.Ball_Bodies]
        new_pos = [(b[1] + v * Dt).astype(np.float32) for b, v in zip(self.Ball_Bodies, new_vel)]
        if self.Swept:
            return self._step_swept(Dt, new_vel, new_pos)
        dists, normals = self.R.Eval_Distances_To(np.stack(new_pos), (planes.Plane, boxes.Box))
        for body, vel, pos, dist, normal in zip(self.Ball_Bodies, new_vel, new_pos, dists, normals):
            if np.float32(dist) <= self.Ball_Radius:
                normal = np.asarray(normal, dtype=np.float32)
                d = np.float32((vel[0] * normal[0] + vel[1] * normal[1]) + vel[2] * normal[2])
                vel = (vel - np.float32(2.0) * d * normal).astype(np.float32)  # Math_Utils.Reflect, math_utils.adb:38-42
                pos = body[1]
            self.R.Set_Primitive(spheres.Sphere, body[0], spheres.Create(pos, self.Ball_Radius, self.Box_Mat))
            body[1], body[2] = pos, vel

    def _step_swept(self, Dt, new_vel, new_pos):
        """the balls' spheres swept from their old centres along their new velocities over the step's length: a ball that
        touches a plane or a box on the way is reflected about the contact's normal and placed at the contact's centre (a ball
        that rests on a surface and moves away from it touches at t = 0 and is let go)"""
        speed = [np.sqrt(np.float32((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])) for v in new_vel]
        drs = np.stack([v / s if s > 0.0 else np.zeros(3, np.float32) for v, s in zip(new_vel, speed)]).astype(np.float32)
        tmax = np.minimum(np.asarray(speed, np.float32) * Dt, np.float32(self.Scene.Max_Dist))
        cast = self.R.Spherecast(np.stack([b[1] for b in self.Ball_Bodies]), drs, self.Ball_Radius, tmax, (planes.Plane, boxes.Box))
        for k, (body, vel, pos) in enumerate(zip(self.Ball_Bodies, new_vel, new_pos)):
            if cast["hit"][k] == 1:
                normal = cast["normal"][k]
                d = np.float32((vel[0] * normal[0] + vel[1] * normal[1]) + vel[2] * normal[2])
                if d < 0.0 or cast["t"][k] > 0.0:
                    vel = (vel - np.float32(2.0) * d * normal).astype(np.float32)  # Math_Utils.Reflect, math_utils.adb:38-42
                    pos = cast["position"][k].copy()
            self.R.Set_Primitive(spheres.Sphere, body[0], spheres.Create(pos, self.Ball_Radius, self.Box_Mat))
            body[1], body[2] = pos, vel

    def Frame(self, Dt=0.01):  # the loop body, main.adb:244-252
        self.Step_Physics(Dt)
        self.R.Update_Partitioning()
        self.R.Render()


def ball_game(Width=1000, Height=1000, Probes=None, Binding=None, Device=0, Swept=False):
    return Ball_Game(Width, Height, Probes, Binding, Device, Swept)


def fisheye_view(R, Width, Height, Fov=np.pi, Mode=0, Tone_Map=True):
    """A fisheye view (equidistant projection, `Fov` radians across the inscribed circle) of whatever R renders, through
    Renderer.Camera_Rays warped on the host and Renderer.Shade_Rays: the pinhole camera of draw_screen.glsl:20-24 cannot
    see half a sphere, its rays can be bent to.  Frames come first -- the rays see the probes as the last one left them.
    -> (Height, Width, 3) colours, black outside the circle."""
    org, _ = R.Camera_Rays(Width, Height)
    o = org.reshape(Height, Width, 3).astype(np.float64)

    def unit(v):
        return v / np.linalg.norm(v)
    # the camera's frame from its own rays: their origins span the image plane, u to the right and v up, both in [-1, 1]
    centre = o.mean(axis=(0, 1))
    right = unit(o[:, -1].mean(axis=0) - o[:, 0].mean(axis=0)) if Width > 1 else np.array([1.0, 0.0, 0.0])
    up = unit(o[0].mean(axis=0) - o[-1].mean(axis=0)) if Height > 1 else np.array([0.0, 1.0, 0.0])
    forward = np.cross(right, up)
    u, v = (o - centre) @ right, (o - centre) @ up
    r = np.hypot(u, v)
    theta = r * (0.5 * Fov)
    s = np.sin(theta) / np.maximum(r, 1e-12)
    drs = (s * u)[..., None] * right + (s * v)[..., None] * up + np.cos(theta)[..., None] * forward
    eye = np.broadcast_to(centre, drs.shape)
    out = R.Shade_Rays(eye.reshape(-1, 3).astype(np.float32), drs.reshape(-1, 3).astype(np.float32), Mode=Mode, Tone_Map=Tone_Map)
    image = out["rgb"].reshape(Height, Width, 3)
    image[r > 1.0] = 0.0
    return image


def foggy_fisheye_view(R, Width, Height, Fov=np.pi, Step=0.1, Rays=None):
    """fisheye_view with the lights' fog: the same rays (fisheye_view's construction), Renderer.Shade_Rays for the linear
    colour, t and hit, Renderer.Inscatter_Rays along every ray up to its hit (max_dist on a miss) in steps of `Step`, composed
    as render_volumetrics composes them -- colour * exp (-len tau) + L -- and tone-mapped (draw_screen.glsl:29) on the host.
    The shafts of the light_shafts scene through a lens the froxel grid cannot serve.  `Rays` ((origins, directions), each
    (Width * Height, 3)) replaces the lens: the pinhole's own Camera_Rays give what the frame approximates with froxels.
    -> (Height, Width, 3) colours, black outside the circle."""
    r = np.zeros((Height, Width))
    if Rays is None:
        org, _ = R.Camera_Rays(Width, Height)
        o = org.reshape(Height, Width, 3).astype(np.float64)

        def unit(v):
            return v / np.linalg.norm(v)
        centre = o.mean(axis=(0, 1))
        right = unit(o[:, -1].mean(axis=0) - o[:, 0].mean(axis=0)) if Width > 1 else np.array([1.0, 0.0, 0.0])
        up = unit(o[0].mean(axis=0) - o[-1].mean(axis=0)) if Height > 1 else np.array([0.0, 1.0, 0.0])
        forward = np.cross(right, up)
        u, v = (o - centre) @ right, (o - centre) @ up
        r = np.hypot(u, v)
        theta = r * (0.5 * Fov)
        s = np.sin(theta) / np.maximum(r, 1e-12)
        drs = (s * u)[..., None] * right + (s * v)[..., None] * up + np.cos(theta)[..., None] * forward
        org, drs = np.broadcast_to(centre, drs.shape).reshape(-1, 3).astype(np.float32), drs.reshape(-1, 3).astype(np.float32)
    else:
        org, drs = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3) for a in Rays)
    seen = R.Shade_Rays(org, drs, Mode=0, Tone_Map=False)
    max_dist = np.float32(R.Scene.Max_Dist)
    tmax = np.where(seen["hit"] != 0, np.minimum(seen["t"], max_dist), max_dist).astype(np.float32)
    fog = R.Inscatter_Rays(org, drs, tmax, Step)
    tau = 0.1  # volumetrics.glsl:12
    x = seen["rgb"].astype(np.float64) * np.exp(-fog["len"].astype(np.float64) * tau)[:, None] + fog["rgb"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        image = ((x / (x + 1.0)) ** float(np.float32(0.4545))).astype(np.float32).reshape(Height, Width, 3)
    image[r > 1.0] = 0.0
    return image


def lit_points(R=None, Count=64, Frames=4, Radius=1.6, Binding=None):
    """A ring of `Count` points the host owns -- no primitive of the scene -- round the sphere of the global_illumination
    room, normals pointing away from it, seen from the camera, each with a material of the host's own: what light arrives at
    them after `Frames` frames, through Renderer.Shade_Points in mode 0.  The probes light what the scene never heard of.
    -> (positions, normals, colours), each (Count, 3); the colours are linear."""
    own = R is None
    if own:
        R = global_illumination(64, 64, Binding=Binding)
    chalk = R.Add_Material(materials.Create((0.8, 0.8, 0.8), 0.0, 0.9))  # (the host registers its materials with the calls it has)
    for _ in range(Frames):
        R.Render()
    a = np.arange(Count) * (2.0 * np.pi / Count)
    out = np.stack([np.cos(a), np.zeros(Count), np.sin(a)], axis=1)
    pos = (np.array([3.0, 4.0, 3.0]) + Radius * out).astype(np.float32)
    nrm = out.astype(np.float32)
    view = pos - np.array([2.0, 2.0, 0.0], dtype=np.float32)  # from the eye to the point
    view = (view / np.linalg.norm(view, axis=1, keepdims=True)).astype(np.float32)
    rgb = R.Shade_Points(pos, nrm, view, np.full(Count, chalk, np.int32), Mode=0)
    if own:
        R.Destroy()
    return pos, nrm, rgb


def path_traced_view(R, Width, Height, Samples=64, Bounces=3, Seed=1, Slice=16):
    """What renderer R's camera sees, twice over the same rays (Camera_Rays): path traced -- Renderer.Path_Trace in slices of
    `Slice` samples, the sums handed back in, divided by the count -- and as the frame itself shows it in mode 0 (the pixel
    program along the frame's rays: direct light, the probes' irradiance, the reflection's tap, occlusion).  Both go through
    draw_screen.glsl:29 on the host.  The first is the ground truth the probes approximate; render some frames before the call
    so that they have settled.  -> (path traced, frame), each (Height, Width, 3), and the two linear images likewise."""
    org, drs = R.Camera_Rays(Width, Height)
    sums, first = None, 0
    while first < Samples:
        count = min(int(Slice), Samples - first)
        sums = R.Path_Trace(org, drs, Seed=Seed, Sample_First=first, Sample_Count=count, Bounces=Bounces, Rgb_Accum=sums)["rgb"]
        first += count
    traced = (sums if sums is not None else np.zeros_like(org)).astype(np.float64) / max(int(Samples), 1)
    frame = R.Shade_Rays(org, drs, Mode=0, Tone_Map=False)["rgb"].astype(np.float64)

    def tone(x):  # draw_screen.glsl:29
        with np.errstate(invalid="ignore"):
            return ((x / (x + 1.0)) ** float(np.float32(0.4545))).astype(np.float32).reshape(Height, Width, 3)
    return tone(traced), tone(frame), traced.reshape(Height, Width, 3), frame.reshape(Height, Width, 3)


def path_traced_frame(R, Width, Height, Samples=64, Bounces=3, Seed=1, Jitter=True, Slice=16, Adaptive=None):
    """What renderer R's camera sees, path traced into the renderer's own accumulator: Path_Frame_Begin, Path_Frame_Accumulate in
    slices of `Slice` samples -- nothing is fetched or carried in between, the sums stay on the device -- and the resolve on the
    device.  With Jitter every sample goes through its own point of its pixel, so edges are anti-aliased; without it the image is
    path_traced_view's.  -> (tone-mapped (Height, Width, 3) float32, the window's bytes (Height, Width, 4) uint8, the linear
    image (Height, Width, 3) float32).  Adaptive = (Min_Samples, Tolerance) or (Min_Samples, Tolerance, Floor): the accumulator
    is an adaptive one with Max_Samples = Samples, every slice is a round for the pixels whose noise is still above the
    tolerance, and a fourth result is the (Height, Width) int32 image of the samples each pixel took."""
    if Adaptive is not None:
        rule = dict(zip(("Min_Samples", "Tolerance", "Floor"), Adaptive))
        R.Path_Frame_Begin_Adaptive(Width, Height, Seed=Seed, Bounces=Bounces, Jitter=Jitter, Max_Samples=max(int(Samples), int(rule["Min_Samples"])), **rule)
    else:
        R.Path_Frame_Begin(Width, Height, Seed=Seed, Bounces=Bounces, Jitter=Jitter)
    first = 0
    while first < Samples:
        count = min(int(Slice), Samples - first)
        R.Path_Frame_Accumulate(count)
        first += count
    shown = R.Path_Frame_Read(Tone_Map=True, Rgb=True, Rgba8=True)
    linear = R.Path_Frame_Read(Tone_Map=False)["rgb"]
    count = R.Path_Frame_Stats(Moments=False)["count"] if Adaptive is not None else None
    R.Path_Frame_End()
    if Adaptive is not None:
        return shown["rgb"], shown["rgba8"], linear, count
    return shown["rgb"], shown["rgba8"], linear


def scene_mesh(Path=None, R=None, Spacing=0.1, Binding=None):
    """The sphere and the box of the global_illumination room as a quad mesh, without the room's walls: Renderer.Surface_Mesh
    over the kinds (Sphere, Box) on a grid of `Spacing` round the two bodies, written to `Path` as Wavefront OBJ where one is
    given.  -> the mesh, {positions, quads, normals, index}"""
    from . import meshes
    own = R is None
    if own:
        R = global_illumination(64, 64, Binding=Binding)
    lo, hi = np.array([1.0, -2.0, 1.5]), np.array([5.0, 5.5, 6.0])  # round the sphere ((3, 4, 3), 1) and the box ((3, 0, 4) +- 1.5)
    cells = np.ceil((hi - lo) / Spacing).astype(np.int32)
    mesh = R.Surface_Mesh(lo, Spacing, cells, 0.0, (spheres.Sphere, boxes.Box))
    if Path is not None:
        meshes.Write_Obj(Path, mesh["positions"], mesh["quads"], mesh["normals"])
    if own:
        R.Destroy()
    return mesh


SCENES = {"simple_scene": simple_scene, "global_illumination": global_illumination,
          "light_shafts": light_shafts, "obj_mesh": obj_mesh}
