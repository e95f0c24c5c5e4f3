"""MDH_INFO_CULL (closest_primitive_info, mdh_device.h): the typed arg-min of a hit point skips a sphere or a box behind
closest_primitive's wave-ballot culls.  No output may change in any bit (tests/test_hit_info_host.py holds the rule in numpy):

  * mdh_raycast on 4096 rays per scene against orc_probe_raycast -- hit, index, steps and t word for word -- in the room and in
    three scenes built for ties (a sphere tangent to a wall, a box face in a wall's plane, two boxes sharing a face).  The ray
    queries have no census variant: all four scenes run k_ray_query <0>, the RUN-TIME-COUNT loops of the typed arg-min.  The rays
    leave one point in wavefronts of 64 aimed at one place: patches of the walls (both culls fire), the sphere, the tangent
    point, faces, edges and corners of the boxes;
  * one 64x64 frame of the tangent-sphere and of the box-in-wall scene, whose census is the rooms' -- k_screen <ROOM | POW2>, the
    straight-line ROOM branch, where the strictness of the culls decides the index -- from a camera along the wall through the
    gap at the tangent point and from one low at the foot of the box where its face lies in the floor, with and without the
    geometry buffer, against the oracle word for word (image, geometry buffer, both atlases);
  * one 64x64 global_illumination frame per camera of tests/test_gpu_best_first.py, one whose image is mostly the sphere and
    one mostly the box, with and without the geometry buffer, against the oracle word for word -- marching, and recording then
    replaying."""
import numpy as np
import pytest

import ray_query_cases as Q
import test_gpu_best_first as BF
import test_gpu_folded_twins as T
from helpers import SMALL_PROBES, snapshot
from madarch_amd import _binding as B
from madarch_amd import examples, materials, renderers, scenes, windows
from madarch_amd.lights import spot_lights
from madarch_amd.primitives import boxes, planes, spheres

pytestmark = pytest.mark.gpu

SCENES = {  # spheres, boxes (the six planes of the examples' room around them)
    "room": ([((3.0, 4.0, 3.0), 1.0)], [((3.0, 0.0, 4.0), (1.5, 1.5, 1.5))]),
    "tangent_sphere": ([((0.0, 4.0, 3.0), 1.0)], [((3.0, 0.0, 4.0), (1.5, 1.5, 1.5))]),
    "box_in_wall": ([((3.0, 4.0, 3.0), 1.0)], [((3.0, 0.5, 4.0), (1.5, 1.5, 1.5))]),
    "twin_boxes": ([((3.0, 4.0, 3.0), 1.0)], [((2.0, 0.0, 4.0), (1.0, 1.5, 1.5)), ((4.0, 0.0, 4.0), (1.0, 1.5, 1.5))]),
}
# the cameras of the frames: those of tests/test_gpu_best_first.py, one in front of the sphere and one in front of the box.  Under the
# oracle at 64x64 the box is 3456 of the 4096 pixels of its camera; the sphere is 1272 of its camera's -- the image plane is 2 x 2
# with the eye 1.5 behind it, and a tenth in front of a sphere of radius 1 that is the largest share it reaches (twenty whole tiles).
CAMERAS = dict(BF.CAMERAS, sphere=((3.0, 4.0, 1.9), 0.0, 0.0), box=((3.0, 0.3, 1.8), 0.0, 0.0))


def tie_scene(binding, name, w=16, h=16, probes=SMALL_PROBES):
    """examples.global_illumination's declaration (spheres, planes, boxes) with the scene's own solids"""
    sph, bxs = SCENES[name]
    scene = scenes.Compile(All_Primitives=[(spheres.Sphere, 20), (planes.Plane, 10), (boxes.Box, 10)], All_Lights=[(spot_lights.Spot_Light, 4)],
                           Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(w, h, name), scene, Probes=probes, Volumetrics=renderers.No_Volumetrics, Binding=binding)
    mat = R.Add_Material(materials.Create((0.5, 0.5, 0.5), 0.0, 0.6))
    for n, o in examples._ROOM_PLANES:
        R.Add_Primitive(planes.Plane, planes.Create(n, o, mat))
    for c, r in sph:
        R.Add_Primitive(spheres.Sphere, spheres.Create(c, r, mat))
    for c, e in bxs:
        R.Add_Primitive(boxes.Box, boxes.Create(c, e, mat))
    R.Set_Light(1, spot_lights.Spot_Light, spot_lights.Create((3.5, 5.0, 2.0), (1.0, 0.0, 0.0), 3.1415 / 4.0, (0.9, 0.9, 0.8)))
    return R


def aimed_rays(name, seed=23):
    """64 wavefronts of 64 rays, each wavefront from one origin at one place of the scene"""
    rng = np.random.RandomState(seed)
    sph, bxs = SCENES[name]
    lo, hi = np.array([-1.0, -1.0, -6.0]), np.array([7.0, 7.0, 7.0])
    targets = []
    for a in range(3):  # patches of the six walls
        for v in (lo[a], hi[a]):
            for _ in range(4):
                p = lo + rng.rand(3) * (hi - lo) + (rng.rand(64, 3) - 0.5) * 0.3
                p[:, a] = v
                targets.append(p)
    for c, r in sph:
        for _ in range(6):
            d = rng.normal(size=3) + (rng.rand(64, 3) - 0.5) * 0.3
            targets.append(np.array(c) + r * d / np.linalg.norm(d, axis=1, keepdims=True))
        t = np.tile(np.array(c) - np.array([r, 0.0, 0.0]), (64, 1))  # the point nearest to the wall x = -1 and its surroundings
        t[1:, 1:] += (rng.rand(63, 2) - 0.5) * 0.02
        targets.append(t); targets.append(t + (rng.rand(64, 3) - 0.5) * 0.01)
    k = 0
    while len(targets) < 64:  # faces, edges and corners of the boxes in turn
        c, e = (np.array(v) for v in bxs[k % len(bxs)])
        u = rng.rand(64, 3) * 2 - 1
        ax, sg = (k // len(bxs)) % 3, (1.0 if (k // (3 * len(bxs))) % 2 else -1.0)
        u[:, ax] = sg
        kind = (k // (6 * len(bxs))) % 3
        if kind >= 1:
            u[:, (ax + 1) % 3] = rng.choice([-1.0, 1.0], 64)
        if kind == 2:
            u[:, (ax + 2) % 3] = rng.choice([-1.0, 1.0], 64)
        targets.append(c + u * e)
        k += 1
    org, drs = [], []
    for t in targets[:64]:
        o = np.array([2.0, 2.0, 0.0]) + (rng.rand(3) - 0.5)
        d = t - o
        org.append(np.tile(o, (64, 1))); drs.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    return np.concatenate(org).astype(np.float32), np.concatenate(drs).astype(np.float32)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_raycast_is_the_oracles(hip, orc, name):
    org, drs = aimed_rays(name)
    assert len(org) == 4096
    Ro = tie_scene(orc, name)
    want = Q.orc_raycast(orc, Ro, org, drs)
    Ro.Destroy()
    R = tie_scene(hip, name)
    got = R.Raycast(org, drs)
    R.Destroy()
    assert (want["hit"] != 0).mean() > 0.9  # (a closed room)
    kinds = np.unique(want["index"][want["hit"] != 0])
    assert len(kinds) >= 7, kinds  # every wall, and the solids
    for k in ("hit", "index", "steps"):
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %d rays" % (name, k, int((got[k] != want[k]).sum()))
    assert np.array_equal(T.bits(got["t"]), T.bits(want["t"])), "%s: t differs at %d rays" % (name, int((T.bits(got["t"]) != T.bits(want["t"])).sum()))


# the ROOM-census tie scenes as frames: (camera, the flat indices the oracle's geometry buffer must hold -- the solid and the wall it touches)
TIE_FRAMES = {"tangent_sphere": (((-0.6, 4.0, 0.8), 0.0, 0.0), (0, 22)), "box_in_wall": (((3.0, -0.5, 0.8), 0.0, 0.3), (30, 20))}


def tie_renderer(binding, name):
    R = tie_scene(binding, name, 64, 64, examples.GI_8X8X8_PROBES)
    pos, yaw, pitch = TIE_FRAMES[name][0]
    R.Set_Camera_Position(pos)
    R.Set_Camera_Orientation(T.rotation(yaw, pitch))
    R.Set_Option(B.OPT_GBUFFER, 1)
    return R


@pytest.mark.parametrize("name", sorted(TIE_FRAMES))
def test_tie_scene_frames_are_the_oracles(hip, orc, name):
    """one sphere, one box, six folded planes, no partition: the screen pass takes its ROOM variant"""
    Ro = tie_renderer(orc, name)
    want = snapshot(Ro, 2)
    Ro.Destroy()
    seen = np.unique(want["gb_index"])
    assert all(i in seen for i in TIE_FRAMES[name][1]), seen  # (the solid and the wall it touches are both in the image)
    for gbuffer in (1, 0):
        R = tie_renderer(hip, name)
        R.Set_Option(B.OPT_GBUFFER, gbuffer)
        if gbuffer:
            got = snapshot(R, 2)
        else:
            R.Render(); R.Render()
            got = {"image": R.Read_Framebuffer(), "radiance": R.Read_Texture(B.TEX_RADIANCE), "irradiance": R.Read_Texture(B.TEX_IRRADIANCE)}
        R.Destroy()
        for k in got:
            assert np.array_equal(T.bits(got[k]), T.bits(want[k])), "%s gbuffer %d: %s differs from the oracle in %d words" % (name, gbuffer, k, int((T.bits(got[k]) != T.bits(want[k])).sum()))


@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_frames_are_the_oracles(hip, orc, camera):
    """with and without the geometry buffer (assert_frames renders both)"""
    cam = CAMERAS[camera]
    T.assert_frames(hip, T.oracle_frames(orc, "8x8x8", cam, 64, 64), "8x8x8", cam, 64, 64)


@pytest.mark.parametrize("gbuffer", [1, 0])
@pytest.mark.parametrize("camera", ["sphere", "box", "gap"])
def test_recording_and_replaying_frames_are_the_oracles(hip, orc, camera, gbuffer):
    """MDH_OPT_SCREEN_REPLAY 1 over three static frames -- plain, recording, replaying -- against a renderer that marches every
    pass, whose second frame is the oracle's: the recorded arg-min is the marching kernel's"""
    cam = CAMERAS[camera]
    outs, kinds = [], []
    for replay in (1, 0):
        R = T.renderer(hip, "8x8x8", cam, 64, 64)
        R.Set_Option(B.OPT_GBUFFER, gbuffer)
        R.Set_Option(B.OPT_SCREEN_REPLAY, replay)
        frames = []
        for _ in range(3):
            R.Render()
            frames.append([R.Read_Framebuffer()] + (list(R.Read_Gbuffer()) if gbuffer else []))
        outs.append(frames)
        kinds.append(R.Screen_Replay_Stats())
        R.Destroy()
    assert kinds[0] == (1, 1, 1) and kinds[1] == (3, 0, 0), kinds
    for f, (a, b) in enumerate(zip(*outs)):
        for n, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(T.bits(x), T.bits(y)), "frame %d, output %d: %d words differ" % (f, n, int((T.bits(x) != T.bits(y)).sum()))
    assert np.array_equal(T.bits(outs[1][1][0]), T.bits(T.oracle_frames(orc, "8x8x8", cam, 64, 64)["image"]))
