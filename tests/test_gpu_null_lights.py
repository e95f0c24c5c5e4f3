"""null_light (mdh_device.h, MDH_SKIP_NULL_BRDF): lights that add exactly nothing to a point skip the BRDF and the shadow ray.

Scenes built so that wavefronts are all null, mixed, or one step outside the predicate, rendered by the product and by
the oracle (which shades every light): the framebuffer, both atlases and the geometry buffer are compared word for word
where the oracle's value is finite, and must be NaN where it is NaN.  tests/test_null_brdf_claim.py holds the claim
itself in numpy."""
import numpy as np
import pytest

from helpers import SMALL_PROBES, make, snapshot
from madarch_amd import _binding as B

W, H, FRAMES = 44, 28, 3
SPOT_AT = (3.5, 5.0, 2.0)  # the headline room's spot light (examples.global_illumination) looks along +x with aperture pi / 4
SPOT_COLOUR = (0.9, 0.9, 0.8)
AWAY = (SPOT_AT, (0.0, 0.0, -1.0), 3.1415 / 4.0, SPOT_COLOUR)   # towards the wall behind the camera: nothing the camera sees is inside
EDGE = (SPOT_AT, (1.0, 0.0, 0.0), 3.1415 / 4.0, SPOT_COLOUR)    # the headline light: the cone's edge runs over the wall, the sphere and the box
NARROW = ((2.0, 6.0, 3.0), (0.1, -1.0, 0.3), 0.35, (0.8, 0.7, 0.9))  # a small pool of light on the floor and the box


def _headline(b, spots, second_sphere=False, mats=()):
    from madarch_amd import materials
    from madarch_amd.lights import spot_lights
    from madarch_amd.primitives import spheres
    R = make("global_illumination", W, H, b, probes=SMALL_PROBES)
    if second_sphere:  # two spheres are not the rooms' census: the brute-force scan
        R.Add_Primitive(spheres.Sphere, spheres.Create((0.5, 0.2, 3.5), 0.7, 4))
    for i, s in enumerate(spots):
        R.Set_Light(i + 1, spot_lights.Spot_Light, spot_lights.Create(*s))
    for m, (alb, met, rough) in mats:
        R.Set_Material(m, materials.Create(alb, met, rough))
    return R


def _point_room(b, lights, second_sphere=False, partition=False, wall_colour=(1.0, 0.0, 0.0)):
    """The headline room's geometry and materials under point lights; `partition`: behind the space partition (whose kernel
    variants leave the predicate out, mdh_march.h: the case holds that they still shade every light as the oracle does)."""
    from madarch_amd import examples, materials, renderers, scenes, windows
    from madarch_amd.lights import point_lights
    from madarch_amd.primitives import boxes, planes, spheres
    part = scenes.Partitioning_Settings(Enable=True, Index_Count=12, Grid_Dimensions=(3, 3, 4), Grid_Spacing=(3.0, 3.0, 3.5), Grid_Offset=(-1.0, -1.0, -6.0)) \
        if partition else scenes.Partitioning_Settings(Enable=False)
    scene = scenes.Compile([(spheres.Sphere, 4), (planes.Plane, 6), (boxes.Box, 2)], [(point_lights.Point_Light, 2)], Partitioning=part)
    R = renderers.Create(windows.Open(W, H), scene, Probes=SMALL_PROBES, Volumetrics=renderers.No_Volumetrics, Binding=b)
    for m, (alb, met, rough) in enumerate((((0.0, 0.0, 0.0), 0.0, 0.6), (wall_colour, 0.0, 0.6), ((0.0, 0.0, 1.0), 0.0, 0.6), ((0.1, 0.1, 0.1), 0.9, 0.1),
                                           ((0.0, 1.0, 0.0), 0.8, 0.3))):
        R.Set_Material(m, materials.Create(alb, met, rough))
    for (n, o), m in zip(examples._ROOM_PLANES, (0, 0, 1, 2, 0, 0)):
        R.Add_Primitive(planes.Plane, planes.Create(n, o, m))
    R.Add_Primitive(spheres.Sphere, spheres.Create((3.0, 4.0, 3.0), 1.0, 3))
    if second_sphere:
        R.Add_Primitive(spheres.Sphere, spheres.Create((0.5, 0.2, 3.5), 0.7, 4))
    R.Add_Primitive(boxes.Box, boxes.Create((3.0, 0.0, 4.0), (1.5, 1.5, 1.5), 4))
    R.Set_Camera_Position((2.0, 2.0, 0.0))
    for i, (pos, colour) in enumerate(lights):
        R.Set_Light(i + 1, point_lights.Point_Light, point_lights.Create(pos, colour))
    R.Set_Option(B.OPT_SCREEN_MODE, 0)
    R.Set_Option(B.OPT_ATLAS_FORMAT, 0)
    R.Set_Option(B.OPT_GBUFFER, 1)
    if partition:
        R.Update_Partitioning(Method=renderers.GPU_Fast)
    return R


# a point light level with the box's top (y = 1.5: NdotL there is 0 or a rounding error away from it) and beside the sphere:
# the box's far sides, the sphere's far half and the floor behind the box face away from it or see it at a grazing angle
GRAZING = [((0.5, 1.5, 3.0), (0.9, 0.8, 0.7))]
# 1e-3 in front of the wall x = 7 with a colour of 1e38: colour / (dist^2 * 0.03) overflows within three units of the light,
# and along that wall NdotL = 1e-3 / dist falls below EPS where the radiance is +inf
BLINDING = [((6.999, 3.0, 4.0), (1e38, 1e38, 1e38))]
# one material each outside the predicate's range (and roughness 0, its edge: a2 = 0, NDF = 0 / 0 at NdotH = 1)
BAD_MATS = ((0, ((0.0, 0.0, 0.0), 0.0, 2.5)), (1, ((1.0, 0.0, 0.0), 1.5, 0.6)), (2, ((0.0, 0.0, 2.0), 0.0, 0.6)), (3, ((0.1, 0.1, 0.1), 0.9, 0.0)))

CASES = {
    "a_all_null_census": lambda b: _headline(b, [AWAY]),
    "a_all_null_scan": lambda b: _headline(b, [AWAY], second_sphere=True),
    "b_cone_edge_census": lambda b: _headline(b, [EDGE]),
    "b_cone_edge_scan": lambda b: _headline(b, [EDGE], second_sphere=True),
    "b_narrow_cone_census": lambda b: _headline(b, [NARROW]),
    "c_point_grazing_census": lambda b: _point_room(b, GRAZING),
    "c_point_grazing_scan": lambda b: _point_room(b, GRAZING, second_sphere=True),
    "c_point_grazing_partition": lambda b: _point_room(b, GRAZING, partition=True),
    "d_point_overflowing_radiance": lambda b: _point_room(b, BLINDING, wall_colour=(1.0, 0.5, 0.25)),
    "e_materials_outside_the_range": lambda b: _headline(b, [EDGE], mats=BAD_MATS),
    "f_null_then_lit": lambda b: _headline(b, [AWAY, NARROW]),
    "f_lit_then_null": lambda b: _headline(b, [NARROW, AWAY]),
    "f_two_points_lit_then_away": lambda b: _point_room(b, [((3.0, 6.5, 3.0), (0.9, 0.9, 0.9)), GRAZING[0]]),
}


def _assert_words(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, name
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), name
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN at other places than the oracle's" % name
    gw, ww = got.view(np.uint32), want.view(np.uint32)
    diff = (gw != ww) & ~nan
    assert not diff.any(), "%s: %d of %d words differ, first at %s: %r against %r" % (
        name, diff.sum(), diff.size, tuple(np.argwhere(diff)[0]), got[tuple(np.argwhere(diff)[0])], want[tuple(np.argwhere(diff)[0])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_null_lights_word_for_word(hip, orc, name):
    outs = []
    for b in (hip, orc):
        R = CASES[name](b)
        outs.append(snapshot(R, FRAMES))
        R.Destroy()
    got, want = outs
    assert sorted(got) == sorted(want)
    for k in ("image", "radiance", "irradiance", "gb_index", "gb_t", "gb_steps"):
        _assert_words("%s %s" % (name, k), got[k], want[k])
    if name.startswith("d_"):  # the case is what it claims to be: the overflow reaches the outputs
        assert np.isnan(want["image"]).any() or np.isinf(want["image"]).any()
    else:  # (materials outside the range and cells outside the partition's grid leave some NaN pixels: compared as such above)
        assert np.isfinite(want["image"]).mean() > 0.9 and np.nanmax(want["image"]) > 0.0
