"""segment_clear (mdh_device.h, MDH_VIS_CLEAR): scenes built to put probe-visibility segments at the edge of the bound.

A cleared ray is not marched; its result must be the march's.  Each scene is rendered by the product and by the
oracle and every output is compared bit for bit -- the image included -- besides the parity bar."""
import numpy as np
import pytest

from helpers import assert_parity, same_bits, snapshot
from madarch_amd import _binding as B

ROOM6 = (((0, 1, 0), 1.0), ((0, -1, 0), 7.0), ((1, 0, 0), 1.0), ((-1, 0, 0), 7.0), ((0, 0, 1), 6.0), ((0, 0, -1), 7.0))


def _render(b, planes_, spheres_, boxes_, probes, camera, light, W=40, H=24, spec=2, frames=2):
    from madarch_amd import materials, renderers, scenes, windows
    from madarch_amd.lights import point_lights
    from madarch_amd.primitives import boxes, planes, spheres
    scene = scenes.Compile([(spheres.Sphere, 6), (planes.Plane, 10), (boxes.Box, 6)], [(point_lights.Point_Light, 2)],
                           Partitioning=scenes.Partitioning_Settings(Enable=False))
    R = renderers.Create(windows.Open(W, H), scene, Probes=probes, Volumetrics=renderers.No_Volumetrics, Binding=b)
    for m, (alb, met, rough) in enumerate((((0.8, 0.8, 0.8), 0.0, 0.6), ((0.9, 0.1, 0.1), 0.0, 0.5), ((0.1, 0.2, 0.9), 0.7, 0.2),
                                           ((0.3, 0.3, 0.3), 0.9, 0.1))):
        R.Set_Material(m, materials.Create(alb, met, rough))
    for i, (n, o) in enumerate(planes_):
        R.Add_Primitive(planes.Plane, planes.Create(n, o, i % 2))
    for i, (c, r) in enumerate(spheres_):
        R.Add_Primitive(spheres.Sphere, spheres.Create(c, r, 3 if i % 2 == 0 else 2))
    for i, (c, e) in enumerate(boxes_):
        R.Add_Primitive(boxes.Box, boxes.Create(c, e, 2 if i % 2 == 0 else 1))
    R.Set_Light(1, point_lights.Point_Light, point_lights.Create(light, (0.9, 0.9, 0.8)))
    R.Set_Camera_Position(camera)
    R.Set_Option(B.OPT_GBUFFER, 1)
    R.Set_Option(B.OPT_INDIRECT_SPECULAR, spec)
    return snapshot(R, frames)


def _probes(dims, spacing):
    from madarch_amd import renderers
    n = dims[0] * dims[1] * dims[2]
    pcx = next(c for c in range(int(np.sqrt(n)), 0, -1) if n % c == 0)
    return renderers.Probe_Settings(Radiance_Resolution=8, Irradiance_Resolution=6, Probe_Count=(pcx, n // pcx),
                                    Grid_Dimensions=dims, Grid_Spacing=spacing)


# probes at (i, j, k) * spacing; the rooms hold the camera and the light
SCENES = {
    # the rooms' census (six axis planes, one sphere, one box: the ROOM kernels) with the sphere's surface 0.001 to
    # 0.006 off the segments between neighbouring probes and the box's edge along a probe row
    "sphere_grazing_room": dict(planes=ROOM6, spheres=[((2.0, 2.0 + 0.5 + 0.0035, 2.0), 0.5)], boxes=[((4.0, 0.6, 2.0 + 1.0 + 0.002), (0.5, 0.6, 1.0))],
                                probes=((4, 4, 4), (2.0, 2.0, 2.0)), camera=(2.0, 3.0, -4.0), light=(3.0, 6.0, -2.0)),
    # several spheres, near and through the segments, and boxes whose corners sit next to probes
    "spheres_and_box_corners": dict(planes=ROOM6, spheres=[((1.0, 1.0, 1.0 + 0.2), 0.199), ((3.0, 1.0, 2.0), 0.2005), ((2.0, 4.0, 2.0), 0.05)],
                                    boxes=[((2.0 + 0.301, 2.0 + 0.301, 2.0 + 0.301), (0.3, 0.3, 0.3)), ((0.5, 3.0 - 0.2505, 4.0), (0.25, 0.25, 0.5))],
                                    probes=((5, 5, 5), (1.0, 1.0, 1.0)), camera=(2.0, 2.5, -4.0), light=(5.0, 6.0, 0.0)),
    # a wall through a probe plane (x = 0) and one just in front of a probe row (y >= 0.002)
    "probes_on_and_behind_walls": dict(planes=(((0, 1, 0), -0.002), ((0, -1, 0), 7.0), ((1, 0, 0), 0.0), ((-1, 0, 0), 7.0), ((0, 0, 1), 6.0), ((0, 0, -1), 7.0)),
                                       spheres=[((3.0, 3.0, 3.0), 0.8)], boxes=[((5.0, 1.0, 5.0), (0.5, 1.0, 0.5))],
                                       probes=((4, 4, 4), (2.0, 2.0, 2.0)), camera=(3.0, 3.0, -4.0), light=(3.0, 6.0, 0.0)),
    # planes that are not axis-aligned (the general scan) cutting between probes
    "tilted_planes": dict(planes=ROOM6 + (((0.6, 0.8, 0.0), -2.0 + 0.003), ((0.0, -0.6, 0.8), 1.5)),
                          spheres=[((2.0, 4.0, 4.0), 0.5)], boxes=[((5.0, 1.0, 2.0), (0.5, 0.5, 0.5))],
                          probes=((4, 4, 4), (2.0, 2.0, 2.0)), camera=(3.0, 4.0, -4.0), light=(1.0, 6.0, 0.0)),
    # a box with a zero extent (a plate in the plane x = 2, on a probe plane) and a point-like one
    "zero_extent_box": dict(planes=ROOM6, spheres=[((4.0, 4.0, 2.0), 0.3)], boxes=[((2.0, 2.0, 2.0), (0.0, 1.0, 1.0)), ((4.0, 2.0, 4.0), (0.0, 0.0, 0.0))],
                            probes=((4, 4, 4), (2.0, 2.0, 2.0)), camera=(3.0, 3.0, -4.0), light=(5.0, 6.0, -1.0)),
    # far from the origin: delta = 2^-12 (1 + lim) is ~0.15 here, far above EPS
    "large_coordinates": dict(planes=(((0, 1, 0), -290.0), ((0, -1, 0), 310.0), ((1, 0, 0), -290.0), ((-1, 0, 0), 310.0), ((0, 0, 1), -290.0), ((0, 0, -1), 310.0)),
                              spheres=[((300.0, 300.5, 303.0), 0.35)], boxes=[((303.0, 297.0, 300.0 + 0.16), (1.0, 1.0, 0.0))],
                              probes=((4, 4, 4), (100.0, 100.0, 100.0)), camera=(300.0, 302.0, 293.0), light=(300.0, 308.0, 298.0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [2, 3])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_clearance_scene_bit_exact(hip, orc, name, spec):
    s = SCENES[name]
    outs = [_render(b, s["planes"], s["spheres"], s["boxes"], _probes(*s["probes"]), s["camera"], s["light"], spec=spec) for b in (hip, orc)]
    assert_parity(*outs)
    for k in outs[1]:
        assert same_bits(outs[0][k], outs[1][k]), k
