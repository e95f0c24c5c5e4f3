"""Whole frames of the CPU oracle against tests/ref64.py, a float64 renderer written from the reference's shaders that
shares nothing with the oracle.  The pins (test_oracle_pins.py, test_oracle_pins64.py) hold the pieces; this file holds
how they are assembled into a pixel and a radiance texel: the camera with an orientation, ambient occlusion, the
composition of pixel_color_probes, the radiance pass's addressing, screen modes 1 and 2, the triangle's distance against
the geometric one, and Eval_Distances_To on thousands of points.

Fragile pixels are decided by the float64 renderer alone (ref64.fragile: three runs, two of them with every ray
jittered by 2^-18) and are at most 5 % of a case; every other pixel must agree (ref64.hold).

The second half holds the passes the pins only hold in pieces, whole and with no share that may fail: the irradiance
fold over every texel of the atlas (with hysteresis, in both formats, over a sparse atlas), the optional mip chain, the
froxel texture under two lights (one a spot light), the scattering texture over written froxels and inside a whole
frame, and the volumetric composition of a pixel.  The shapes are those of tests/test_gpu_ref64_passes.py, where the
kernels change form; here they prove ref64's new code and show that the fragile caps hold for the reference alone.

The space partition -- its builders, its lookup and frames marched through a table -- is held in
test_ref64_partition_oracle.py.  Not covered: user-defined kinds, indirect-specular modes 1 and 3 (restated in
test_oracle_pins64.py)."""
import pytest

import ref64_cases as cases
from helpers import ODD_PROBES, SMALL_PROBES

W, H = 36, 24


@pytest.mark.parametrize("camera", ["identity", "rotated"])
@pytest.mark.parametrize("scene", ["room", "open"])
@pytest.mark.parametrize("mode", [1, 2])
def test_camera_and_screen_modes(orc, mode, scene, camera):
    """draw_screen.glsl:20-24 (the matrix acts on the direction and on the fragment's position) under BASELINE configs 1
    (0.5 n + 0.5, no tone map) and 2 (direct light times AO, tone map)"""
    cases.run_screen(orc, "mode %d %s %s" % (mode, scene, camera), scene, W, H, mode, camera=camera)


@pytest.mark.parametrize("ao", [0, 3, 5])
@pytest.mark.parametrize("scene", ["room", "open"])
def test_ambient_occlusion_steps(orc, scene, ao):
    """lighting.glsl:51-69: weights 1 / 2^i, 0.6 + 0.4 sum / max; on mode 2, where it multiplies the direct light"""
    cases.run_screen(orc, "mode 2 %s ao %d" % (scene, ao), scene, W, H, 2, camera="rotated", ao=ao)


@pytest.mark.parametrize("ao", [0, 3, 5])
@pytest.mark.parametrize("spec", [0, 2])
@pytest.mark.parametrize("scene", ["room", "open"])
def test_pixel_color_probes_over_written_atlases(orc, scene, spec, ao):
    """render_probes.glsl:246-291 whole: ao * (direct + indirect), the roughness < 0.75 gate, compute_indirect_lighting with
    L = reflect (dir, n) and V = -dir, the sky; both atlases written as seeded random arrays, the screen pass alone"""
    cases.run_screen(orc, "mode 0 %s spec %d ao %d" % (scene, spec, ao), scene, W, H, 0, camera="rotated", ao=ao, spec=spec)


@pytest.mark.parametrize("probes,atlas", [(SMALL_PROBES, 1), (ODD_PROBES, 1), (ODD_PROBES, 0)], ids=["small-f32", "odd-f32", "odd-rgb8"])
def test_radiance_pass_whole_atlas(orc, probes, atlas):
    """compute_probe_radiance.glsl:16-27 with probe_utils.glsl: which probe and which ray a texel belongs to, where the probe
    stands, and the probe pass's defines (no direct specular); two lights, one of them a spot light"""
    cases.run_radiance(orc, "radiance %s" % ("rgb8" if atlas == 0 else "f32"), probes, atlas)


@pytest.mark.parametrize("kinds", cases.KIND_SETS, ids=["-".join(k) for k in cases.KIND_SETS])
def test_eval_distances_to(orc, kinds):
    """Eval_Distance_To (madarch-renderers.adb:499-526) on several thousand seeded points, the triangle against the
    GEOMETRIC distance (closest point by barycentric regions), with a long thin and a nearly degenerate triangle"""
    cases.run_distance(orc, "distance " + "-".join(kinds), kinds)


# ---------------------------------------------------------------------------------------- the irradiance fold
@pytest.mark.parametrize("sparse", [False, True], ids=["uniform", "sparse"])
@pytest.mark.parametrize("rres,ires", cases.IRRADIANCE_SHAPES, ids=["%dx%d" % s for s in cases.IRRADIANCE_SHAPES])
def test_irradiance_fold_whole_atlas(orc, rres, ires, sparse):
    """update_probe_irradiance.glsl:8-43 with probe_utils.glsl, every texel of the atlas"""
    cases.run_irradiance(orc, "irradiance %dx%d%s" % (rres, ires, " sparse" if sparse else ""), cases.irradiance_probes(rres, ires), 1, sparse=sparse)


@pytest.mark.parametrize("rres,ires", [(16, 8), (12, 6)])
def test_irradiance_fold_rgb8(orc, rres, ires):
    cases.run_irradiance(orc, "irradiance %dx%d rgb8" % (rres, ires), cases.irradiance_probes(rres, ires), 0)


@pytest.mark.parametrize("atlas", [1, 0], ids=["f32", "rgb8"])
@pytest.mark.parametrize("rres,ires", [(16, 8), (12, 6), (8, 10)])
def test_irradiance_fold_with_hysteresis(orc, rres, ires, atlas):
    """stored = mix (fresh, previous, 0.35) over a written previous atlas (not in the reference: irradiance_blend)"""
    cases.run_irradiance(orc, "irradiance %dx%d hysteresis %s" % (rres, ires, "rgb8" if atlas == 0 else "f32"), cases.irradiance_probes(rres, ires),
                         atlas, hysteresis=350)


@pytest.mark.parametrize("atlas", [1, 0], ids=["f32", "rgb8"])
def test_radiance_mip_chain(orc, atlas):
    cases.run_mips(orc, "mips %s" % ("rgb8" if atlas == 0 else "f32"), atlas)


# ---------------------------------------------------------------------------------------- the volumetric passes
@pytest.mark.parametrize("case", sorted(cases.FROXEL_CASES), ids=lambda c: c.replace(" ", "-"))
def test_froxel_texture(orc, case):
    """compute_frustrum_visibility.glsl:8-42 whole, a point light and a spot light"""
    cases.run_froxels(orc, "froxels " + case, **cases.FROXEL_CASES[case])


@pytest.mark.parametrize("case", sorted(cases.SCATTERING_CASES), ids=lambda c: c.replace(" ", "-"))
def test_scattering_texture(orc, case):
    """accumulate_scattering.glsl:9-48 whole: over written froxels, inside a whole frame, and as a pass of its own"""
    cases.run_scattering(orc, "scattering " + case, **cases.SCATTERING_CASES[case])


@pytest.mark.parametrize("sres", [(24, 24), (23, 21)], ids=["24x24", "23x21"])
@pytest.mark.parametrize("size", [(36, 24), (1, 1)], ids=["36x24", "1x1"])
def test_pixel_with_volumetrics(orc, size, sres):
    """volumetrics.glsl:34-54 inside pixel_color_probes: the 3 x 3 depth-aware pick over a written scattering texture"""
    cases.run_screen(orc, "volumetric pixel %dx%d over %dx%d" % (size + sres), "room", size[0], size[1], 0, camera="rotated", vol=cases.volume(sres=sres))
