"""The HIP library's irradiance fold, mip chain and volumetric passes held DIRECTLY against tests/ref64.py, the float64
renderer written from the reference's shaders, through the cases of test_ref64_oracle.py (tests/ref64_cases.py) with
the same tolerances and the same rule: fragile texels are decided by float64 alone and are at most 5 % of a case, every
other texel must agree.  The shapes are the smallest at which each kernel takes each of its forms.

Irradiance (k_irradiance), radiance resolution x irradiance resolution, eight probes in (4, 2) tiles unless said:
  8 x 8    one turn of 64 taps, two chunks: the tap index clamps and the loop body runs once
  16 x 8   four turns, with the steady-state prefetch
  5 x 2    25 taps, less than one chunk of 32: the tap-by-tap form, 4 of 64 lanes fold
  12 x 6   ODD_PROBES, 15 x 5 tiles: 144 taps = 4.5 chunks, 36 lanes
  10 x 3   100 taps, 9 lanes
  8 x 10   100 texels per probe: the general form, one round of its loop
  8 x 17   289 texels: two rounds
  48 x 16  72 KiB of LDS, through hipFuncSetAttribute
each over a uniform and over a sparse atlas (a tap from the wrong lane, chunk or turn then shows as tens of per cent);
RGB8, and hysteresis in both formats, where the issue of a format or of the blend can differ.

Froxels (k_visibility), the three froxel-to-lane layouts: 8 x 8 x 8 (4 x 4 x 4 blocks), 24 x 6 x 4 (8 x 8 tiles of the
24 x 24 image, vh no multiple of 4), 10 x 7 x 3 (row-major, 210 froxels: a partial last workgroup); a point and a spot
light, the room and the open scene, the camera with and without an orientation.

Scattering (k_scat_fold): 483 texels (no multiple of a workgroup's 16); ten coarse steps (only the fold's tail loop, the two
step sizes different); exactly 128 steps (a texel fills the chunk of 128 and the loop leaves on its second turn);
several chunks; equal step sizes (every sample on a slice boundary); and the march fused into the visibility pass's
launch, which runs only inside a whole frame, beside the scattering pass's own march outside one.

The float64 results are computed here, on the GPU machine, inside the tests, once per case."""
import pytest

import ref64_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sparse", [False, True], ids=["uniform", "sparse"])
@pytest.mark.parametrize("rres,ires", cases.IRRADIANCE_SHAPES, ids=["%dx%d" % s for s in cases.IRRADIANCE_SHAPES])
def test_irradiance_fold_whole_atlas(hip, rres, ires, sparse):
    cases.run_irradiance(hip, "hip irradiance %dx%d%s" % (rres, ires, " sparse" if sparse else ""), cases.irradiance_probes(rres, ires), 1, sparse=sparse)


@pytest.mark.parametrize("rres,ires", [(16, 8), (12, 6)])
def test_irradiance_fold_rgb8(hip, rres, ires):
    cases.run_irradiance(hip, "hip irradiance %dx%d rgb8" % (rres, ires), cases.irradiance_probes(rres, ires), 0)


@pytest.mark.parametrize("atlas", [1, 0], ids=["f32", "rgb8"])
@pytest.mark.parametrize("rres,ires", [(16, 8), (12, 6), (8, 10)])
def test_irradiance_fold_with_hysteresis(hip, rres, ires, atlas):
    cases.run_irradiance(hip, "hip irradiance %dx%d hysteresis %s" % (rres, ires, "rgb8" if atlas == 0 else "f32"), cases.irradiance_probes(rres, ires),
                         atlas, hysteresis=350)


def test_irradiance_fold_after_the_large_tile(hip):
    """the 48 x 16 fold, then 16 x 8 twice on one renderer over two atlases: the second pass folds through the tap scratch
    that the first allocated, and after a renderer whose fold asked for the large LDS"""
    cases.run_irradiance(hip, "hip irradiance 48x16", cases.irradiance_probes(48, 16), 1)
    cases.run_irradiance(hip, "hip irradiance 16x8, second pass", cases.irradiance_probes(16, 8), 1, passes=2)


@pytest.mark.parametrize("atlas", [1, 0], ids=["f32", "rgb8"])
def test_radiance_mip_chain(hip, atlas):
    cases.run_mips(hip, "hip mips %s" % ("rgb8" if atlas == 0 else "f32"), atlas)


@pytest.mark.parametrize("case", sorted(cases.FROXEL_CASES), ids=lambda c: c.replace(" ", "-"))
def test_froxel_texture(hip, case):
    cases.run_froxels(hip, "hip froxels " + case, **cases.FROXEL_CASES[case])


@pytest.mark.parametrize("case", sorted(cases.SCATTERING_CASES), ids=lambda c: c.replace(" ", "-"))
def test_scattering_texture(hip, case):
    cases.run_scattering(hip, "hip scattering " + case, **cases.SCATTERING_CASES[case])


@pytest.mark.parametrize("sres", [(24, 24), (23, 21)], ids=["24x24", "23x21"])
@pytest.mark.parametrize("size", [(36, 24), (1, 1)], ids=["36x24", "1x1"])
def test_pixel_with_volumetrics(hip, size, sres):
    cases.run_screen(hip, "hip volumetric pixel %dx%d over %dx%d" % (size + sres), "room", size[0], size[1], 0, camera="rotated", vol=cases.volume(sres=sres))
