"""The HIP library held DIRECTLY against tests/ref64.py, the float64 renderer written from the reference's shaders: the
cases of test_ref64_oracle.py through the `hip` fixture with the same masks and tolerances (ref64.hold), and the
shapes and variants where a kernel, not the oracle, goes wrong: frame sizes down to one pixel and through
MDH_OPT_SCREEN_SPLIT's halves and quadrants, the room's census kernels and the general ones, both atlas formats on
power-of-two and odd probe settings, frames in flight, Eval_Distances_To's point counts round a wavefront, and the
table residency forced.  The float64 results are computed here, on the GPU machine, inside the tests.
The irradiance fold, the mip chain and the volumetric passes are held in tests/test_gpu_ref64_passes.py."""
import pytest

import ref64_cases as cases
from helpers import ODD_PROBES, SMALL_PROBES
from madarch_amd import _binding as B

pytestmark = pytest.mark.gpu

W, H = 36, 24


@pytest.mark.parametrize("camera", ["identity", "rotated"])
@pytest.mark.parametrize("scene", ["room", "open"])
@pytest.mark.parametrize("mode", [1, 2])
def test_camera_and_screen_modes(hip, mode, scene, camera):
    cases.run_screen(hip, "hip mode %d %s %s" % (mode, scene, camera), scene, W, H, mode, camera=camera)


@pytest.mark.parametrize("ao", [0, 3, 5])
@pytest.mark.parametrize("scene", ["room", "open"])
def test_ambient_occlusion_steps(hip, scene, ao):
    cases.run_screen(hip, "hip mode 2 %s ao %d" % (scene, ao), scene, W, H, 2, camera="rotated", ao=ao)


@pytest.mark.parametrize("ao", [0, 3, 5])
@pytest.mark.parametrize("spec", [0, 2])
@pytest.mark.parametrize("scene", ["room", "open"])
def test_pixel_color_probes_over_written_atlases(hip, scene, spec, ao):
    cases.run_screen(hip, "hip mode 0 %s spec %d ao %d" % (scene, spec, ao), scene, W, H, 0, camera="rotated", ao=ao, spec=spec)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("size", [(1, 1), (9, 3), (61, 37)])
def test_frame_sizes(hip, size, mode):
    """one pixel, less than a tile, and partial tiles at the right and lower edge"""
    cases.run_screen(hip, "hip %dx%d mode %d" % (size + (mode,)), "room", size[0], size[1], mode, camera="rotated")


@pytest.mark.parametrize("limit", [0, 60, 2560], ids=["whole", "halves", "quadrants"])
def test_split_tiles(hip, limit):
    """44 x 28 = 6 x 4 = 24 tiles, the last column and row partial: MDH_OPT_SCREEN_SPLIT 2560 gives a tile to four
    wavefronts (4 x 24 <= 2560), 60 to two (2 x 24 <= 60 < 4 x 24), 0 to one"""
    def prepare(R):
        R.Set_Option(B.OPT_SCREEN_SPLIT, limit)
    cases.run_screen(hip, "hip split %d" % limit, "room", 44, 28, 0, camera="rotated", prepare=prepare)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("second_sphere", [False, True], ids=["room-census", "general"])
def test_kernel_variants(hip, second_sphere, mode):
    """the room as it is runs the MDH_PF_ROOM kernels; with a second sphere it runs the general ones"""
    cases.run_screen(hip, "hip variant %d mode %d" % (second_sphere, mode), "room", W, H, mode, camera="rotated",
                     scene_kw={"second_sphere": second_sphere})


@pytest.mark.parametrize("atlas", [1, 0], ids=["f32", "rgb8"])
@pytest.mark.parametrize("probes", [SMALL_PROBES, ODD_PROBES], ids=["small", "odd"])
def test_radiance_pass_whole_atlas(hip, probes, atlas):
    """SMALL_PROBES runs the MDH_PF_POW2 kernels, ODD_PROBES the divisions"""
    cases.run_radiance(hip, "hip radiance %s" % ("rgb8" if atlas == 0 else "f32"), probes, atlas)


@pytest.mark.parametrize("overlap", [0, 2])
def test_frames_in_flight(hip, overlap):
    """Three whole frames through Render, none waited for, then the written atlases, the screen pass and the read-back.
    With OPT_FRAME_OVERLAP 2 the three frames are pipelined (mdh_frame_begin .. mdh_frame_end): their probe passes run on
    the probe stream and rotate the atlas sets, their screen passes alternate between two streams and two framebuffers.
    The atlases must land in the set the last frame left current, behind that frame's passes; the screen pass must read
    that set and draw, behind the alternate stream's frame, the framebuffer that the read-back then takes.  What the
    pipelined probe passes compute is not held here (the passes alone are, in test_gpu_ref64_passes.py; what they compute
    with frames in flight is held against the oracle in test_gpu_parity.py)."""
    def prepare(R):
        R.Set_Option(B.OPT_FRAME_OVERLAP, overlap)
        assert R.Get_Option(B.OPT_FRAME_OVERLAP) == overlap
    cases.run_screen(hip, "hip overlap %d, mode 0" % overlap, "room", W, H, 0, camera="rotated", prepare=prepare, burst=3)


@pytest.mark.parametrize("overlap", [0, 2])
@pytest.mark.parametrize("mode", [1, 2])
def test_frames_in_flight_screen_only(hip, mode, overlap):
    """A burst of three identical frames through Render, read after the last.  Modes 1 and 2 run no probe passes, but
    with OPT_FRAME_OVERLAP 2 their frames are pipelined all the same: the screen passes alternate between the main and
    the alternate stream and between the two framebuffers, so the third frame is drawn on the alternate stream into the
    second framebuffer, and the read-back has to wait for that stream and take that buffer."""
    def prepare(R):
        R.Set_Option(B.OPT_FRAME_OVERLAP, overlap)
        assert R.Get_Option(B.OPT_FRAME_OVERLAP) == overlap
    cases.run_screen(hip, "hip overlap %d, mode %d" % (overlap, mode), "room", W, H, mode, camera="rotated", prepare=prepare, frames=3)


@pytest.mark.parametrize("kinds", cases.KIND_SETS, ids=["-".join(k) for k in cases.KIND_SETS])
def test_eval_distances_to(hip, kinds):
    cases.run_distance(hip, "hip distance " + "-".join(kinds), kinds)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4099])
def test_eval_distances_to_point_counts(hip, count):
    """round a wavefront's 64 lanes, and a last partial block"""
    cases.run_distance(hip, "hip distance %d points" % count, cases.KIND_SETS[-1], count=count)


def test_eval_distances_to_with_forced_table_residency(hip):
    """the same points through Geo<true>: the scene's table read from device memory (forced as tests/test_gpu_large_scenes.py does)"""
    def prepare(R):
        R.Set_Option(B.OPT_TABLE_RESIDENCY, 1)
        assert R.Get_Option(B.OPT_TABLE_RESIDENCY) == 1
    cases.run_distance(hip, "hip distance, table in device memory", cases.KIND_SETS[-1], prepare=prepare)
    cases.run_distance(hip, "hip distance, triangles, table in device memory", ("Triangle",), prepare=prepare)
