"""The space partition of the CPU oracle against tests/ref64.py (the sibling of test_ref64_oracle.py): the tables the three
builders write, the lookup at seeded points round and beyond the grid, and whole frames and a radiance pass marched
through a table.  ref64's partition is written from the reference's text alone (madarch-scenes.adb:799-1187,
madarch-renderers.adb:539-755, compute_scene_partitioning.glsl) and shares nothing with the oracle or the kernels, which
share their lookups with each other.

Tables: every record that float64 can decide (ref64.decision_margin; at most 5 % of a case's records cannot be) must be
the builder's, and the warnings counted.  Frames: over the table read back from the oracle, held by ref64.hold at its
tolerances and its 5 % cap; each case first shows, in float64 alone, that its table changes the frame.
The grids and scenes are ref64_cases.GRIDS and ref64_cases.rows; tests/test_gpu_ref64_partition.py runs the HIP library
through the same cases."""
import numpy as np
import pytest

import ref64
import ref64_cases as cases


@pytest.mark.parametrize("method", ["CPU_Fast", "GPU_Fast"])
@pytest.mark.parametrize("grid", ["A", "B", "C", "D"])
def test_tables(orc, grid, method):
    """C is odd: GPU_Fast leaves records unwritten and writes the others where the lookup does not read them; D: the CPU
    builders read the binary32 settings, the GPU builder and the lookup their six-digit text"""
    cases.run_partition_table(orc, "table %s %s" % (grid, method), "plain", grid, method)


@pytest.mark.parametrize("grid", ["A", "E"])
def test_tables_cpu_best(orc, grid):
    """Find_Candidates: the order of first acceptance over the 27 sample points"""
    cases.run_partition_table(orc, "table %s CPU_Best" % grid, "plain", grid, "CPU_Best")


@pytest.mark.parametrize("method", ["CPU_Fast", "GPU_Fast"])
def test_tables_that_overflow(orc, method):
    """34 spheres and an index_count of 8: lists are cut kind by kind in declared order, every cut is a warning (Q7).
    (CPU_Best accepts at most a handful of candidates per cell and cuts nothing here.)"""
    cases.run_partition_table(orc, "table A %s, index_count 8" % method, "34 spheres", "A", method, index_count=8, overflow=True)


@pytest.mark.parametrize("method", ["CPU_Fast", "GPU_Fast"])
def test_tables_with_exact_ties(orc, method):
    """grid F on its scene's lattice: a wall exactly as far as the threshold is no candidate (`dist < threshold`, strictly)"""
    cases.run_partition_table(orc, "table F %s" % method, "ties", "F", method, ties=True)


@pytest.mark.parametrize("border", ["Clamp", "Fallback"])
def test_lookups_round_the_grid(orc, border):
    cases.run_partition_lookups(orc, "lookups A %s" % border, border)


FRAMES = [("A", "Clamp", "CPU_Fast"), ("A", "Fallback", "CPU_Fast"), ("B", "Clamp", "CPU_Fast"), ("C", "Clamp", "GPU_Fast")]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("grid,border,method", FRAMES, ids=["-".join(f) for f in FRAMES])
def test_frames_through_a_table(orc, grid, border, method, mode):
    """modes 1 and 2; A Fallback in mode 2 is the case whose shadow steps reach a negative radicand (the grid is smaller
    than the room: a ray that leaves it goes from a cell's few candidates to the full scan)"""
    cases.run_partition_screen(orc, "partition %s %s %s mode %d" % (grid, border, method, mode), "plain", grid, method, mode, border=border,
                               negative=(mode == 2 and border == "Fallback"))


def test_pixel_color_probes_through_a_table(orc):
    """mode 0 over written atlases with specular mode 2: the reflected ray, the cage's visibility rays, the soft shadows and the
    occlusion samples all go through the table"""
    cases.run_partition_screen(orc, "partition A Clamp mode 0", "plain", "A", "CPU_Fast", 0)


@pytest.mark.parametrize("grid", sorted(cases.PARTITION_RADIANCE))
def test_radiance_pass_through_a_table(orc, grid):
    cases.run_partition_radiance(orc, "partition radiance %s" % grid, grid)


@pytest.mark.parametrize("case", sorted(c for c in cases.PARTITION_FRAMES if not cases.PARTITION_FRAMES[c].get("resident")),
                         ids=lambda c: c.replace(" ", "-"))
def test_frames_of_the_gpu_file(orc, case):
    """the frames tests/test_gpu_ref64_partition.py chooses by kernel variant, on the oracle: the scenes' variants (34 spheres,
    triangles, two radii), grid D, one pixel and 61 x 37 (not the two with the table residency forced, an option of the library) -- so that their float64 conditions and caps are shown to hold here"""
    cases.run_partition_frame(orc, case)


def test_the_nan_ignoring_minimum_changes_no_case_without_a_partition():
    """Run.softshadows takes the square root of the radicand as it is and lets min ignore the NaN.  Without a partition the
    distance is 1-Lipschitz and the radicand cannot be negative -- softshadows asserts that at every step of every case that
    has no partition -- so every earlier case computes what it computed with the radicand clamped at 0.  Shown here on the
    two scenes of test_ref64_oracle.py, where no pixel reports one and the unclamped root is the clamped one."""
    for scene in ("room", "open"):
        desc = cases.describe(scene, "rotated")
        out = ref64.screen(desc, 36, 24, 2)
        assert not out["negative"].any()
        assert np.isfinite(out["colour"]).all()
