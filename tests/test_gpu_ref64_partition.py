"""The HIP library's space partition held DIRECTLY against tests/ref64.py: the cases of test_ref64_partition_oracle.py
through the `hip` fixture, chosen by kernel variant.  The oracle and the kernels share the source of their lookups, so a
misreading of the reference that both share passes every parity test; ref64's partition is written from the reference's
text alone.

Tables: k_partition_build (GPU_Fast) on every grid, k_partition_build_gtab with the table residency forced, the host
builders once each.  The candidate sets the kernels keep as bits (k_partition_bits) are held by the frames: a wrong bit moves a
march.  Frames (ref64_cases.PARTITION_FRAMES): the small straight-line form, the general form with a division by the spacing,
the Fallback variants with their negative shadow radicands, global residency, more than 32 of a kind, triangles in the
partition, two sphere radii, an odd grid built on the device, settings with more than six digits, one pixel and partial
tiles; the radiance pass on two grids.  test_cases_reach_their_variants reads from the diagnostic build which kernel
family each frame ran.  The float64 side is computed here, on the GPU machine, and cached per process."""
import os
import subprocess
import sys

import pytest

import ref64_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITERAL = os.path.join(ROOT, "madarch_amd", "csrc", "libmadarch_hip_literal.so")


@pytest.mark.parametrize("grid", ["A", "B", "C", "D"])
def test_tables_built_on_the_device(hip, grid):
    """k_partition_build: C is odd (the even dispatch, the skewed record index), D has more than six digits"""
    cases.run_partition_table(hip, "hip table %s GPU_Fast" % grid, "plain", grid, "GPU_Fast")


def test_table_built_on_the_device_with_forced_residency(hip):
    """k_partition_build_gtab, on the odd grid"""
    cases.run_partition_table(hip, "hip table C GPU_Fast, table in device memory", "plain", "C", "GPU_Fast", prepare=cases.force_residency)


@pytest.mark.parametrize("method", ["CPU_Best", "CPU_Fast"])
def test_tables_built_on_the_host(hip, method):
    cases.run_partition_table(hip, "hip table A %s" % method, "plain", "A", method)


@pytest.mark.parametrize("method", ["CPU_Fast", "GPU_Fast"])
def test_tables_that_overflow(hip, method):
    cases.run_partition_table(hip, "hip table A %s, index_count 8" % method, "34 spheres", "A", method, index_count=8, overflow=True)


@pytest.mark.parametrize("method", ["CPU_Fast", "GPU_Fast"])
def test_tables_with_exact_ties(hip, method):
    cases.run_partition_table(hip, "hip table F %s" % method, "ties", "F", method, ties=True)


@pytest.mark.parametrize("case", sorted(cases.PARTITION_FRAMES), ids=lambda c: c.replace(" ", "-"))
def test_frames_through_a_table(hip, case):
    cases.run_partition_frame(hip, case)


@pytest.mark.parametrize("grid", sorted(cases.PARTITION_RADIANCE))
def test_radiance_pass_through_a_table(hip, grid):
    """k_radiance with the partition: the general form on A, the small form on B"""
    cases.run_partition_radiance(hip, "hip partition radiance %s" % grid, grid)


SCRIPT = r"""
import ctypes as C, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import ref64_cases as cases
from madarch_amd import _binding as B
hip = B.hip_binding()
assert hasattr(hip.lib, "mdh_diag_variant"), "not the literal build"
hip.lib.mdh_diag_variant.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
def variant(R, p):
    v = np.zeros(2, np.int32)
    assert hip.lib.mdh_diag_variant(R._h, p, v.ctypes.data) == 0
    R.Destroy()
    return int(v[0])
for case in sorted(cases.PARTITION_FRAMES):
    got, want = variant(cases.render_partition_frame(hip, case), B.PASS_SCREEN), cases.PARTITION_FRAMES[case]["pfk"]
    print("screen   %%-20s variant %%3d" %% (case, got))
    assert got == want, ("variant", case, got, want)
for grid in sorted(cases.PARTITION_RADIANCE):
    got, want = variant(cases.render_partition_radiance(hip, grid), B.PASS_RADIANCE), cases.PARTITION_RADIANCE[grid]
    print("radiance %%-20s variant %%3d" %% (grid, got))
    assert got == want, ("variant", grid, got, want)
print("PARTITION_VARIANTS_OK")
""" % (ROOT, ROOT)


def test_cases_reach_their_variants():
    """each frame case once on the diagnostic (literal) build, in a child process: mdh_diag_variant must report the kernel family the
    case is named for, so that no case drifts to another kernel unnoticed"""
    assert os.path.exists(LITERAL), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, MADARCH_HIP_LIBRARY=LITERAL)
    out = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, timeout=300, env=env)
    print(out.stdout)
    assert "PARTITION_VARIANTS_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
