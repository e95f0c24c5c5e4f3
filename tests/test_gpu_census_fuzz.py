"""The census fuzzer (tests/fuzz_census.py) in the GPU suite: random scenes of the rooms' census (MDH_PF_ROOM), of the
partition's small form (MDH_PF_PSMALL) and one change away from either, on the HIP library against the oracle with the
bar of tests/test_gpu_fuzz.py.  The diagnostic build's mdh_diag_variant confirms that every seed runs the kernel variant
its family is meant to reach, so the fuzzer cannot drift to the general kernels unnoticed.
scripts/fuzz_parity.py --census room|psmall|near runs further seeds."""
import os
import subprocess
import sys
import time

import pytest

import fuzz_census
from fuzz_scenes import compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITERAL = os.path.join(ROOT, "madarch_amd", "csrc", "libmadarch_hip_literal.so")
ROOM, PSMALL, NEAR = fuzz_census.seeds("room", 0, 32), fuzz_census.seeds("psmall", 0, 16), fuzz_census.seeds("near", 0, 20)


@pytest.mark.parametrize("seed", ROOM + PSMALL + NEAR)
def test_census_scene(hip, orc, seed):
    compare(fuzz_census.build(seed, hip), fuzz_census.build(seed, orc))


SCRIPT = r"""
import ctypes as C, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import fuzz_census as fc
from madarch_amd import _binding as B
hip = B.hip_binding()
assert hasattr(hip.lib, "mdh_diag_variant"), "not the literal build"
hip.lib.mdh_diag_variant.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
counts = {}
for seed in %r:
    R, desc, st = fc.create(seed, hip)
    R.Render()
    want = fc.expected_pfk(desc)
    pr = R.Probes
    p2 = lambda v: v > 0 and v & (v - 1) == 0
    pow2 = int(p2(pr.Probe_Count[0]) and p2(pr.Probe_Count[1]) and p2(pr.Radiance_Resolution) and p2(pr.Irradiance_Resolution))
    for p in [B.PASS_SCREEN] + ([B.PASS_RADIANCE] if st["mode"] == 0 else []):
        v = np.zeros(2, np.int32)
        assert hip.lib.mdh_diag_variant(R._h, p, v.ctypes.data) == 0
        assert v[0] == want, ("variant", seed, fc.describe(seed)[1], B.PASS_NAMES[p], int(v[0]), want)
        assert v[1] == pow2, ("pow2", seed, B.PASS_NAMES[p], int(v[1]), pow2)
    R.Destroy()
    key = (fc.family(seed), fc.census(desc), want)
    counts[key] = counts.get(key, 0) + 1
for k in sorted(counts, key=str):
    print("family %%-6s census %%-6s variant %%2d: %%d seeds" %% (k[0], k[1], k[2], counts[k]))
print("CENSUS_VARIANTS_OK")
""" % (ROOT, ROOT, ROOM + PSMALL + NEAR)


def test_seeds_reach_their_census():
    assert os.path.exists(LITERAL), "build first (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, MADARCH_HIP_LIBRARY=LITERAL)
    t = time.time()
    out = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    print("wall time %.1f s" % (time.time() - t))
    assert "CENSUS_VARIANTS_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
