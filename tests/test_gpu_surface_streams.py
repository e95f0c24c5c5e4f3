"""mdh_surface_mesh_device on the device, with torch tensors as the device memory: the bits of the host-array call (which
tests/test_gpu_surface_mesh.py holds against the restatement over the oracle) from tensors and from plain addresses, under
every capacity, the order with the caller's stream without a host wait, and pageable or short arrays refused before a launch.

The checks themselves are tests/surface_device_checks.py and run in ONE child process, started by the first test that asks,
exactly as tests/test_gpu_sweep_streams.py starts its own: PyTorch has to be imported before the library is loaded.  Each
test below is one check's verdict."""
import json
import os
import subprocess
import sys

import pytest

import surface_device_checks as checks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("surface_streams") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "surface_device_checks.py"), out]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(run.stdout[-6000:])
    print(run.stderr[-3000:])
    assert os.path.exists(out), "the checks' process wrote nothing (exit status %d):\n%s" % (run.returncode, run.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert "__error__" not in got, got["__error__"]
    return got


@pytest.mark.parametrize("name", list(checks.CHECKS))
def test_device_surface_mesh(verdicts, name):
    assert name in verdicts, "the checks' process ended before '%s'" % name
    v = verdicts[name]
    print("%.1f s" % v["seconds"])
    assert v["ok"], v["log"]
