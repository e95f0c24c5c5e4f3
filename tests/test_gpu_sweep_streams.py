"""mdh_spherecast_device and mdh_contacts_device on the device, with torch tensors as the device memory: in every variant
the bits of the host-array calls (which tests/test_gpu_sweeps.py holds against the chain over the oracle), no bit moved by
the refill threshold, the grid or the order of the rays, every ray and centre answered exactly once and nothing else
written, bad rays and centres refused by the lane that takes them, the order with the caller's stream, nothing edited,
every rejection before a launch.

The checks themselves are tests/sweep_device_checks.py and run in ONE child process, started by the first test that asks,
exactly as tests/test_gpu_ray_streams.py starts its own: PyTorch has to be imported before the library is loaded.  Each
test below is one check's verdict.
(No ray here can reach the kernels' stall guard: max_dist is 20, where half an ulp is a thousandth of epsilon.)"""
import json
import os
import subprocess
import sys

import pytest

import sweep_device_checks as checks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sweep_streams") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "sweep_device_checks.py"), out]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(run.stdout[-6000:])
    print(run.stderr[-3000:])
    assert os.path.exists(out), "the checks' process wrote nothing (exit status %d):\n%s" % (run.returncode, run.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert "__error__" not in got, got["__error__"]
    return got


@pytest.mark.parametrize("name", list(checks.CHECKS))
def test_device_sweeps(verdicts, name):
    assert name in verdicts, "the checks' process ended before '%s'" % name
    v = verdicts[name]
    print("%.1f s" % v["seconds"])
    assert v["ok"], v["log"]
