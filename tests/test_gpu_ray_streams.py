"""mdh_raycast_device, mdh_raycast_visibility_device, mdh_softshadows_device and mdh_ray_query_wait on the device, with
torch tensors as the device memory: the oracle's bits for every variant k_ray_stream is built for, no bit moved by the
refill threshold, the grid or the order of the rays, every ray answered exactly once and nothing else written, bad rays
refused by the lane that takes them, the order with the caller's stream, nothing edited, every rejection before a launch.

The checks themselves are tests/ray_stream_device_checks.py and run in ONE child process, started by the first test that
asks: PyTorch has to be imported before the library is loaded, and this process loaded the
library long ago -- on the system's runtime, which every other test keeps.  Each test below is one check's verdict.
(No ray here can reach the kernels' stall guard: max_dist is 20, where half an ulp is a thousandth of epsilon.)"""
import json
import os
import subprocess
import sys

import pytest

import ray_stream_device_checks as checks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ray_streams") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "ray_stream_device_checks.py"), out]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    print(run.stdout[-6000:])
    print(run.stderr[-3000:])
    assert os.path.exists(out), "the checks' process wrote nothing (exit status %d):\n%s" % (run.returncode, run.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert "__error__" not in got, got["__error__"]
    return got


@pytest.mark.parametrize("name", list(checks.CHECKS))
def test_device_queries(verdicts, name):
    assert name in verdicts, "the checks' process ended before '%s'" % name
    v = verdicts[name]
    print("%.1f s" % v["seconds"])
    assert v["ok"], v["log"]
