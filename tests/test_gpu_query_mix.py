"""Every family of queries -- ray queries, swept spheres and contacts, shaded rays, shaded points, path tracing,
in-scattering; host form, then device form on two caller streams alternately -- on ONE renderer, each answer held bit for bit
against the same call made alone on a fresh renderer, and each kernel time against the host's clock around its call.  The
families share one bridge between the streams, one pair of timing events and one staging buffer ("The query path"):
65 rays are one past a wavefront, and 300 rays behind a first host batch of 64 make the staging buffer grow past its floor
of 256 rays while a device query may still be on the query stream.

The checks themselves are tests/query_mix_device_checks.py and run in ONE child process, started by the first test that
asks, as tests/test_gpu_ray_streams.py starts its own: PyTorch has to be imported before the library is loaded
(INTEGRATION.md section 5).  Each test below is one check's verdict."""
import json
import os
import subprocess
import sys

import pytest

import query_mix_device_checks as checks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("query_mix") / "verdicts.json")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tests", "query_mix_device_checks.py"), out]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(run.stdout[-12000:])
    print(run.stderr[-3000:])
    assert os.path.exists(out), "the checks' process wrote nothing (exit status %d):\n%s" % (run.returncode, run.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert "__error__" not in got, got["__error__"]
    return got


@pytest.mark.parametrize("name", list(checks.CHECKS))
def test_query_mix(verdicts, name):
    assert name in verdicts, "the checks' process ended before '%s'" % name
    v = verdicts[name]
    print("%.1f s" % v["seconds"])
    assert v["ok"], v["log"]
