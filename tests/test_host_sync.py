"""The owners of the host side's device resources (madarch_amd/csrc/mdh_host.h: DevBuf, Event, create_all, Fence,
RingUse) on the CPU: tests/host_sync_check.cpp replaces the runtime functions they call by stand-ins that log, and
holds the logs against what the renderer's code did by hand before -- under the address and undefined-behaviour
sanitizers, so a handle freed twice, used after its release or never freed ends the program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_owners_against_logged_runtime_calls(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no hip_runtime_api.h under " + ROCM)
    exe = str(tmp_path / "host_sync_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "madarch_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host_sync_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host_sync_check: ok" in out.stdout
