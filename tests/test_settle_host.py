"""MDH_OPT_PROBE_SETTLE on the host.  SettleTracker (madarch_amd/csrc/mdh_host.h) decides, without waiting for the device,
whether a frame's probe passes may be left out: tests/settle_check.cpp drives it with scripted sequences -- slots arriving
0 to 4 passes late, a changed pass inside a run, an edit between enqueue and arrival, the ring wrapping, a schedule switch,
the option toggled, more than one rank -- and states exactly which frames leave their passes out, under the address and
undefined-behaviour sanitizers.  Beside it: the option's number in all four interfaces and the counter's entry point."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_tracker_against_scripted_sequences(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no hip_runtime_api.h under " + ROCM)
    exe = str(tmp_path / "settle_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "madarch_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "settle_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "settle_check: ok" in out.stdout


def test_option_and_counter_in_every_interface():
    from madarch_amd import _binding as B
    from madarch_amd import renderers
    header = text("include", "madarch_hip.h")
    assert int(re.search(r"MDH_OPT_PROBE_SETTLE\s*=\s*(\d+)", header).group(1)) == 23
    assert B.OPT_PROBE_SETTLE == 23
    assert re.search(r"Opt_Probe_Settle\s*=\s*MDH_OPT_PROBE_SETTLE\s*;", text("include", "madarch.hpp"))
    assert int(re.search(r"Opt_Probe_Settle\s*:\s*constant int\s*:=\s*(\d+)\s*;", text("ada", "madarch_hip.ads")).group(1)) == 23
    assert re.search(r"int32_t\s+mdh_probe_settle_stats\s*\(\s*mdh_renderer\s*\*", header)
    assert "probe_settle_stats" in B.HIP_ONLY_ABI
    assert callable(renderers.Renderer.Probe_Settle_Stats)
    # exactness needs as many unchanged passes as there are atlas sets; the margin keeps short static runs as they were
    host = text("madarch_amd", "csrc", "mdh_host.h")
    sets = int(re.search(r"#define MDH_ATLAS_SETS (\d+)", text("madarch_amd", "csrc", "mdh_api.hip")).group(1))
    assert int(re.search(r"#define MDH_SETTLE_PASSES (\d+)", host).group(1)) == 16 >= sets
