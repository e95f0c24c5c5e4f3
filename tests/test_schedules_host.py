"""The pass-to-pass schedules on the host.  ReplaySchedule (madarch_amd/csrc/mdh_host.h) decides whether a radiance or a
screen pass marches, records or replays (MDH_OPT_RADIANCE_REPLAY, MDH_OPT_SCREEN_REPLAY); ResortClock decides when the probe
rays and the screen's tiles are sorted again (MDH_OPT_RADIANCE_ORDER, MDH_OPT_SCREEN_ORDER).  Neither makes a runtime call:
tests/schedule_check.cpp drives them with scripted passes -- a standing key, changing and alternating keys, a change during
replay, recording never admissible, records without a buffer, regrowth, the option toggled in both flavours, a failed
allocation, the clock's two periods, force and forget -- and states the exact REC of every pass and every pass that sorts,
under the address and undefined-behaviour sanitizers.  Beside it: the renderer holds the schedules and nothing flat."""
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


def test_schedules_against_scripted_passes(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no hip_runtime_api.h under " + ROCM)
    exe = str(tmp_path / "schedule_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "madarch_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "schedule_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "schedule_check: ok" in out.stdout


def test_renderer_holds_the_schedules_and_nothing_flat():
    api = text("madarch_amd", "csrc", "mdh_api.hip")
    host = text("madarch_amd", "csrc", "mdh_host.h")
    for member in (r"ReplaySchedule<RadRecKey>\s+rad_replay;", r"ReplaySchedule<ScrRecKey>\s+scr_replay;",
                   r"ResortClock<RadOrderOf>\s+rad_order;", r"ResortClock<ScrOrderOf>\s+scr_order;"):
        assert len(re.findall(member, api)) == 1, member
    flat = r"\b(rad|scr)_(rec|seen)_(key|valid)\b(?!\()|\bscr_rec_no_memory\b|\b(rad|scr)_replay_stats\b|\b(rad|scr)_order_\w+"
    assert re.findall(flat, api) == []
    # each rule stands once, in the header; the periods went with it and can still be set from the command line
    assert "MDH_RAD_RESORT" not in re.sub(r"//[^\n]*", "", api)
    for macro, value in (("MDH_RAD_RESORT", 64), ("MDH_RAD_RESORT_MOVING", 8)):
        assert re.search(r"#ifndef %s\n#define %s %d\n#endif" % (macro, macro, value), host)
    assert len(re.findall(r"age >= MDH_RAD_RESORT\b", host)) == 1 and len(re.findall(r"age >= MDH_RAD_RESORT_MOVING\b", host)) == 1
