"""MDH_OPT_SCREEN_REPLAY on the host: the option's number in all four interfaces, the counter's entry point declared,
exported and bound, and the per-pixel record of the size DESIGN.md states."""
import ctypes
import os
import re

from madarch_amd import _binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_option_number_in_every_interface():
    header = text("include", "madarch_hip.h")
    assert int(re.search(r"MDH_OPT_SCREEN_REPLAY\s*=\s*(\d+)", header).group(1)) == 22
    assert B.OPT_SCREEN_REPLAY == 22
    assert re.search(r"Opt_Screen_Replay\s*=\s*MDH_OPT_SCREEN_REPLAY\s*;", text("include", "madarch.hpp"))
    assert int(re.search(r"Opt_Screen_Replay\s*:\s*constant int\s*:=\s*(\d+)\s*;", text("ada", "madarch_hip.ads")).group(1)) == 22


def test_stats_entry_point_declared_exported_bound():
    header = text("include", "madarch_hip.h")
    assert re.search(r"int32_t\s+mdh_screen_replay_stats\s*\(\s*mdh_renderer\s*\*r,\s*int64_t\s*\*plain,\s*int64_t\s*\*recording,\s*int64_t\s*\*replaying\s*\)\s*;", header)
    assert "screen_replay_stats" in B.HIP_ONLY_ABI
    lib = ctypes.CDLL(B.HIP_LIBRARY)
    assert lib.mdh_screen_replay_stats is not None
    from madarch_amd import renderers
    assert callable(renderers.Renderer.Screen_Replay_Stats)


def test_record_size():
    """32 bytes per pixel: DESIGN.md's figure, the source's static_assert and the built library's own answer."""
    design = text("DESIGN.md")
    assert re.search(r"PixelRecord[^.]*\b32 bytes", design)
    march = text("madarch_amd", "csrc", "mdh_march.h")
    assert re.search(r"static_assert\(sizeof\(PixelRecord\) == 32", march)
    lib = ctypes.CDLL(B.HIP_LIBRARY)
    lib.mdh_screen_record_bytes.restype = ctypes.c_int32
    assert lib.mdh_screen_record_bytes() == 32
