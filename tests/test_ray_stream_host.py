"""The device-array ray queries (mdh_raycast_device, mdh_raycast_visibility_device, mdh_softshadows_device,
mdh_ray_query_wait) without a device.  tests/ray_stream_check.cpp drives the hand-out of madarch_amd/csrc/mdh_ray_stream.h
-- 1, 4 and 16 wavefronts over one counter, scripted ray lengths, every refill threshold and batch size around the
wavefront -- and the ray-validity predicate at its edge values, under the address and undefined-behaviour sanitizers.
Beside it: the two options and the four entry points in all four interfaces, and the Python argument checks."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_hand_out_and_predicate_against_scripted_rays(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "ray_stream_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "madarch_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "ray_stream_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ray_stream_check: ok" in out.stdout


def test_the_kernels_include_the_checked_header():
    """what the CPU checks is what the device runs: mdh_kernels.h includes the header and calls its functions, the host's
    check of host arrays calls the same predicate, and the header brings no HIP runtime with it"""
    header = text("madarch_amd", "csrc", "mdh_ray_stream.h")
    assert not re.search(r"#\s*include", header)
    kernels = text("madarch_amd", "csrc", "mdh_kernels.h")
    assert '#include "mdh_ray_stream.h"' in kernels
    for fn in ("rs_refills", "rs_ray_of", "rs_drained", "rs_ray_valid", "rs_tmax_valid"):
        assert re.search(r"\b%s\s*\(" % fn, header) and re.search(r"\b%s\s*\(" % fn, kernels), fn
    api = text("madarch_amd", "csrc", "mdh_api.hip")
    assert "rs_finite(" in api and "rs_tmax_valid(" in api


def test_options_and_entry_points_in_every_interface():
    from madarch_amd import _binding as B
    from madarch_amd import renderers
    header, hpp, ads = text("include", "madarch_hip.h"), text("include", "madarch.hpp"), text("ada", "madarch_hip.ads")
    for name, number in (("RAY_STREAM_REFILL", 24), ("RAY_STREAM_GROUPS", 25)):
        assert int(re.search(r"MDH_OPT_%s\s*=\s*(\d+)" % name, header).group(1)) == number
        assert getattr(B, "OPT_" + name) == number
        mixed = "_".join(w.capitalize() for w in name.split("_"))
        assert re.search(r"Opt_%s\s*=\s*MDH_OPT_%s\s*;" % (mixed, name), hpp), mixed
        assert int(re.search(r"Opt_%s\s*:\s*constant int\s*:=\s*(\d+)\s*;" % mixed, ads).group(1)) == number
    for fn, method in (("raycast_device", "Raycast_Device"), ("raycast_visibility_device", "Raycast_Visibility_Device"),
                       ("softshadows_device", "Softshadows_Device"), ("ray_query_wait", "Ray_Query_Wait")):
        assert re.search(r"int32_t\s+mdh_%s\s*\(\s*mdh_renderer\s*\*" % fn, header), fn
        assert fn in B.HIP_ONLY_ABI and fn not in B.ABI
        assert callable(getattr(renderers.Renderer, method))
        assert re.search(r"\bmdh_%s\s*\(" % fn, hpp) and re.search(r"\b%s\s*\(" % method, hpp), fn
        assert re.search(r'External_Name\s*=>\s*"mdh_%s"' % fn, ads), fn
    # the three queries end in the stream
    for fn in ("raycast_device", "raycast_visibility_device", "softshadows_device"):
        assert re.search(r"mdh_%s\s*\([^;]*void\s*\*\s*stream\s*\)\s*;" % fn, header), fn
        assert B.HIP_ONLY_ABI[fn][1][-1] is B._P
    assert 1 <= int(re.search(r"#define MDH_RAY_STREAM_REFILL_DEFAULT (\d+)", text("madarch_amd", "csrc", "mdh_ray_stream.h")).group(1)) <= 64


def test_madarch_amd_does_not_import_torch():
    code = "import sys; import madarch_amd; from madarch_amd import renderers, _binding; assert 'torch' not in sys.modules"
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.check_call([sys.executable, "-c", code], env=env, cwd=ROOT)


class Fake:
    """what Renderer._device_array asks of an array, and nothing of torch"""

    def __init__(self, values, dtype="torch.float32", cuda=True, contiguous=True, address=0x7F0000001000):
        self._values, self.dtype, self.is_cuda, self._contiguous, self._address = values, dtype, cuda, contiguous, address

    def numel(self):
        return self._values

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._address


class NoLibrary:
    """a binding whose every call is an error: the argument checks come before any library call"""

    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def test_python_argument_checks_raise_before_any_library_call():
    from madarch_amd import renderers
    R = renderers.Renderer.__new__(renderers.Renderer)
    R._b, R._h = NoLibrary(), None
    n = 10
    f3, f1, i1 = Fake(3 * n), Fake(n), Fake(n, "torch.int32")
    bad = [
        ("non-contiguous origins", lambda: R.Raycast_Device(Fake(3 * n, contiguous=False), f3, i1)),
        ("float64 directions", lambda: R.Raycast_Device(f3, Fake(3 * n, "torch.float64"), i1)),
        ("float32 hits", lambda: R.Raycast_Device(f3, f3, Fake(n))),
        ("int32 t", lambda: R.Raycast_Device(f3, f3, i1, T=Fake(n, "torch.int32"))),
        ("short hits", lambda: R.Raycast_Device(f3, f3, Fake(n - 1, "torch.int32"))),
        ("short normals", lambda: R.Raycast_Device(f3, f3, i1, Normal=Fake(3 * n - 1))),
        ("short directions", lambda: R.Raycast_Device(f3, Fake(3 * n - 1), i1)),
        ("host origins", lambda: R.Raycast_Device(Fake(3 * n, cuda=False), f3, i1)),
        ("no hits", lambda: R.Raycast_Device(f3, f3, None)),
        ("more rays than the origins hold", lambda: R.Raycast_Device(f3, f3, i1, N=n + 1)),
        ("a negative count", lambda: R.Raycast_Device(f3, f3, i1, N=-1)),
        ("addresses without a count", lambda: R.Raycast_Device(0x1000, 0x2000, 0x3000)),
        ("a list", lambda: R.Raycast_Device([0.0] * 30, f3, i1)),
        ("short lengths", lambda: R.Raycast_Visibility_Device(f3, f3, Fake(n - 1), f1)),
        ("int32 visibility", lambda: R.Raycast_Visibility_Device(f3, f3, f1, i1)),
        ("non-contiguous lengths", lambda: R.Softshadows_Device(f3, f3, 0.0, Fake(n, contiguous=False), 64.0, f1)),
        ("short shadows", lambda: R.Softshadows_Device(f3, f3, 0.0, f1, 64.0, Fake(n - 1))),
        ("float16 shadows", lambda: R.Softshadows_Device(f3, f3, 0.0, f1, 64.0, Fake(n, "torch.float16"))),
    ]
    for what, call in bad:
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")
    # what is accepted: objects that say less about themselves, numpy's spelling of the types, plain addresses with a count
    dev = renderers.Renderer._device_array
    assert dev(Fake(n, "float32"), "x", n, "float32").value == 0x7F0000001000
    assert dev(0x1000, "x", n, "int32").value == 0x1000 and dev(None, "x", n, "int32", True) is None
    assert renderers.Renderer._ray_count(f3, None) == n and renderers.Renderer._ray_count(0x1000, 7) == 7
