"""mdh_shade_rays, mdh_shade_rays_device, mdh_camera_rays and mdh_camera_rays_device without a device: the four entry
points in all four interfaces, the Python argument checks, the predicate that stands in for a stall guard at its edge
values (tests/shade_rays_check.cpp under the address and undefined-behaviour sanitizers), and the float64 side of the
device test's free rays: few enough of them are fragile that the device test cannot hide behind the cap."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = (("shade_rays", "Shade_Rays"), ("shade_rays_device", "Shade_Rays_Device"), ("camera_rays", "Camera_Rays"),
                ("camera_rays_device", "Camera_Rays_Device"))


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_entry_points_in_every_interface():
    from madarch_amd import _binding as B
    from madarch_amd import renderers
    header, hpp, ads = text("include", "madarch_hip.h"), text("include", "madarch.hpp"), text("ada", "madarch_hip.ads")
    for fn, method in ENTRY_POINTS:
        assert re.search(r"int32_t\s+mdh_%s\s*\(\s*mdh_renderer\s*\*" % fn, header), fn
        assert fn in B.HIP_ONLY_ABI and fn not in B.ABI
        assert callable(getattr(renderers.Renderer, method))
        assert re.search(r"\bmdh_%s\s*\(" % fn, hpp) and re.search(r"\b%s\s*\(" % method, hpp), fn
        assert re.search(r'External_Name\s*=>\s*"mdh_%s"' % fn, ads), fn
    # the device variants end in the stream; the shading calls take mode and tone_map between the rays and the colours
    for fn in ("shade_rays_device", "camera_rays_device"):
        assert re.search(r"mdh_%s\s*\([^;]*void\s*\*\s*stream\s*\)\s*;" % fn, header), fn
        assert B.HIP_ONLY_ABI[fn][1][-1] is B._P
    for fn in ("shade_rays", "shade_rays_device"):
        assert re.search(r"mdh_%s\s*\([^;]*dir_xyz\s*,\s*int32_t\s+mode\s*,\s*int32_t\s+tone_map\s*,\s*float\s*\*\s*rgb_out" % fn, header), fn
        assert B.HIP_ONLY_ABI[fn][1][4:6] == [B._I, B._I]
    assert len(B.HIP_ONLY_ABI["shade_rays"][1]) == 11 and len(B.HIP_ONLY_ABI["shade_rays_device"][1]) == 12
    assert len(B.HIP_ONLY_ABI["camera_rays"][1]) == 5 and len(B.HIP_ONLY_ABI["camera_rays_device"][1]) == 6
    # the header says that no fog is composed
    assert re.search(r"NO VOLUMETRICS", header)


def test_the_library_exports_them_and_refuses_a_null_renderer():
    from madarch_amd import _binding as B
    b = B.hip_binding()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    assert b.shade_rays(None, 1, p, p, 0, 0, p, None, None, None, None) == B.MDH_E_INVALID
    assert b.shade_rays_device(None, 1, p, p, 0, 0, p, None, None, None, None, None) == B.MDH_E_INVALID
    assert b.camera_rays(None, 1, 1, p, p) == B.MDH_E_INVALID
    assert b.camera_rays_device(None, 1, 1, p, p, None) == B.MDH_E_INVALID


def test_madarch_amd_still_imports_no_torch():
    code = "import sys; import madarch_amd; from madarch_amd import renderers, _binding; assert 'torch' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT)


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
    host = np.zeros((n, 3), np.float32)
    bad = [
        ("non-contiguous origins", lambda: R.Shade_Rays_Device(Fake(3 * n, contiguous=False), f3, f3)),
        ("float64 directions", lambda: R.Shade_Rays_Device(f3, Fake(3 * n, "torch.float64"), f3)),
        ("int32 colours", lambda: R.Shade_Rays_Device(f3, f3, Fake(3 * n, "torch.int32"))),
        ("float32 hits", lambda: R.Shade_Rays_Device(f3, f3, f3, Hit=f1)),
        ("int32 t", lambda: R.Shade_Rays_Device(f3, f3, f3, T=i1)),
        ("short colours", lambda: R.Shade_Rays_Device(f3, f3, Fake(3 * n - 1))),
        ("short directions", lambda: R.Shade_Rays_Device(f3, Fake(3 * n - 1), f3)),
        ("short steps", lambda: R.Shade_Rays_Device(f3, f3, f3, Steps=Fake(n - 1, "torch.int32"))),
        ("host origins", lambda: R.Shade_Rays_Device(Fake(3 * n, cuda=False), f3, f3)),
        ("host colours", lambda: R.Shade_Rays_Device(f3, f3, Fake(3 * n, cuda=False))),
        ("no colours", lambda: R.Shade_Rays_Device(f3, f3, None)),
        ("mode 1", lambda: R.Shade_Rays_Device(f3, f3, f3, Mode=1)),
        ("mode 3", lambda: R.Shade_Rays_Device(f3, f3, f3, Mode=3)),
        ("more rays than the origins hold", lambda: R.Shade_Rays_Device(f3, f3, f3, N=n + 1)),
        ("a negative count", lambda: R.Shade_Rays_Device(f3, f3, f3, N=-1)),
        ("addresses without a count", lambda: R.Shade_Rays_Device(0x1000, 0x2000, 0x3000)),
        ("a numpy array as device memory", lambda: R.Shade_Rays_Device(host, f3, f3)),
        ("host arrays: mode 1", lambda: R.Shade_Rays(host, host, Mode=1)),
        ("host arrays: two shapes", lambda: R.Shade_Rays(host, host[:-1])),
        ("host arrays: not (n, 3)", lambda: R.Shade_Rays(host.reshape(-1), host.reshape(-1))),
        ("a frame without pixels", lambda: R.Camera_Rays(0, 12)),
        ("a frame of negative height", lambda: R.Camera_Rays(20, -1)),
        ("short camera origins", lambda: R.Camera_Rays_Device(20, 12, Fake(3 * 240 - 1), Fake(3 * 240))),
        ("int32 camera directions", lambda: R.Camera_Rays_Device(20, 12, Fake(3 * 240), Fake(3 * 240, "torch.int32"))),
        ("host camera origins", lambda: R.Camera_Rays_Device(20, 12, Fake(3 * 240, cuda=False), Fake(3 * 240))),
        ("non-contiguous camera directions", lambda: R.Camera_Rays_Device(20, 12, Fake(3 * 240), Fake(3 * 240, contiguous=False))),
        ("no camera directions", lambda: R.Camera_Rays_Device(20, 12, Fake(3 * 240), None)),
        ("a device frame without pixels", lambda: R.Camera_Rays_Device(0, 0, Fake(0), Fake(0))),
    ]
    for what, call in bad:
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")


def test_predicate_at_its_edge_values(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "shade_rays_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "madarch_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "shade_rays_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shade_rays_check: ok" in out.stdout


def test_the_kernel_and_the_host_call_the_checked_predicate():
    """what the CPU checks is what the device runs: the lanes and the host-array call apply rs_shade_ray_valid, the call
    applies the scene's half, and the header still brings no HIP runtime with it"""
    header = text("madarch_amd", "csrc", "mdh_ray_stream.h")
    assert not re.search(r"#\s*include", header)
    kernels, api = text("madarch_amd", "csrc", "mdh_kernels.h"), text("madarch_amd", "csrc", "mdh_api.hip")
    assert re.search(r"\brs_shade_ray_valid\s*\(", header) and re.search(r"\brs_shade_extent_valid\s*\(", header)
    assert re.search(r"\brs_shade_ray_valid\s*\(", kernels) and re.search(r"\brs_shade_ray_valid\s*\(", api)
    assert re.search(r"\brs_shade_extent_valid\s*\(", api)
    # the kernel is k_ray_shade, in the seven general variants and both modes, named last
    body = api[api.index("static const void *kernel_ptr(const PassKernel &k)\n{"):]
    assert re.search(r"MDH_SH\(0\) MDH_SH\(1\) MDH_SH\(9\) MDH_SH\(64\) MDH_SH\(65\) MDH_SH\(73\) MDH_SH\(192\)", body)
    assert body.index("MDH_SH(0)") > body.index("MDH_RS(192)")
    assert "k_ray_shade<PF, 0>" in api and "k_ray_shade<PF, 2>" in api


@pytest.mark.parametrize("name,mode", [("room", 0), ("room", 2), ("open", 0), ("open", 2)])
def test_free_rays_are_not_fragile_in_float64(name, mode):
    """the rays of tests/test_gpu_shade_rays.py's float64 test stay within FRAGILE_CAP by the float64 runs alone"""
    import ref64
    import shade_rays_cases as S
    runs = S.free_runs(name, mode)
    assert len(runs) == 3 and runs[0]["colour"].shape == (S.N_FREE, 3)
    share = float(ref64.fragile(runs, colour=True).mean())
    print("%s mode %d: fragile share %.4f" % (name, mode, share))
    assert share <= ref64.FRAGILE_CAP
    # the rays mean something: the room's all hit, some of the open scene's leave it
    hit = runs[0]["hit"]
    assert hit.all() if name == "room" else (0.0 < hit.mean() < 1.0)
