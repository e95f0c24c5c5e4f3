"""mdh_shade_points, mdh_shade_points_device and mdh_primitive_material without a device: the three entry points in all
four interfaces, the Python argument checks, the predicate that stands in for a stall guard at its edge values
(tests/shade_points_check.cpp under the address and undefined-behaviour sanitizers), and the float64 side of the device
test's free points: few enough of them are fragile that the device test cannot hide behind the cap."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = (("shade_points", "Shade_Points"), ("shade_points_device", "Shade_Points_Device"), ("primitive_material", "Primitive_Material"))


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
    # the device variant ends in the stream; both take mode and tone_map between the material ids and the colours
    assert re.search(r"mdh_shade_points_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", header)
    assert B.HIP_ONLY_ABI["shade_points_device"][1][-1] is B._P
    for fn in ("shade_points", "shade_points_device"):
        assert re.search(r"mdh_%s\s*\([^;]*pos_xyz\s*,\s*const\s+float\s*\*\s*normal_xyz\s*,\s*const\s+float\s*\*\s*view_dir_xyz\s*,\s*const\s+int32_t\s*\*\s*material_ids\s*,"
                         r"\s*int32_t\s+mode\s*,\s*int32_t\s+tone_map\s*,\s*float\s*\*\s*rgb_out" % fn, header), fn
        assert B.HIP_ONLY_ABI[fn][1][6:8] == [B._I, B._I]
    assert len(B.HIP_ONLY_ABI["shade_points"][1]) == 9 and len(B.HIP_ONLY_ABI["shade_points_device"][1]) == 10
    assert len(B.HIP_ONLY_ABI["primitive_material"][1]) == 4
    assert re.search(r"#define\s+MDH_POINT_IRRADIANCE\s+3\b", header) and renderers.Renderer.POINT_IRRADIANCE == 3
    # the header says that no fog is composed and that the direction bound is tighter than a ray's
    assert re.search(r"NO VOLUMETRICS", header[header.index("What light arrives"):])
    assert re.search(r"TIGHTER", header)


def test_the_library_exports_them_and_refuses_a_null_renderer():
    from madarch_amd import _binding as B
    b = B.hip_binding()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    for mode in (0, 2, 3):
        assert b.shade_points(None, 1, p, p, p, p, mode, 0, p) == B.MDH_E_INVALID
        assert b.shade_points_device(None, 1, p, p, p, p, mode, 0, p, None) == B.MDH_E_INVALID
    assert b.primitive_material(None, 1, p, p) == B.MDH_E_INVALID


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
    f3, i1 = Fake(3 * n), Fake(n, "torch.int32")
    host = np.zeros((n, 3), np.float32)
    ids = np.zeros(n, np.int32)
    bad = [
        ("non-contiguous positions", lambda: R.Shade_Points_Device(Fake(3 * n, contiguous=False), f3, f3, i1, f3)),
        ("float64 normals", lambda: R.Shade_Points_Device(f3, Fake(3 * n, "torch.float64"), f3, i1, f3)),
        ("float32 material ids", lambda: R.Shade_Points_Device(f3, f3, f3, Fake(n), f3)),
        ("int32 colours", lambda: R.Shade_Points_Device(f3, f3, f3, i1, Fake(3 * n, "torch.int32"))),
        ("short colours", lambda: R.Shade_Points_Device(f3, f3, f3, i1, Fake(3 * n - 1))),
        ("short view directions", lambda: R.Shade_Points_Device(f3, f3, Fake(3 * n - 1), i1, f3)),
        ("short material ids", lambda: R.Shade_Points_Device(f3, f3, f3, Fake(n - 1, "torch.int32"), f3)),
        ("host positions", lambda: R.Shade_Points_Device(Fake(3 * n, cuda=False), f3, f3, i1, f3)),
        ("no colours", lambda: R.Shade_Points_Device(f3, f3, f3, i1, None)),
        ("mode 0 without view directions", lambda: R.Shade_Points_Device(f3, f3, None, i1, f3)),
        ("mode 2 without material ids", lambda: R.Shade_Points_Device(f3, f3, f3, None, f3, Mode=2)),
        ("mode 1", lambda: R.Shade_Points_Device(f3, f3, f3, i1, f3, Mode=1)),
        ("mode 4", lambda: R.Shade_Points_Device(f3, f3, f3, i1, f3, Mode=4)),
        ("mode 3 tone-mapped", lambda: R.Shade_Points_Device(f3, f3, None, None, f3, Mode=3, Tone_Map=True)),
        ("more points than the positions hold", lambda: R.Shade_Points_Device(f3, f3, f3, i1, f3, N=n + 1)),
        ("a negative count", lambda: R.Shade_Points_Device(f3, f3, f3, i1, f3, N=-1)),
        ("addresses without a count", lambda: R.Shade_Points_Device(0x1000, 0x2000, 0x3000, 0x4000, 0x5000)),
        ("a numpy array as device memory", lambda: R.Shade_Points_Device(host, f3, f3, i1, f3)),
        ("host arrays: mode 1", lambda: R.Shade_Points(host, host, host, ids, Mode=1)),
        ("host arrays: mode 3 tone-mapped", lambda: R.Shade_Points(host, host, Mode=3, Tone_Map=True)),
        ("host arrays: two shapes", lambda: R.Shade_Points(host, host[:-1], host, ids)),
        ("host arrays: not (n, 3)", lambda: R.Shade_Points(host.reshape(-1), host.reshape(-1), host, ids)),
        ("host arrays: mode 0 without view directions", lambda: R.Shade_Points(host, host, None, ids)),
        ("host arrays: mode 2 without material ids", lambda: R.Shade_Points(host, host, host, None, Mode=2)),
        ("host arrays: short material ids", lambda: R.Shade_Points(host, host, host, ids[:-1])),
        ("host arrays: short view directions", lambda: R.Shade_Points(host, host, host[:-1], ids)),
    ]
    for what, call in bad:
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")


def test_predicate_at_its_edge_values(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "shade_points_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "madarch_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "shade_points_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "shade_points_check: ok" in out.stdout


def test_the_kernel_and_the_host_call_the_checked_predicate():
    """what the CPU checks is what the device runs: the lanes and the host-array call apply rs_shade_point_valid, the call
    keeps the scene's half, and the header still brings no HIP runtime with it"""
    header = text("madarch_amd", "csrc", "mdh_ray_stream.h")
    assert not re.search(r"#\s*include", header)
    kernels, api, march = text("madarch_amd", "csrc", "mdh_kernels.h"), text("madarch_amd", "csrc", "mdh_api.hip"), text("madarch_amd", "csrc", "mdh_march.h")
    assert re.search(r"\brs_shade_point_valid\s*\(", header)
    assert re.search(r"\brs_shade_point_valid\s*\(", kernels) and re.search(r"\brs_shade_point_valid\s*\(", api)
    points = api[api.index("static int shade_points_check("):api.index('extern "C" int32_t mdh_primitive_material')]
    assert "shade_scene_check(r)" in points and points.count("ray_arrays_check(") == 1 and "settle_bump" not in points
    # the kernel is k_point_shade, in the seven general variants and three modes, named last: nothing older moves
    body = api[api.index("static const void *kernel_ptr(const PassKernel &k)\n{"):]
    assert re.search(r"MDH_PT\(0\) MDH_PT\(1\) MDH_PT\(9\) MDH_PT\(64\) MDH_PT\(65\) MDH_PT\(73\) MDH_PT\(192\)\s*return nullptr;", body)
    assert body.index("MDH_PT(0)") > body.index("MDH_SH(192)") and body.index("MDH_PT(0)") > body.index("k_camera_rays<>")
    for mode in (0, 2, 3):
        assert "k_point_shade<PF, %d>" % mode in api
    assert "GK_k_point_shade" in api
    # the entry into the pixel program is a template parameter whose default leaves every other instantiation alone
    assert re.search(r"bool NULLB = true, bool POINT = false>\s*MDH_DEV f3 shade_structured", march)


@pytest.mark.parametrize("name,mode", [("room", 0), ("room", 2), ("open", 0), ("open", 2)])
def test_free_points_are_not_fragile_in_float64(name, mode):
    """the points of tests/test_gpu_shade_points.py's float64 test stay within FRAGILE_CAP by the float64 runs alone, and
    enough of them see direct light for mode 2 to test anything"""
    import ref64
    import shade_points_cases as P
    runs = P.free_runs(name, mode)
    assert len(runs) == 3 and runs[0]["colour"].shape == (P.N_FREE, 3)
    bad = P.fragile(runs)
    lit = int((runs[0]["direct"].max(axis=1) > 1e-3).sum())
    print("%s mode %d: %d of %d fragile, %d fragile for their irradiance alone, %d see direct light" % (
        name, mode, int(bad.sum()), P.N_FREE, int(P.fragile(runs, "irradiance").sum()), lit))
    assert float(bad.mean()) <= ref64.FRAGILE_CAP
    assert float(P.fragile(runs, "irradiance").mean()) <= ref64.FRAGILE_CAP
    assert 4 * lit >= P.N_FREE
    assert np.isfinite(runs[0]["colour"]).all()
