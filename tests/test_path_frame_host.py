"""The path-traced frame (mdh_path_frame_begin, .._accumulate, .._read, .._rays, .._info, .._end, mdh_path_pixel_uv) without a
device: the entry points in all four interfaces, the Python argument checks against a binding that must not be called, and a
pixel's screen position as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/path_frame_check.cpp) held bit for bit against the numpy restatement of tests/path_frame_cases.py -- and the same bits
through the library's mdh_path_pixel_uv."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import path_frame_cases as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = (("path_frame_begin", "Path_Frame_Begin"), ("path_frame_accumulate", "Path_Frame_Accumulate"), ("path_frame_read", "Path_Frame_Read"),
                ("path_frame_read_device", "Path_Frame_Read_Device"), ("path_frame_rays", "Path_Frame_Rays"), ("path_frame_rays_device", "Path_Frame_Rays_Device"),
                ("path_frame_info", "Path_Frame_Info"), ("path_frame_end", "Path_Frame_End"), ("path_pixel_uv", "Path_Pixel_Uv"))


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ------------------------------------------------------------------------------------ 1. entry points
def test_entry_points_in_every_interface():
    from madarch_amd import _binding as B
    from madarch_amd import examples, renderers
    header, hpp, ads = text("include", "madarch_hip.h"), text("include", "madarch.hpp"), text("ada", "madarch_hip.ads")
    for fn, method in ENTRY_POINTS:
        assert re.search(r"int32_t\s+mdh_%s\s*\(" % fn, header), fn
        assert fn in B.HIP_ONLY_ABI and fn not in B.ABI
        assert callable(getattr(renderers.Renderer, method))
        assert re.search(r"\bmdh_%s\s*\(" % fn, hpp) and re.search(r"\b%s\s*\(" % method, hpp), fn
        assert re.search(r'External_Name\s*=>\s*"mdh_%s"' % fn, ads), fn
    assert re.search(r"mdh_path_frame_begin\s*\(\s*mdh_renderer\s*\*\s*r\s*,\s*int32_t\s+width\s*,\s*int32_t\s+height\s*,\s*uint32_t\s+seed\s*,\s*int32_t\s+bounces\s*,"
                     r"\s*int32_t\s+jitter\s*\)", header)
    assert B.HIP_ONLY_ABI["path_frame_begin"][1] == [B._P, B._I, B._I, C.c_uint32, B._I, B._I]
    for fn in ("path_frame_read_device", "path_frame_rays_device"):
        assert re.search(r"mdh_%s\s*\([^;]*void\s*\*\s*stream\s*\)\s*;" % fn, header), fn
        assert B.HIP_ONLY_ABI[fn][1][-1] is B._P
    # the jitter takes no renderer
    assert re.search(r"mdh_path_pixel_uv\s*\(\s*int32_t\s+width\s*,", header)
    assert re.search(r"#define\s+MDH_PATH_FRAME_MAX_PIXELS\s+67108864\b", header) and B.PATH_FRAME_MAX_PIXELS == 1 << 26
    # the header says whose business a restart after an edit is, that the camera is captured and that no fog is composed
    at = header.index("#define MDH_PATH_FRAME_MAX_PIXELS")
    comment = header[header.rindex("/*", 0, at):at]
    assert "RESTARTING AFTER AN EDIT IS THE HOST'S BUSINESS" in comment and "CAPTURES THE CAMERA" in comment and "NO VOLUMETRICS" in comment
    assert callable(examples.path_traced_frame) and callable(examples.path_traced_view)
    cpp = text("examples", "path_trace.cpp")
    assert "--jitter" in cpp and "Path_Frame_Begin" in cpp and "Path_Frame_Accumulate" in cpp and "Path_Frame_Read" in cpp
    design = text("DESIGN.md")
    assert "A path-traced frame" in design and "k_path_frame" in design


def test_the_library_exports_them_and_refuses_a_null_renderer():
    from madarch_amd import _binding as B
    b = B.hip_binding()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    n = C.c_int32(-5)
    assert b.path_frame_begin(None, 4, 4, 1, 3, 1) == B.MDH_E_INVALID
    assert b.path_frame_accumulate(None, 1) == B.MDH_E_INVALID
    assert b.path_frame_read(None, 0, p, None, None, C.byref(n)) == B.MDH_E_INVALID and n.value == -5
    assert b.path_frame_read_device(None, 0, p, None, None, None, None) == B.MDH_E_INVALID
    assert b.path_frame_rays(None, 0, p, p) == B.MDH_E_INVALID and b.path_frame_rays_device(None, 0, p, p, None) == B.MDH_E_INVALID
    assert b.path_frame_info(None, None, None, None, None, None) == B.MDH_E_INVALID and b.path_frame_end(None) == B.MDH_E_INVALID
    # the jitter needs no renderer and no device
    bad = [(0, 4, 1, 0), (4, 0, 1, 0), (8193, 8192, 1, 0), (4, 4, -1, 0), (4, 4, 1, -1), (4, 4, 17, 0)]
    for w, h, count, sample in bad:
        assert b.path_pixel_uv(w, h, 1, 0, count, sample, 1, p) == B.MDH_E_INVALID, (w, h, count, sample)
    assert b.path_pixel_uv(4, 4, 1, 14, 3, 0, 1, p) == B.MDH_E_INVALID  # (ids 14 .. 16 of 16 pixels)
    assert b.path_pixel_uv(4, 4, 1, 0, 4, 0, 2, p) == B.MDH_E_INVALID and b.path_pixel_uv(4, 4, 1, 0, 4, 0, 1, None) == B.MDH_E_INVALID
    assert b.path_pixel_uv(4, 4, 1, 0, 0, 0, 1, None) == B.MDH_OK and b.path_pixel_uv(4, 4, 1, 12, 4, 0, 1, p) == B.MDH_OK


def test_madarch_amd_still_imports_no_torch():
    code = "import sys; import madarch_amd; from madarch_amd import renderers, _binding, examples; assert 'torch' not in sys.modules"
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
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def test_python_argument_checks_raise_before_any_library_call():
    from madarch_amd import renderers
    R = renderers.Renderer.__new__(renderers.Renderer)
    R._b, R._h = NoLibrary(), None
    w, h = 5, 4
    n = w * h
    f3, i1 = Fake(3 * n), Fake(n, "torch.int32")
    none = NoLibrary()
    bad = [
        ("no width", lambda: R.Path_Frame_Begin(0, h)),
        ("a negative height", lambda: R.Path_Frame_Begin(w, -1)),
        ("more than 2^26 pixels", lambda: R.Path_Frame_Begin(8193, 8192)),
        ("seven bounces", lambda: R.Path_Frame_Begin(w, h, Bounces=7)),
        ("negative bounces", lambda: R.Path_Frame_Begin(w, h, Bounces=-1)),
        ("a seed of 33 bits", lambda: R.Path_Frame_Begin(w, h, Seed=2 ** 32)),
        ("a negative seed", lambda: R.Path_Frame_Begin(w, h, Seed=-1)),
        ("a jitter of 2", lambda: R.Path_Frame_Begin(w, h, Jitter=2)),
        ("a jitter that is a string", lambda: R.Path_Frame_Begin(w, h, Jitter="yes")),
        ("a negative count", lambda: R.Path_Frame_Accumulate(-1)),
        ("a count of 2^31", lambda: R.Path_Frame_Accumulate(2 ** 31)),
        ("a tone map of 2", lambda: R.Path_Frame_Read(Tone_Map=2)),
        ("a negative sample", lambda: R.Path_Frame_Rays(Sample=-1)),
        ("device read: a tone map of 2", lambda: R.Path_Frame_Read_Device(w, h, f3, Tone_Map=2)),
        ("device read: no width", lambda: R.Path_Frame_Read_Device(0, h, f3)),
        ("device read: short colours", lambda: R.Path_Frame_Read_Device(w, h, Fake(3 * n - 1))),
        ("device read: int32 colours", lambda: R.Path_Frame_Read_Device(w, h, Fake(3 * n, "torch.int32"))),
        ("device read: float32 bytes", lambda: R.Path_Frame_Read_Device(w, h, f3, Rgba8=Fake(n))),
        ("device read: short bytes", lambda: R.Path_Frame_Read_Device(w, h, f3, Rgba8=Fake(n - 1, "torch.int32"))),
        ("device read: host sums", lambda: R.Path_Frame_Read_Device(w, h, f3, i1, Fake(3 * n, cuda=False))),
        ("device read: non-contiguous sums", lambda: R.Path_Frame_Read_Device(w, h, f3, i1, Fake(3 * n, contiguous=False))),
        ("device read: a numpy array", lambda: R.Path_Frame_Read_Device(w, h, np.zeros((n, 3), np.float32))),
        ("device rays: no origins", lambda: R.Path_Frame_Rays_Device(w, h, None, f3)),
        ("device rays: short directions", lambda: R.Path_Frame_Rays_Device(w, h, f3, Fake(3 * n - 3))),
        ("device rays: a negative sample", lambda: R.Path_Frame_Rays_Device(w, h, f3, f3, Sample=-1)),
        ("device rays: int32 origins", lambda: R.Path_Frame_Rays_Device(w, h, Fake(3 * n, "torch.int32"), f3)),
        ("uv: no width", lambda: R.Path_Pixel_Uv(0, h, Binding=none)),
        ("uv: more pixels than the frame has", lambda: R.Path_Pixel_Uv(w, h, Id_First=10, N=11, Binding=none)),
        ("uv: a negative count", lambda: R.Path_Pixel_Uv(w, h, N=-1, Binding=none)),
        ("uv: a negative sample", lambda: R.Path_Pixel_Uv(w, h, Sample=-1, Binding=none)),
        ("uv: a jitter of 3", lambda: R.Path_Pixel_Uv(w, h, Jitter=3, Binding=none)),
        ("uv: a seed of 33 bits", lambda: R.Path_Pixel_Uv(w, h, Seed=2 ** 32, Binding=none)),
    ]
    for what, call in bad:
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")


def test_the_kernels_and_the_host_call_the_checked_functions():
    """what the CPU checks is what the device runs: the kernels and mdh_path_pixel_uv call the header's function, the header keeps
    its single include, the new kernels live in a header of their own outside the hiprtc build and are named behind every older one"""
    header = text("madarch_amd", "csrc", "mdh_path.h")
    assert re.findall(r"#\s*include\s*(\S+)", header) == ['"mdh_ray_stream.h"']
    frame, kernels, api = text("madarch_amd", "csrc", "mdh_path_frame.h"), text("madarch_amd", "csrc", "mdh_kernels.h"), text("madarch_amd", "csrc", "mdh_api.hip")
    assert re.search(r"\bpath_pixel_uv\s*\(", frame) and re.search(r"\bpath_pixel_uv\s*\(", api) and re.search(r"\bpath_frame_size_valid\s*\(", api)
    for fn in ("march_plain<PART>", "sdf_info<PART>", "primitive_info<", "path_direct<PART>", "path_scatter_at(", "path_ray_valid(", "camera_ray("):
        assert fn in frame, fn
    assert "atomic" not in frame.split("#pragma once")[1] and "__shared__" not in frame
    assert kernels.index('#include "mdh_path_frame.h"') > kernels.index('#include "mdh_surface.h"')
    assert kernels.index('#include "mdh_path_frame.h"') < kernels.index("#endif", kernels.index('#include "mdh_surface.h"'))  # (outside the hiprtc build)
    assert "mdh_path_frame.h" not in text("madarch_amd", "csrc", "embed_sources.py")
    body = api[api.index("static const void *kernel_ptr(const PassKernel &k)\n{"):]
    assert body.index("static const void *kernel_ptr_path_frame(const PassKernel &k)\n{") > body.index("static const void *kernel_ptr_surface(const PassKernel &k)\n{")
    assert re.search(r"MDH_PFR\(0\) MDH_PFR\(1\) MDH_PFR\(9\) MDH_PFR\(64\) MDH_PFR\(65\) MDH_PFR\(73\) MDH_PFR\(192\)", body)
    assert "k_path_frame<PF, true>" in api and "k_path_frame<PF, false>" in api and "k_path_frame_rays<>" in api and "k_path_frame_resolve<>" in api


# ------------------------------------------------------------------------------------ 2. the stand-alone program
@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("path_frame") / "path_frame_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "madarch_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "path_frame_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "path_frame_check: ok" in out.stdout
    lines = out.stdout.splitlines()
    return {k: [ln.split()[1:] for ln in lines if ln.startswith(k + " ")] for k in "PM"}


def rows_of(check_output):
    rows = check_output["P"]
    args = np.array([[int(x) for x in r[:7]] for r in rows], dtype=np.int64)  # width height seed sample jitter i j
    got = np.array([[int(r[7], 16), int(r[8], 16)] for r in rows], dtype=np.uint32).view(np.float32)
    return args, got


def test_positions_bit_for_bit(check_output):
    args, got = rows_of(check_output)
    assert len(args) == 2 * 3 * 2 * (1 + 6 + 240 + 4)
    sizes = {(int(w), int(h)) for w, h in args[:, :2]}
    assert sizes == {(1, 1), (3, 2), (20, 12), (1920, 1080)}
    corners = args[args[:, 0] == 1920][:, 5:7]
    assert {tuple(c) for c in corners.tolist()} == {(0, 0), (1919, 0), (0, 1079), (1919, 1079)}
    seen = 0
    for key in {tuple(k) for k in args[:, :5].tolist()}:
        w, h, seed, sample, jitter = key
        at = (args[:, :5] == np.array(key)).all(axis=1)
        i, j = args[at, 5], args[at, 6]
        u, v = PF.pixel_uv(w, h, seed, sample, bool(jitter), i, j)
        want = np.stack([u, v], axis=1)
        assert np.array_equal(want.view(np.uint32), got[at].view(np.uint32)), key
        cu = ((2 * i + 1).astype(np.float32) / np.float32(w)).astype(np.float32) - np.float32(1.0)
        cv = -(((2 * j + 1).astype(np.float32) / np.float32(h)).astype(np.float32) - np.float32(1.0))
        if not jitter:
            assert np.array_equal(got[at][:, 0].view(np.uint32), cu.view(np.uint32)) and np.array_equal(got[at][:, 1].view(np.uint32), cv.view(np.uint32)), key
        else:
            assert (np.abs(got[at][:, 0].astype(np.float64) - cu) <= 1.0 / w).all() and (np.abs(got[at][:, 1].astype(np.float64) - cv) <= 1.0 / h).all(), key
            if w * h > 1 and len(i) > 4:
                assert (got[at][:, 0] != cu).mean() > 0.95  # (the jitter does move them)
        seen += int(at.sum())
    assert seen == len(args)


def test_mean_offset_of_one_pixel(check_output):
    (mx, my), = check_output["M"]
    bound = 6.0 / np.sqrt(3.0 * 4096)
    print("mean offsets %s %s of the half-width, bound %.4f" % (mx, my, bound))
    assert abs(float(mx)) <= bound and abs(float(my)) <= bound
    # the same 4 096 samples in numpy
    s = np.arange(4096)
    u, v = PF.pixel_uv(20, 12, PF.SEED, s, True, np.full(4096, 7), np.full(4096, 5))
    cu, cv = (2.0 * 7 + 1.0) / 20 - 1.0, -((2.0 * 5 + 1.0) / 12 - 1.0)
    assert abs(((u.astype(np.float64) - cu) * 20).mean() - float(mx)) < 1e-6 and abs(((v.astype(np.float64) - cv) * 12).mean() - float(my)) < 1e-6


def test_the_library_gives_the_same_bits(check_output):
    from madarch_amd import renderers
    args, got = rows_of(check_output)
    for key in {tuple(k) for k in args[:, :5].tolist()}:
        w, h, seed, sample, jitter = key
        at = (args[:, :5] == np.array(key)).all(axis=1)
        uv = renderers.Renderer.Path_Pixel_Uv(w, h, Seed=seed, Sample=sample, Jitter=bool(jitter))
        assert uv.shape == (w * h, 2)
        ids = args[at, 6] * w + args[at, 5]
        assert np.array_equal(uv[ids].view(np.uint32), got[at].view(np.uint32)), key
        # a slice of the ids is the slice of the whole
        part = renderers.Renderer.Path_Pixel_Uv(w, h, Seed=seed, Id_First=w * h // 2, N=w * h - w * h // 2, Sample=sample, Jitter=bool(jitter))
        assert np.array_equal(part.view(np.uint32), uv[w * h // 2:].view(np.uint32)), key
    # the whole 20 x 12 frame against numpy, a sample the program did not print
    uv = renderers.Renderer.Path_Pixel_Uv(20, 12, Seed=77, Sample=123456, Jitter=True)
    u, v = PF.pixel_uv(20, 12, 77, 123456, True)
    assert np.array_equal(uv.view(np.uint32), np.stack([u, v], axis=1).view(np.uint32))
