"""The adaptive path-traced frame (mdh_path_frame_begin_adaptive, mdh_path_frame_stats, mdh_path_frame_stats_device, mdh_path_pixel_active)
without a device: the entry points in all four interfaces, a null renderer, the Python argument checks against a binding that
must not be called, the stopping rule through the library against the numpy restatement of tests/path_adaptive_cases.py, and
the same rule as a stand-alone program under the address and undefined-behaviour sanitizers (tests/path_adaptive_check.cpp)
whose printed bits both are held against."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import path_adaptive_cases as PA
from test_path_frame_host import Fake, NoLibrary, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = (("path_frame_begin_adaptive", "Path_Frame_Begin_Adaptive"), ("path_frame_stats", "Path_Frame_Stats"), ("path_frame_stats_device", "Path_Frame_Stats_Device"),
                ("path_pixel_active", "Path_Pixel_Active"))


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
    assert re.search(r"mdh_path_frame_begin_adaptive\s*\(\s*mdh_renderer\s*\*\s*r\s*,\s*int32_t\s+width\s*,\s*int32_t\s+height\s*,\s*uint32_t\s+seed\s*,\s*int32_t\s+bounces\s*,"
                     r"\s*int32_t\s+jitter\s*,\s*int32_t\s+min_samples\s*,\s*int32_t\s+max_samples\s*,\s*float\s+tolerance\s*,\s*float\s+floor\s*\)", header)
    assert B.HIP_ONLY_ABI["path_frame_begin_adaptive"][1] == [B._P, B._I, B._I, C.c_uint32, B._I, B._I, B._I, B._I, B._F, B._F]
    assert re.search(r"mdh_path_frame_stats_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", header) and B.HIP_ONLY_ABI["path_frame_stats_device"][1][-1] is B._P
    assert re.search(r"mdh_path_pixel_active\s*\(\s*int32_t\s+n_pixels\s*,", header)  # (the rule takes no renderer)
    # the option, in every interface, beside the ray stream's in the switch of the options that end no settle run
    assert re.search(r"MDH_OPT_PATH_FRAME_COMPACT\s*=\s*26\b", header) and B.OPT_PATH_FRAME_COMPACT == 26
    assert "MDH_OPT_PATH_FRAME_COMPACT" in hpp and re.search(r"Opt_Path_Frame_Compact\s*:\s*constant\s+int\s*:=\s*26", ads)
    api = text("madarch_amd", "csrc", "mdh_api.hip")
    assert re.search(r"case MDH_OPT_RAY_STREAM_REFILL:[^\n]*case MDH_OPT_PATH_FRAME_COMPACT:\s*break;", api)
    # the header says that the rule is evaluated at round boundaries only and what is not claimed
    at = header.index("int32_t mdh_path_frame_begin_adaptive")
    comment = header[header.rindex("/*", 0, at):at]
    assert "TWO ROUNDS OF 2 ARE NOT ONE ROUND OF 4" in comment and "BIASED VARIANCE ESTIMATE" in comment and "SAMPLE INDEX k" in comment
    assert "BIASED VARIANCE ESTIMATE" in text("madarch_amd", "csrc", "mdh_path.h")
    design = text("DESIGN.md")
    assert "An adaptive path-traced frame" in design and "k_path_frame_adaptive" in design and "biased variance estimate" in design
    assert "Adaptive" in examples.path_traced_frame.__code__.co_varnames
    cpp = text("examples", "path_trace.cpp")
    assert "--adaptive" in cpp and "Path_Frame_Begin_Adaptive" in cpp and "Path_Frame_Stats" in cpp


def test_the_library_exports_them_and_refuses_a_null_renderer():
    from madarch_amd import _binding as B
    b = B.hip_binding()
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    assert b.path_frame_begin_adaptive(None, 4, 4, 1, 3, 1, 2, 8, 0.1, 0.01) == B.MDH_E_INVALID
    assert b.path_frame_stats(None, p, None, None, None) == B.MDH_E_INVALID and b.path_frame_stats_device(None, p, None, None, None, None) == B.MDH_E_INVALID
    assert all(v == 0.0 for v in buf)
    # the rule needs no renderer and no device
    count = np.array([1, 2, 3], np.int32)
    m = np.array([1.0, 2.0, 3.0], np.float32)
    out = np.full(4, 9, np.uint8)
    fp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    bad = [(0, 4, 0.1, 0.01), (5, 4, 0.1, 0.01), (1, (1 << 24) + 1, 0.1, 0.01), (1, 4, -0.1, 0.01), (1, 4, 0.1, -0.01), (1, 4, float("nan"), 0.01), (1, 4, 0.1, float("inf"))]
    for lo, hi, tol, floor in bad:
        assert b.path_pixel_active(3, fp(count), fp(m), fp(m), lo, hi, tol, floor, fp(out)) == B.MDH_E_INVALID, (lo, hi, tol, floor)
    assert b.path_pixel_active(-1, fp(count), fp(m), fp(m), 1, 4, 0.1, 0.01, fp(out)) == B.MDH_E_INVALID
    for hole in range(4):
        args = [fp(count), fp(m), fp(m), fp(out)]
        args[hole] = None
        assert b.path_pixel_active(3, args[0], args[1], args[2], 1, 4, 0.1, 0.01, args[3]) == B.MDH_E_INVALID, hole
    assert (out == 9).all()
    assert b.path_pixel_active(0, None, None, None, 1, 4, 0.1, 0.01, None) == B.MDH_OK
    assert b.path_pixel_active(3, fp(count), fp(m), fp(m), 1, 1 << 24, 0.0, 0.0, fp(out)) == B.MDH_OK and out[3] == 9 and set(out[:3]) <= {0, 1}


def test_python_argument_checks_raise_before_any_library_call():
    from madarch_amd import renderers
    R = renderers.Renderer.__new__(renderers.Renderer)
    R._b, R._h = NoLibrary(), None
    w, h = 5, 4
    n = w * h
    none = NoLibrary()
    ok = np.ones(3, np.float32)
    bad = [
        ("no width", lambda: R.Path_Frame_Begin_Adaptive(0, h)),
        ("more than 2^26 pixels", lambda: R.Path_Frame_Begin_Adaptive(8193, 8192)),
        ("seven bounces", lambda: R.Path_Frame_Begin_Adaptive(w, h, Bounces=7)),
        ("a jitter of 2", lambda: R.Path_Frame_Begin_Adaptive(w, h, Jitter=2)),
        ("a seed of 33 bits", lambda: R.Path_Frame_Begin_Adaptive(w, h, Seed=2 ** 32)),
        ("no minimum", lambda: R.Path_Frame_Begin_Adaptive(w, h, Min_Samples=0)),
        ("a minimum above the maximum", lambda: R.Path_Frame_Begin_Adaptive(w, h, Min_Samples=9, Max_Samples=8)),
        ("a maximum above 2^24", lambda: R.Path_Frame_Begin_Adaptive(w, h, Max_Samples=2 ** 24 + 1)),
        ("a negative tolerance", lambda: R.Path_Frame_Begin_Adaptive(w, h, Tolerance=-0.1)),
        ("a NaN tolerance", lambda: R.Path_Frame_Begin_Adaptive(w, h, Tolerance=float("nan"))),
        ("a tolerance beyond float32", lambda: R.Path_Frame_Begin_Adaptive(w, h, Tolerance=1e39)),
        ("a negative floor", lambda: R.Path_Frame_Begin_Adaptive(w, h, Floor=-1.0)),
        ("an infinite floor", lambda: R.Path_Frame_Begin_Adaptive(w, h, Floor=float("inf"))),
        ("device stats: no width", lambda: R.Path_Frame_Stats_Device(0, h, Fake(n, "torch.int32"))),
        ("device stats: float32 counts", lambda: R.Path_Frame_Stats_Device(w, h, Fake(n))),
        ("device stats: short counts", lambda: R.Path_Frame_Stats_Device(w, h, Fake(n - 1, "torch.int32"))),
        ("device stats: short moments", lambda: R.Path_Frame_Stats_Device(w, h, None, Fake(2 * n - 1))),
        ("device stats: int32 moments", lambda: R.Path_Frame_Stats_Device(w, h, None, Fake(2 * n, "torch.int32"))),
        ("device stats: an int32 active word", lambda: R.Path_Frame_Stats_Device(w, h, None, None, Fake(1, "torch.int32"))),
        ("device stats: an empty total", lambda: R.Path_Frame_Stats_Device(w, h, None, None, None, Fake(0, "torch.int64"))),
        ("device stats: host counts", lambda: R.Path_Frame_Stats_Device(w, h, Fake(n, "torch.int32", cuda=False))),
        ("device stats: non-contiguous moments", lambda: R.Path_Frame_Stats_Device(w, h, None, Fake(2 * n, contiguous=False))),
        ("device stats: a numpy array", lambda: R.Path_Frame_Stats_Device(w, h, np.zeros(n, np.int32))),
        ("rule: no minimum", lambda: R.Path_Pixel_Active([1, 2, 3], ok, ok, 0, 4, 0.1, 0.01, Binding=none)),
        ("rule: a minimum above the maximum", lambda: R.Path_Pixel_Active([1, 2, 3], ok, ok, 5, 4, 0.1, 0.01, Binding=none)),
        ("rule: a negative tolerance", lambda: R.Path_Pixel_Active([1, 2, 3], ok, ok, 1, 4, -0.1, 0.01, Binding=none)),
        ("rule: a NaN floor", lambda: R.Path_Pixel_Active([1, 2, 3], ok, ok, 1, 4, 0.1, float("nan"), Binding=none)),
        ("rule: moments of another length", lambda: R.Path_Pixel_Active([1, 2, 3], ok[:2], ok, 1, 4, 0.1, 0.01, Binding=none)),
        ("rule: two-dimensional counts", lambda: R.Path_Pixel_Active([[1, 2, 3]], ok, ok, 1, 4, 0.1, 0.01, Binding=none)),
    ]
    for what, call in bad:
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")


def test_the_kernel_and_the_host_call_the_one_rule():
    """what the CPU checks is what the device runs: the kernels and mdh_path_pixel_active call the header's one inline function, the
    update is the header's too, the new kernels live in a header of their own outside the hiprtc build, are named behind every
    older kernel, and hold no atomic"""
    header = text("madarch_amd", "csrc", "mdh_path.h")
    assert re.findall(r"#\s*include\s*(\S+)", header) == ['"mdh_ray_stream.h"']
    assert len(re.findall(r"MDH_PATH_FN\s+bool\s+path_pixel_active\s*\(", header)) == 1
    adaptive, kernels, api = text("madarch_amd", "csrc", "mdh_path_frame_adaptive.h"), text("madarch_amd", "csrc", "mdh_kernels.h"), text("madarch_amd", "csrc", "mdh_api.hip")
    code = adaptive.split("#pragma once")[1]
    assert re.search(r"\bpath_pixel_active\s*\(", code) and re.search(r"\bpath_pixel_update\s*\(", code)
    assert re.search(r"\bpath_pixel_active\s*\(", api) and re.search(r"\bpath_adaptive_valid\s*\(", api)
    for fn in ("path_frame_ray(", "march_plain<PART>", "sdf_info<PART>", "primitive_info<", "path_direct<PART>", "path_scatter_at(", "path_ray_valid(", "path_dir_finite("):
        assert fn in code, fn
    assert "atomic" not in code
    # the empty workgroup's exit stands before the barrier
    body = code[code.index("void k_path_frame_adaptive("):]
    assert body.index(">= listed) return;") < body.index("stage_table(sc);")
    assert kernels.index('#include "mdh_path_frame_adaptive.h"') > kernels.index('#include "mdh_path_frame.h"')
    assert kernels.index('#include "mdh_path_frame_adaptive.h"') < kernels.index("#endif", kernels.index('#include "mdh_surface.h"'))  # (outside the hiprtc build)
    assert "mdh_path_frame_adaptive.h" not in text("madarch_amd", "csrc", "embed_sources.py")
    table = api[api.index("static const void *kernel_ptr(const PassKernel &k)\n{"):]
    assert table.index("static const void *kernel_ptr_path_adaptive(const PassKernel &k)\n{") > table.index("static const void *kernel_ptr_path_frame(const PassKernel &k)\n{")
    assert re.search(r"MDH_PFA\(0\) MDH_PFA\(1\) MDH_PFA\(9\) MDH_PFA\(64\) MDH_PFA\(65\) MDH_PFA\(73\) MDH_PFA\(192\)", table)
    # the plain frame's kernels are as they were
    assert "k_path_frame<PF, true>" in api and "k_path_frame<PF, false>" in api and "path_pixel_active" not in text("madarch_amd", "csrc", "mdh_path_frame.h")


# ------------------------------------------------------------------------------------ 2. the rule through the library
def lib_active(n, m1, m2, lo, hi, tol, floor):
    from madarch_amd import renderers
    return renderers.Renderer.Path_Pixel_Active(n, m1, m2, lo, hi, tol, floor)


def states_from_samples(rng, pixels, samples, constant=False):
    """states as the kernel forms them: `samples` updates of seeded radiance a pixel"""
    n, m1, m2 = np.zeros(pixels, np.int64), np.zeros(pixels, np.float32), np.zeros(pixels, np.float32)
    base = rng.uniform(0.0, 3.0, (pixels, 3)).astype(np.float32)
    for _ in range(samples):
        rgb = base if constant else (base * rng.uniform(0.0, 2.0, (pixels, 3))).astype(np.float32)
        n, m1, m2 = PA.update(rgb, n, m1, m2)
    return n.astype(np.int32), m1, m2


def test_the_rule_on_the_host_equals_numpy():
    rng = np.random.RandomState(20261021)
    seen = {"active": 0, "retired": 0}
    for samples in (1, 2, 3, 5, 8, 13):
        n, m1, m2 = states_from_samples(rng, 512, samples)
        for lo, hi in ((1, 16), (2, 8), (4, 4), (8, 8), (3, 5), (1, 1 << 24)):
            for tol in (0.0, 0.02, 0.1, 0.5):
                for floor in (0.0, 0.01, 2.0):
                    want = PA.active(n, m1, m2, lo, hi, tol, floor)
                    got = lib_active(n, m1, m2, lo, hi, tol, floor)
                    assert np.array_equal(got, want), (samples, lo, hi, tol, floor)
                    if samples < lo:
                        assert want.all()  # n < min
                    if samples >= hi:
                        assert not want.any()  # n = max, min = max
                    seen["active"] += int(want.sum())
                    seen["retired"] += int((~want).sum())
    assert seen["active"] > 1000 and seen["retired"] > 1000
    # raw random states, the variance of either sign
    n = rng.randint(0, 12, 4096).astype(np.int32)
    m1 = (rng.standard_normal(4096) * 10.0).astype(np.float32)
    m2 = (rng.standard_normal(4096) * 30.0).astype(np.float32)
    for tol in (0.0, 0.05):
        assert np.array_equal(lib_active(n, m1, m2, 2, 10, tol, 0.01), PA.active(n, m1, m2, 2, 10, tol, 0.01))


def test_zero_variance_negative_variance_and_tolerance_zero():
    rng = np.random.RandomState(7)
    # constant samples: two of them have exactly zero variance (y + y and y y + y y are exact) and retire at min_samples under tolerance 0
    n, m1, m2 = states_from_samples(rng, 256, 2, constant=True)
    assert not PA.active(n, m1, m2, 2, 6, 0.0, 0.0).any() and not lib_active(n, m1, m2, 2, 6, 0.0, 0.0).any()
    assert lib_active(n, m1, m2, 3, 6, 0.0, 0.0).all()  # (below min_samples they run)
    # tolerance 0 keeps every pixel of positive variance running to max_samples
    n, m1, m2 = states_from_samples(rng, 256, 3)
    positive = PA.active(n, m1, m2, 1, 1 << 24, 0.0, 0.0)
    assert positive.sum() > 200 and np.array_equal(lib_active(n, m1, m2, 2, 6, 0.0, 0.0), positive)
    assert not lib_active(np.full(256, 6, np.int32), m1, m2, 2, 6, 0.0, 0.0).any()
    # a state whose variance rounds negative: searched among constant samples, whose exact variance is 0
    found = None
    for samples in range(3, 40):
        n, m1, m2 = states_from_samples(rng, 2048, samples, constant=True)
        with np.errstate(all="ignore"):
            c = n.astype(np.float32)
            mean = (m1 / c).astype(np.float32)
            var = ((m2 / c).astype(np.float32) - (mean * mean).astype(np.float32)).astype(np.float32)
        at = np.nonzero(var < 0)[0]
        if len(at):
            found = (n[at], m1[at], m2[at])
            break
    assert found is not None, "no state with a negative rounded variance among constant samples"
    n, m1, m2 = found
    print("%d states whose variance rounds negative, n = %d" % (len(n), n[0]))
    for tol in (0.0, 0.1):
        assert not PA.active(n, m1, m2, 2, 1 << 24, tol, 0.01).any() and not lib_active(n, m1, m2, 2, 1 << 24, tol, 0.01).any()  # retired


def test_nan_and_infinite_moments_retire_or_run_as_the_rule_says():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    m1 = np.array([nan, 1.0, nan, inf, 1.0, inf, -inf, PA.BAD, 1e30, 1.0], np.float32)
    m2 = np.array([1.0, nan, nan, 1.0, inf, inf, inf, PA.BAD, 1e30, 1e38], np.float32)
    for count in (0, 1, 2, 5, 8):
        n = np.full(len(m1), count, np.int32)
        for tol in (0.0, 0.1):
            want = PA.active(n, m1, m2, 2, 8, tol, 0.01)
            assert np.array_equal(lib_active(n, m1, m2, 2, 8, tol, 0.01), want), (count, tol)
            assert not want[[0, 1, 2, 7]].any()  # a NaN retires, at any count: a pixel that was not traced does not count up
            if count < 2:
                assert want[[3, 4, 5, 6, 8, 9]].all()  # (below min_samples an infinity still runs)
            if count == 8:
                assert not want.any()
    # inf - inf in the variance: NaN, retired
    assert not lib_active(np.array([4], np.int32), np.array([inf], np.float32), np.array([inf], np.float32), 2, 8, 0.1, 0.01).any()


# ------------------------------------------------------------------------------------ 3. the stand-alone program
@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("path_adaptive") / "path_adaptive_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "madarch_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "path_adaptive_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "path_adaptive_check: ok" in out.stdout
    lines = out.stdout.splitlines()
    return {k: [ln.split()[1:] for ln in lines if ln.startswith(k + " ")] for k in "UA"}


def f32(words):
    return np.array([int(x, 16) for x in words], dtype=np.uint32).view(np.float32)


def test_updates_bit_for_bit(check_output):
    rows = check_output["U"]
    assert len(rows) > 500
    rgb = np.stack([f32([r[c] for r in rows]) for c in range(3)], axis=1)
    n0, m1, m2 = np.array([int(r[3]) for r in rows]), f32([r[4] for r in rows]), f32([r[5] for r in rows])
    n, w1, w2 = PA.update(rgb, n0, m1, m2)
    assert np.array_equal(n, np.array([int(r[6]) for r in rows]))
    assert np.array_equal(w1.view(np.uint32), f32([r[7] for r in rows]).view(np.uint32)) and np.array_equal(w2.view(np.uint32), f32([r[8] for r in rows]).view(np.uint32))


def test_the_rule_bit_for_bit_and_the_library_gives_the_same(check_output):
    rows = check_output["A"]
    assert len(rows) > 5000
    n, m1, m2 = np.array([int(r[0]) for r in rows], np.int32), f32([r[1] for r in rows]), f32([r[2] for r in rows])
    lo, hi = np.array([int(r[3]) for r in rows]), np.array([int(r[4]) for r in rows])
    tol, floor = f32([r[5] for r in rows]), f32([r[6] for r in rows])
    got = np.array([int(r[7]) for r in rows], bool)
    assert got.any() and (~got).any()
    seen = 0
    for key in {tuple(k) for k in np.stack([lo, hi, tol.view(np.uint32), floor.view(np.uint32)], axis=1).tolist()}:
        at = (lo == key[0]) & (hi == key[1]) & (tol.view(np.uint32) == key[2]) & (floor.view(np.uint32) == key[3])
        t, f = float(tol[at][0]), float(floor[at][0])
        assert np.array_equal(PA.active(n[at], m1[at], m2[at], key[0], key[1], t, f), got[at]), key
        assert np.array_equal(lib_active(n[at], m1[at], m2[at], key[0], key[1], t, f), got[at]), key
        seen += int(at.sum())
    assert seen == len(rows)
