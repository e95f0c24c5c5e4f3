"""mdh_path_trace, mdh_path_trace_device and mdh_path_scatter without a device: the three entry points in all four
interfaces, the Python argument checks, the sampler as a stand-alone program under the address and undefined-behaviour
sanitizers (tests/path_sampler_check.cpp) held against the numpy restatements of tests/path_trace_cases.py -- the random
numbers bit for bit, the directions against float64, the distribution's first moments -- the furnace-free plane on the
float64 side, and the float64 side of the device test's free rays: few enough are fragile that it cannot hide behind the cap."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import path_trace_cases as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = (("path_trace", "Path_Trace"), ("path_trace_device", "Path_Trace_Device"), ("path_scatter", "Path_Scatter"))


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ------------------------------------------------------------------------------------ a. entry points
def test_entry_points_in_every_interface():
    from madarch_amd import _binding as B
    from madarch_amd import renderers
    header, hpp, ads = text("include", "madarch_hip.h"), text("include", "madarch.hpp"), text("ada", "madarch_hip.ads")
    for fn, method in ENTRY_POINTS:
        assert re.search(r"int32_t\s+mdh_%s\s*\(" % fn, header), fn
        assert fn in B.HIP_ONLY_ABI and fn not in B.ABI
        assert callable(getattr(renderers.Renderer, method))
        assert re.search(r"\bmdh_%s\s*\(" % fn, hpp) and re.search(r"\b%s\s*\(" % method, hpp), fn
        assert re.search(r'External_Name\s*=>\s*"mdh_%s"' % fn, ads), fn
    for fn in ("path_trace", "path_trace_device"):
        assert re.search(r"mdh_%s\s*\(\s*mdh_renderer\s*\*\s*r\s*,\s*int32_t\s+n\s*,[^;]*uint32_t\s+seed\s*,\s*uint32_t\s+id_first\s*,\s*int32_t\s+sample_first\s*,"
                         r"\s*int32_t\s+sample_count\s*,\s*int32_t\s+bounces\s*,\s*float\s*\*\s*rgb_accum" % fn, header), fn
        assert B.HIP_ONLY_ABI[fn][1][4:9] == [C.c_uint32, C.c_uint32, B._I, B._I, B._I]
    assert re.search(r"mdh_path_trace_device\s*\([^;]*void\s*\*\s*stream\s*\)\s*;", header)
    assert B.HIP_ONLY_ABI["path_trace_device"][1][-1] is B._P
    assert len(B.HIP_ONLY_ABI["path_trace"][1]) == 13 and len(B.HIP_ONLY_ABI["path_trace_device"][1]) == 14 and len(B.HIP_ONLY_ABI["path_scatter"][1]) == 9
    # the sampler takes no renderer
    assert re.search(r"mdh_path_scatter\s*\(\s*int32_t\s+n\s*,", header)
    # the header says that no fog is composed, at the path tracer
    at = header.index("mdh_path_trace(")
    assert "NO VOLUMETRICS" in header[header.rindex("/*", 0, at):at]
    # the three deviations from the reference's file stand in the kernel's comment and in DESIGN.md
    for doc in (text("madarch_amd", "csrc", "mdh_kernels.h"), text("DESIGN.md")):
        low = doc.lower()
        assert "render_path.glsl" in doc and "masked" in low and "once" in low and "offset" in low


def test_the_library_exports_them_and_refuses_a_null_renderer():
    from madarch_amd import _binding as B
    b = B.hip_binding()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    assert b.path_trace(None, 1, p, p, 1, 0, 0, 1, 3, p, None, None, None) == B.MDH_E_INVALID
    assert b.path_trace_device(None, 1, p, p, 1, 0, 0, 1, 3, p, None, None, None, None) == B.MDH_E_INVALID
    # the sampler needs no renderer and no device
    assert b.path_scatter(-1, p, p, p, 1, 0, 0, 0, p) == B.MDH_E_INVALID
    assert b.path_scatter(1, None, p, p, 1, 0, 0, 0, p) == B.MDH_E_INVALID and b.path_scatter(1, p, p, p, 1, 0, -1, 0, p) == B.MDH_E_INVALID
    assert b.path_scatter(0, None, None, None, 1, 0, 0, 0, None) == B.MDH_OK


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
    n = 10
    f3, f1, i1 = Fake(3 * n), Fake(n), Fake(n, "torch.int32")
    host = np.zeros((n, 3), np.float32)
    none = NoLibrary()
    bad = [
        ("seven bounces", lambda: R.Path_Trace(host, host, Bounces=7)),
        ("negative bounces", lambda: R.Path_Trace(host, host, Bounces=-1)),
        ("a negative first sample", lambda: R.Path_Trace(host, host, Sample_First=-1)),
        ("a negative count", lambda: R.Path_Trace(host, host, Sample_Count=-1)),
        ("a sum beyond 2^31", lambda: R.Path_Trace(host, host, Sample_First=2 ** 31 - 2, Sample_Count=2)),
        ("a seed of 33 bits", lambda: R.Path_Trace(host, host, Seed=2 ** 32)),
        ("a negative id", lambda: R.Path_Trace(host, host, Id_First=-1)),
        ("two shapes", lambda: R.Path_Trace(host, host[:-1])),
        ("not (n, 3)", lambda: R.Path_Trace(host.reshape(-1), host.reshape(-1))),
        ("sums of another shape", lambda: R.Path_Trace(host, host, Rgb_Accum=np.zeros((n - 1, 3), np.float32))),
        ("device: seven bounces", lambda: R.Path_Trace_Device(f3, f3, f3, Bounces=7)),
        ("device: no sums", lambda: R.Path_Trace_Device(f3, f3, None)),
        ("device: short sums", lambda: R.Path_Trace_Device(f3, f3, Fake(3 * n - 1))),
        ("device: int32 sums", lambda: R.Path_Trace_Device(f3, f3, Fake(3 * n, "torch.int32"))),
        ("device: host sums", lambda: R.Path_Trace_Device(f3, f3, Fake(3 * n, cuda=False))),
        ("device: non-contiguous origins", lambda: R.Path_Trace_Device(Fake(3 * n, contiguous=False), f3, f3)),
        ("device: float32 hits", lambda: R.Path_Trace_Device(f3, f3, f3, Hit=f1)),
        ("device: int32 t", lambda: R.Path_Trace_Device(f3, f3, f3, T=i1)),
        ("device: more rays than the origins hold", lambda: R.Path_Trace_Device(f3, f3, f3, N=n + 1)),
        ("device: addresses without a count", lambda: R.Path_Trace_Device(0x1000, 0x2000, 0x3000)),
        ("device: a numpy array", lambda: R.Path_Trace_Device(host, f3, f3)),
        ("device: a negative first sample", lambda: R.Path_Trace_Device(f3, f3, f3, Sample_First=-1)),
        ("scatter: two shapes", lambda: R.Path_Scatter(host, host[:-1], 0.5, Binding=none)),
        ("scatter: roughness of another length", lambda: R.Path_Scatter(host, host, np.zeros(n - 1, np.float32), Binding=none)),
        ("scatter: a negative bounce", lambda: R.Path_Scatter(host, host, 0.5, Bounce=-1, Binding=none)),
        ("scatter: a negative sample", lambda: R.Path_Scatter(host, host, 0.5, Sample=-1, Binding=none)),
        ("scatter: a seed of 33 bits", lambda: R.Path_Scatter(host, host, 0.5, Seed=2 ** 32, Binding=none)),
    ]
    for what, call in bad:
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")


def test_the_kernel_and_the_host_call_the_checked_functions():
    """what the CPU checks is what the device runs: the lanes and mdh_path_scatter call the header's functions, the header
    brings no HIP runtime, and the kernels are the newest family, named behind every older one"""
    header = text("madarch_amd", "csrc", "mdh_path.h")
    assert re.findall(r"#\s*include\s*(\S+)", header) == ['"mdh_ray_stream.h"']
    assert not re.search(r"\bsinf?\s*\(|\bfract\b", header.split("#pragma once")[1])
    kernels, api = text("madarch_amd", "csrc", "mdh_kernels.h"), text("madarch_amd", "csrc", "mdh_api.hip")
    assert re.search(r"\bpath_scatter_at\s*\(", kernels) and re.search(r"\bpath_scatter_at\s*\(", api)
    assert re.search(r"\bpath_ray_valid\s*\(", kernels) and re.search(r"\bpath_ray_valid\s*\(", api) and re.search(r"\bpath_bounces_valid\s*\(", api)
    body = api[api.index("static const void *kernel_ptr(const PassKernel &k)\n{"):]
    assert re.search(r"MDH_PATH\(0\) MDH_PATH\(1\) MDH_PATH\(9\) MDH_PATH\(64\) MDH_PATH\(65\) MDH_PATH\(73\) MDH_PATH\(192\)\s*return nullptr;", body)
    assert body.index("MDH_PATH(0)") > body.index("MDH_PT(192)")
    assert "k_path_trace<PF>" in api
    # no atomics and no shared counter in the kernel
    kernel = kernels[kernels.index("void k_path_trace("):kernels.index("the window's pixels")]
    assert "atomic" not in kernel and "__shared__" not in kernel


# ------------------------------------------------------------------------------------ b. the sampler as a stand-alone program
@pytest.fixture(scope="module")
def sampler_output(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("path_sampler") / "path_sampler_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "madarch_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "path_sampler_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "path_sampler_check: ok" in out.stdout
    lines = out.stdout.splitlines()
    return {k: [l.split()[1:] for l in lines if l.startswith(k + " ")] for k in "USC"}


def f32(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint32).view(np.float32)


def test_random_numbers_bit_for_bit(sampler_output):
    rows = sampler_output["U"]
    assert len(rows) == 10 * 10 * 3 * 3 * 3
    args = np.array([[int(x) for x in r[:5]] for r in rows], dtype=np.uint64).astype(np.uint32)
    got = np.array([int(r[5], 16) for r in rows], dtype=np.uint32)
    want = PT.u01(args[:, 0], args[:, 1], args[:, 2], args[:, 3], args[:, 4])
    assert np.array_equal(want.view(np.uint32), got)
    u = got.view(np.float32)
    assert (u >= 0.0).all() and (u < 1.0).all() and np.array_equal(np.floor(u.astype(np.float64) * 2 ** 24), u.astype(np.float64) * 2 ** 24)
    # the numbers are not all alike: every argument moves them
    assert len(np.unique(got)) > 0.99 * len(got)
    assert 0.45 < u.mean() < 0.55


# the largest error of the stand-alone program's directions against scatter64, per component, measured on this build: 2.55e-7
# (some 4 ulp of 1: the frame's products, the polynomial sine and cosine, the normalisation).  Four times that is allowed.
SCATTER_MEASURED, SCATTER_ATOL = 2.55e-7, 1.02e-6


def test_sampler_against_float64(sampler_output):
    rows = sampler_output["S"]
    assert len(rows) == 11 * 3 * 12
    v = np.stack([f32(r[1:]) for r in rows])  # d, n, rough, u, out
    D, N, rough, u, out = v[:, 0:3], v[:, 3:6], v[:, 6], v[:, 7:10], v[:, 10:13]
    # the cases: the six axis normals, lengths 0.5 and 1.7, three roughnesses, both branches
    axes = {tuple(x) for x in N[np.abs(N).sum(axis=1) == 1.0].astype(int).tolist()}
    assert axes == {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)}
    lengths = np.sqrt((N.astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(lengths - 0.5) < 1e-3).any() and (np.abs(lengths - 1.7) < 5e-3).any()
    assert set(rough.tolist()) == {0.0, 0.5, 1.0}
    cosine = u[:, 0] < rough
    assert cosine.sum() > 100 and (~cosine).sum() > 100
    assert np.isfinite(out).all()
    length = np.sqrt((out.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 4.0 * 2.0 ** -23
    want = PT.scatter64(D, N, rough, u)
    err = np.abs(out.astype(np.float64) - want).max()
    print("largest error against float64: %.3g (allowed %.3g)" % (err, SCATTER_ATOL))
    assert err <= SCATTER_ATOL
    # the cosine branch stays on the normal's side, roughness 0 is the mirror direction
    n = N / lengths[:, None]
    assert ((out * n).sum(axis=1)[cosine] >= -1e-6).all()
    mirror = rough == 0.0
    refl = D - n * (2.0 * (n * D).sum(axis=1))[:, None]
    assert np.abs(out[mirror] - refl[mirror] / np.linalg.norm(refl[mirror], axis=1, keepdims=True)).max() < 1e-6


# ------------------------------------------------------------------------------------ c. the distribution
def test_cosine_distribution(sampler_output):
    rows = sampler_output["C"]
    assert len(rows) == 4096
    d = np.stack([f32(r) for r in rows]).astype(np.float64)
    n = np.array([0.48, -0.6, 0.64])
    assert abs(np.linalg.norm(n) - 1.0) < 1e-12
    cos = d @ n
    print("mean dot (dir, n) = %.4f" % cos.mean())
    assert abs(cos.mean() - 2.0 / 3.0) <= 6.0 / (64.0 * np.sqrt(18.0))  # 0.0221
    t = np.cross(n, [0.0, 0.0, 1.0])
    t /= np.linalg.norm(t)
    for tangent in (t, np.cross(n, t)):
        m = (d @ tangent).mean()
        print("mean tangential component = %.4f" % m)
        assert abs(m) <= 6.0 / (64.0 * np.sqrt(4.0))  # 0.047
    # the stand-alone program's directions are the numpy restatement's
    want = PT.scatter64(np.tile([[0.0, 0.0, -1.0]], (4096, 1)), np.tile(n.astype(np.float32)[None, :], (4096, 1)), 1.0,
                        PT.numbers(PT.SEED_PATHS, np.arange(4096), 0, 0))
    assert np.abs(d - want).max() <= SCATTER_ATOL


# ------------------------------------------------------------------------------------ d. the furnace-free plane, in float64
def test_plane_estimator_in_float64():
    org, drs = PT.plane_rays()
    assert len(org) == PT.PLANE_RAYS and (drs[:, 1] < -0.2).all()
    t = (-1.0 - org[:, 1]) / drs[:, 1]
    assert (t > 0).all() and (t < 19.0).all()  # every ray hits the floor inside max_dist
    est = PT.ref_plane()
    mean, dev = PT.plane_expected()
    worst = (np.abs(est - mean[None, :]) / dev[None, :]).max()
    print("largest deviation %.3f of its bound" % worst)
    assert (np.abs(est - mean[None, :]) <= dev[None, :]).all()


# ------------------------------------------------------------------------------------ e. the float64 side of the free rays
@pytest.mark.parametrize("samples", PT.FREE_SAMPLES)
@pytest.mark.parametrize("name", ["room", "open"])
def test_free_rays_are_not_fragile_in_float64(name, samples):
    import ref64
    runs = PT.free_runs(name, samples)
    assert len(runs) == 3 and runs[0]["colour"].shape == (PT.N_FREE, 3)
    share = float(PT.fragile(runs, samples).mean())
    print("%s, %d samples: fragile share %.4f" % (name, samples, share))
    assert share <= ref64.FRAGILE_CAP
    assert np.isfinite(runs[0]["colour"]).all()
