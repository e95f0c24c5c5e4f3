"""mdh_inscatter_points, mdh_inscatter_rays and their _device forms without a device: the four entry points in every
interface, the library's exports and its refusal of a null renderer, the Python argument checks, the predicates the host and
the lanes share, and the float64 side of the device test's free rays -- few enough of them are fragile (at most half of
ref64.FRAGILE_CAP) that the device test cannot hide behind the cap.

Measured on the CPU with the construction of tests/inscatter_cases.py (its seeds): none of the room's 192 rays and one of
the open scene's (0.5 %) is fragile with the lengths given (march = 0), none and five of their 8 336 and 8 901 sample points;
of the marched lengths one (0.5 %) and none.  The issue's own draws measured 0.5 % and 0 %, and for rays whose length ends
AT the surface (march = 1) 11.5 % and 5.7 % for their colour, which is why the colour test gives the lengths and the marched
length is held by itself."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import inscatter_cases as IC
import ref64
import ref64_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = (("inscatter_points", "Inscatter_Points"), ("inscatter_points_device", "Inscatter_Points_Device"),
                ("inscatter_rays", "Inscatter_Rays"), ("inscatter_rays_device", "Inscatter_Rays_Device"))


def text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


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
    for fn in ("inscatter_points", "inscatter_points_device"):
        assert re.search(r"mdh_%s\s*\(\s*mdh_renderer\s*\*\s*r\s*,\s*int32_t\s+n\s*,\s*const\s+float\s*\*\s*pos_xyz\s*,\s*const\s+float\s*\*\s*dir_xyz\s*,"
                         r"\s*const\s+float\s*\*\s*f\s*,\s*float\s*\*\s*rgb_out" % fn, header), fn
    for fn in ("inscatter_rays", "inscatter_rays_device"):
        assert re.search(r"mdh_%s\s*\(\s*mdh_renderer\s*\*\s*r\s*,\s*int32_t\s+n\s*,\s*const\s+float\s*\*\s*org_xyz\s*,\s*const\s+float\s*\*\s*dir_xyz\s*,"
                         r"\s*const\s+float\s*\*\s*tmax\s*,\s*int32_t\s+march\s*,\s*float\s+step\s*,\s*float\s*\*\s*rgb_out\s*,\s*float\s*\*\s*len_out\s*,"
                         r"\s*int32_t\s*\*\s*steps_out" % fn, header), fn
        assert B.HIP_ONLY_ABI[fn][1][5:7] == [B._I, B._F]
    for fn in ("inscatter_points_device", "inscatter_rays_device"):
        assert re.search(r"mdh_%s\s*\([^;]*void\s*\*\s*stream\s*\)\s*;" % fn, header)
        assert B.HIP_ONLY_ABI[fn][1][-1] is B._P
    assert [len(B.HIP_ONLY_ABI[fn][1]) for fn, _ in ENTRY_POINTS] == [6, 7, 10, 11]
    assert re.search(r"#define\s+MDH_INSCATTER_MAX_STEPS\s+4096\b", header)
    assert renderers.Renderer.INSCATTER_MAX_STEPS == 4096
    assert callable(examples.foggy_fisheye_view)
    # the older calls still say that they compose no fog, and now say where it is to be had
    for call in ("mdh_shade_rays(", "mdh_path_trace("):
        at = header.index(call)
        comment = header[header.rindex("/*", 0, at):at]
        assert "NO VOLUMETRICS" in comment and "mdh_inscatter_rays" in comment, call
    # the header states the association of the sample point
    assert "(dir * f) + org" in header


def test_the_library_exports_them_and_refuses_a_null_renderer():
    from madarch_amd import _binding as B
    b = B.hip_binding()
    buf = (C.c_float * 6)()
    p = C.cast(buf, C.c_void_p)
    assert b.inscatter_points(None, 1, p, p, None, p) == B.MDH_E_INVALID
    assert b.inscatter_points_device(None, 1, p, p, None, p, None) == B.MDH_E_INVALID
    assert b.inscatter_rays(None, 1, p, p, p, 0, 0.1, p, None, None) == B.MDH_E_INVALID
    assert b.inscatter_rays_device(None, 1, p, p, p, 0, 0.1, p, None, None, None) == B.MDH_E_INVALID
    assert (np.frombuffer(buf, dtype=np.float32) == 0.0).all()


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
    host, lens = np.zeros((n, 3), np.float32), np.ones(n, np.float32)
    bad = [
        ("points: two shapes", lambda: R.Inscatter_Points(host, host[:-1])),
        ("points: not (n, 3)", lambda: R.Inscatter_Points(host.reshape(-1), host.reshape(-1))),
        ("points: f of another length", lambda: R.Inscatter_Points(host, host, lens[:-1])),
        ("rays: two shapes", lambda: R.Inscatter_Rays(host, host[:-1], lens, 0.1)),
        ("rays: lengths of another length", lambda: R.Inscatter_Rays(host, host, lens[:-1], 0.1)),
        ("rays: no lengths", lambda: R.Inscatter_Rays(host, host, None, 0.1)),
        ("rays: a step of zero", lambda: R.Inscatter_Rays(host, host, lens, 0.0)),
        ("rays: a negative step", lambda: R.Inscatter_Rays(host, host, lens, -0.1)),
        ("rays: a step that is not a number", lambda: R.Inscatter_Rays(host, host, lens, float("nan"))),
        ("rays: an infinite step", lambda: R.Inscatter_Rays(host, host, lens, float("inf"))),
        ("rays: march 2", lambda: R.Inscatter_Rays(host, host, lens, 0.1, March=2)),
        ("rays: march as a float", lambda: R.Inscatter_Rays(host, host, lens, 0.1, March=0.5)),
        ("device points: no colours", lambda: R.Inscatter_Points_Device(f3, f3, None)),
        ("device points: short colours", lambda: R.Inscatter_Points_Device(f3, f3, Fake(3 * n - 1))),
        ("device points: int32 f", lambda: R.Inscatter_Points_Device(f3, f3, f3, F=i1)),
        ("device points: host positions", lambda: R.Inscatter_Points_Device(Fake(3 * n, cuda=False), f3, f3)),
        ("device points: a numpy array", lambda: R.Inscatter_Points_Device(host, f3, f3)),
        ("device points: addresses without a count", lambda: R.Inscatter_Points_Device(0x1000, 0x2000, 0x3000)),
        ("device rays: no lengths", lambda: R.Inscatter_Rays_Device(f3, f3, None, 0.1, f3)),
        ("device rays: no colours", lambda: R.Inscatter_Rays_Device(f3, f3, f1, 0.1, None)),
        ("device rays: float32 steps", lambda: R.Inscatter_Rays_Device(f3, f3, f1, 0.1, f3, Steps=f1)),
        ("device rays: int32 lengths out", lambda: R.Inscatter_Rays_Device(f3, f3, f1, 0.1, f3, Len=i1)),
        ("device rays: non-contiguous origins", lambda: R.Inscatter_Rays_Device(Fake(3 * n, contiguous=False), f3, f1, 0.1, f3)),
        ("device rays: more rays than the origins hold", lambda: R.Inscatter_Rays_Device(f3, f3, f1, 0.1, f3, N=n + 1)),
        ("device rays: a step of zero", lambda: R.Inscatter_Rays_Device(f3, f3, f1, 0.0, f3)),
        ("device rays: march 2", lambda: R.Inscatter_Rays_Device(f3, f3, f1, 0.1, f3, March=2)),
    ]
    for what, call in bad:
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")


def test_the_host_and_the_lanes_apply_one_predicate(tmp_path):
    """mdh_ray_stream.h holds the predicates, the kernels and the host's checks call them, and they decide the edges as the
    header states them (a small program of its own over the header: no HIP runtime in it)"""
    kernels, api = text("madarch_amd", "csrc", "mdh_kernels.h"), text("madarch_amd", "csrc", "mdh_api.hip")
    for fn in ("rs_inscatter_tmax_valid", "rs_inscatter_f_valid"):
        assert re.search(r"\b%s\s*\(" % fn, kernels) and re.search(r"\b%s\s*\(" % fn, api), fn
    assert re.search(r"\brs_inscatter_step_valid\s*\(", api)
    for family in ("GK_k_point_inscatter", "GK_k_ray_inscatter"):
        assert family in api
    body = api[api.index("static const void *kernel_ptr(const PassKernel &k)\n{"):]
    assert re.search(r"MDH_INS\(0\) MDH_INS\(1\) MDH_INS\(9\) MDH_INS\(64\) MDH_INS\(65\) MDH_INS\(73\) MDH_INS\(192\)\s*return nullptr;", body)
    assert body.index("MDH_INS(0)") > body.index("MDH_PATH(192)")  # the newest kernels last: nothing older moves
    # the visibility rays are the guarded march of the ray queries, and k_visibility keeps its own, unguarded copy
    ins = kernels[kernels.index("MDH_DEV f3 inscatter("):kernels.index("struct InscatterPointArgs")]
    assert "raycast_visibility<PART, true>" in ins
    vis = kernels[kernels.index("void k_visibility("):kernels.index("scattering pass")]
    assert "raycast_visibility<PART>(sc, pos, L, L_dist)" in vis
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = tmp_path / "predicates.cpp"
    src.write_text(r'''
#include "mdh_ray_stream.h"
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
int main()
{
   const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
   int bad = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("failed: %s\n", #c); ++bad; } } while (0)
   EXPECT(MDH_INSCATTER_MAX_STEPS == 4096);
   EXPECT(rs_inscatter_tmax_valid(0.0f, 20.0f) && rs_inscatter_tmax_valid(-0.0f, 20.0f) && rs_inscatter_tmax_valid(20.0f, 20.0f));
   EXPECT(!rs_inscatter_tmax_valid(-1e-30f, 20.0f) && !rs_inscatter_tmax_valid(std::nextafterf(20.0f, inf), 20.0f));
   EXPECT(!rs_inscatter_tmax_valid(nan, 20.0f) && !rs_inscatter_tmax_valid(inf, 20.0f) && !rs_inscatter_tmax_valid(1.0f, nan));
   EXPECT(rs_inscatter_step_valid(0.1f, 20.0f) && rs_inscatter_step_valid(20.0f / 4096.0f, 20.0f));
   EXPECT(!rs_inscatter_step_valid(std::nextafterf(20.0f / 4096.0f, 0.0f), 20.0f));
   EXPECT(!rs_inscatter_step_valid(0.0f, 20.0f) && !rs_inscatter_step_valid(-0.1f, 20.0f) && !rs_inscatter_step_valid(nan, 20.0f));
   EXPECT(!rs_inscatter_step_valid(inf, 20.0f) && !rs_inscatter_step_valid(0.1f, inf) && !rs_inscatter_step_valid(0.1f, nan));
   EXPECT(rs_inscatter_f_valid(0.0f) && rs_inscatter_f_valid(-3.0f) && !rs_inscatter_f_valid(nan) && !rs_inscatter_f_valid(-inf));
   // the step cap bounds the serial loop: with len <= max_dist <= 4096 step, f passes len after at most 4097 + rounding turns
   for (float step : {20.0f / 4096.0f, 0.007f, 0.1f}) {
      int n = 0;
      for (float f = 0.0f; f < 20.0f && n < 100000; f += step) ++n;
      EXPECT(n <= MDH_INSCATTER_MAX_STEPS + 2);
   }
   std::printf(bad ? "predicates: FAILED\n" : "predicates: ok\n");
   return bad != 0;
}
''')
    exe = str(tmp_path / "predicates")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "madarch_amd", "csrc"), "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "predicates: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_the_chains_lengths_have_the_steps_they_are_named_for():
    for step in IC.CHAIN_STEPS:
        for count in IC.CHAIN_COUNTS:
            t = IC.tmax_for(step, count)
            assert IC.steps_of(step, t) == count and 0.0 <= float(t) <= 20.0, (step, count, t)
    # every count is met in the batches, in every variant
    for name in ("room", "mesh, triangle BVH"):
        seen, first = set(), 0
        for n in IC.CHAIN_BATCHES:
            seen |= set(IC.chain_rays(name, n, first)[2])
            first += n
        assert seen == set(IC.CHAIN_COUNTS)
    # the sequence by repeated addition is not k * step where the step is not representable
    f = IC.f_sequence(0.1, 129)
    assert (f != (np.arange(130, dtype=np.float32) * np.float32(0.1))).any()
    assert np.array_equal(IC.f_sequence(2.0 ** -5, 129), np.arange(130, dtype=np.float32) * np.float32(2.0 ** -5))


@pytest.mark.parametrize("name", ["room", "open"])
def test_free_rays_are_not_fragile_in_float64(name):
    ray_runs, point_runs = IC.free_runs(name)
    desc, org, drs, tmax, counts, P, D, F, ray = IC.free_samples(name)
    assert len(org) == IC.N_FREE and ray_runs[0]["colour"].shape == (IC.N_FREE, 3) and point_runs[0]["colour"].shape == (len(P), 3)
    assert np.isfinite(ray_runs[0]["colour"]).all() and (ray_runs[0]["colour"].max(axis=1) > 0.0).mean() > 0.5
    assert (tmax >= 0.0).all() and (tmax <= 6.0).all() and max(counts) > 64  # (more than one chunk of steps)
    share, _ = ref64.hold_values(name + ": rays", ray_runs, ray_runs[0]["colour"], RC.SCATTER_RTOL, RC.SCATTER_ATOL, cap=0.5 * ref64.FRAGILE_CAP)
    assert share <= 0.5 * ref64.FRAGILE_CAP
    share, _ = ref64.hold_values(name + ": points", point_runs, point_runs[0]["colour"], RC.FROXEL_RTOL, RC.FROXEL_ATOL, cap=0.5 * ref64.FRAGILE_CAP)
    assert share <= 0.5 * ref64.FRAGILE_CAP
    share = float(IC.march_fragile(IC.march_runs(name)).mean())
    print("%s: marched lengths, fragile share %.4f" % (name, share))
    assert share <= ref64.FRAGILE_CAP
