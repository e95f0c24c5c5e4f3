// The static VALU counts behind scripts/ray_bounds_estimate.py: one block of closest_primitive's ROOM step per kernel, beside an
// empty kernel with the same loads and stores (b_base for the step's blocks, r_base for the set-up).  Cross-compile with the Makefile's
// flags and count the v_ instructions per kernel:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
//         -fno-gpu-flush-denormals-to-zero -fno-vectorize -fno-slp-vectorize --cuda-device-only -S -o ray_bounds_probe.s scripts/probes/ray_bounds_probe.hip
//   python3 scripts/probes/count_valu.py ray_bounds_probe.s
//
// b_sphere - b_base: the sphere's cull test (d2, tsum, the squared compare); b_box - b_base: the box's (q, m, thr); b_cmp - b_base: one
// bound's compare; r_setup - r_base: ray_bounds.  The roots behind the ballots are left out: the question is what a step pays to decide
// against them.  Never run on a device.
#include "../../madarch_amd/csrc/mdh_device.h"
#define LANE (blockIdx.x * blockDim.x + threadIdx.x)
extern "C" __global__ void b_base(const float *in, float *out) { const int l = LANE; f3 x = F3(in[l], in[l + 64], in[l + 128]); float closest = in[l + 192];
   out[l] = closest + x.x + x.y + x.z; }
extern "C" __global__ void b_sphere(const float *in, float *out, float4 a) { const int l = LANE; f3 x = F3(in[l], in[l + 64], in[l + 128]); float closest = in[l + 192];
   const float d2 = dot2(xyz(a) - x); const float tsum = closest + a.w;
   const bool need = !(tsum < 0.0f) && !(d2 > (tsum * tsum) * 1.000001f);
   out[l] = __ballot(need) != 0ull ? d2 : closest + x.x + x.y + x.z; }
extern "C" __global__ void b_box(const float *in, float *out, float4 c, float4 e) { const int l = LANE; f3 x = F3(in[l], in[l + 64], in[l + 128]); float closest = in[l + 192];
   const f3 q = abs3(xyz(c) - x) - xyz(e); const float m = max_(q.x, max_(q.y, q.z));
   const float thr = closest > 0.0f ? closest * 1.000001f : closest;
   out[l] = __ballot(!(m > thr)) != 0ull ? q.x + q.y + q.z + m : closest + x.x + x.y + x.z; }
extern "C" __global__ void b_cmp(const float *in, float *out) { const int l = LANE; f3 x = F3(in[l], in[l + 64], in[l + 128]); float closest = in[l + 192]; const float hs = in[l + 256];
   out[l] = __ballot(!(hs > closest)) != 0ull ? 1.0f : closest + x.x + x.y + x.z; }
// the set-up: o, d, tmax in; the table's header is not in LDS here, so thr and lim come as arguments
extern "C" __global__ void r_base(const float *in, float *out) { const int l = LANE; f3 o = F3(in[l], in[l + 64], in[l + 128]), d = F3(in[l + 192], in[l + 256], in[l + 320]); float tmax = in[l + 384];
   out[l] = o.x + o.y + o.z + d.x + d.y + d.z + tmax; out[l + 64] = tmax; }
extern "C" __global__ void r_setup(const float *in, float *out, float4 s, float4 b0, float4 b1, float thr, float lim) { const int l = LANE; f3 o = F3(in[l], in[l + 64], in[l + 128]), d = F3(in[l + 192], in[l + 256], in[l + 320]); float tmax = in[l + 384];
   bool ok = thr > 0.0f && tmax >= 0.0f;
   ok = ok && __builtin_fabsf(o.x) <= lim && __builtin_fabsf(o.y) <= lim && __builtin_fabsf(o.z) <= lim;
   ok = ok && __builtin_ldexpf(__builtin_fabsf(dot2(d) - 1.0f), 18) <= 1.0f;
   const float E = __builtin_ldexpf(lim + tmax, -14);
   float hs, hb;
   { const f3 w = xyz(s) - o; const f3 q = w - d * __builtin_amdgcn_fmed3f(dot(w, d), 0.0f, tmax); hs = (__builtin_amdgcn_sqrtf(dot2(q)) - s.w) - E; }
   { const f3 w = xyz(b0) - o; const f3 q = w - d * __builtin_amdgcn_fmed3f(dot(w, d), 0.0f, tmax); const float q2 = dot2(q), rq = __builtin_amdgcn_rsqf(q2); const f3 e = xyz(b1);
     const float sup = ((__builtin_fabsf(q.x) * e.x + __builtin_fabsf(q.y) * e.y) + __builtin_fabsf(q.z) * e.z) * rq;
     hb = (q2 * rq - sup) - E * (1.0f + 2.0f * ((e.x + e.y) + e.z) * rq); }
   const int off = ok ? 0 : -1;
   hs = __int_as_float(__float_as_int(hs) | off); hb = __int_as_float(__float_as_int(hb) | off);
   out[l] = hs + (o.x + o.y + o.z + d.x + d.y + d.z + tmax); out[l + 64] = hb; }
