// The static VALU counts behind scripts/cold_code_estimate.py: one block of the screen kernel's straight-line code per kernel, beside an
// empty kernel with the same loads and stores (p_base for the arg-min's candidates, s_base for segment_clear's blocks).  Cross-compile
// with the Makefile's flags and count the v_ instructions per kernel:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
//         -fno-gpu-flush-denormals-to-zero -fno-vectorize -fno-slp-vectorize --cuda-device-only -S -o cold_code_probe.s scripts/probes/cold_code_probe.hip
//   python3 scripts/probes/count_valu.py cold_code_probe.s
//
// On the commit before MDH_INFO_CULL: p_base 8, p_sphere 55, p_box 63, s_base 11, s_faces 34, s_all6 61, s_sphere 38 -- a sphere candidate 47,
// a box candidate 55, segment_clear's sphere block 27, its three face axes 23, its three cross axes 27.  Never run on a device.
#include "../../madarch_amd/csrc/mdh_device.h"
// inputs: in[0..] per lane; outputs out[] per lane
#define LANE (blockIdx.x * blockDim.x + threadIdx.x)
extern "C" __global__ void p_base(const float *in, float *out) { const int l = LANE; f3 x = F3(in[l], in[l + 64], in[l + 128]); float c = in[l + 192]; int b = __float_as_int(in[l + 256]); out[l] = c + x.x + x.y + x.z; out[l + 64] = __int_as_float(b); }
extern "C" __global__ void p_sphere(const float *in, float *out, float4 a, int idx) { const int l = LANE; f3 x = F3(in[l], in[l + 64], in[l + 128]); float closest = in[l + 192]; int best = __float_as_int(in[l + 256]);
   const float d_ = sd_sphere(a, x); if (d_ < closest || (d_ == closest && best >= 0 && idx < best)) { closest = d_; best = idx; }
   out[l] = closest + x.x + x.y + x.z; out[l + 64] = __int_as_float(best); }
extern "C" __global__ void p_box(const float *in, float *out, float4 c, float4 e, int idx) { const int l = LANE; f3 x = F3(in[l], in[l + 64], in[l + 128]); float closest = in[l + 192]; int best = __float_as_int(in[l + 256]);
   const float d_ = sd_box(c, e, x); if (d_ < closest || (d_ == closest && best >= 0 && idx < best)) { closest = d_; best = idx; }
   out[l] = closest + x.x + x.y + x.z; out[l + 64] = __int_as_float(best); }
// segment_clear pieces: A, vd, vmax in
extern "C" __global__ void s_base(const float *in, float *out) { const int l = LANE; f3 A = F3(in[l], in[l + 64], in[l + 128]), vd = F3(in[l + 192], in[l + 256], in[l + 320]); float vmax = in[l + 384];
   out[l] = A.x + A.y + A.z + vd.x + vd.y + vd.z + vmax; }
extern "C" __global__ void s_faces(const float *in, float *out, float4 c, float4 e4, float thr) { const int l = LANE; f3 A = F3(in[l], in[l + 64], in[l + 128]), vd = F3(in[l + 192], in[l + 256], in[l + 320]); float vmax = in[l + 384];
   const f3 hv = vd * (vmax * 0.5f), ah = abs3(hv); const f3 m = (A + hv) - xyz(c); const f3 e = xyz(e4) + F3s(thr);
   const bool sep = __builtin_fabsf(m.x) > e.x + ah.x || __builtin_fabsf(m.y) > e.y + ah.y || __builtin_fabsf(m.z) > e.z + ah.z;
   out[l] = sep ? 1.0f : A.x + A.y + A.z + vd.x + vd.y + vd.z + vmax; }
extern "C" __global__ void s_all6(const float *in, float *out, float4 c, float4 e4, float thr) { const int l = LANE; f3 A = F3(in[l], in[l + 64], in[l + 128]), vd = F3(in[l + 192], in[l + 256], in[l + 320]); float vmax = in[l + 384];
   const f3 hv = vd * (vmax * 0.5f), ah = abs3(hv); const f3 m = (A + hv) - xyz(c); const f3 e = xyz(e4) + F3s(thr);
   const bool sep = __builtin_fabsf(m.x) > e.x + ah.x || __builtin_fabsf(m.y) > e.y + ah.y || __builtin_fabsf(m.z) > e.z + ah.z ||
                          __builtin_fabsf(m.y * hv.z - m.z * hv.y) > e.y * ah.z + e.z * ah.y ||
                          __builtin_fabsf(m.z * hv.x - m.x * hv.z) > e.z * ah.x + e.x * ah.z ||
                          __builtin_fabsf(m.x * hv.y - m.y * hv.x) > e.x * ah.y + e.y * ah.x;
   out[l] = sep ? 1.0f : A.x + A.y + A.z + vd.x + vd.y + vd.z + vmax; }
extern "C" __global__ void s_sphere(const float *in, float *out, float4 a, float thr) { const int l = LANE; f3 A = F3(in[l], in[l + 64], in[l + 128]), vd = F3(in[l + 192], in[l + 256], in[l + 320]); float vmax = in[l + 384];
   const f3 w = xyz(a) - A; const f3 q = w - vd * clamp_(dot(w, vd), 0.0f, vmax); const float rt = a.w + thr;
   out[l] = dot2(q) > rt * rt ? 1.0f : A.x + A.y + A.z + vd.x + vd.y + vd.z + vmax; }
