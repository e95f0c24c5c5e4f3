// The static VALU counts behind scripts/best_approx_estimate.py: the blocks of the second point's best-first search (shade_structured,
// mdh_march.h) one per kernel, beside an empty kernel with the same loads and stores (a_base).  Cross-compile with the Makefile's flags
// and count the v_ instructions per kernel:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
//         -fno-gpu-flush-denormals-to-zero -fno-vectorize -fno-slp-vectorize --cuda-device-only -S -o best_approx_probe.s scripts/probes/best_approx_probe.hip
//   python3 scripts/probes/count_valu.py best_approx_probe.s
//
// a_scan1 - a_base: one corner pass of the exact scan (probes_fresh, cage_probe, grid_to_world, length, sdiv3, the dot product, the
// compare and its selects; the loop's own skip test is a_skip - a_base); a_winner - a_base: the same statements for a per-lane corner,
// without the dot product; a_rank<F> - a_base: best_approx in a wavefront whose lanes all fold the axes of F, that is with 8, 4, 2 and
// 1 corners for F = 0, 1, 3 and 7 -- the per-corner cost is the slope, the set-up and the decision the intercept.  Never run on a device.
#define MDH_BLOCK 256 // (mdh_kernels.h's, which mdh_march.h's park rows are sized by)
#include "../../madarch_amd/csrc/mdh_march.h"
#define LANE (blockIdx.x * blockDim.x + threadIdx.x)
struct In { f3 P, N; i3 gp; int folded, tried; };
MDH_DEV In load(const float *in, int l)
{
   In r;
   r.P = F3(in[l], in[l + 64], in[l + 128]); r.N = F3(in[l + 192], in[l + 256], in[l + 320]);
   r.gp.x = __float_as_int(in[l + 384]); r.gp.y = __float_as_int(in[l + 448]); r.gp.z = __float_as_int(in[l + 512]);
   r.folded = __float_as_int(in[l + 576]); r.tried = __float_as_int(in[l + 640]);
   return r;
}
struct Best { float bd, bvmax; f3 bvd; int bi, bq; };
MDH_DEV void store(float *out, int l, const Best &b, const In &x)
{
   out[l] = b.bd + b.bvmax + x.P.x + x.P.y + x.P.z + x.N.x + x.N.y + x.N.z; out[l + 64] = b.bvd.x; out[l + 128] = b.bvd.y; out[l + 192] = b.bvd.z;
   out[l + 256] = __int_as_float(b.bi + b.bq + x.gp.x + x.gp.y + x.gp.z + x.folded + x.tried);
}
extern "C" __global__ void a_base(KScene sc, KProbes pr, const float *in, float *out)
{
   const int l = LANE; const In x = load(in, l); Best b = {0.0f, 0.0f, F3(0.0f, 0.0f, 0.0f), -1, 0};
   store(out, l, b, x);
}
extern "C" __global__ void a_skip(KScene sc, KProbes pr, const float *in, float *out, int i)
{
   const int l = LANE; const In x = load(in, l); Best b = {0.0f, 0.0f, F3(0.0f, 0.0f, 0.0f), -1, 0};
   if (!((i & x.folded) || ((x.tried >> i) & 1))) b.bi = i;
   store(out, l, b, x);
}
extern "C" __global__ void a_scan1(KScene sc, KProbes pr, const float *in, float *out, int i)
{
   const int l = LANE; const In x = load(in, l); Best b = {0.0f, 0.0f, F3(0.0f, 0.0f, 0.0f), -1, 0};
   {
      const KProbes pq = probes_fresh(pr);
      const i3 q = cage_probe(pq, x.gp, i);
      const f3 pw = grid_to_world(pq, q);
      const f3 hvec = x.P - pw;
      const float dist = length(hvec);
      f3 vd = sdiv3(hvec, dist);
      vd = -vd;
      const float d = dot(-vd, -x.N);
      if (d > b.bd) { b.bd = d; b.bi = i; b.bvd = vd; b.bvmax = dist - MDH_MIN_STEP * 5.0f; b.bq = q.x | (q.y << 10) | (q.z << 20); }
   }
   store(out, l, b, x);
}
extern "C" __global__ void a_winner(KScene sc, KProbes pr, const float *in, float *out)
{
   const int l = LANE; const In x = load(in, l); Best b = {0.0f, 0.0f, F3(0.0f, 0.0f, 0.0f), -1, 0};
   {
      b.bi = x.tried & 7; // (a per-lane index)
      const KProbes pq = probes_fresh(pr);
      const i3 q = cage_probe(pq, x.gp, b.bi);
      const f3 pw = grid_to_world(pq, q);
      const f3 hvec = x.P - pw;
      const float dist = length(hvec);
      f3 vd = sdiv3(hvec, dist);
      vd = -vd;
      b.bvd = vd; b.bvmax = dist - MDH_MIN_STEP * 5.0f; b.bq = q.x | (q.y << 10) | (q.z << 20);
   }
   store(out, l, b, x);
}
// the full expansion of the root behind sqrt_'s wave-wide guard: in a_scan1 and a_winner as code, never executed for a dot2 of 2^-96 or
// more -- a_root_full - a_root_base comes off both
extern "C" __global__ void a_root_base(const float *in, float *out) { const int l = LANE; out[l] = in[l]; }
extern "C" __global__ void a_root_full(const float *in, float *out) { const int l = LANE; out[l] = __builtin_sqrtf(in[l]); }
template <int F> MDH_DEV void rank(const KProbes &pr, const float *in, float *out)
{
   const int l = LANE; In x = load(in, l); Best b = {0.0f, 0.0f, F3(0.0f, 0.0f, 0.0f), -1, 0};
   const int lane_folds = x.folded; // (kept for the stores)
   x.folded = F;
   const int state = best_approx(pr, x.gp, x.folded, x.P, x.N, b.bi);
   b.bq = __ballot(state == 0) != 0ull ? 1 : state;
   x.folded = lane_folds;
   store(out, l, b, x);
}
extern "C" __global__ void a_rank0(KScene sc, KProbes pr, const float *in, float *out) { rank<0>(pr, in, out); }
extern "C" __global__ void a_rank1(KScene sc, KProbes pr, const float *in, float *out) { rank<1>(pr, in, out); }
extern "C" __global__ void a_rank3(KScene sc, KProbes pr, const float *in, float *out) { rank<3>(pr, in, out); }
extern "C" __global__ void a_rank7(KScene sc, KProbes pr, const float *in, float *out) { rank<7>(pr, in, out); }
