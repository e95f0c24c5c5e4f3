// mdh_path.h -- what the path tracer (k_path_trace, mdh_kernels.h; mdh_path_trace, mdh_path_trace_device, mdh_path_scatter,
// mdh_api.hip) decides without a device: the random numbers of a path, the direction of its next segment, and which rays are
// traced at all.  Plain inline functions, no HIP runtime in them: the kernel includes this header and its lanes call them,
// mdh_path_scatter runs the same functions on the host, and tests/path_sampler_check.cpp drives them on the CPU under the
// sanitizers.  Every fp32 operation is one IEEE operation in source order (-ffp-contract=off, correctly rounded roots and
// quotients, no fused multiply-add): host and lane give a result the same bits.
//
// THE RANDOM NUMBERS.  path_u01 (seed, ray_id, sample, bounce, dimension) is a counter-based hash of its five 32-bit words
// and of nothing else -- not of the batch, the launch grid or the order of the rays.  With all arithmetic modulo 2^32:
//    pcg (v):  s = v * 747796405 + 2891336453;   w = ((s >> ((s >> 28) + 4)) ^ s) * 277803737;   pcg = (w >> 22) ^ w
//    h = pcg (seed);  h = pcg (h + ray_id);  h = pcg (h + sample);  h = pcg (h + bounce);  h = pcg (h + dimension)
//    path_u01 = float (h >> 8) * 2^-24
// (the output function of PCG-RXS-M-XS-32 chained over the words).  h >> 8 is below 2^24, so the conversion and the product
// are exact: a binary32 value in [0, 1) with no floating-point operation in front of that product, and no sin.
//
// THE SAMPLER.  path_scatter (dir, normal, roughness, u) restates the model of the reference's glsl/render_path.glsl:26-33
// with three numbers u[0 .. 2] (dimensions 0, 1, 2 of the path's bounce) on n = normal / |normal| -- the normals of triangles
// are far from unit length:
//    u[0] < roughness:   the cosine-weighted direction about n,
//                           d = (t1 cos (2 PI u[2]) + t2 sin (2 PI u[2])) sqrt (u[1]) + n sqrt (1 - u[1])
//    otherwise:          d = reflect (dir, n) + offset * roughness with uniform_vector's formula (random.glsl:43-47)
//                           a = PI u[1], b = 2 PI u[2], offset = (sin b sin a, cos b sin a, cos a)
// and the result is d / |d| in both branches.  THE REFERENCE'S TANGENT FRAME IS NOT KEPT: cosine_direction divides by
// 1 + n.z, which is zero on a wall that faces -z.  (t1, t2) is the branch-free construction with s = copysign (1, n.z),
//    a = -1 / (s + n.z),  b = n.x n.y a,  t1 = (1 + s n.x n.x a,  s b,  -s n.x),  t2 = (b,  s + n.y n.y a,  -n.y)
// whose divisor s + n.z has a magnitude of at least 1: finite for every unit normal.  Sine and cosine are the library's
// sin_ / cos_ (mdh_device.h: Cody-Waite reduction and Cephes polynomials), restated here operation for operation so that
// the host has them too.  A zero normal, or a mirror direction that cancels, gives components that are not finite:
// path_dir_finite says so and the path ends there.
//
// WHICH RAYS ARE TRACED.  The marches carry no stall guard, as in the pixel program: every march parameter has to stay below
// 2^14 ("Path tracing a host's rays": the derivation).  path_ray_valid is rs_shade_ray_valid's bound on
// the primary ray, without the zero direction, which that bound lets through; every later direction is a unit vector up to
// rounding, so a bounce moves the shaded point by less than max_dist + 0.25, and up to MDH_PATH_MAX_BOUNCES bounces keep every
// shadow ray below 13 246.  The scene's half is the host's path_scene_check (mdh_api.hip), which is shade_scene_check without
// the probe grid: no probe is read.
//
// THE PIXELS OF A PATH-TRACED FRAME (mdh_path_frame_*, mdh_path_frame.h).  Pixel (i, j) of a W x H frame, row 0 at the top, has the
// ray id j W + i -- the numbering of mdh_camera_rays -- and for sample s the screen position
//    jx = jitter ? path_u01 (seed, id, s, 0, 3) : 0.5,   jy = jitter ? path_u01 (seed, id, s, 0, 4) : 0.5
//    u = ((float)(2 i) + 2 jx) / (float) W - 1,   v = -(((float)(2 j) + 2 jy) / (float) H - 1)
// each step one binary32 operation: dimensions 3 and 4 of bounce 0 are taken by nobody, path_scatter takes 0 .. 2 of every
// bounce.  2 jx is exact and below 2, so a jittered position stays inside its pixel's footprint, and with 0.5 the numerator
// is (float)(2 i + 1) -- which is how it is formed without jitter: tile_pixel's centre (mdh_kernels.h) and mdh_camera_rays'
// rays to the bit at every size.
#pragma once

#include "mdh_ray_stream.h"

#define MDH_PATH_FN MDH_RS_FN
#define MDH_PATH_MAX_BOUNCES 6 // 5 322 + 6 x 1 025 + 1 774 = 13 246 < 2^14
#define MDH_PATH_DIMS 3        // the numbers path_scatter takes per bounce
#define MDH_PATH_DIM_JX 3      // ... and behind them, at bounce 0, the two of a frame's sub-pixel jitter
#define MDH_PATH_DIM_JY 4
#ifndef MDH_PATH_FRAME_MAX_PIXELS
#define MDH_PATH_FRAME_MAX_PIXELS 67108864 // (madarch_hip.h) a frame's cap, 2^26: 805 MB of sums, every index of its kernels below 2^28
#endif

// ---------------------------------------------------------------------- the random numbers
MDH_PATH_FN unsigned path_pcg(unsigned v)
{
   const unsigned s = v * 747796405u + 2891336453u;
   const unsigned w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
   return (w >> 22) ^ w;
}
MDH_PATH_FN unsigned path_hash(unsigned seed, unsigned ray_id, unsigned sample, unsigned bounce, unsigned dimension)
{
   unsigned h = path_pcg(seed);
   h = path_pcg(h + ray_id);
   h = path_pcg(h + sample);
   h = path_pcg(h + bounce);
   return path_pcg(h + dimension);
}
MDH_PATH_FN float path_u01(unsigned seed, unsigned ray_id, unsigned sample, unsigned bounce, unsigned dimension)
{
   return (float)(path_hash(seed, ray_id, sample, bounce, dimension) >> 8) * 0x1p-24f; // (both exact)
}

// ---------------------------------------------------------------------- the pixels of a frame
// one axis: pixel k of n, its jitter in [0, 1) or none
MDH_PATH_FN float path_pixel_axis(int k, int n, bool jitter, float jk)
{
   const float num = jitter ? (float)(2 * k) + 2.0f * jk : (float)(2 * k + 1);
   return num / (float)n - 1.0f;
}
// (u, v) of pixel (i, j) of a W x H frame for sample `sample`; row 0 = top
MDH_PATH_FN void path_pixel_uv(int i, int j, int W, int H, unsigned seed, unsigned sample, bool jitter, float &u, float &v)
{
   const unsigned id = (unsigned)j * (unsigned)W + (unsigned)i;
   const float jx = jitter ? path_u01(seed, id, sample, 0u, MDH_PATH_DIM_JX) : 0.5f;
   const float jy = jitter ? path_u01(seed, id, sample, 0u, MDH_PATH_DIM_JY) : 0.5f;
   u = path_pixel_axis(i, W, jitter, jx);
   v = -path_pixel_axis(j, H, jitter, jy);
}
MDH_PATH_FN bool path_frame_size_valid(int W, int H) { return W >= 1 && H >= 1 && (long long)W * H <= (long long)MDH_PATH_FRAME_MAX_PIXELS; }

// ---------------------------------------------------------------------- an adaptive frame: a pixel's moments and its stopping rule
// (mdh_path_frame_begin_adaptive, k_path_frame_adaptive in mdh_path_frame_adaptive.h, mdh_path_pixel_active on the host.)  Beside its
// three sums a pixel holds the count n of its completed samples and the moments m1, m2 of y = (r + g) + b.  When a sample with
// radiance (r, g, b) completes, every step one binary32 operation, unfused:
//    y = (r + g) + b;   acc = acc + rgb;   m1 = m1 + y;   m2 = m2 + y * y  (the product rounded, then the sum);   n = n + 1
// path_pixel_active says whether the pixel takes further samples.  THIS IS A STOPPING RULE ON A BIASED VARIANCE ESTIMATE: the
// variance is the plug-in one (divided by n, not n - 1) of a sum of channels, the rule looks at the samples it then stops or
// goes on drawing, and the resolved image of an adaptive frame is NOT CLAIMED TO BE UNBIASED -- min_samples is the host's guard
// against pixels that stop on a lucky start.  A NaN anywhere -- a pixel whose ray was not traced has NaN moments -- retires
// the pixel: such a pixel's count does not advance, so the test for it stands in front of the one for min_samples, or it
// would stay active for ever.  A variance that rounds negative retires it too (e > lim * lim is then false).
#define MDH_PATH_MAX_SAMPLES 16777216 // 2^24: (float) n is exact
MDH_PATH_FN bool path_adaptive_valid(int min_samples, int max_samples, float tolerance, float floor)
{
   return min_samples >= 1 && min_samples <= max_samples && max_samples <= MDH_PATH_MAX_SAMPLES && rs_finite(tolerance) && tolerance >= 0.0f && rs_finite(floor) &&
          floor >= 0.0f;
}
MDH_PATH_FN void path_pixel_update(float r, float g, float b, int &n, float &m1, float &m2)
{
   const float y = (r + g) + b;
   const float yy = y * y;
   m1 = m1 + y;
   m2 = m2 + yy;
   n = n + 1;
}
MDH_PATH_FN bool path_pixel_active(int n, float m1, float m2, int min_samples, int max_samples, float tolerance, float floor)
{
   if (n >= max_samples) return false;
   if (m1 != m1 || m2 != m2) return false; // (not traced, or NaN radiance: the count may stand still)
   if (n < min_samples) return true;
   const float c = (float)n;
   const float mean = m1 / c, q = m2 / c;
   const float mm = mean * mean;
   const float var = q - mm;
   const float e = var / c; // the variance of the mean
   const float lim = tolerance * (mean + floor);
   const float ll = lim * lim;
   return e > ll; // (any NaN: false)
}

// ---------------------------------------------------------------------- which rays are traced
MDH_PATH_FN bool path_bounces_valid(int bounces) { return bounces >= 0 && bounces <= MDH_PATH_MAX_BOUNCES; }
MDH_PATH_FN bool path_ray_valid(float ox, float oy, float oz, float dx, float dy, float dz)
{
   return rs_shade_ray_valid(ox, oy, oz, dx, dy, dz) && (dx != 0.0f || dy != 0.0f || dz != 0.0f); // (a zero direction leads nowhere: no path)
}
MDH_PATH_FN bool path_dir_finite(float x, float y, float z) { return rs_finite(x) && rs_finite(y) && rs_finite(z); }

// ---------------------------------------------------------------------- the sampler
// sin_ and cos_ of mdh_device.h, operation for operation (oracle/orc_math.h fixes the sequence)
MDH_PATH_FN void path_sincos(float x, float &sn, float &cs)
{
   float kf = __builtin_rintf(x * 0.636619772367581f);
   if (!(__builtin_fabsf(kf) < 1.0e9f)) kf = 0.0f;
   const float r = ((x - kf * 1.5703125f) - kf * 4.837512969970703125e-4f) - kf * 7.54978995489188216e-8f;
   const float z = r * r;
   float ps = -1.9515295891e-4f;
   ps = ps * z + 8.3321608736e-3f;
   ps = ps * z + -1.6666654611e-1f;
   const float s = (ps * z) * r + r;
   float pc = 2.443315711809948e-5f;
   pc = pc * z + -1.388731625493765e-3f;
   pc = pc * z + 4.166664568298827e-2f;
   const float c = ((pc * z) * z - 0.5f * z) + 1.0f;
   const int q = (int)kf & 3;
   const float rs = (q & 1) ? c : s, rc = (q & 1) ? s : c;
   sn = (q & 2) ? -rs : rs;
   cs = ((q + 1) & 2) ? -rc : rc;
}
#define MDH_PATH_PI 3.14159265358f // maths.glsl:1
#define MDH_PATH_2PI 6.28318530718f
MDH_PATH_FN float path_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; } // (the library's dot)
// out = v / |v|
MDH_PATH_FN void path_normalize(const float *v, float *out)
{
   const float len = __builtin_sqrtf(path_dot(v, v));
   out[0] = v[0] / len; out[1] = v[1] / len; out[2] = v[2] / len;
}
// the direction of the next segment; out may be dir or normal
MDH_PATH_FN void path_scatter(const float *dir, const float *normal, float roughness, const float *u, float *out)
{
   float n[3], d[3];
   path_normalize(normal, n);
   if (u[0] < roughness) { // diffuse: cosine-weighted about n
      const float s = __builtin_copysignf(1.0f, n[2]);
      const float a = -1.0f / (s + n[2]);
      const float b = (n[0] * n[1]) * a;
      const float t1[3] = {1.0f + ((s * n[0]) * n[0]) * a, s * b, -s * n[0]};
      const float t2[3] = {b, s + (n[1] * n[1]) * a, -n[1]};
      float sn, cs;
      path_sincos(MDH_PATH_2PI * u[2], sn, cs);
      const float r = __builtin_sqrtf(u[1]), h = __builtin_sqrtf(1.0f - u[1]);
      for (int c = 0; c < 3; ++c) d[c] = (t1[c] * cs + t2[c] * sn) * r + n[c] * h;
   } else { // the mirror direction, widened by the roughness
      const float k = 2.0f * path_dot(n, dir);
      float sa, ca, sb, cb;
      path_sincos(MDH_PATH_PI * u[1], sa, ca);
      path_sincos(MDH_PATH_2PI * u[2], sb, cb);
      const float off[3] = {sb * sa, cb * sa, ca};
      for (int c = 0; c < 3; ++c) d[c] = (dir[c] - n[c] * k) + off[c] * roughness;
   }
   path_normalize(d, out);
}
// ... with the numbers of ray `ray_id`, sample `sample`, bounce `bounce`
MDH_PATH_FN void path_scatter_at(const float *dir, const float *normal, float roughness, unsigned seed, unsigned ray_id, unsigned sample, unsigned bounce, float *out)
{
   float u[MDH_PATH_DIMS];
   for (int q = 0; q < MDH_PATH_DIMS; ++q) u[q] = path_u01(seed, ray_id, sample, bounce, (unsigned)q);
   path_scatter(dir, normal, roughness, u, out);
}
