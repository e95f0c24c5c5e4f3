// mdh_ray_stream.h -- what the device-array ray queries (k_ray_stream, mdh_kernels.h; mdh_raycast_device, .., mdh_api.hip)
// decide without a device: which rays are marched at all, and how a wavefront hands the next rays to its idle lanes -- and
// which rays mdh_shade_rays and mdh_shade_rays_device shade (k_ray_shade; tests/shade_rays_check.cpp drives that predicate).
// Plain inline functions, no HIP runtime in them: the kernels include this header, the host's checks call the same
// predicate (ray_query_check), and tests/ray_stream_check.cpp drives the hand-out on the CPU under the sanitizers.
//
// THE HAND-OUT.  A launch owns one 32-bit counter `next`, zero at its start.  A wavefront that refills counts its idle
// lanes (k = the set bits of `idle`), one lane adds k to the counter and broadcasts the value it found there (`base`), and
// the j-th idle lane in lane order takes ray base + j -- if that is below n; otherwise the lane has no ray, and since the
// counter only grows, neither has any lane of this wavefront ever again: the wavefront is drained (rs_drained) and asks no
// more.  A wavefront therefore adds to the counter at most once beyond n, and at most 64 then: the counter cannot wrap
// for n < 2^31 and fewer than 2^25 wavefronts.  No wavefront reads what another one wrote except through the counter.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MDH_RS_FN __host__ __device__ inline
#else
#define MDH_RS_FN inline
#endif

#define MDH_RS_WAVE 64
#define MDH_RS_REFILL_MIN 1
#define MDH_RS_REFILL_MAX 64 // lock step: rounds of 64 consecutive rays, k_ray_query's schedule
#ifndef MDH_RAY_STREAM_REFILL_DEFAULT
#define MDH_RAY_STREAM_REFILL_DEFAULT 64 // MDH_OPT_RAY_STREAM_REFILL as a renderer starts ("Ray queries": the measurement that sets it)
#endif
#define MDH_RS_BAD_BITS 0x7fc00000u // what visibility and soft shadow answer a ray that was not marched with: the quiet NaN

// ---------------------------------------------------------------------- which rays are marched
MDH_RS_FN bool rs_finite(float x)
{
   unsigned u;
   __builtin_memcpy(&u, &x, 4);
   return (u & 0x7f800000u) != 0x7f800000u; // (neither an infinity nor a NaN; denormals are finite)
}
// the six components of a ray
MDH_RS_FN bool rs_ray_valid(float ox, float oy, float oz, float dx, float dy, float dz)
{
   return rs_finite(ox) && rs_finite(oy) && rs_finite(oz) && rs_finite(dx) && rs_finite(dy) && rs_finite(dz);
}
// the length of a visibility or soft-shadow ray: finite and within the scene's max_dist (any finite value below it, negative ones too)
MDH_RS_FN bool rs_tmax_valid(float tmax, float max_dist) { return rs_finite(tmax) && tmax <= max_dist; }

// ---------------------------------------------------------------------- which rays are shaded
// mdh_shade_rays, mdh_shade_rays_device (k_ray_shade, mdh_kernels.h): the marches of the pixel program -- primary, reflection,
// shadow, cage visibility -- carry no stall guard, so a shaded ray has to keep every march parameter below 2^14, where a step of
// at least epsilon still moves it ("Shading a host's rays": the derivation).  The ray's half of the bound:
// every component finite, an origin within MDH_RS_SHADE_EXTENT of 0 along every axis, a direction within MDH_RS_SHADE_DIR.
// The scene's half (rs_shade_extent_valid of max_dist, of every light's position and of the probe grid's far corner) is the
// host's check at the call.
#define MDH_RS_SHADE_EXTENT 1024.0f
#define MDH_RS_SHADE_DIR 2.0f
MDH_RS_FN bool rs_within(float x, float bound) { return rs_finite(x) && x >= -bound && x <= bound; } // (a NaN compares false twice; denormals and both zeros are within)
MDH_RS_FN bool rs_shade_extent_valid(float x) { return rs_within(x, MDH_RS_SHADE_EXTENT); }
MDH_RS_FN bool rs_shade_ray_valid(float ox, float oy, float oz, float dx, float dy, float dz)
{
   return rs_within(ox, MDH_RS_SHADE_EXTENT) && rs_within(oy, MDH_RS_SHADE_EXTENT) && rs_within(oz, MDH_RS_SHADE_EXTENT) &&
          rs_within(dx, MDH_RS_SHADE_DIR) && rs_within(dy, MDH_RS_SHADE_DIR) && rs_within(dz, MDH_RS_SHADE_DIR);
}

// ---------------------------------------------------------------------- which points are shaded
// mdh_shade_points, mdh_shade_points_device (k_point_shade, mdh_kernels.h; tests/shade_points_check.cpp drives this predicate):
// the same program from a point of the host's on, so the same requirement -- every march parameter below 2^14 -- with the
// point's normal and view direction now the host's too ("Lighting a host's points": the derivation).
// Every component finite, the position within MDH_RS_SHADE_EXTENT of 0 along every axis, the normal and the view direction
// within MDH_RS_POINT_DIR, the material id inside the table of n_materials entries.  The direction bound is 1, NOT the 2 of a
// shaded ray: reflect (view, normal) = view - 2 dot (normal, view) normal is as long as |view| (1 + 2 |normal|^2), the
// reflection's hit lies up to max_dist times that from the point, and with components of 2 that is 86 x 1024 -- with
// components of 1 it is 7 sqrt 3 x 1024 < 12 416, and the shadow and visibility rays of that hit stay below 15 966 < 2^14.
// Mode 3 (the irradiance alone) has neither a view direction nor a material: its caller passes zeros.
#define MDH_RS_POINT_DIR 1.0f
MDH_RS_FN bool rs_shade_point_valid(float px, float py, float pz, float nx, float ny, float nz, float vx, float vy, float vz, int material, int n_materials)
{
   return rs_within(px, MDH_RS_SHADE_EXTENT) && rs_within(py, MDH_RS_SHADE_EXTENT) && rs_within(pz, MDH_RS_SHADE_EXTENT) &&
          rs_within(nx, MDH_RS_POINT_DIR) && rs_within(ny, MDH_RS_POINT_DIR) && rs_within(nz, MDH_RS_POINT_DIR) &&
          rs_within(vx, MDH_RS_POINT_DIR) && rs_within(vy, MDH_RS_POINT_DIR) && rs_within(vz, MDH_RS_POINT_DIR) &&
          material >= 0 && material < n_materials;
}

// ---------------------------------------------------------------------- which rays and points gather in-scattered light
// mdh_inscatter_points, mdh_inscatter_rays and their _device forms (k_point_inscatter, k_ray_inscatter, mdh_kernels.h).  Their
// marches carry the stall guard, so finite inputs are all a point needs; a ray's work is bounded by its length over the
// step, and that by the call: tmax within [0, max_dist] per ray, max_dist / step at most MDH_INSCATTER_MAX_STEPS per call.
#ifndef MDH_INSCATTER_MAX_STEPS
#define MDH_INSCATTER_MAX_STEPS 4096 // (madarch_hip.h names the same value)
#endif
// a ray's length: finite, not negative (-0 is 0) and within the scene's max_dist
MDH_RS_FN bool rs_inscatter_tmax_valid(float tmax, float max_dist) { return rs_finite(tmax) && tmax >= 0.0f && tmax <= max_dist; }
// the call's step: finite, above 0, and at most MDH_INSCATTER_MAX_STEPS of it within max_dist (a NaN on either side fails)
MDH_RS_FN bool rs_inscatter_step_valid(float step, float max_dist)
{
   return rs_finite(step) && step > 0.0f && max_dist / step <= (float)MDH_INSCATTER_MAX_STEPS;
}
// a point's distance along its ray, where the caller gives one
MDH_RS_FN bool rs_inscatter_f_valid(float f) { return rs_finite(f); }

// ---------------------------------------------------------------------- which spheres are swept or tested
// mdh_spherecast, mdh_contacts and their _device forms (mdh_kernels.h).  The marches carry the stall guard, so a finite ray is
// all the march needs; the radius and the length are finite and within [0, max_dist] (-0 is 0).
MDH_RS_FN bool rs_sweep_radius_valid(float radius, float max_dist) { return rs_finite(radius) && radius >= 0.0f && radius <= max_dist; }
MDH_RS_FN bool rs_sweep_tmax_valid(float tmax, float max_dist) { return rs_finite(tmax) && tmax >= 0.0f && tmax <= max_dist; }
MDH_RS_FN bool rs_centre_valid(float x, float y, float z) { return rs_finite(x) && rs_finite(y) && rs_finite(z); }

// ---------------------------------------------------------------------- the hand-out
MDH_RS_FN int rs_popcount(unsigned long long m) { return __builtin_popcountll(m); }
// does a wavefront with n_idle idle lanes take new rays?
MDH_RS_FN bool rs_refills(int n_idle, int refill) { return n_idle >= refill || n_idle == MDH_RS_WAVE; }
// the place of `lane` among the idle lanes (bit l of `idle`: lane l is idle)
MDH_RS_FN int rs_idle_rank(unsigned long long idle, int lane) { return rs_popcount(idle & ((1ull << lane) - 1ull)); }
// the ray an idle lane takes from a hand-out that found `base` in the counter, or -1: none, now and for good
MDH_RS_FN long long rs_ray_of(unsigned base, unsigned long long idle, int lane, unsigned n)
{
   const unsigned long long q = (unsigned long long)base + (unsigned)rs_idle_rank(idle, lane);
   return q < (unsigned long long)n ? (long long)q : -1;
}
// after a hand-out of k rays from `base`: has the counter passed n (no later hand-out can yield a ray)?
MDH_RS_FN bool rs_drained(unsigned base, int k, unsigned n) { return (unsigned long long)base + (unsigned)k >= (unsigned long long)n; }
