// path_sampler_check.cpp -- the path tracer's random numbers, its sampler and its ray predicate (madarch_amd/csrc/mdh_path.h) on
// the CPU.  The header is the one k_path_trace includes and mdh_path_scatter calls; tests/test_path_trace_host.py builds this
// program with the address and undefined-behaviour sanitizers, runs it, and holds what it prints against restatements in numpy:
//    U seed ray sample bounce dim bits          path_u01 on a grid of arguments, the result's bits in hex
//    S case dx dy dz nx ny nz rough u0 u1 u2 ox oy oz     path_scatter, every float as its bits in hex
//    C ox oy oz                                 4 096 cosine-branch directions about one normal (path_scatter_at, roughness 1)
// and drives path_ray_valid and path_bounces_valid at their edge values itself.
#include "mdh_path.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static unsigned bits(float f)
{
   unsigned u;
   memcpy(&u, &f, 4);
   return u;
}
static float from_bits(unsigned u)
{
   float f;
   memcpy(&f, &u, 4);
   return f;
}
static bool with(int at, float value)
{
   float v[6] = {1.0f, -2.0f, 3.0f, 0.0f, 0.6f, -0.8f};
   v[at] = value;
   return path_ray_valid(v[0], v[1], v[2], v[3], v[4], v[5]);
}

int main()
{
   // ---- the random numbers
   const unsigned words[] = {0u, 1u, 2u, 63u, 64u, 257u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 20261020u};
   const int nw = (int)(sizeof words / sizeof words[0]);
   for (int a = 0; a < nw; ++a)
      for (int b = 0; b < nw; ++b)
         for (unsigned sample = 0; sample < 3; ++sample)
            for (unsigned bounce = 0; bounce < 7; bounce += 3)
               for (unsigned dim = 0; dim < MDH_PATH_DIMS; ++dim) {
                  const float u = path_u01(words[a], words[b], sample, bounce, dim);
                  EXPECT(u >= 0.0f && u < 1.0f, "path_u01 in [0, 1)");
                  EXPECT((float)(int)(u * 16777216.0f) == u * 16777216.0f, "a multiple of 2^-24");
                  printf("U %u %u %u %u %u %08x\n", words[a], words[b], sample, bounce, dim, bits(u));
               }

   // ---- the sampler: the six axis normals (the back wall's (0, 0, -1) among them), normals of lengths 0.5 and 1.7, three
   // roughnesses, seeded directions and numbers
   const float normals[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1},
                               {0.3f, 0.4f, 0.0f}, {-0.68f, 1.02f, -1.19f}, {0.0f, -0.5f, 0.0f}, {1.0f, -1.2f, 0.68f}, {1e-3f, 2e-3f, -0.5f}};
   const float roughs[] = {0.0f, 0.5f, 1.0f};
   int kase = 0;
   for (const auto &n : normals)
      for (float rough : roughs)
         for (unsigned k = 0; k < 12; ++k, ++kase) {
            float d[3], u[3], out[3];
            // a seeded unit direction that arrives at the surface (uniform_vector's formula, flipped against the normal)
            const float a = 3.14159265f * path_u01(7u, (unsigned)kase, 0u, 0u, 7u), b = 6.2831853f * path_u01(7u, (unsigned)kase, 0u, 0u, 8u);
            d[0] = std::sin(b) * std::sin(a); d[1] = std::cos(b) * std::sin(a); d[2] = std::cos(a);
            if (path_dot(d, n) > 0.0f) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; }
            for (unsigned q = 0; q < 3; ++q) u[q] = path_u01(11u, (unsigned)kase, k, 1u, q);
            path_scatter(d, n, rough, u, out);
            EXPECT(path_dir_finite(out[0], out[1], out[2]), "case %d: finite", kase);
            const double len = std::sqrt((double)out[0] * out[0] + (double)out[1] * out[1] + (double)out[2] * out[2]);
            EXPECT(std::fabs(len - 1.0) <= 4.0 * 0x1p-23, "case %d: |out| = %.9g", kase, len);
            // the wrapper draws the same numbers
            float out2[3];
            path_scatter_at(d, n, rough, 11u, (unsigned)kase, k, 1u, out2);
            EXPECT(bits(out2[0]) == bits(out[0]) && bits(out2[1]) == bits(out[1]) && bits(out2[2]) == bits(out[2]), "case %d: path_scatter_at", kase);
            printf("S %d %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", kase, bits(d[0]), bits(d[1]), bits(d[2]), bits(n[0]), bits(n[1]),
                   bits(n[2]), bits(rough), bits(u[0]), bits(u[1]), bits(u[2]), bits(out[0]), bits(out[1]), bits(out[2]));
         }
   // out may be dir or normal
   {
      float d[3] = {0.6f, -0.8f, 0.0f}, n[3] = {0.0f, 2.0f, 0.0f}, u[3] = {0.25f, 0.5f, 0.75f}, ref[3];
      path_scatter(d, n, 0.5f, u, ref);
      float d2[3] = {d[0], d[1], d[2]}, n2[3] = {n[0], n[1], n[2]};
      path_scatter(d2, n, 0.5f, u, d2);
      path_scatter(d, n2, 0.5f, u, n2);
      EXPECT(!memcmp(d2, ref, 12) && !memcmp(n2, ref, 12), "in place");
      // what ends a path: a zero normal
      float z[3] = {0.0f, 0.0f, 0.0f}, out[3];
      path_scatter(d, z, 0.5f, u, out);
      EXPECT(!path_dir_finite(out[0], out[1], out[2]), "a zero normal gives no direction");
   }

   // ---- the distribution's sample: 4 096 cosine-branch directions about one normal, under a fixed seed
   {
      const float n[3] = {0.48f, -0.6f, 0.64f}, d[3] = {0.0f, 0.0f, -1.0f};
      for (unsigned i = 0; i < 4096; ++i) {
         float out[3];
         path_scatter_at(d, n, 1.0f, 20261020u, i, 0u, 0u, out);
         printf("C %08x %08x %08x\n", bits(out[0]), bits(out[1]), bits(out[2]));
      }
   }

   // ---- which rays are traced: rs_shade_ray_valid's edges, and the bounces
   const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
   const float snan = from_bits(0x7fa00000u), denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
   EXPECT(MDH_RS_SHADE_EXTENT == 1024.0f && MDH_RS_SHADE_DIR == 2.0f && MDH_PATH_MAX_BOUNCES == 6, "the bound the derivation was made for");
   EXPECT(5322 + MDH_PATH_MAX_BOUNCES * 1025 + 1774 < 16384, "the derivation");
   EXPECT(path_ray_valid(0.0f, -0.0f, denorm, -denorm, 0.0f, 0.0f), "zeros and denormals are traced");
   EXPECT(!path_ray_valid(1.0f, 2.0f, 3.0f, 0.0f, -0.0f, 0.0f) && rs_shade_ray_valid(1.0f, 2.0f, 3.0f, 0.0f, -0.0f, 0.0f), "a zero direction is not, though it is inside the bound");
   EXPECT(path_ray_valid(1024.0f, -1024.0f, 1024.0f, 2.0f, -2.0f, 2.0f), "the bounds themselves are traced");
   for (int at = 0; at < 6; ++at) {
      const float edge = at < 3 ? 1024.0f : 2.0f;
      const float above = std::nextafter(edge, inf), below = std::nextafter(edge, 0.0f);
      EXPECT(with(at, edge) && with(at, -edge), "component %d at its bound", at);
      EXPECT(with(at, below) && with(at, -below), "component %d just inside", at);
      EXPECT(!with(at, above) && !with(at, -above), "component %d one float outside", at);
      EXPECT(with(at, denorm) && with(at, -denorm) && with(at, 0.0f) && with(at, -0.0f), "component %d tiny", at);
      EXPECT(!with(at, inf) && !with(at, -inf), "component %d infinite", at);
      EXPECT(!with(at, nan) && !with(at, -nan) && !with(at, snan), "component %d not a number", at);
      EXPECT(!with(at, big) && !with(at, -big), "component %d the largest float", at);
   }
   EXPECT(!with(3, 1024.0f) && !with(4, 3.0f) && with(0, 3.0f) && !with(1, 2000.0f), "each half has its own bound");
   EXPECT(path_bounces_valid(0) && path_bounces_valid(6) && !path_bounces_valid(7) && !path_bounces_valid(-1) && !path_bounces_valid(0x7fffffff), "bounces 0 .. 6");
   EXPECT(path_dir_finite(0.0f, -1.0f, denorm) && !path_dir_finite(nan, 0.0f, 0.0f) && !path_dir_finite(0.0f, inf, 0.0f) && !path_dir_finite(0.0f, 0.0f, -inf), "path_dir_finite");

   if (g_fail) { printf("path_sampler_check: %d failures\n", g_fail); return 1; }
   printf("path_sampler_check: ok\n");
   return 0;
}
