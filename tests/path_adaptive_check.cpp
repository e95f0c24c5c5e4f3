// path_adaptive_check -- the moments and the stopping rule of an adaptive path-traced frame (csrc/mdh_path.h: path_pixel_update,
// path_pixel_active) as a stand-alone program on the CPU, built with -ffp-contract=off under the address and undefined-behaviour
// sanitizers and run directly by tests/test_path_adaptive_host.py.  It checks what needs no second opinion -- the order of the
// rule's early exits, that a NaN retires, that constant samples have exactly zero variance -- and prints states and verdicts
// for the numpy restatement of tests/path_adaptive_cases.py and for the library's mdh_path_pixel_active:
//    U  r g b  n m1 m2  ->  n m1 m2           one update (floats as bits in hex)
//    A  n m1 m2 min max tolerance floor  active
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mdh_path.h"

static unsigned bits(float x)
{
   unsigned b;
   memcpy(&b, &x, 4);
   return b;
}
static float from_bits(unsigned b)
{
   float x;
   memcpy(&x, &b, 4);
   return x;
}
static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static unsigned lcg_state = 20261021u;
static unsigned lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }
static float uniform() { return (float)(lcg() >> 8) * 0x1p-24f; }

static bool rule(int n, float m1, float m2, int lo, int hi, float tol, float floor)
{
   const bool active = path_pixel_active(n, m1, m2, lo, hi, tol, floor);
   printf("A %d %08x %08x %d %d %08x %08x %d\n", n, bits(m1), bits(m2), lo, hi, bits(tol), bits(floor), active ? 1 : 0);
   return active;
}

int main()
{
   const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
   const float tols[] = {0.0f, 0.01f, 0.05f, 0.5f};
   const float floors[] = {0.0f, 0.01f, 1.0f};
   // states as the kernel forms them: up to 12 samples of radiance a pixel, of four kinds
   for (int pixel = 0; pixel < 160; ++pixel) {
      const int kind = pixel & 3; // 0: noisy, 1: constant (zero variance), 2: nearly constant, 3: mostly black with fireflies
      const float base = 0.05f + 3.0f * uniform();
      int n = 0;
      float m1 = 0.0f, m2 = 0.0f;
      const int samples = 1 + (int)(lcg() % 12u);
      for (int s = 0; s < samples; ++s) {
         float r, g, b;
         if (kind == 0) { r = 2.0f * uniform(); g = 2.0f * uniform(); b = 2.0f * uniform(); }
         else if (kind == 1) { r = base; g = 0.5f * base; b = 0.25f * base; }
         else if (kind == 2) { r = base + 1e-4f * uniform(); g = base; b = base; }
         else { r = g = b = uniform() < 0.2f ? 40.0f * uniform() : 0.0f; }
         const int n0 = n;
         const float a1 = m1, a2 = m2;
         path_pixel_update(r, g, b, n, m1, m2);
         printf("U %08x %08x %08x %d %08x %08x %d %08x %08x\n", bits(r), bits(g), bits(b), n0, bits(a1), bits(a2), n, bits(m1), bits(m2));
         EXPECT(n == n0 + 1, "the count advances by one");
         const int lo = 1 + (int)(lcg() % 4u), hi = lo + (int)(lcg() % 10u);
         const float tol = tols[lcg() % 4u], floor = floors[lcg() % 3u];
         const bool active = rule(n, m1, m2, lo, hi, tol, floor);
         if (n >= hi) EXPECT(!active, "n = %d >= max = %d stays active", n, hi);
         else if (n < lo) EXPECT(active, "n = %d < min = %d retires", n, lo);
         if (kind == 1 && n >= lo && n <= 2) EXPECT(!active, "constant samples, n = %d: y + y and y y + y y are exact, the variance is exactly 0", n);
      }
   }
   // the edges: n < min, n = max, min = max, NaN and infinite moments, tolerance 0
   const float m1s[] = {0.0f, 1.0f, 3.5f, 1e30f, inf, -inf, nan, from_bits(0x7fc00000u), -2.0f, 1e-30f};
   const float m2s[] = {0.0f, 1.0f, 7.0f, 1e30f, inf, nan, from_bits(0x7fc00000u), 3.0625f, 1e-38f};
   const int counts[] = {0, 1, 2, 3, 4, 7, 8, 16777216};
   const int ranges[][2] = {{1, 1}, {1, 8}, {2, 8}, {4, 4}, {8, 8}, {3, 16777216}, {16777216, 16777216}};
   for (float m1 : m1s)
      for (float m2 : m2s)
         for (int n : counts)
            for (const auto &range : ranges)
               for (float tol : {0.0f, 0.05f}) {
                  const bool active = rule(n, m1, m2, range[0], range[1], tol, 0.01f);
                  if (n >= range[1] || m1 != m1 || m2 != m2) EXPECT(!active, "n = %d of %d .. %d, moments %08x %08x stays active", n, range[0], range[1], bits(m1), bits(m2));
                  else if (n < range[0]) EXPECT(active, "n = %d below min = %d retires", n, range[0]);
               }
   // the quiet NaN of a pixel that was not traced retires at n = 0, whatever min_samples is
   EXPECT(!path_pixel_active(0, from_bits(0x7fc00000u), from_bits(0x7fc00000u), 2, 8, 0.0f, 0.0f), "an untraced pixel stays active");
   // tolerance 0: exactly zero variance retires at min_samples, any positive one runs to max_samples
   EXPECT(!path_pixel_active(2, 2.0f, 2.0f, 2, 6, 0.0f, 0.0f), "zero variance at min_samples");
   EXPECT(path_pixel_active(2, 2.0f, 2.5f, 2, 6, 0.0f, 0.0f) && path_pixel_active(5, 5.0f, 5.5f, 2, 6, 0.0f, 0.0f) && !path_pixel_active(6, 6.0f, 6.5f, 2, 6, 0.0f, 0.0f),
          "positive variance under tolerance 0 runs to max_samples");
   EXPECT(path_adaptive_valid(1, 1, 0.0f, 0.0f) && path_adaptive_valid(2, 16777216, 0.5f, 1.0f) && !path_adaptive_valid(0, 4, 0.1f, 0.1f) && !path_adaptive_valid(5, 4, 0.1f, 0.1f) &&
          !path_adaptive_valid(1, 16777217, 0.1f, 0.1f) && !path_adaptive_valid(1, 4, -0.1f, 0.1f) && !path_adaptive_valid(1, 4, 0.1f, -1.0f) && !path_adaptive_valid(1, 4, nan, 0.1f) &&
          !path_adaptive_valid(1, 4, 0.1f, inf), "path_adaptive_valid");
   if (failures) { printf("path_adaptive_check: %d FAILED\n", failures); return 1; }
   printf("path_adaptive_check: ok\n");
   return 0;
}
