// shade_rays_check.cpp -- the predicate that decides which rays mdh_shade_rays and mdh_shade_rays_device shade
// (madarch_amd/csrc/mdh_ray_stream.h: rs_shade_ray_valid, rs_shade_extent_valid) at its edge values, on the CPU.  The header is
// the one the kernels include and the host's checks call; tests/test_shade_rays_host.py builds this program with the address
// and undefined-behaviour sanitizers and runs it.
#include "mdh_ray_stream.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static float from_bits(unsigned u)
{
   float f;
   memcpy(&f, &u, 4);
   return f;
}

// a ray that is shaded, with component `at` (0 .. 2 the origin, 3 .. 5 the direction) replaced
static bool with(int at, float value)
{
   float v[6] = {1.0f, -2.0f, 3.0f, 0.0f, 0.6f, -0.8f};
   v[at] = value;
   return rs_shade_ray_valid(v[0], v[1], v[2], v[3], v[4], v[5]);
}

int main()
{
   const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
   const float snan = from_bits(0x7fa00000u), denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
   const float above_1024 = std::nextafter(1024.0f, inf), below_1024 = std::nextafter(1024.0f, 0.0f);
   const float above_2 = std::nextafter(2.0f, inf), below_2 = std::nextafter(2.0f, 0.0f);
   EXPECT(MDH_RS_SHADE_EXTENT == 1024.0f && MDH_RS_SHADE_DIR == 2.0f, "the bound the derivation was made for");
   EXPECT(above_1024 > 1024.0f && from_bits(0x44800001u) == above_1024, "the next float above 1024");

   EXPECT(rs_shade_ray_valid(0.0f, -0.0f, denorm, -denorm, 0.0f, 0.0f), "zeros, denormals and a zero direction are shaded");
   EXPECT(rs_shade_ray_valid(1024.0f, -1024.0f, 1024.0f, 2.0f, -2.0f, 2.0f), "the bounds themselves are shaded");
   for (int at = 0; at < 6; ++at) {
      const bool org = at < 3;
      const float edge = org ? 1024.0f : 2.0f, above = org ? above_1024 : above_2, below = org ? below_1024 : below_2;
      EXPECT(with(at, edge) && with(at, -edge), "component %d at its bound", at);
      EXPECT(with(at, below) && with(at, -below), "component %d just inside", at);
      EXPECT(!with(at, above) && !with(at, -above), "component %d one float outside", at);
      EXPECT(with(at, denorm) && with(at, -denorm) && with(at, 0.0f) && with(at, -0.0f), "component %d tiny", at);
      EXPECT(!with(at, inf) && !with(at, -inf), "component %d infinite", at);
      EXPECT(!with(at, nan) && !with(at, -nan) && !with(at, snan), "component %d not a number", at);
      EXPECT(!with(at, big) && !with(at, -big), "component %d the largest float", at);
   }
   // a direction may be as long as an origin may not, and the other way round
   EXPECT(!with(3, 1024.0f) && !with(4, 3.0f) && with(0, 3.0f) && !with(1, 2000.0f), "each half has its own bound");

   // the scene's half: max_dist, a light's coordinate, the probe grid's far corner
   EXPECT(rs_shade_extent_valid(20.0f) && rs_shade_extent_valid(1024.0f) && rs_shade_extent_valid(-1024.0f) && rs_shade_extent_valid(0.0f) && rs_shade_extent_valid(denorm), "inside");
   EXPECT(!rs_shade_extent_valid(above_1024) && !rs_shade_extent_valid(-above_1024) && !rs_shade_extent_valid(4096.0f) && !rs_shade_extent_valid(5000.0f), "outside");
   EXPECT(!rs_shade_extent_valid(inf) && !rs_shade_extent_valid(-inf) && !rs_shade_extent_valid(nan) && !rs_shade_extent_valid(1.0e10f), "not finite, or far");

   // what is shaded is marched by the other queries too: the shading predicate implies rs_ray_valid
   EXPECT(rs_ray_valid(1024.0f, -1024.0f, 0.0f, 2.0f, -2.0f, denorm), "a shaded ray is a finite ray");
   EXPECT(rs_within(1.0f, 1.0f) && !rs_within(std::nextafter(1.0f, 2.0f), 1.0f) && !rs_within(nan, inf) && !rs_within(inf, inf), "rs_within");

   if (g_fail) { printf("shade_rays_check: %d failures\n", g_fail); return 1; }
   printf("shade_rays_check: ok\n");
   return 0;
}
