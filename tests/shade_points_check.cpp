// shade_points_check.cpp -- the predicate that decides which points mdh_shade_points and mdh_shade_points_device shade
// (madarch_amd/csrc/mdh_ray_stream.h: rs_shade_point_valid) at its edge values, on the CPU.  The header is the one the
// kernels include and the host's check calls; tests/test_shade_points_host.py builds this program with the address and
// undefined-behaviour sanitizers and runs it.
#include "mdh_ray_stream.h"

#include <climits>
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

static const int TABLE = 20; // the renderer's material table

// a point that is shaded, with component `at` (0 .. 2 the position, 3 .. 5 the normal, 6 .. 8 the view direction) replaced
static bool with(int at, float value, int material = 3, int table = TABLE)
{
   float v[9] = {1.0f, -2.0f, 3.0f, 0.0f, 0.6f, -0.8f, 0.36f, -0.48f, 0.8f};
   v[at] = value;
   return rs_shade_point_valid(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], material, table);
}

int main()
{
   const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
   const float snan = from_bits(0x7fa00000u), denorm = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
   const float above_1024 = std::nextafter(1024.0f, inf), below_1024 = std::nextafter(1024.0f, 0.0f);
   const float above_1 = std::nextafter(1.0f, inf), below_1 = std::nextafter(1.0f, 0.0f);
   EXPECT(MDH_RS_SHADE_EXTENT == 1024.0f && MDH_RS_POINT_DIR == 1.0f, "the bound the derivation was made for");
   EXPECT(from_bits(0x44800001u) == above_1024 && from_bits(0x3f800001u) == above_1, "the next floats above the bounds");

   EXPECT(rs_shade_point_valid(0.0f, -0.0f, denorm, -denorm, 0.0f, 0.0f, 0.0f, -0.0f, denorm, 0, TABLE), "zeros, denormals, a zero normal and a zero view direction are shaded");
   EXPECT(rs_shade_point_valid(1024.0f, -1024.0f, 1024.0f, 1.0f, -1.0f, 1.0f, -1.0f, 1.0f, -1.0f, TABLE - 1, TABLE), "the bounds themselves are shaded");
   for (int at = 0; at < 9; ++at) {
      const bool pos = at < 3;
      const float edge = pos ? 1024.0f : 1.0f, above = pos ? above_1024 : above_1, below = pos ? below_1024 : below_1;
      EXPECT(with(at, edge) && with(at, -edge), "component %d at its bound", at);
      EXPECT(with(at, below) && with(at, -below), "component %d just inside", at);
      EXPECT(!with(at, above) && !with(at, -above), "component %d one float outside", at);
      EXPECT(with(at, denorm) && with(at, -denorm) && with(at, 0.0f) && with(at, -0.0f), "component %d tiny", at);
      EXPECT(!with(at, inf) && !with(at, -inf), "component %d infinite", at);
      EXPECT(!with(at, nan) && !with(at, -nan) && !with(at, snan), "component %d not a number", at);
      EXPECT(!with(at, big) && !with(at, -big), "component %d the largest float", at);
   }
   // a position may be as far as a normal may not be long; the 2 of a shaded ray's direction is outside
   EXPECT(!with(3, 1024.0f) && !with(7, 2.0f) && !with(4, 2.0f) && with(0, 2.0f) && !with(1, 2000.0f), "each part has its own bound");

   // the material id: inside the table
   EXPECT(with(0, 1.0f, 0) && with(0, 1.0f, TABLE - 1), "the table's first and last entry");
   EXPECT(!with(0, 1.0f, -1) && !with(0, 1.0f, TABLE) && !with(0, 1.0f, INT_MIN) && !with(0, 1.0f, INT_MAX), "-1, the table's size, the extremes");
   EXPECT(!with(0, 1.0f, 0, 0) && with(0, 1.0f, 0, 1) && !with(0, 1.0f, 1, 1), "an empty table names nothing; mode 3 passes id 0 of a table of 1");

   // what is shaded as a point is finite as a ray
   EXPECT(rs_ray_valid(1024.0f, -1024.0f, 0.0f, 1.0f, -1.0f, denorm), "a shaded point is finite");

   if (g_fail) { printf("shade_points_check: %d failures\n", g_fail); return 1; }
   printf("shade_points_check: ok\n");
   return 0;
}
