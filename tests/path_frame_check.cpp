// path_frame_check -- the screen positions of a path-traced frame's pixels (csrc/mdh_path.h: path_pixel_uv) as a stand-alone
// program on the CPU, built with -ffp-contract=off under the address and undefined-behaviour sanitizers and run directly by
// tests/test_path_frame_host.py.  It checks what needs no second opinion -- without jitter the pixel's centre bit for bit, with
// jitter a position inside the pixel's footprint, the mean offset of 4 096 samples of one pixel -- and prints the positions'
// bits for the numpy restatement of tests/path_frame_cases.py:
//    P  width height seed sample jitter i j  u v      (bits in hex)
//    M  mean offset along x and along y in units of the pixel's half-width (decimal)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mdh_path.h"

static unsigned bits(float x)
{
   unsigned b;
   memcpy(&b, &x, 4);
   return b;
}
static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void pixel(int W, int H, unsigned seed, int sample, int i, int j)
{
   // the centre as mdh_camera_rays forms it
   const float cu = (float)(2 * i + 1) / (float)W - 1.0f, cv = -((float)(2 * j + 1) / (float)H - 1.0f);
   for (int jitter = 0; jitter < 2; ++jitter) {
      float u = 7.0f, v = 7.0f;
      path_pixel_uv(i, j, W, H, seed, (unsigned)sample, jitter != 0, u, v);
      printf("P %d %d %u %d %d %d %d %08x %08x\n", W, H, seed, sample, jitter, i, j, bits(u), bits(v));
      if (!jitter) {
         EXPECT(bits(u) == bits(cu) && bits(v) == bits(cv), "%d x %d pixel (%d, %d): not the centre", W, H, i, j);
         // ... which is the issue's own formula where 2 i + 1 is exact
         const float fu = ((float)(2 * i) + 2.0f * 0.5f) / (float)W - 1.0f, fv = -(((float)(2 * j) + 2.0f * 0.5f) / (float)H - 1.0f);
         EXPECT(bits(u) == bits(fu) && bits(v) == bits(fv), "%d x %d pixel (%d, %d): not the jitter formula at 0.5", W, H, i, j);
      } else {
         EXPECT(std::fabs((double)u - (double)cu) <= 1.0 / W, "%d x %d pixel (%d, %d): u leaves the footprint", W, H, i, j);
         EXPECT(std::fabs((double)v - (double)cv) <= 1.0 / H, "%d x %d pixel (%d, %d): v leaves the footprint", W, H, i, j);
         EXPECT(u >= -1.0f && u <= 1.0f && v >= -1.0f && v <= 1.0f, "%d x %d pixel (%d, %d): outside the screen", W, H, i, j);
      }
   }
}

int main()
{
   const unsigned seeds[] = {20261020u, 1u};
   const int samples[] = {0, 1, 5};
   const int sizes[][2] = {{1, 1}, {3, 2}, {20, 12}};
   for (unsigned seed : seeds)
      for (int sample : samples) {
         for (const auto &wh : sizes)
            for (int j = 0; j < wh[1]; ++j)
               for (int i = 0; i < wh[0]; ++i) pixel(wh[0], wh[1], seed, sample, i, j);
         const int W = 1920, H = 1080;
         pixel(W, H, seed, sample, 0, 0); pixel(W, H, seed, sample, W - 1, 0); pixel(W, H, seed, sample, 0, H - 1); pixel(W, H, seed, sample, W - 1, H - 1);
      }
   // 4 096 samples of one pixel: uniform on [-1, 1] in units of the half-width has mean 0 and variance 1 / 3
   {
      const int W = 20, H = 12, i = 7, j = 5, n = 4096;
      const double cu = (2.0 * i + 1.0) / W - 1.0, cv = -((2.0 * j + 1.0) / H - 1.0);
      double mx = 0.0, my = 0.0;
      std::vector<float> us(n);
      for (int s = 0; s < n; ++s) {
         float u, v;
         path_pixel_uv(i, j, W, H, 20261020u, (unsigned)s, true, u, v);
         us[s] = u;
         mx += ((double)u - cu) * W; my += ((double)v - cv) * H;
      }
      mx /= n; my /= n;
      printf("M %.9f %.9f\n", mx, my);
      const double bound = 6.0 / std::sqrt(3.0 * n);
      EXPECT(std::fabs(mx) <= bound && std::fabs(my) <= bound, "mean offsets %.5f, %.5f beyond %.5f", mx, my, bound);
      int distinct = 0;
      for (int s = 1; s < n; ++s) distinct += us[s] != us[s - 1];
      EXPECT(distinct > n * 99 / 100, "the samples of a pixel repeat");
   }
   EXPECT(path_frame_size_valid(1, 1) && path_frame_size_valid(8192, 8192) && !path_frame_size_valid(8193, 8192) && !path_frame_size_valid(0, 5) && !path_frame_size_valid(5, -1) &&
          !path_frame_size_valid(1 << 30, 1 << 30), "path_frame_size_valid");
   if (failures) { printf("path_frame_check: %d FAILED\n", failures); return 1; }
   printf("path_frame_check: ok\n");
   return 0;
}
