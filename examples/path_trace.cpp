// examples/path_trace.cpp -- the room of examples/global_illumination.cpp seen twice through the same camera rays: by the DDGI
// frame (FRAMES frames of probe feedback, then the pixel program along the frame's rays, linear) and by the path tracer
// (Renderer.Path_Trace: SAMPLES samples a pixel in slices of SLICE, BOUNCES bounces), the ground truth the probes approximate.
// Prints the mean absolute difference between the two linear images, per channel and over the pixels whose ray hits the scene:
// a number to look at, held against nothing.  Then the same view as a path-traced FRAME: the renderer's own accumulator
// (Path_Frame_Begin, Path_Frame_Accumulate in the same slices, Path_Frame_Read) -- no rays fetched, the sums stay on the device,
// the resolve runs there.  Without --jitter its sums are the first image's bit for bit (the program says how many pixels
// differ: none); with --jitter every sample goes through its own point of its pixel and the edges are anti-aliased.  out.ppm
// is the accumulator's image, the window's bytes as Path_Frame_Read hands them out.  With --adaptive TOLERANCE the accumulator is
// an adaptive one (Path_Frame_Begin_Adaptive: at least SLICE and at most SAMPLES samples a pixel, every slice a round for the pixels
// whose noise is still above the tolerance) and the program prints how many samples were taken instead of W H SAMPLES.
// Usage: path_trace [--jitter] [--adaptive TOLERANCE] W H [SAMPLES [BOUNCES [SEED [FRAMES [SLICE [out.ppm]]]]]]
#include "madarch.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace Madarch;

int main(int argc, char **argv)
{
   bool jitter = false, adaptive = false;
   float tolerance = 0.0f;
   { // --jitter and --adaptive TOLERANCE, wherever they stand
      int kept = 1;
      for (int q = 1; q < argc; ++q) {
         if (!strcmp(argv[q], "--jitter")) jitter = true;
         else if (!strcmp(argv[q], "--adaptive") && q + 1 < argc) { adaptive = true; tolerance = (float)atof(argv[++q]); }
         else argv[kept++] = argv[q];
      }
      argc = kept;
   }
   const int W = argc > 1 ? atoi(argv[1]) : 256, H = argc > 2 ? atoi(argv[2]) : 256;
   const int samples = argc > 3 ? atoi(argv[3]) : 64, bounces = argc > 4 ? atoi(argv[4]) : 3;
   const uint32_t seed = argc > 5 ? (uint32_t)strtoul(argv[5], nullptr, 10) : 1u;
   const int frames = argc > 6 ? atoi(argv[6]) : 16, slice = std::max(1, argc > 7 ? atoi(argv[7]) : 16);
   try {
      Scenes::Scene Scene = Scenes::Compile({{Primitives::Spheres::Sphere, 20}, {Primitives::Planes::Plane, 10}, {Primitives::Boxes::Box, 10}},
                                            {{Lights::Spot_Lights::Spot_Light, 4}}, Scenes::Partitioning_Settings{false});
      Windows::Window Window = Windows::Open(W, H, "Path_Trace");
      Renderers::Renderer Renderer = Renderers::Create(Window, Scene, {}, Renderers::No_Volumetrics, 0);
      Materials::Id Wall_Mat_1 = Renderer.Add_Material(Materials::Create({0.0f, 0.0f, 0.0f}, 0.0f, 0.6f));
      Materials::Id Wall_Mat_2 = Renderer.Add_Material(Materials::Create({1.0f, 0.0f, 0.0f}, 0.0f, 0.6f));
      Materials::Id Wall_Mat_3 = Renderer.Add_Material(Materials::Create({0.0f, 0.0f, 1.0f}, 0.0f, 0.6f));
      Materials::Id Sphere_Mat = Renderer.Add_Material(Materials::Create({0.1f, 0.1f, 0.1f}, 0.9f, 0.1f));
      Materials::Id Box_Mat = Renderer.Add_Material(Materials::Create({0.0f, 1.0f, 0.0f}, 0.8f, 0.3f));
      const Entities::Entity Planes[] = {
         Primitives::Planes::Create({0.0f, 1.0f, 0.0f}, 1.0f, Wall_Mat_1), Primitives::Planes::Create({0.0f, -1.0f, 0.0f}, 7.0f, Wall_Mat_1),
         Primitives::Planes::Create({1.0f, 0.0f, 0.0f}, 1.0f, Wall_Mat_2), Primitives::Planes::Create({-1.0f, 0.0f, 0.0f}, 7.0f, Wall_Mat_3),
         Primitives::Planes::Create({0.0f, 0.0f, 1.0f}, 6.0f, Wall_Mat_1), Primitives::Planes::Create({0.0f, 0.0f, -1.0f}, 7.0f, Wall_Mat_1)};
      for (auto &Plane : Planes) Renderer.Add_Primitive(Primitives::Planes::Plane, Plane);
      Renderer.Add_Primitive(Primitives::Spheres::Sphere, Primitives::Spheres::Create({3.0f, 4.0f, 3.0f}, 1.0f, Sphere_Mat));
      Renderer.Add_Primitive(Primitives::Boxes::Box, Primitives::Boxes::Create({3.0f, 0.0f, 4.0f}, {1.5f, 1.5f, 1.5f}, Box_Mat));
      Renderer.Set_Camera_Position({2.0f, 2.0f, 0.0f});
      Renderer.Set_Light(1, Lights::Spot_Lights::Spot_Light, Lights::Spot_Lights::Create({3.5f, 5.0f, 2.0f}, {1.0f, 0.0f, 0.0f}, 3.1415f / 4.0f, {0.9f, 0.9f, 0.8f}));

      for (int f = 0; f < frames; ++f) Renderer.Render();
      Renderer.Finish();
      std::vector<float> Origins, Directions;
      Renderer.Camera_Rays(W, H, Origins, Directions);
      const Renderers::Renderer::Ray_Colours Frame = Renderer.Shade_Rays(Origins, Directions, 0, false); // the frame's pixel program, linear
      Renderers::Renderer::Path_Colours Paths;
      for (int first = 0; first < samples; first += slice) // the sums go back in: any slicing, the same bits
         Paths = Renderer.Path_Trace(Origins, Directions, seed, 0, first, std::min(slice, samples - first), bounces, Paths.Rgb);

      double diff[3] = {0.0, 0.0, 0.0};
      size_t hits = 0;
      const size_t n = (size_t)W * H;
      for (size_t q = 0; q < n; ++q) {
         if (Paths.Hit[q] != 1) continue;
         ++hits;
         for (int c = 0; c < 3; ++c) diff[c] += std::fabs((double)Paths.Rgb[3 * q + c] / std::max(samples, 1) - (double)Frame.Rgb[3 * q + c]);
      }
      printf("path_trace %dx%d: %d samples, %d bounces, seed %u, %d frames of DDGI; %zu of %zu pixels hit\n", W, H, samples, bounces, seed, frames, hits, n);
      printf("mean |path traced - DDGI frame| over the hit pixels, linear: r %.6f g %.6f b %.6f\n", hits ? diff[0] / hits : 0.0, hits ? diff[1] / hits : 0.0,
             hits ? diff[2] / hits : 0.0);
      // the same view in the renderer's own accumulator
      if (adaptive && samples > 0) Renderer.Path_Frame_Begin_Adaptive(W, H, seed, bounces, jitter, std::min(slice, samples), samples, tolerance, 0.01f);
      else Renderer.Path_Frame_Begin(W, H, seed, bounces, jitter);
      for (int first = 0; first < samples; first += slice) Renderer.Path_Frame_Accumulate(std::min(slice, samples - first)); // (nothing waits)
      if (samples > 0) {
         const Renderers::Renderer::Path_Frame_Image Image = Renderer.Path_Frame_Read(true, false, true, true); // tone-mapped bytes and the raw sums
         size_t differ = 0;
         double moved = 0.0;
         for (size_t q = 0; q < 3 * n; ++q) {
            differ += memcmp(&Image.Sums[q], &Paths.Rgb[q], 4) != 0;
            moved += std::fabs((double)Image.Sums[q] - (double)Paths.Rgb[q]) / samples;
         }
         if (!adaptive)
            printf("path-traced frame, %s: %d samples in the accumulator; %zu of %zu sums differ from the rays' (mean |difference| %.6f)\n",
                   jitter ? "jittered" : "pixel centres", Image.Samples, differ, 3 * n, moved / (3.0 * n));
         if (adaptive) { // (every pixel has its own count: its sums are not the rays' sums over SAMPLES, and are not held against them)
            printf("path-traced frame, %s, adaptive: at most %d samples a pixel\n", jitter ? "jittered" : "pixel centres", Image.Samples);
            const Renderers::Renderer::Path_Frame_Statistics Stats = Renderer.Path_Frame_Stats(false, false);
            printf("adaptive, tolerance %g: %lld samples taken of %lld, %lld pixels still above the tolerance\n", (double)tolerance, (long long)Stats.Total_Samples,
                   (long long)n * samples, (long long)Stats.Active);
         }
         if (argc > 8) { // the window's bytes
            FILE *out = fopen(argv[8], "wb");
            if (!out) return 2;
            fprintf(out, "P6\n%d %d\n255\n", W, H);
            for (size_t q = 0; q < n; ++q)
               for (int c = 0; c < 3; ++c) fputc((int)((Image.Rgba8[q] >> (8 * c)) & 255u), out);
            fclose(out);
         }
      }
      Renderer.Path_Frame_End();
   } catch (const std::exception &e) {
      fprintf(stderr, "path_trace: %s\n", e.what());
      return 1;
   }
   return 0;
}
