// examples/fisheye.cpp -- a fisheye view of the global_illumination room: the scene of examples/global_illumination.cpp,
// a few frames so that the probes hold light, then the camera's own rays (Renderer.Camera_Rays) bent on the host into an
// equidistant projection of FOV degrees and shaded through the frame's pixel program (Renderer.Shade_Rays) -- what the
// pinhole camera of draw_screen.glsl:20-24 cannot show.  Usage: fisheye W H FRAMES [FOV [out.f32]]
#include "madarch.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace Madarch;

int main(int argc, char **argv)
{
   const int W = argc > 1 ? atoi(argv[1]) : 512, H = argc > 2 ? atoi(argv[2]) : 512, frames = argc > 3 ? atoi(argv[3]) : 8;
   const double fov = (argc > 4 ? atof(argv[4]) : 180.0) * 3.14159265358979 / 180.0;
   try {
      Scenes::Scene Scene = Scenes::Compile({{Primitives::Spheres::Sphere, 20}, {Primitives::Planes::Plane, 10}, {Primitives::Boxes::Box, 10}},
                                            {{Lights::Spot_Lights::Spot_Light, 4}}, Scenes::Partitioning_Settings{false});
      Windows::Window Window = Windows::Open(W, H, "Fisheye");
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

      for (int f = 0; f < frames; ++f) Renderer.Render(); // the probes gather light; the rays below see the last frame's atlases

      // the camera's rays, bent: this camera keeps its identity orientation, so u runs along x, v along y and it looks along z;
      // pixel (i, j) is at (u, v) = its origin minus the image's centre
      std::vector<float> Origins, Directions;
      Renderer.Camera_Rays(W, H, Origins, Directions);
      double centre[3] = {0, 0, 0};
      for (size_t q = 0; q < (size_t)W * H; ++q)
         for (int c = 0; c < 3; ++c) centre[c] += Origins[3 * q + c] / ((double)W * H);
      std::vector<bool> inside((size_t)W * H);
      for (size_t q = 0; q < (size_t)W * H; ++q) {
         const double u = Origins[3 * q] - centre[0], v = Origins[3 * q + 1] - centre[1], r = std::hypot(u, v);
         const double theta = r * 0.5 * fov, s = r > 1e-12 ? std::sin(theta) / r : 0.0;
         inside[q] = r <= 1.0;
         Directions[3 * q] = (float)(s * u); Directions[3 * q + 1] = (float)(s * v); Directions[3 * q + 2] = (float)std::cos(theta);
         for (int c = 0; c < 3; ++c) Origins[3 * q + c] = (float)centre[c]; // one eye
      }
      Renderers::Renderer::Ray_Colours View = Renderer.Shade_Rays(Origins, Directions, 0, true);
      double sum = 0;
      size_t hits = 0;
      for (size_t q = 0; q < (size_t)W * H; ++q) {
         if (!inside[q]) View.Rgb[3 * q] = View.Rgb[3 * q + 1] = View.Rgb[3 * q + 2] = 0.0f; // outside the circle
         for (int c = 0; c < 3; ++c) sum += View.Rgb[3 * q + c] == View.Rgb[3 * q + c] ? View.Rgb[3 * q + c] : 0;
         hits += View.Hit[q] == 1;
      }
      if (argc > 5) {
         FILE *out = fopen(argv[5], "wb");
         if (!out) return 2;
         fwrite(View.Rgb.data(), sizeof(float), View.Rgb.size(), out);
         fclose(out);
      }
      printf("fisheye %dx%d frames %d fov %.0f hits %zu mean %.6f\n", W, H, frames, fov * 180.0 / 3.14159265358979, hits, sum / View.Rgb.size());
   } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }
   return 0;
}
