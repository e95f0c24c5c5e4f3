// examples/obj_mesh.cpp -- the reference program examples/obj_mesh/main.adb:30-75,139-169 restated with the C++
// mirror: 1000 triangles behind a 30x20x20 partition of 0.1 cells built with GPU_Fast, one point light, the default
// probes.  There is no mesh loader: a torus of 25 x 20 quads (exactly 1000 triangles) stands for media/suzanne.obj.
// The scene's table does not fit a workgroup's LDS: the library reads its geometry from device memory
// (MDH_OPT_TABLE_RESIDENCY reads 1).  Usage: obj_mesh [--bvh] W H FRAMES [out.f32 [out.ppm]]
// --bvh: the same mesh without the partition (Partitioning => (Enable => False)) and MDH_OPT_TRIANGLE_BVH on -- the exact
// scan over all 1000 triangles, walked through the library's bounding-volume hierarchy.
#include "madarch.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace Madarch;

// vertex (i, j) of the torus: ring radius R around the y axis, tube radius r (madarch_amd/meshes.py: torus, axis 1)
static Vector3 Torus_Vertex(int i, int j, int nu, int nv, double R, double r)
{
   const double u = 2.0 * M_PI * (i % nu) / nu, v = 2.0 * M_PI * (j % nv) / nv, ring = R + r * cos(v);
   return {(float)(ring * sin(u)), (float)(r * sin(v)), (float)(ring * cos(u))};
}

int main(int argc, char **argv)
{
   bool Triangle_BVH = false;
   for (int i = 1; i < argc; ++i)
      if (std::string(argv[i]) == "--bvh") { // (anywhere among the arguments; the others keep their order)
         Triangle_BVH = true;
         for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
         --argc; --i;
      }
   const int W = argc > 1 ? atoi(argv[1]) : 1000, H = argc > 2 ? atoi(argv[2]) : 1000, frames = argc > 3 ? atoi(argv[3]) : 1;
   try {
      Scenes::Partitioning_Settings Partitioning_Settings;
      Partitioning_Settings.Enable = !Triangle_BVH;
      Partitioning_Settings.Index_Count = 150;
      Partitioning_Settings.Border_Behavior = Scenes::Clamp;
      Partitioning_Settings.Grid_Dimensions = {30, 20, 20};
      Partitioning_Settings.Grid_Spacing = {0.1f, 0.1f, 0.1f};
      Partitioning_Settings.Grid_Offset = {0.0f, 0.0f, 0.0f};
      Scenes::Scene Scene = Scenes::Compile({{Primitives::Triangles::Triangle, 1000}}, {{Lights::Point_Lights::Point_Light, 4}}, Partitioning_Settings);
      Renderers::Renderer Renderer = Renderers::Create(Windows::Open(W, H, "Obj_Mesh"), Scene, {}, Renderers::No_Volumetrics);
      if (Triangle_BVH) Renderer.Set_Option(Renderers::Renderer::Opt_Triangle_BVH, 1);
      Entities::Entity Point_Light_Instance = Lights::Point_Lights::Create({0.0f, 1.0f, -5.0f}, {0.9f, 0.9f, 0.9f});
      Materials::Id Mesh_Mat = Renderer.Add_Material(Materials::Create({0.8f, 0.2f, 0.1f}, 0.0f, 1.0f));

      const Vector3 Suzanne_Offset = {1.5f, 1.0f, 1.0f};
      auto Add_Triangle = [&](Vector3 A, Vector3 B, Vector3 C) { // main.adb:142-153
         for (int a = 0; a < 3; ++a) { A[a] += Suzanne_Offset[a]; B[a] += Suzanne_Offset[a]; C[a] += Suzanne_Offset[a]; }
         Renderer.Add_Primitive(Primitives::Triangles::Triangle, Primitives::Triangles::Create(A, B, C, Mesh_Mat));
      };
      const int nu = 25, nv = 20;
      for (int i = 0; i < nu; ++i)
         for (int j = 0; j < nv; ++j) {
            const Vector3 a = Torus_Vertex(i, j, nu, nv, 0.6, 0.25), b = Torus_Vertex(i + 1, j, nu, nv, 0.6, 0.25),
                          c = Torus_Vertex(i + 1, j + 1, nu, nv, 0.6, 0.25), d = Torus_Vertex(i, j + 1, nu, nv, 0.6, 0.25);
            Add_Triangle(a, b, c);
            Add_Triangle(a, c, d);
         }
      if (!Triangle_BVH) Renderer.Update_Partitioning(Renderers::GPU_Fast);
      Renderer.Set_Light(1, Lights::Point_Lights::Point_Light, Point_Light_Instance);
      Renderer.Set_Camera_Position({0.0f, 1.0f, -5.0f});

      for (int f = 0; f < frames; ++f) {
         Renderer.Render();
         Renderer.Swap_Buffers();
      }
      std::vector<float> image = Renderer.Read_Framebuffer();
      if (argc > 4) {
         FILE *out = fopen(argv[4], "wb");
         if (!out) return 2;
         fwrite(image.data(), sizeof(float), image.size(), out);
         fclose(out);
      }
      if (argc > 5) { // the window's pixels of the last frame as a binary PPM
         const uint8_t *px = Renderer.Front_Buffer();
         FILE *out = fopen(argv[5], "wb");
         if (!out) return 2;
         fprintf(out, "P6\n%d %d\n255\n", W, H);
         for (size_t i = 0; i < (size_t)W * H; ++i) fwrite(px + 4 * i, 1, 3, out);
         fclose(out);
      }
      double sum = 0;
      for (float v : image) sum += (v == v) ? v : 0;
      printf("obj_mesh %dx%d frames %d mean %.6f\n", W, H, frames, sum / image.size());
   } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return 1;
   }
   return 0;
}
