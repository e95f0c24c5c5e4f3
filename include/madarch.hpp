// madarch.hpp -- C++ host-side mirror of Madarch's Ada packages over the C ABI of
// madarch_hip.h (header only).
//
// The reference's host language is Ada (no Ada toolchain exists in this pipeline), so the
// host side above the C ABI is restated in C++ package for package, with the Ada names:
//   Madarch::Values, Components, Entities, Materials, Primitives::{Spheres, Planes, Boxes,
//   Triangles}, Lights::{Point_Lights, Spot_Lights}, GPU_Types, Scenes, Windows, Renderers.
// Reference files: madarch/madarch-*.ads, madarch/support/gpu_types-*.adb (cited per item).
// Ada exceptions map to Program_Error / Constraint_Error below.  examples/*.cpp restate the
// three example programs with it; madarch_amd/ is the same mirror in Python.
#pragma once

#include "madarch_hip.h"

#include <cstdlib>
#include <algorithm>
#include <sys/stat.h>
#include <atomic>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace Madarch {

struct Program_Error : std::runtime_error { using std::runtime_error::runtime_error; };
struct Constraint_Error : std::runtime_error { using std::runtime_error::runtime_error; };

using Single = float;  // GL.Types.Single
using Int = int32_t;   // GL.Types.Int
using Vector3 = std::array<Single, 3>;                 // Singles.Vector3
using Matrix3 = std::array<std::array<Single, 3>, 3>;  // Singles.Matrix3, [row][column]

// ---------------------------------------------------------------- madarch-values.ads:8-27
namespace Values {
enum Value_Kind { Vector3_Kind = 0, Float_Kind = 1, Int_Kind = 2 };
struct Value {
   Value_Kind Kind = Float_Kind;
   Vector3 Vector3_Value{};
   Single Float_Value = 0;
   Int Int_Value = 0;
};
inline Value Vector3(const Madarch::Vector3 &x) { Value v; v.Kind = Vector3_Kind; v.Vector3_Value = x; return v; }
inline Value Float(Single x) { Value v; v.Kind = Float_Kind; v.Float_Value = x; return v; }
inline Value Int(Madarch::Int x) { Value v; v.Kind = Int_Kind; v.Int_Value = x; return v; }
} // namespace Values

// ------------------------------------------------------------- madarch-components.ads
namespace Components {
struct Component_Internal { std::string Name; Values::Value_Kind Kind; };
using Component = std::shared_ptr<const Component_Internal>; // compared by identity, as the access type is
inline Component Create(const std::string &Name, Values::Value_Kind Kind) { return std::make_shared<Component_Internal>(Component_Internal{Name, Kind}); }
inline const std::string &Get_Name(const Component &C) { return C->Name; }
inline Values::Value_Kind Get_Kind(const Component &C) { return C->Kind; }
using Component_Array = std::vector<Component>;
} // namespace Components

// ------------------------------------------------------------- madarch-entities.adb:2-43
namespace Entities {
class Entity {
 public:
   using Item = std::pair<Components::Component, Values::Value>;
   Entity() = default;
   explicit Entity(std::vector<Item> values) : values_(std::make_shared<std::vector<Item>>(std::move(values))) {}
   Values::Value Get(const Components::Component &Comp) const
   {
      for (auto &cv : *values_)
         if (cv.first == Comp) return cv.second;
      throw Program_Error("Entity does not have given component.");
   }
   void Set(const Components::Component &Comp, const Values::Value &V)
   {
      for (auto &cv : *values_)
         if (cv.first == Comp) { cv.second = V; return; }
      throw Program_Error("Entity does not have given component.");
   }
   void Foreach(const std::function<void(const Components::Component &, const Values::Value &)> &Proc) const
   {
      for (auto &cv : *values_) Proc(cv.first, cv.second);
   }
 private:
   std::shared_ptr<std::vector<Item>> values_; // reference semantics, as the Ada access type
};
inline Entity Create(std::vector<Entity::Item> Values) { return Entity(std::move(Values)); }
} // namespace Entities

// ------------------------- support/gpu_types-base.ads:21-37, -structs.adb:11-38, -fixed_arrays.adb:17-39
namespace GPU_Types {
inline int Pad(int x, int amount) { while (x % amount) ++x; return x; }
inline int Alignment(Values::Value_Kind k) { return k == Values::Vector3_Kind ? 16 : 4; }
inline int Size(Values::Value_Kind k) { return k == Values::Vector3_Kind ? 12 : 4; }
// std140 struct of an entity kind (Compute_Prim_Struct_Type, madarch-scenes.adb:1272-1288)
struct Struct {
   Components::Component_Array Comps;
   int Size_Bytes() const
   {
      int total = 0;
      for (auto &c : Comps) total = Pad(total, Alignment(c->Kind)) + Size(c->Kind);
      return total;
   }
   int Offset_Of(const Components::Component &Comp) const
   {
      int off = 0;
      for (auto &c : Comps) {
         off = Pad(off, Alignment(c->Kind));
         if (c == Comp) return off;
         off += Size(c->Kind);
      }
      throw Program_Error("Index out of bounds");
   }
   int Stride() const { return Pad(Size_Bytes(), 16); }
};
// Write_Entity + Write_Value (madarch-renderers.adb:323-347) into one element image
inline std::vector<uint8_t> Element_Blob(const Struct &S, const Entities::Entity &Ent)
{
   std::vector<uint8_t> blob((size_t)S.Size_Bytes(), 0);
   Ent.Foreach([&](const Components::Component &c, const Values::Value &v) {
      int off = S.Offset_Of(c);
      if (v.Kind == Values::Vector3_Kind) std::memcpy(&blob[off], v.Vector3_Value.data(), 12);
      else if (v.Kind == Values::Float_Kind) std::memcpy(&blob[off], &v.Float_Value, 4);
      else std::memcpy(&blob[off], &v.Int_Value, 4);
   });
   return blob;
}
} // namespace GPU_Types

// ------------------------------------------------------------- madarch-materials.ads:10-25
namespace Materials {
using Id = Int;
inline const Components::Component Albedo = Components::Create("albedo", Values::Vector3_Kind);
inline const Components::Component Metallic = Components::Create("metallic", Values::Float_Kind);
inline const Components::Component Roughness = Components::Create("roughness", Values::Float_Kind);
inline Entities::Entity Create(const Vector3 &Instance_Albedo, Single Instance_Metallic, Single Instance_Roughness)
{
   return Entities::Create({{Albedo, Values::Vector3(Instance_Albedo)}, {Metallic, Values::Float(Instance_Metallic)}, {Roughness, Values::Float(Instance_Roughness)}});
}
} // namespace Materials

// ------------------------------------------------------------- madarch-primitives.ads:13-60
// A primitive KIND = name + components; the distance/normal/material functions of the four
// built-in kinds are hand-written device code in libmadarch_hip (madarch_amd/csrc).
namespace Primitives {
struct Primitive_Internal { std::string Name; Components::Component_Array Comps; };
using Primitive = std::shared_ptr<const Primitive_Internal>;
inline Primitive Create(const std::string &Name, Components::Component_Array Comps) { return std::make_shared<Primitive_Internal>(Primitive_Internal{Name, std::move(Comps)}); }
inline const std::string &Get_Name(const Primitive &P) { return P->Name; }
using Primitive_Array = std::vector<Primitive>;

namespace Materials { // madarch-primitives-materials.ads:8
inline const Components::Component Material_Id = Components::Create("material_id", Values::Int_Kind);
}
namespace Spheres { // madarch-primitives-spheres.ads:10-33
inline const Components::Component Center = Components::Create("center", Values::Vector3_Kind);
inline const Components::Component Radius = Components::Create("radius", Values::Float_Kind);
inline const Primitive Sphere = Primitives::Create("Sphere", {Center, Radius, Materials::Material_Id});
inline Entities::Entity Create(const Vector3 &C, Single R, Int Material_Id)
{
   return Entities::Create({{Center, Values::Vector3(C)}, {Radius, Values::Float(R)}, {Materials::Material_Id, Values::Int(Material_Id)}});
}
} // namespace Spheres
namespace Planes { // madarch-primitives-planes.ads:10-33
inline const Components::Component Normal = Components::Create("normal", Values::Vector3_Kind);
inline const Components::Component Offset = Components::Create("offset", Values::Float_Kind);
inline const Primitive Plane = Primitives::Create("Plane", {Normal, Offset, Materials::Material_Id});
inline Entities::Entity Create(const Vector3 &N, Single O, Int Material_Id)
{
   return Entities::Create({{Normal, Values::Vector3(N)}, {Offset, Values::Float(O)}, {Materials::Material_Id, Values::Int(Material_Id)}});
}
} // namespace Planes
namespace Boxes { // madarch-primitives-boxes.ads:10-31
inline const Components::Component Center = Components::Create("center", Values::Vector3_Kind);
inline const Components::Component Side = Components::Create("side", Values::Vector3_Kind);
inline const Primitive Box = Primitives::Create("Box", {Center, Side, Materials::Material_Id});
inline Entities::Entity Create(const Vector3 &C, const Vector3 &S, Int Material_Id)
{
   return Entities::Create({{Center, Values::Vector3(C)}, {Side, Values::Vector3(S)}, {Materials::Material_Id, Values::Int(Material_Id)}});
}
} // namespace Boxes
namespace Triangles { // madarch-primitives-triangles.ads:10-35
inline const Components::Component V1 = Components::Create("v1", Values::Vector3_Kind);
inline const Components::Component V2 = Components::Create("v2", Values::Vector3_Kind);
inline const Components::Component V3 = Components::Create("v3", Values::Vector3_Kind);
inline const Primitive Triangle = Primitives::Create("Triangle", {V1, V2, V3, Materials::Material_Id});
inline Entities::Entity Create(const Vector3 &A, const Vector3 &B, const Vector3 &C, Int Material_Id)
{
   return Entities::Create({{V1, Values::Vector3(A)}, {V2, Values::Vector3(B)}, {V3, Values::Vector3(C)}, {Materials::Material_Id, Values::Int(Material_Id)}});
}
} // namespace Triangles
} // namespace Primitives

// ------------------------------------------------------------- madarch-lights.ads:7-37
namespace Lights {
struct Light_Internal { std::string Name; Components::Component_Array Comps; };
using Light = std::shared_ptr<const Light_Internal>;
inline Light Create(const std::string &Name, Components::Component_Array Comps) { return std::make_shared<Light_Internal>(Light_Internal{Name, std::move(Comps)}); }
namespace Point_Lights { // madarch-lights-point_lights.ads:14-35
inline const Components::Component Position = Components::Create("position", Values::Vector3_Kind);
inline const Components::Component Color = Components::Create("color", Values::Vector3_Kind);
inline const Light Point_Light = Lights::Create("PointLight", {Position, Color});
inline Entities::Entity Create(const Vector3 &P, const Vector3 &C) { return Entities::Create({{Position, Values::Vector3(P)}, {Color, Values::Vector3(C)}}); }
} // namespace Point_Lights
namespace Spot_Lights { // madarch-lights-spot_lights.ads:14-41
inline const Components::Component Position = Components::Create("position", Values::Vector3_Kind);
inline const Components::Component Direction = Components::Create("direction", Values::Vector3_Kind);
inline const Components::Component Aperture = Components::Create("aperture", Values::Float_Kind);
inline const Components::Component Color = Components::Create("color", Values::Vector3_Kind);
inline const Light Spot_Light = Lights::Create("SpotLight", {Position, Direction, Aperture, Color});
inline Entities::Entity Create(const Vector3 &P, const Vector3 &D, Single A, const Vector3 &C)
{
   return Entities::Create({{Position, Values::Vector3(P)}, {Direction, Values::Vector3(D)}, {Aperture, Values::Float(A)}, {Color, Values::Vector3(C)}});
}
} // namespace Spot_Lights
} // namespace Lights

// ------------------------------------------------------------- madarch-scenes.ads:13-76
namespace Scenes {
enum Partitioning_Border_Behavior { Clamp = 0, Fallback = 1 };
enum Codegen_Loop_Strategy { Split = 0, Unify = 1 };
struct Partitioning_Settings { // scenes.ads:30-41
   bool Enable = true;
   int Index_Count = 20;
   Partitioning_Border_Behavior Border_Behavior = Clamp;
   std::array<Int, 3> Grid_Dimensions{10, 10, 20};
   Vector3 Grid_Spacing{1.0f, 1.0f, 1.0f};
   Vector3 Grid_Offset{-1.5f, -1.5f, -10.0f};
};
struct Primitive_Count { Primitives::Primitive Prim; int Count; };
struct Light_Count { Lights::Light Light; int Count; };

struct Scene_Internal {
   std::vector<Primitive_Count> Prims;
   std::vector<Light_Count> Lits;
   Partitioning_Settings Partitioning_Config;
   Single Max_Dist;
   Codegen_Loop_Strategy Loop_Strategy;
   int Kind_Index(const Primitives::Primitive &P) const
   {
      for (size_t i = 0; i < Prims.size(); ++i)
         if (Prims[i].Prim == P) return (int)i;
      throw Program_Error("primitive kind is not part of the scene");
   }
   int Kind_Index(const Lights::Light &L) const
   {
      for (size_t i = 0; i < Lits.size(); ++i)
         if (Lits[i].Light == L) return (int)i;
      throw Program_Error("light kind is not part of the scene");
   }
};
using Scene = std::shared_ptr<const Scene_Internal>;
// Scenes.Compile (scenes.ads:47-53).  The reference emits GLSL here; this back end has the
// built-in kinds as device code, so a compiled scene is its description.
inline Scene Compile(std::vector<Primitive_Count> All_Primitives, std::vector<Light_Count> All_Lights,
                     Partitioning_Settings Partitioning = {}, Single Max_Dist = 20.0f, Codegen_Loop_Strategy Loop_Strategy = Unify)
{
   return std::make_shared<Scene_Internal>(Scene_Internal{std::move(All_Primitives), std::move(All_Lights), Partitioning, Max_Dist, Loop_Strategy});
}
} // namespace Scenes

// ------------------------------------------------------------- madarch-windows.ads:12-31 (headless)
namespace Windows {
struct Window { int Width = 0, Height = 0; std::string Title; };
inline Window Open(int Width, int Height, const std::string &Title = "") { return Window{Width, Height, Title}; }
} // namespace Windows

// ------------------------------------------------------------- madarch-renderers.ads:21-97
namespace Renderers {
struct Probe_Settings { // renderers.ads:23-29
   Int Radiance_Resolution = 32, Irradiance_Resolution = 8;
   std::array<Int, 2> Probe_Count{6, 6};
   std::array<Int, 3> Grid_Dimensions{4, 3, 3};
   Vector3 Grid_Spacing{2.0f, 3.0f, 3.0f};
};
struct Volumetrics_Settings { // renderers.ads:33-41
   bool Enabled = true;
   std::array<Int, 3> Visibility_Resolution{100, 100, 100};
   Single Visibility_Step_Size = 0.1f;
   std::array<Int, 2> Scattering_Resolution{250, 250};
   Single Scattering_Step_Size = 0.1f;
};
inline const Volumetrics_Settings No_Volumetrics{false, {100, 100, 100}, 0.1f, {250, 250}, 0.1f};
enum Partitioning_Update_Method { CPU_Best = 0, CPU_Fast = 1, GPU_Fast = 2 }; // renderers.ads:93

inline void Check(int32_t status)
{
   if (status == MDH_OK) return;
   if (status == MDH_E_INDEX) throw Constraint_Error(mdh_last_error());
   throw Program_Error(mdh_last_error());
}

class Renderer {
 public:
   Renderer() = default;
   Renderer(mdh_renderer *h, Windows::Window w, Scenes::Scene s) : h_(h, [](mdh_renderer *p) { mdh_destroy(p); }), window_(std::move(w)), scene_(std::move(s)) {}
   void Render() const { Check(mdh_render(h_.get())); Check(mdh_finish(h_.get())); } // renderers.adb:302-321
   void Set_Material(Materials::Id Index, const Entities::Entity &E) const // renderers.adb:349-367
   {
      Vector3 a = E.Get(Materials::Albedo).Vector3_Value;
      Check(mdh_set_material(h_.get(), Index, a.data(), E.Get(Materials::Metallic).Float_Value, E.Get(Materials::Roughness).Float_Value));
   }
   Materials::Id Add_Material(const Entities::Entity &E) const // renderers.adb:369-377
   {
      Vector3 a = E.Get(Materials::Albedo).Vector3_Value;
      int32_t id = -1;
      Check(mdh_add_material(h_.get(), a.data(), E.Get(Materials::Metallic).Float_Value, E.Get(Materials::Roughness).Float_Value, &id));
      return id;
   }
   void Set_Primitive(const Primitives::Primitive &Prim, int Index, const Entities::Entity &E) const // renderers.adb:379-398
   {
      auto blob = GPU_Types::Element_Blob(GPU_Types::Struct{Prim->Comps}, E);
      Check(mdh_set_primitive(h_.get(), scene_->Kind_Index(Prim), Index, blob.data(), (int32_t)blob.size()));
   }
   void Add_Primitive(const Primitives::Primitive &Prim, const Entities::Entity &E) const // renderers.adb:435-456
   {
      auto blob = GPU_Types::Element_Blob(GPU_Types::Struct{Prim->Comps}, E);
      Check(mdh_add_primitive(h_.get(), scene_->Kind_Index(Prim), blob.data(), (int32_t)blob.size(), nullptr));
   }
   void Set_Light(int Index, const Lights::Light &Lit, const Entities::Entity &E) const // renderers.adb:458-483
   {
      auto blob = GPU_Types::Element_Blob(GPU_Types::Struct{Lit->Comps}, E);
      Check(mdh_set_light(h_.get(), Index, scene_->Kind_Index(Lit), blob.data(), (int32_t)blob.size()));
   }
   void Set_Camera_Position(const Vector3 &P) const { Check(mdh_set_camera_position(h_.get(), P.data())); } // renderers.adb:485-490
   void Set_Camera_Orientation(const Matrix3 &M) const // renderers.adb:492-497; [row][column] -> column-major
   {
      float cm[9];
      for (int c = 0; c < 3; ++c)
         for (int r = 0; r < 3; ++r) cm[3 * c + r] = M[r][c];
      Check(mdh_set_camera_orientation(h_.get(), cm));
   }
   Single Eval_Distance_To(const Vector3 &Position, const Primitives::Primitive_Array &Prims, Vector3 &Normal) const // renderers.adb:499-526
   {
      std::vector<int32_t> kinds;
      for (auto &p : Prims) kinds.push_back(scene_->Kind_Index(p));
      float d = 0;
      Check(mdh_eval_distance_to(h_.get(), 1, Position.data(), kinds.data(), (int32_t)kinds.size(), Normal.data(), &d));
      return d;
   }
   // ---- ray queries (raymarching.glsl:4-56), batched on the device beside the frames in flight; they edit nothing.
   // Origins and Directions hold 3 floats a ray (directions as given, not normalised); scenes of built-in kinds only
   static size_t Ray_Count(const std::vector<float> &Origins, const std::vector<float> &Directions)
   {
      if (Origins.size() % 3 != 0 || Directions.size() != Origins.size()) throw Constraint_Error("origins and directions hold 3 floats a ray");
      return Origins.size() / 3;
   }
   struct Ray_Hits { std::vector<int32_t> Hit, Index, Steps; std::vector<float> T, Position, Normal; }; // Index as in the geometry buffer, -1 = miss
   Ray_Hits Raycast(const std::vector<float> &Origins, const std::vector<float> &Directions) const
   {
      const size_t n = Ray_Count(Origins, Directions);
      Ray_Hits o;
      o.Hit.resize(n); o.Index.resize(n); o.Steps.resize(n); o.T.resize(n); o.Position.resize(3 * n); o.Normal.resize(3 * n);
      Check(mdh_raycast(h_.get(), (int32_t)n, Origins.data(), Directions.data(), o.Hit.data(), o.Index.data(), o.T.data(), o.Steps.data(), o.Position.data(), o.Normal.data()));
      return o;
   }
   std::vector<float> Raycast_Visibility(const std::vector<float> &Origins, const std::vector<float> &Directions, const std::vector<float> &Max_Dists) const
   {
      const size_t n = Ray_Count(Origins, Directions);
      if (Max_Dists.size() != n) throw Constraint_Error("one length per ray");
      std::vector<float> vis(n);
      Check(mdh_raycast_visibility(h_.get(), (int32_t)n, Origins.data(), Directions.data(), Max_Dists.data(), vis.data()));
      return vis;
   }
   std::vector<float> Softshadows(const std::vector<float> &Origins, const std::vector<float> &Directions, Single Min_Dist, const std::vector<float> &Max_Dists, Single K) const
   {
      const size_t n = Ray_Count(Origins, Directions);
      if (Max_Dists.size() != n) throw Constraint_Error("one length per ray");
      std::vector<float> out(n);
      Check(mdh_softshadows(h_.get(), (int32_t)n, Origins.data(), Directions.data(), Min_Dist, Max_Dists.data(), K, out.data()));
      return out;
   }
   // ... and for arrays in memory the device addresses (N rays; every output of Raycast_Device but Hit may be null): asynchronous,
   // behind what Stream (a hipStream_t, null = the default stream) holds at the call; work given to Stream afterwards sees the
   // answers.  A ray that is not finite is not marched: Hit = -1 / NaN.  Ray_Query_Wait: the host's wait for all of them
   void Raycast_Device(int32_t N, const float *Origins, const float *Directions, int32_t *Hit, int32_t *Index = nullptr, float *T = nullptr, int32_t *Steps = nullptr,
                       float *Position = nullptr, float *Normal = nullptr, void *Stream = nullptr) const
   {
      Check(mdh_raycast_device(h_.get(), N, Origins, Directions, Hit, Index, T, Steps, Position, Normal, Stream));
   }
   void Raycast_Visibility_Device(int32_t N, const float *Origins, const float *Directions, const float *Max_Dists, float *Visibility, void *Stream = nullptr) const
   {
      Check(mdh_raycast_visibility_device(h_.get(), N, Origins, Directions, Max_Dists, Visibility, Stream));
   }
   void Softshadows_Device(int32_t N, const float *Origins, const float *Directions, Single Min_Dist, const float *Max_Dists, Single K, float *Out, void *Stream = nullptr) const
   {
      Check(mdh_softshadows_device(h_.get(), N, Origins, Directions, Min_Dist, Max_Dists, K, Out, Stream));
   }
   void Ray_Query_Wait() const { Check(mdh_ray_query_wait(h_.get())); }
   // ---- what a ray sees: pixel_color_probes (render_probes.glsl:246-291) along rays of the host's, through the screen pass's
   // pixel program.  Mode 0 (the fixed mode) or 2 (direct light times occlusion); linear colour, or with Tone_Map the
   // framebuffer's bits; a miss is the sky along the ray; never any fog.  Index, T, Steps as in the geometry buffer
   struct Ray_Colours { std::vector<float> Rgb, T; std::vector<int32_t> Hit, Index, Steps; };
   Ray_Colours Shade_Rays(const std::vector<float> &Origins, const std::vector<float> &Directions, int32_t Mode = 0, bool Tone_Map = false) const
   {
      const size_t n = Ray_Count(Origins, Directions);
      Ray_Colours o;
      o.Rgb.resize(3 * n); o.T.resize(n); o.Hit.resize(n); o.Index.resize(n); o.Steps.resize(n);
      Check(mdh_shade_rays(h_.get(), (int32_t)n, Origins.data(), Directions.data(), Mode, Tone_Map ? 1 : 0, o.Rgb.data(), o.Hit.data(), o.Index.data(), o.T.data(), o.Steps.data()));
      return o;
   }
   // ... for arrays in memory the device addresses, asynchronous and ordered with Stream as Raycast_Device is (every output but Rgb
   // may be null).  A ray that is not finite, starts beyond 1024 along an axis or has a direction component beyond 2: NaN, Hit = -1
   void Shade_Rays_Device(int32_t N, const float *Origins, const float *Directions, float *Rgb, int32_t *Hit = nullptr, int32_t *Index = nullptr, float *T = nullptr,
                          int32_t *Steps = nullptr, int32_t Mode = 0, bool Tone_Map = false, void *Stream = nullptr) const
   {
      Check(mdh_shade_rays_device(h_.get(), N, Origins, Directions, Mode, Tone_Map ? 1 : 0, Rgb, Hit, Index, T, Steps, Stream));
   }
   // the rays of a Width x Height frame of the current camera, rows top first, 3 floats a ray: the frame's rays to the bit
   void Camera_Rays(int32_t Width, int32_t Height, std::vector<float> &Origins, std::vector<float> &Directions) const
   {
      if (Width <= 0 || Height <= 0) throw Constraint_Error("a frame has at least one pixel");
      Origins.resize((size_t)Width * Height * 3); Directions.resize((size_t)Width * Height * 3);
      Check(mdh_camera_rays(h_.get(), Width, Height, Origins.data(), Directions.data()));
   }
   void Camera_Rays_Device(int32_t Width, int32_t Height, float *Origins, float *Directions, void *Stream = nullptr) const
   {
      Check(mdh_camera_rays_device(h_.get(), Width, Height, Origins, Directions, Stream));
   }
   // ---- what light arrives at a point the host owns: pixel_color_probes from the hit on (render_probes.glsl:253-285) at points that
   // need not lie on a primitive.  View_Dirs: the direction each point is seen ALONG; Material_Ids: what Add_Material returned.
   // Mode 0 (the fixed mode), 2 (direct light times occlusion) or 3 (MDH_POINT_IRRADIANCE: sample_irradiance alone -- View_Dirs and
   // Material_Ids may be empty, no tone map).  3 floats a point; never any fog
   std::vector<float> Shade_Points(const std::vector<float> &Positions, const std::vector<float> &Normals, const std::vector<float> &View_Dirs,
                                   const std::vector<int32_t> &Material_Ids, int32_t Mode = 0, bool Tone_Map = false) const
   {
      const size_t n = Ray_Count(Positions, Normals);
      if (Mode != MDH_POINT_IRRADIANCE && (View_Dirs.size() != 3 * n || Material_Ids.size() != n)) throw Constraint_Error("one view direction and one material id per point");
      std::vector<float> Rgb(3 * n);
      Check(mdh_shade_points(h_.get(), (int32_t)n, Positions.data(), Normals.data(), Mode == MDH_POINT_IRRADIANCE ? nullptr : View_Dirs.data(),
                             Mode == MDH_POINT_IRRADIANCE ? nullptr : Material_Ids.data(), Mode, Tone_Map ? 1 : 0, Rgb.data()));
      return Rgb;
   }
   // ... for arrays in memory the device addresses, asynchronous and ordered with Stream as Shade_Rays_Device is.  A point that is not
   // finite, lies beyond 1024, has a normal or view component beyond 1 or names no material: NaN in all three colours
   void Shade_Points_Device(int32_t N, const float *Positions, const float *Normals, const float *View_Dirs, const int32_t *Material_Ids, float *Rgb,
                            int32_t Mode = 0, bool Tone_Map = false, void *Stream = nullptr) const
   {
      Check(mdh_shade_points_device(h_.get(), N, Positions, Normals, View_Dirs, Material_Ids, Mode, Tone_Map ? 1 : 0, Rgb, Stream));
   }
   // the material id of every primitive index (the numbering of Read_Gbuffer and Raycast; -1 for -1): Raycast's hits for Shade_Points
   std::vector<int32_t> Primitive_Material(const std::vector<int32_t> &Index) const
   {
      std::vector<int32_t> Material(Index.size());
      Check(mdh_primitive_material(h_.get(), (int32_t)Index.size(), Index.data(), Material.data()));
      return Material;
   }
   // ---- ground truth for the probes: a path tracer along rays of the host's (the reference's render_path.glsl made to run).  Rgb holds
   // SUMS: samples Sample_First .. Sample_First + Sample_Count - 1 are added to Rgb_Accum (empty: zeros) in that order, the host divides by
   // the count; ray i has id Id_First + i and its random numbers depend on (Seed, id, sample, bounce) alone.  Hit, Index, T: the primary
   // segment.  Bounces 0 .. 6; never any fog, no atlas, no occlusion
   struct Path_Colours { std::vector<float> Rgb, T; std::vector<int32_t> Hit, Index; };
   Path_Colours Path_Trace(const std::vector<float> &Origins, const std::vector<float> &Directions, uint32_t Seed = 0, uint32_t Id_First = 0, int32_t Sample_First = 0,
                           int32_t Sample_Count = 1, int32_t Bounces = 3, const std::vector<float> &Rgb_Accum = std::vector<float>()) const
   {
      const size_t n = Ray_Count(Origins, Directions);
      if (!Rgb_Accum.empty() && Rgb_Accum.size() != 3 * n) throw Constraint_Error("one colour sum per ray");
      Path_Colours o;
      o.Rgb = Rgb_Accum.empty() ? std::vector<float>(3 * n, 0.0f) : Rgb_Accum;
      o.T.resize(n); o.Hit.resize(n); o.Index.resize(n);
      Check(mdh_path_trace(h_.get(), (int32_t)n, Origins.data(), Directions.data(), Seed, Id_First, Sample_First, Sample_Count, Bounces, o.Rgb.data(), o.Hit.data(),
                           o.Index.data(), o.T.data()));
      return o;
   }
   // ... for arrays in memory the device addresses, asynchronous and ordered with Stream as Shade_Rays_Device is; the sums stay on the device
   // from call to call.  A ray that is not finite, starts beyond 1024 or has a direction component beyond 2: NaN, Hit = -1
   void Path_Trace_Device(int32_t N, const float *Origins, const float *Directions, float *Rgb_Accum, int32_t *Hit = nullptr, int32_t *Index = nullptr, float *T = nullptr,
                          uint32_t Seed = 0, uint32_t Id_First = 0, int32_t Sample_First = 0, int32_t Sample_Count = 1, int32_t Bounces = 3, void *Stream = nullptr) const
   {
      Check(mdh_path_trace_device(h_.get(), N, Origins, Directions, Seed, Id_First, Sample_First, Sample_Count, Bounces, Rgb_Accum, Hit, Index, T, Stream));
   }
   // the sampler by itself, on the host, the lanes' bits: no launch and no renderer.  3 floats a direction, one roughness each
   static std::vector<float> Path_Scatter(const std::vector<float> &Directions, const std::vector<float> &Normals, const std::vector<float> &Roughness, uint32_t Seed = 0,
                                          uint32_t Id_First = 0, int32_t Sample = 0, int32_t Bounce = 0)
   {
      const size_t n = Roughness.size();
      if (Directions.size() != 3 * n || Normals.size() != 3 * n) throw Constraint_Error("one direction, one normal and one roughness per path");
      std::vector<float> Out(3 * n);
      Check(mdh_path_scatter((int32_t)n, Directions.data(), Normals.data(), Roughness.data(), Seed, Id_First, Sample, Bounce, Out.data()));
      return Out;
   }
   // ---- a path-traced frame: Path_Trace's estimator over the pixels of a frame of the camera, the sums kept on the device from call
   // to call.  Begin captures the camera and fixes Seed, Bounces and Jitter; Accumulate adds the next samples and does not wait;
   // Read is the resolve on the device (sums / samples, the tone map, the window's bytes); restarting after an edit is the caller's
   struct Path_Frame_State { int32_t Width = 0, Height = 0, Samples = 0, Bounces = 0, Jitter = 0; };
   struct Path_Frame_Image { int32_t Width = 0, Height = 0, Samples = 0; std::vector<float> Rgb; std::vector<uint32_t> Rgba8; std::vector<float> Sums; };
   void Path_Frame_Begin(int32_t Width, int32_t Height, uint32_t Seed = 0, int32_t Bounces = 3, bool Jitter = true) const
   {
      Check(mdh_path_frame_begin(h_.get(), Width, Height, Seed, Bounces, Jitter ? 1 : 0));
   }
   void Path_Frame_Accumulate(int32_t Sample_Count = 1) const { Check(mdh_path_frame_accumulate(h_.get(), Sample_Count)); }
   // ... an ADAPTIVE accumulator: a count and two moments a pixel; Path_Frame_Accumulate is then one round for the pixels the stopping
   // rule keeps running (evaluated at round boundaries only: two rounds of 2 are not one round of 4), Read divides by the pixel's own
   // count.  A stopping rule on a biased variance estimate: Min_Samples is the caller's guard
   void Path_Frame_Begin_Adaptive(int32_t Width, int32_t Height, uint32_t Seed = 0, int32_t Bounces = 3, bool Jitter = true, int32_t Min_Samples = 4,
                                  int32_t Max_Samples = 64, float Tolerance = 0.05f, float Floor = 0.01f) const
   {
      Check(mdh_path_frame_begin_adaptive(h_.get(), Width, Height, Seed, Bounces, Jitter ? 1 : 0, Min_Samples, Max_Samples, Tolerance, Floor));
   }
   struct Path_Frame_Statistics { std::vector<int32_t> Count; std::vector<float> Moments; int64_t Active = 0, Total_Samples = 0; };
   // the counts (one a pixel), the moments (m1, m2 a pixel), the pixels still running and the samples taken; waits for the device
   Path_Frame_Statistics Path_Frame_Stats(bool Count = true, bool Moments = true) const
   {
      const Path_Frame_State S = Path_Frame_Info();
      const size_t n = (size_t)S.Width * (size_t)S.Height;
      Path_Frame_Statistics Out;
      if (Count) Out.Count.resize(n);
      if (Moments) Out.Moments.resize(2 * n);
      Check(mdh_path_frame_stats(h_.get(), Out.Count.empty() ? nullptr : Out.Count.data(), Out.Moments.empty() ? nullptr : Out.Moments.data(), &Out.Active, &Out.Total_Samples));
      return Out;
   }
   // ... into arrays the device addresses (Active, Total_Samples: one int64 each), asynchronous and ordered with Stream
   void Path_Frame_Stats_Device(int32_t *Count, float *Moments = nullptr, int64_t *Active = nullptr, int64_t *Total_Samples = nullptr, void *Stream = nullptr) const
   {
      Check(mdh_path_frame_stats_device(h_.get(), Count, Moments, Active, Total_Samples, Stream));
   }
   // the rule by itself, on the host, the lanes' function: no launch, no renderer
   static std::vector<uint8_t> Path_Pixel_Active(const std::vector<int32_t> &Count, const std::vector<float> &M1, const std::vector<float> &M2, int32_t Min_Samples,
                                                 int32_t Max_Samples, float Tolerance, float Floor)
   {
      if (M1.size() != Count.size() || M2.size() != Count.size()) throw std::invalid_argument("Path_Pixel_Active: one count and two moments a pixel");
      std::vector<uint8_t> Out(Count.size() + 1);
      Check(mdh_path_pixel_active((int32_t)Count.size(), Count.data(), M1.data(), M2.data(), Min_Samples, Max_Samples, Tolerance, Floor, Out.data()));
      Out.resize(Count.size());
      return Out;
   }
   Path_Frame_State Path_Frame_Info() const
   {
      Path_Frame_State S;
      Check(mdh_path_frame_info(h_.get(), &S.Width, &S.Height, &S.Samples, &S.Bounces, &S.Jitter));
      return S;
   }
   // rows top first; 3 floats a pixel in Rgb and Sums, one word (R in the low byte) in Rgba8; only what is asked for is computed
   Path_Frame_Image Path_Frame_Read(bool Tone_Map = false, bool Rgb = true, bool Rgba8 = false, bool Sums = false) const
   {
      const Path_Frame_State S = Path_Frame_Info();
      Path_Frame_Image Out;
      Out.Width = S.Width; Out.Height = S.Height;
      const size_t n = (size_t)S.Width * (size_t)S.Height;
      if (Rgb) Out.Rgb.resize(3 * n);
      if (Rgba8) Out.Rgba8.resize(n);
      if (Sums) Out.Sums.resize(3 * n);
      Check(mdh_path_frame_read(h_.get(), Tone_Map ? 1 : 0, Out.Rgb.empty() ? nullptr : Out.Rgb.data(), Out.Rgba8.empty() ? nullptr : Out.Rgba8.data(),
                                Out.Sums.empty() ? nullptr : Out.Sums.data(), &Out.Samples));
      return Out;
   }
   // ... into arrays the device addresses, asynchronous and ordered with Stream (a hipStream_t); returns the samples
   int32_t Path_Frame_Read_Device(float *Rgb, uint32_t *Rgba8 = nullptr, float *Sums = nullptr, bool Tone_Map = false, void *Stream = nullptr) const
   {
      int32_t Samples = 0;
      Check(mdh_path_frame_read_device(h_.get(), Tone_Map ? 1 : 0, Rgb, Rgba8, Sums, &Samples, Stream));
      return Samples;
   }
   // the rays the accumulator gives its pixels for one sample: (origins, directions), 3 floats a pixel
   std::pair<std::vector<float>, std::vector<float>> Path_Frame_Rays(int32_t Sample = 0) const
   {
      const Path_Frame_State S = Path_Frame_Info();
      const size_t n = (size_t)S.Width * (size_t)S.Height;
      std::vector<float> Org(3 * n + 3), Dir(3 * n + 3); // (never null: without an accumulator the library says so)
      Check(mdh_path_frame_rays(h_.get(), Sample, Org.data(), Dir.data()));
      Org.resize(3 * n); Dir.resize(3 * n);
      return {Org, Dir};
   }
   void Path_Frame_Rays_Device(float *Origins, float *Directions, int32_t Sample = 0, void *Stream = nullptr) const
   {
      Check(mdh_path_frame_rays_device(h_.get(), Sample, Origins, Directions, Stream));
   }
   void Path_Frame_End() const { Check(mdh_path_frame_end(h_.get())); }
   // the jitter by itself, on the host, the lanes' bits: (u, v) of N pixels from Id_First on, 2 floats a pixel; no launch, no renderer
   static std::vector<float> Path_Pixel_Uv(int32_t Width, int32_t Height, uint32_t Seed, uint32_t Id_First, int32_t N, int32_t Sample = 0, bool Jitter = true)
   {
      std::vector<float> Uv(2 * (size_t)(N > 0 ? N : 0) + 2);
      Check(mdh_path_pixel_uv(Width, Height, Seed, Id_First, N, Sample, Jitter ? 1 : 0, Uv.data()));
      Uv.resize(2 * (size_t)(N > 0 ? N : 0));
      return Uv;
   }
   // ---- the lights' fog at points and along rays of the host's (compute_frustrum_visibility.glsl:8-19, accumulate_scattering.glsl:17-28),
   // without the froxel grid or the camera it is bound to.  Points: sample_lights (position, direction), times exp (-F tau) where F
   // (one distance per point) is not empty.  Rays: L = 0; for (f = 0; f < len; f += Step) L = L + inscatter ((dir * f) + org, dir) * exp (-f tau);
   // Rgb = L * Step; Len is Max_Dists, or with March the distance to what the ray hits where that is shorter; Steps the loop's turns
   std::vector<float> Inscatter_Points(const std::vector<float> &Positions, const std::vector<float> &Directions, const std::vector<float> &F = std::vector<float>()) const
   {
      const size_t n = Ray_Count(Positions, Directions);
      if (!F.empty() && F.size() != n) throw Constraint_Error("one distance per point");
      std::vector<float> Rgb(3 * n);
      Check(mdh_inscatter_points(h_.get(), (int32_t)n, Positions.data(), Directions.data(), F.empty() ? nullptr : F.data(), Rgb.data()));
      return Rgb;
   }
   struct Inscattered { std::vector<float> Rgb, Len; std::vector<int32_t> Steps; };
   Inscattered Inscatter_Rays(const std::vector<float> &Origins, const std::vector<float> &Directions, const std::vector<float> &Max_Dists, float Step, bool March = false) const
   {
      const size_t n = Ray_Count(Origins, Directions);
      if (Max_Dists.size() != n) throw Constraint_Error("one length per ray");
      Inscattered o;
      o.Rgb.resize(3 * n); o.Len.resize(n); o.Steps.resize(n);
      Check(mdh_inscatter_rays(h_.get(), (int32_t)n, Origins.data(), Directions.data(), Max_Dists.data(), March ? 1 : 0, Step, o.Rgb.data(), o.Len.data(), o.Steps.data()));
      return o;
   }
   // ... for arrays in memory the device addresses, asynchronous and ordered with Stream as Raycast_Device is.  F, Len and Steps may be null.
   // A point or ray that is not finite, or a length outside 0 .. max_dist: NaN in Rgb and Len, Steps = -1
   void Inscatter_Points_Device(int32_t N, const float *Positions, const float *Directions, float *Rgb, const float *F = nullptr, void *Stream = nullptr) const
   {
      Check(mdh_inscatter_points_device(h_.get(), N, Positions, Directions, F, Rgb, Stream));
   }
   void Inscatter_Rays_Device(int32_t N, const float *Origins, const float *Directions, const float *Max_Dists, float Step, float *Rgb, float *Len = nullptr,
                              int32_t *Steps = nullptr, bool March = false, void *Stream = nullptr) const
   {
      Check(mdh_inscatter_rays_device(h_.get(), N, Origins, Directions, Max_Dists, March ? 1 : 0, Step, Rgb, Len, Steps, Stream));
   }
   // ---- swept spheres and contacts, for a host that owns moving bodies (madarch_hip.h: mdh_spherecast, mdh_contacts).  Kinds
   // empty: the scene as every pass sees it; kind indices in scene order otherwise: the exact minimum over those kinds' instances.
   // Radii and Max_Dists may be null (0, the scene's max_dist); every output but Hit and Dist may be null
   void Spherecast(int32_t N, const float *Origins, const float *Directions, const float *Radii, const float *Max_Dists, const std::vector<int32_t> &Kinds,
                   int32_t *Hit, int32_t *Index = nullptr, float *T = nullptr, int32_t *Steps = nullptr, float *Position = nullptr, float *Normal = nullptr) const
   {
      Check(mdh_spherecast(h_.get(), N, Origins, Directions, Radii, Max_Dists, Kinds.empty() ? nullptr : Kinds.data(), (int32_t)Kinds.size(), Hit, Index, T, Steps, Position, Normal));
   }
   void Contacts(int32_t N, const float *Centres, const float *Radii, const std::vector<int32_t> &Kinds, float *Dist, int32_t *Index = nullptr, float *Normal = nullptr) const
   {
      Check(mdh_contacts(h_.get(), N, Centres, Radii, Kinds.empty() ? nullptr : Kinds.data(), (int32_t)Kinds.size(), Dist, Index, Normal));
   }
   // ... for arrays the device addresses, ordered with Stream (Raycast_Device's contract; Ray_Query_Wait is the host's wait)
   void Spherecast_Device(int32_t N, const float *Origins, const float *Directions, const float *Radii, const float *Max_Dists, const std::vector<int32_t> &Kinds,
                          int32_t *Hit, int32_t *Index = nullptr, float *T = nullptr, int32_t *Steps = nullptr, float *Position = nullptr, float *Normal = nullptr,
                          void *Stream = nullptr) const
   {
      Check(mdh_spherecast_device(h_.get(), N, Origins, Directions, Radii, Max_Dists, Kinds.empty() ? nullptr : Kinds.data(), (int32_t)Kinds.size(), Hit, Index, T, Steps,
                                  Position, Normal, Stream));
   }
   void Contacts_Device(int32_t N, const float *Centres, const float *Radii, const std::vector<int32_t> &Kinds, float *Dist, int32_t *Index = nullptr, float *Normal = nullptr,
                        void *Stream = nullptr) const
   {
      Check(mdh_contacts_device(h_.get(), N, Centres, Radii, Kinds.empty() ? nullptr : Kinds.data(), (int32_t)Kinds.size(), Dist, Index, Normal, Stream));
   }
   // ---- the scene's surface as a mesh: surface nets over a grid (madarch_hip.h: mdh_surface_mesh has the definition).  Kinds as
   // for Contacts.  Surface_Mesh counts, allocates and calls again; the _Device form takes arrays with their capacities, and
   // Counts (2 int32 the device addresses) holds what was found, whatever the capacities
   struct Mesh {
      std::vector<float> Positions, Normals; // 3 a vertex
      std::vector<int32_t> Index, Quads;     // one a vertex, 4 a quad
   };
   Mesh Surface_Mesh(const float (&Origin)[3], float Spacing, const int32_t (&Cells)[3], float Iso = 0.0f, const std::vector<int32_t> &Kinds = {}) const
   {
      const int32_t *kinds = Kinds.empty() ? nullptr : Kinds.data();
      int32_t counts[2] = {0, 0};
      Check(mdh_surface_mesh(h_.get(), Origin, Spacing, Cells, Iso, kinds, (int32_t)Kinds.size(), 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, counts));
      Mesh m;
      const int32_t nv = counts[0], nq = counts[1];
      m.Positions.resize(3 * (size_t)nv); m.Normals.resize(3 * (size_t)nv); m.Index.resize((size_t)nv); m.Quads.resize(4 * (size_t)nq);
      Check(mdh_surface_mesh(h_.get(), Origin, Spacing, Cells, Iso, kinds, (int32_t)Kinds.size(), nv, nq, nv ? m.Positions.data() : nullptr, nv ? m.Normals.data() : nullptr,
                             nv ? m.Index.data() : nullptr, nq ? m.Quads.data() : nullptr, nullptr, counts));
      return m;
   }
   void Surface_Mesh_Device(const float (&Origin)[3], float Spacing, const int32_t (&Cells)[3], float Iso, const std::vector<int32_t> &Kinds, int32_t Vertex_Capacity,
                            int32_t Quad_Capacity, float *Positions, float *Normals, int32_t *Index, int32_t *Quads, float *Field, int32_t *Counts, void *Stream = nullptr) const
   {
      Check(mdh_surface_mesh_device(h_.get(), Origin, Spacing, Cells, Iso, Kinds.empty() ? nullptr : Kinds.data(), (int32_t)Kinds.size(), Vertex_Capacity, Quad_Capacity,
                                    Positions, Normals, Index, Quads, Field, Counts, Stream));
   }
   void Update_Partitioning(Partitioning_Update_Method Method = GPU_Fast) const { Check(mdh_update_partitioning(h_.get(), (int32_t)Method)); } // renderers.adb:757-775
   // ---- headless additions
   std::vector<float> Read_Framebuffer() const // replaces Swap_Buffers: H*W*3 floats, row 0 = top
   {
      std::vector<float> out((size_t)window_.Width * window_.Height * 3);
      Check(mdh_read_framebuffer(h_.get(), out.data()));
      return out;
   }
   // Swap_Buffers itself (renderers.adb:320): the window's RGBA8 pixels, enqueued behind the frame without a host wait ...
   void Swap_Buffers() const { Check(mdh_swap_buffers(h_.get())); }
   // ... and fetched: H*W*4 bytes owned by the renderer (valid until the second next Swap_Buffers); waits for the last swap only
   const uint8_t *Front_Buffer() const
   {
      const uint8_t *p = nullptr;
      Check(mdh_front_buffer(h_.get(), &p, nullptr));
      return p;
   }
   void Set_Option(int32_t Option, int32_t Value) const { Check(mdh_set_option(h_.get(), Option, Value)); }
   static constexpr int32_t Opt_Probe_Settle = MDH_OPT_PROBE_SETTLE; // Set_Option (.., 0): probe passes launched in every frame (default 1: left out once the atlases have stopped changing, the same bits; any edit launches them again)
   static constexpr int32_t Opt_Path_Frame_Compact = MDH_OPT_PATH_FRAME_COMPACT; // Set_Option (.., 0 / 1): an adaptive path-traced frame compacts the pixels still running (default 0, the measured one; the same bits)
   static constexpr int32_t Opt_Ray_Stream_Refill = MDH_OPT_RAY_STREAM_REFILL; // Set_Option (.., 1 .. 64): the idle lanes at which a device-array ray query's wavefront takes new rays (64: lock step; the same bits)
   static constexpr int32_t Opt_Ray_Stream_Groups = MDH_OPT_RAY_STREAM_GROUPS; // Set_Option (.., k): at most k workgroups for such a query (0, default: as many as the device holds at once)
   static constexpr int32_t Opt_Screen_Replay = MDH_OPT_SCREEN_REPLAY; // Set_Option (.., 1): the screen pass's marches replayed while camera and geometry stand still, the same bits (default 0)
   static constexpr int32_t Opt_Radiance_Replay = MDH_OPT_RADIANCE_REPLAY; // Set_Option (.., 0): probe rays marched in every pass (default 1: replayed while the geometry stands still, the same bits)
   static constexpr int32_t Opt_Triangle_BVH = MDH_OPT_TRIANGLE_BVH; // Set_Option (.., 1): triangles walked through a BVH, the same bits (scenes without partition or user-defined kinds)
   int32_t Get_Option(int32_t Option) const { int32_t Value = 0; Check(mdh_get_option(h_.get(), Option, &Value)); return Value; } // (MDH_OPT_TABLE_RESIDENCY: 1 for scenes larger than LDS)
   // ---- one frame on the N GPUs of a node, one process per GPU (include/madarch_hip.h, mdh_comm_*): after Join_Node,
   // Render of every rank is one frame of the sharded schedule.  The 128-byte communicator id travels from rank 0 to
   // the others through `Id_File` (written under a temporary name and renamed, so a reader never sees half of it).
   // A file left by an earlier run must never be taken for this one's: rank 0 removes it (and its temporary) BEFORE it
   // makes the new id and again once every rank has joined; the others only accept a file that is no older than their
   // own call (minus `Timeout_S`: the ranks of a run start within that) and, when the launcher hands every rank the same
   // `Nonce`, one that carries it.  The collective join itself runs under the same timeout: a rank whose peers never
   // arrive reports that and leaves the process (ncclCommInitRank cannot be cancelled) instead of hanging for ever.
   void Join_Node(int Rank, int World, const std::string &Id_File, double Timeout_S = 120.0, const std::string &Nonce = "") const
   {
      uint8_t id[MDH_COMM_ID_BYTES];
      const std::string tmp = Id_File + ".tmp";
      const auto wall0 = std::chrono::system_clock::now();
      if (Rank == 0) {
         std::remove(Id_File.c_str());
         std::remove(tmp.c_str());
         Check(mdh_comm_unique_id(id));
         FILE *f = fopen(tmp.c_str(), "wb");
         if (!f || fwrite(id, 1, sizeof id, f) != sizeof id || (!Nonce.empty() && fwrite(Nonce.data(), 1, Nonce.size(), f) != Nonce.size())) throw Program_Error("cannot write the communicator id file");
         fclose(f);
         if (rename(tmp.c_str(), Id_File.c_str()) != 0) throw Program_Error("cannot publish the communicator id file");
      } else {
         const auto t0 = std::chrono::steady_clock::now();
         for (;;) {
            bool fresh = false;
            struct stat sb;
            if (stat(Id_File.c_str(), &sb) == 0) {
               const double age_before_call = std::chrono::duration<double>(wall0 - std::chrono::system_clock::from_time_t(sb.st_mtime)).count();
               fresh = age_before_call <= Timeout_S;
            }
            if (fresh) {
               std::vector<uint8_t> buf(sizeof id + Nonce.size() + 1);
               FILE *f = fopen(Id_File.c_str(), "rb");
               const size_t n = f ? fread(buf.data(), 1, buf.size(), f) : 0;
               if (f) fclose(f);
               if (n == sizeof id + Nonce.size() && std::equal(Nonce.begin(), Nonce.end(), buf.begin() + sizeof id)) { std::copy(buf.begin(), buf.begin() + sizeof id, id); break; }
            }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > Timeout_S) throw Program_Error("rank 0 never published the communicator id file of this run");
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
         }
      }
      // the join under a watchdog
      std::atomic<int> state{0}; // 0 joining, 1 joined, 2 failed
      std::string error;
      mdh_renderer *h = h_.get();
      std::thread joiner([&] {
         const int32_t rc = mdh_comm_init(h, id, Rank, World);
         if (rc != 0) error = mdh_last_error();
         state = rc == 0 ? 1 : 2;
      });
      const auto t1 = std::chrono::steady_clock::now();
      while (state == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count() <= Timeout_S) std::this_thread::sleep_for(std::chrono::milliseconds(5));
      if (state == 0) {
         fprintf(stderr, "rank %d: the ranks of the node did not all join within %.0f s: leaving\n", Rank, Timeout_S);
         (void)mdh_comm_abort(h);
         std::_Exit(70);
      }
      joiner.join();
      if (Rank == 0) std::remove(Id_File.c_str()); // (every rank holds the id: the collective join has returned)
      if (state == 2) throw Program_Error(error);
   }
   // ---- the same sharded frame without a collective library: the peer exchange (include/madarch_hip.h, mdh_peer_*).  Every rank
   // publishes its 512 bytes of interprocess handles as a file of `Dir` and reads the others'; Render is then the sharded frame,
   // its exchange being device-to-device copies between the ranks' processes (one process per rank, one node; several ranks
   // may share ONE GPU).  `Dir` must be this run's own (files of an earlier run are refused by their age, as in Join_Node).
   static void Publish_File(const std::string &Path, const void *Data, size_t N)
   {
      const std::string tmp = Path + ".tmp";
      FILE *f = fopen(tmp.c_str(), "wb");
      if (!f || fwrite(Data, 1, N, f) != N) throw Program_Error("cannot write " + tmp);
      fclose(f);
      if (rename(tmp.c_str(), Path.c_str()) != 0) throw Program_Error("cannot publish " + Path);
   }
   static std::vector<uint8_t> Await_File(const std::string &Path, size_t N, std::chrono::system_clock::time_point Since, double Timeout_S)
   {
      const auto t0 = std::chrono::steady_clock::now();
      for (;;) {
         struct stat sb;
         if (stat(Path.c_str(), &sb) == 0 && std::chrono::duration<double>(Since - std::chrono::system_clock::from_time_t(sb.st_mtime)).count() <= Timeout_S) {
            std::vector<uint8_t> buf(N + 1);
            FILE *f = fopen(Path.c_str(), "rb");
            const size_t n = f ? fread(buf.data(), 1, buf.size(), f) : 0;
            if (f) fclose(f);
            if (n == N) { buf.resize(N); return buf; }
         }
         if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > Timeout_S) throw Program_Error("a rank never published " + Path);
         std::this_thread::sleep_for(std::chrono::milliseconds(10));
      }
   }
   void Join_Peers(int Rank, int World, const std::string &Dir, double Timeout_S = 120.0) const
   {
      const auto wall0 = std::chrono::system_clock::now();
      uint8_t blob[MDH_PEER_BLOB_BYTES];
      Check(mdh_peer_export(h_.get(), blob));
      Publish_File(Dir + "/peer_" + std::to_string(Rank) + ".blob", blob, sizeof blob);
      std::vector<uint8_t> all((size_t)World * MDH_PEER_BLOB_BYTES);
      for (int q = 0; q < World; ++q) {
         const auto b = Await_File(Dir + "/peer_" + std::to_string(q) + ".blob", MDH_PEER_BLOB_BYTES, wall0, Timeout_S);
         std::copy(b.begin(), b.end(), all.begin() + (size_t)q * MDH_PEER_BLOB_BYTES);
      }
      Check(mdh_peer_init(h_.get(), all.data(), Rank, World));
   }
   // every rank has reached this point of the run (a file per rank and tag): e.g. before anybody leaves the exchange --
   // a rank's atlases must outlive the peers' last copies out of them
   static void Peers_Barrier(int Rank, int World, const std::string &Dir, const std::string &Tag, double Timeout_S = 120.0)
   {
      const auto wall0 = std::chrono::system_clock::now();
      const uint8_t one = 1;
      Publish_File(Dir + "/" + Tag + "_" + std::to_string(Rank), &one, 1);
      for (int q = 0; q < World; ++q) (void)Await_File(Dir + "/" + Tag + "_" + std::to_string(q), 1, wall0, Timeout_S);
   }
   void Finish() const { Check(mdh_finish(h_.get())); }
   void Leave_Node() const { Check(mdh_comm_destroy(h_.get())); }
   void Barrier() const { Check(mdh_comm_barrier(h_.get())); }
   double Max_Over_Ranks(double V) const { Check(mdh_comm_max_f64(h_.get(), &V)); return V; }
   // the ranks' tiles of the last frame summed into Root's framebuffer: what Root's window shows
   void Gather_Frame(int Root = 0) const { Check(mdh_comm_reduce_framebuffer(h_.get(), Root)); }
   mdh_renderer *Handle() const { return h_.get(); }
   const Windows::Window &Window() const { return window_; }
 private:
   std::shared_ptr<mdh_renderer> h_;
   Windows::Window window_;
   Scenes::Scene scene_;
};

// Renderers.Create (madarch-renderers.adb:91-300)
inline Renderer Create(const Windows::Window &Window, const Scenes::Scene &Scene, const Probe_Settings &Probes = {},
                       const Volumetrics_Settings &Volumetrics = {}, int Device = 0)
{
   std::vector<std::vector<mdh_component>> comps;
   auto decls = [&](auto &items, auto name_of) {
      std::vector<mdh_kind_decl> out;
      for (auto &it : items) {
         auto &kind = name_of(it);
         comps.emplace_back();
         for (auto &c : kind->Comps) comps.back().push_back(mdh_component{c->Name.c_str(), (int32_t)c->Kind});
         out.push_back(mdh_kind_decl{kind->Name.c_str(), it.Count, (int32_t)kind->Comps.size(), nullptr});
      }
      return out;
   };
   auto pk = decls(Scene->Prims, [](const Scenes::Primitive_Count &p) -> const Primitives::Primitive & { return p.Prim; });
   size_t npk = pk.size();
   auto lk = decls(Scene->Lits, [](const Scenes::Light_Count &l) -> const Lights::Light & { return l.Light; });
   for (size_t i = 0; i < pk.size(); ++i) pk[i].components = comps[i].data();
   for (size_t i = 0; i < lk.size(); ++i) lk[i].components = comps[npk + i].data();
   mdh_scene_desc d{};
   d.n_prim_kinds = (int32_t)pk.size(); d.prim_kinds = pk.data();
   d.n_light_kinds = (int32_t)lk.size(); d.light_kinds = lk.data();
   const auto &p = Scene->Partitioning_Config;
   d.partitioning.enable = p.Enable; d.partitioning.index_count = p.Index_Count; d.partitioning.border_behavior = p.Border_Behavior;
   for (int a = 0; a < 3; ++a) { d.partitioning.grid_dimensions[a] = p.Grid_Dimensions[a]; d.partitioning.grid_spacing[a] = p.Grid_Spacing[a]; d.partitioning.grid_offset[a] = p.Grid_Offset[a]; }
   d.max_dist = Scene->Max_Dist;
   d.loop_strategy = Scene->Loop_Strategy;
   mdh_probe_settings ps{Probes.Radiance_Resolution, Probes.Irradiance_Resolution, {Probes.Probe_Count[0], Probes.Probe_Count[1]},
                         {Probes.Grid_Dimensions[0], Probes.Grid_Dimensions[1], Probes.Grid_Dimensions[2]},
                         {Probes.Grid_Spacing[0], Probes.Grid_Spacing[1], Probes.Grid_Spacing[2]}};
   mdh_volumetrics vs{Volumetrics.Enabled ? 1 : 0, {Volumetrics.Visibility_Resolution[0], Volumetrics.Visibility_Resolution[1], Volumetrics.Visibility_Resolution[2]},
                      Volumetrics.Visibility_Step_Size, {Volumetrics.Scattering_Resolution[0], Volumetrics.Scattering_Resolution[1]}, Volumetrics.Scattering_Step_Size};
   mdh_renderer *h = nullptr;
   Check(mdh_create(Window.Width, Window.Height, &d, &ps, &vs, Device, &h));
   return Renderer(h, Window, Scene);
}
} // namespace Renderers
} // namespace Madarch
