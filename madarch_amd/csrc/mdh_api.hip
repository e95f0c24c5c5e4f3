// mdh_api.hip -- libmadarch_hip.so: the C ABI of include/madarch_hip.h.
//
// Host side of the MI355X back end: what Madarch.Renderers does with OpenGL
// objects (reference madarch/madarch-renderers.adb:91-497, support/gpu_buffers.adb,
// support/render_passes.adb) is done here with HIP memory, one stream per renderer
// and the kernels of mdh_kernels.h.  There is no CPU rendering path: without a
// gfx950 device mdh_create fails with MDH_E_NO_DEVICE.
#include "../../include/madarch_hip.h"
#include "mdh_kernels.h"
#include "mdh_host.h" // DevBuf, Event, Fence, RingUse: what owns the buffers, events and orderings below
#include "mdh_jit_sources.inc" // the three device headers as string literals (Makefile), for the hiprtc build of user-defined kinds

#include <dlfcn.h>
#include <unistd.h>
#include <hip/hiprtc.h> // types only: the library is opened on first use (no link-time dependency)
#include <rccl/rccl.h>  // types only, likewise: librccl is opened by the first mdh_comm_* call

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

static thread_local char g_err[512];
static int seterr(int code, const char *msg)
{
   snprintf(g_err, sizeof g_err, "%s", msg);
   return code;
}
#define HIP_TRY(expr)                                                                               \
   do {                                                                                             \
      hipError_t e_ = (expr);                                                                       \
      if (e_ != hipSuccess) {                                                                       \
         snprintf(g_err, sizeof g_err, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
         return MDH_E_DEVICE;                                                                       \
      }                                                                                             \
   } while (0)

extern "C" const char *mdh_last_error(void) { return g_err; }
#if MDH_FAST_NUMERICS
extern "C" const char *mdh_version(void) { return "madarch-hip 0.3 (gfx950) FAST-NUMERICS EXPERIMENT BUILD: tolerance only, not the oracle's bits"; }
#elif MDH_HYBRID_NUMERICS
extern "C" const char *mdh_version(void) { return "madarch-hip 0.4 (gfx950) HYBRID-NUMERICS EXPERIMENT BUILD: exact march loops and primary ray, hardware rcp / sqrt / exp / log in shading"; }
#else
extern "C" const char *mdh_version(void) { return "madarch-hip 0.4 (gfx950)"; }
#endif

// ------------------------------------------------------------------ std140 layout
// = GPU_Types (support/gpu_types-base.ads:21-37, gpu_types-structs.adb:11-38,
// gpu_types-fixed_arrays.adb:17-39)
static int pad_to(int x, int a) { while (x % a) ++x; return x; }
static int base_align(int kind) { return kind == MDH_VEC3 ? 16 : 4; }
static int base_size(int kind) { return kind == MDH_VEC3 ? 12 : 4; }

struct Kind {
   int type = -1, max_count = 0, ncomp = 0;
   std::string comp_name[8];
   int comp_kind[8], comp_off[8];
   int elem_size = 0, stride = 0, count_off = 0, array_off = 0;
   int f_a = -1, f_b = -1, f_c = -1, f_d = -1; // resolved field offsets
   // user-defined kinds (PK_CUSTOM): the three MDH_X programs and the packed instance size
   std::vector<int32_t> x_dist, x_nrm, x_mat;
   int inst_floats = 0;
   int offset_of(const char *name, int kind) const
   {
      for (int i = 0; i < ncomp; ++i)
         if (comp_name[i] == name && comp_kind[i] == kind) return comp_off[i];
      return -1;
   }
};

// An MDH_X program is accepted only if every word is a known instruction with in-range
// operands (nothing the caller hands over is trusted to index the register file or the instance).
static bool valid_program(const int32_t *code, int n, int inst_floats, int n_args)
{
   if (!code || n < 1 || n > MDH_X_MAX_WORDS) return false;
   for (int pc = 0; pc < n; ++pc) {
      const uint32_t w = (uint32_t)code[pc];
      const int op = w & 255, d = (w >> 8) & 255, a = (w >> 16) & 255, b = (w >> 24) & 255;
      if (op >= MDH_X_OPS || d >= MDH_X_REGS) return false;
      switch (op) {
      case MDH_X_LIT: if (++pc >= n) return false; break;
      case MDH_X_COMP: if (a >= inst_floats) return false; break;
      case MDH_X_POINT: if (a >= n_args) return false; break;
      case MDH_X_SEL:
         if (a >= MDH_X_REGS || b >= MDH_X_REGS || ++pc >= n || (uint32_t)code[pc] >= MDH_X_REGS) return false;
         break;
      default: if (a >= MDH_X_REGS || b >= MDH_X_REGS) return false; break;
      }
   }
   return true;
}

static bool resolve_kind(Kind &k, const mdh_kind_decl &d, bool is_light)
{
   static const char *P[4] = {"Sphere", "Plane", "Box", "Triangle"};
   static const char *L[2] = {"PointLight", "SpotLight"};
   if (!d.name || !d.components) return false;
   // A kind's behaviour is its expressions (madarch-primitives.ads:24-30, madarch-lights.ads:20-24), never its name: one
   // that brings programs runs them, whatever it is called; the hand-written device functions are taken only by a kind
   // that brings none and carries one of the library's own names (the reference's own six kinds).
   k.type = -1;
   const bool has_programs = d.dist_code || d.normal_code || d.material_code;
   if (!has_programs)
      for (int t = 0; t < (is_light ? 2 : 4); ++t)
         if (strcmp(d.name, is_light ? L[t] : P[t]) == 0) k.type = t;
   const bool custom = has_programs && d.dist_code && d.normal_code && (is_light || d.material_code);
   if (custom) k.type = is_light ? (int)LK_CUSTOM : (int)PK_CUSTOM;
   if (k.type < 0 || d.n_components < 1 || d.n_components > 8 || d.max_count < 0) return false;
   k.max_count = d.max_count;
   k.ncomp = d.n_components;
   int off = 0;
   for (int i = 0; i < k.ncomp; ++i) {
      k.comp_name[i] = d.components[i].name ? d.components[i].name : "";
      k.comp_kind[i] = d.components[i].kind;
      off = pad_to(off, base_align(k.comp_kind[i]));
      k.comp_off[i] = off;
      off += base_size(k.comp_kind[i]);
   }
   k.elem_size = off;
   k.stride = pad_to(off, 16);
   if (custom) {
      for (int i = 0; i < k.ncomp; ++i) {
         if (k.comp_kind[i] != MDH_VEC3 && k.comp_kind[i] != MDH_FLOAT && k.comp_kind[i] != MDH_INT) return false;
         k.inst_floats += k.comp_kind[i] == MDH_VEC3 ? 3 : 1;
      }
      if (is_light) { // Sample (pos, normal, dir, dist: 10 argument floats) and Position (none)
         if (!valid_program(d.dist_code, d.dist_len, k.inst_floats, 10) || !valid_program(d.normal_code, d.normal_len, k.inst_floats, 0)) return false;
      } else if (!valid_program(d.dist_code, d.dist_len, k.inst_floats, 3) || !valid_program(d.normal_code, d.normal_len, k.inst_floats, 3) ||
                 !valid_program(d.material_code, d.material_len, k.inst_floats, 0))
         return false;
      k.x_dist.assign(d.dist_code, d.dist_code + d.dist_len);
      k.x_nrm.assign(d.normal_code, d.normal_code + d.normal_len);
      if (!is_light) k.x_mat.assign(d.material_code, d.material_code + d.material_len);
      return true;
   }
   if (!is_light) {
      k.f_d = k.offset_of("material_id", MDH_INT);
      switch (k.type) {
      case PK_SPHERE: k.f_a = k.offset_of("center", MDH_VEC3); k.f_b = k.offset_of("radius", MDH_FLOAT); k.f_c = 0; break;
      case PK_PLANE: k.f_a = k.offset_of("normal", MDH_VEC3); k.f_b = k.offset_of("offset", MDH_FLOAT); k.f_c = 0; break;
      case PK_BOX: k.f_a = k.offset_of("center", MDH_VEC3); k.f_b = k.offset_of("side", MDH_VEC3); k.f_c = 0; break;
      default: k.f_a = k.offset_of("v1", MDH_VEC3); k.f_b = k.offset_of("v2", MDH_VEC3); k.f_c = k.offset_of("v3", MDH_VEC3); break;
      }
   } else {
      k.f_a = k.offset_of("position", MDH_VEC3);
      if (k.type == LK_POINT) { k.f_b = k.offset_of("color", MDH_VEC3); k.f_c = 0; k.f_d = 0; }
      else { k.f_b = k.offset_of("direction", MDH_VEC3); k.f_c = k.offset_of("aperture", MDH_FLOAT); k.f_d = k.offset_of("color", MDH_VEC3); }
   }
   return k.f_a >= 0 && k.f_b >= 0 && k.f_c >= 0 && k.f_d >= 0;
}

// Single'Image keeps 6 significant digits: literals that reach the shaders through
// the generated GLSL text are rounded that way (scenes.adb:21-24,1200-1201;
// renderers.adb:119-134)
static float image_roundtrip(float x)
{
   char buf[64];
   snprintf(buf, sizeof buf, "%.5E", (double)x);
   return strtof(buf, nullptr);
}

// ------------------------------------------------------ the triangle BVH (MDH_OPT_TRIANGLE_BVH)
// Host side of bvh_triangles (mdh_device.h, where the layout and the margin argument are): a top-down build over the
// triangles of the committed scene, median of the centroids along the longest axis of their bounds, leaves of at most four
// triangles, nodes in depth-first order with skip links.  Deterministic: ties of the sort go to the lower index.
// Plain C++, no device: mdh_bvh_build hands it to tests.
struct BvhImage {
   std::vector<float4> nodes;  // two per node: {lo.xyz, skip} {hi.xyz, leaf}
   std::vector<int32_t> perm;  // the walked triangles in leaf order, then the always-evaluated ones in index order
   int n_always = 0, leaves = 0, depth = 0;
   float delta = 0.0f;
};
// Does the margin argument cover this triangle (9 floats)?  Finite, every coordinate within 2^20, no edge below 2^-12, and
// |nor| >= 2^-6 L^2 with L its longest edge; evaluated in double on the float vertices.
static bool bvh_covers(const float *v)
{
   for (int i = 0; i < 9; ++i)
      if (!(std::fabs(v[i]) <= 0x1p20f)) return false; // (NaN fails too)
   double e[3][3], l2[3];
   for (int a = 0; a < 3; ++a) { e[0][a] = (double)v[3 + a] - v[a]; e[1][a] = (double)v[6 + a] - v[3 + a]; e[2][a] = (double)v[a] - v[6 + a]; }
   for (int k = 0; k < 3; ++k) l2[k] = e[k][0] * e[k][0] + e[k][1] * e[k][1] + e[k][2] * e[k][2];
   const double lmax2 = std::max(l2[0], std::max(l2[1], l2[2])), lmin2 = std::min(l2[0], std::min(l2[1], l2[2]));
   if (!(lmin2 >= 0x1p-24)) return false;
   const double n[3] = {e[0][1] * e[2][2] - e[0][2] * e[2][1], e[0][2] * e[2][0] - e[0][0] * e[2][2], e[0][0] * e[2][1] - e[0][1] * e[2][0]};
   const double n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
   return n2 >= 0x1p-12 * lmax2 * lmax2;
}
struct BvhBuilder {
   const float *tri;
   BvhImage &out;
   std::vector<int32_t> ids;
   std::vector<float> cen; // 3 per triangle
   int node(int lo, int hi, int depth)
   {
      const int at = (int)out.nodes.size() / 2;
      out.nodes.resize(out.nodes.size() + 2);
      out.depth = std::max(out.depth, depth);
      float bl[3] = {INFINITY, INFINITY, INFINITY}, bh[3] = {-INFINITY, -INFINITY, -INFINITY}, cl[3] = {INFINITY, INFINITY, INFINITY}, ch[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (int q = lo; q < hi; ++q) {
         const float *v = tri + 9 * (size_t)ids[q];
         for (int c = 0; c < 9; ++c) { bl[c % 3] = std::min(bl[c % 3], v[c]); bh[c % 3] = std::max(bh[c % 3], v[c]); }
         for (int a = 0; a < 3; ++a) { cl[a] = std::min(cl[a], cen[3 * (size_t)ids[q] + a]); ch[a] = std::max(ch[a], cen[3 * (size_t)ids[q] + a]); }
      }
      int32_t leaf = -1;
      if (hi - lo <= 4) {
         leaf = (int32_t)out.perm.size() * 8 + (hi - lo);
         for (int q = lo; q < hi; ++q) out.perm.push_back(ids[q]);
         ++out.leaves;
      } else {
         int axis = 0;
         for (int a = 1; a < 3; ++a) if (ch[a] - cl[a] > ch[axis] - cl[axis]) axis = a;
         std::sort(ids.begin() + lo, ids.begin() + hi, [&](int32_t x, int32_t y) {
            const float cx = cen[3 * (size_t)x + axis], cy = cen[3 * (size_t)y + axis];
            return cx < cy || (cx == cy && x < y);
         });
         const int mid = lo + (hi - lo) / 2;
         node(lo, mid, depth + 1);
         node(mid, hi, depth + 1);
      }
      const int32_t skip = (int32_t)out.nodes.size() / 2;
      float fs, fl;
      memcpy(&fs, &skip, 4); memcpy(&fl, &leaf, 4);
      float4 a, b;
      a.x = bl[0]; a.y = bl[1]; a.z = bl[2]; a.w = fs;
      b.x = bh[0]; b.y = bh[1]; b.z = bh[2]; b.w = fl;
      out.nodes[2 * (size_t)at] = a; out.nodes[2 * (size_t)at + 1] = b;
      return at;
   }
};
static void bvh_build(const float *tri, int n, BvhImage &out)
{
   out = BvhImage();
   BvhBuilder b{tri, out, {}, {}};
   std::vector<int32_t> always;
   float lim = 0.0f;
   b.cen.resize(3 * (size_t)n);
   for (int i = 0; i < n; ++i) {
      const float *v = tri + 9 * (size_t)i;
      if (!bvh_covers(v)) { always.push_back(i); continue; }
      b.ids.push_back(i);
      for (int c = 0; c < 9; ++c) lim = std::max(lim, std::fabs(v[c]));
      for (int a = 0; a < 3; ++a) b.cen[3 * (size_t)i + a] = (float)(((double)v[a] + v[3 + a] + v[6 + a]) / 3.0);
   }
   out.perm.reserve(n);
   if (!b.ids.empty()) b.node(0, (int)b.ids.size(), 1);
   out.perm.insert(out.perm.end(), always.begin(), always.end());
   out.n_always = (int)always.size();
   out.delta = std::ldexp(1.0f + lim, -10);
}
// The builder by itself, without a renderer or a device: `tri_xyz` = n_tris x 9 floats (v1, v2, v3).  nodes_out takes the
// nodes as the kernels read them, 32 bytes each (room for max (1, 2 n_tris) of them), perm_out n_tris ints -- the walked
// triangles in leaf order, then the always-evaluated list --, delta_out[0] the margin delta and delta_out[1] rho.
// Returns the length of the always-evaluated list, or -MDH_E_INVALID.
extern "C" int32_t mdh_bvh_build(const float *tri_xyz, int32_t n_tris, void *nodes_out, int32_t *n_nodes, int32_t *perm_out, float *delta_out)
{
   if (n_tris < 0 || (n_tris > 0 && (!tri_xyz || !perm_out)) || !nodes_out || !n_nodes || !delta_out) { seterr(MDH_E_INVALID, "bad argument"); return -MDH_E_INVALID; }
   BvhImage im;
   bvh_build(tri_xyz, n_tris, im);
   if (!im.nodes.empty()) memcpy(nodes_out, im.nodes.data(), im.nodes.size() * sizeof(float4));
   if (n_tris > 0) memcpy(perm_out, im.perm.data(), (size_t)n_tris * 4);
   *n_nodes = (int32_t)im.nodes.size() / 2;
   delta_out[0] = im.delta; delta_out[1] = MDH_BVH_RHO;
   return im.n_always;
}

// -------------------------------------------------------------------- the renderer
#define MAX_MATERIALS 20 // glsl/materials.glsl:9
#ifndef MDH_ATLAS_SETS
#define MDH_ATLAS_SETS 3 // sets of probe atlases (and volumetric textures) that pipelined frames rotate through
#endif
#define MDH_LDS_WORKGROUP_BUDGET ((size_t)64 * 1024) // the LDS a workgroup may allocate: commit_scene fits the scene table into it, rad_replay_pick the recording kernel's rows

struct mdh_renderer {
   int W = 0, H = 0, device = 0;
   hipStream_t stream = nullptr;
   int npk = 0, nlk = 0;
   Kind pk[MDH_MAX_KINDS], lk[MDH_MAX_LIGHT_KINDS];
   int prim_base[MDH_MAX_KINDS] = {0};
   int host_count[MDH_MAX_KINDS] = {0}; // All_Primitives lengths (renderers.ads:128)
   float max_dist = 20.0f;
   mdh_partitioning part{};
   float pg_spacing[3], pg_offset[3], part_gpu_diag = 0.0f;
   int part_cells = 0, part_warnings = 0;
   mdh_probe_settings probes{};
   mdh_volumetrics vol{};
   float vstep = 0.1f, sstep = 0.1f;
   std::vector<uint8_t> scene_ubo; // std140 image of uniform block 1 (scenes.adb:551-600)
   int total_light_off = 0;
   uint8_t materials_ubo[16 + 32 * MAX_MATERIALS] = {0}; // renderers.adb:77-89
   int last_material_index = 0;
   float cam_pos[3] = {0, 0, 0}, cam_m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; // renderers.adb:225-226
   // options
   int opt_atlas = 0, opt_mode = 0, opt_ao = 3, opt_gbuffer = 0, opt_rank = 0, opt_world = 1, opt_timing = 0, opt_ada_div = 1, opt_spec = 2, opt_hyst = 0;
   // device state
   std::vector<float4> table_host;
   // The scene table lives in a ring of buffers: an edit (Set_Light every frame in the reference's examples) is
   // packed into the NEXT buffer and uploaded asynchronously from pinned memory while the frames in flight keep
   // reading theirs -- a scene edit does not drain the frame pipeline.  A buffer is rewritten only after the last
   // kernels that were launched with it have finished (tab_use, per stream).
   static const int TAB_RING = 4;
   DevBuf<float4> d_table_ring[TAB_RING];
   PinnedBuf<float4> h_table_ring[TAB_RING];
   int tab_slot = 0;
   static const int NSTREAMS = HOST_NSTREAMS; // main, probe, alternate, query, volumetric (stream_index)
   RingUse<TAB_RING> tab_use;
   Fence table_fence;     // signalled after the last upload, on the stream that made it
   size_t table_cap = 0;  // float4 every buffer of the ring holds
   bool table_dirty = true;
   // The space-partition table, in a ring like the scene table: Update_Partitioning builds into the next buffer
   // on the stream that uses it first and returns; frames in flight keep the buffer they were launched with
   // (KScene::part_table travels by value).  The builders' warning count comes back through pinned memory
   // and is waited for only when somebody asks (mdh_partition_warnings).
   static const int PART_RING = 4;
   DevBuf<int> d_part_ring[PART_RING];
   int part_slot = 0;
   RingUse<PART_RING> part_use;
   Fence part_fence; // the last build (its version counts Update_Partitioning's builds)
   Event ev_warn;    // the last read-back of its warning count
   DevBuf<int> d_warn;
   PinnedBuf<int> h_warn;
   bool warn_pending = false;
   hipStream_t query_stream = nullptr; // Eval_Distance_To: beside the frames in flight, not behind them
   hipStream_t vol_stream = nullptr;   // the camera-only volumetric passes of pipelined frames, beside their probe passes
   DevBuf<float> d_query; // Eval_Distance_To: points, normals, distances of the largest batch so far (7 floats a query)
   DevBuf<float> d_rays;  // the ray queries (mdh_raycast, ..): rays and results of the largest batch so far (MDH_RAY_WORDS words a ray)
   hipEvent_t rq_e0 = nullptr, rq_e1 = nullptr; // MDH_OPT_TIMING: around a ray query's kernel (taken from free_events once, handed back by mdh_destroy)
   bool rq_timed = false; // (the query in flight recorded them)
   double rq_ms = 0.0;    // ... and the time of the last one timed (mdh_ray_query_time)
   // the device-array ray queries (mdh_raycast_device, ..): the counter k_ray_stream's wavefronts take their rays from (one:
   // the launches follow one another on the query stream)
   DevBuf<unsigned> d_rq_next;
   // the surface mesher (mdh_surface_mesh, ..): the corners' values, the cells' vertices and the workgroups' counts of the
   // largest grid so far, and the host form's results of the largest capacities so far; used on the query stream alone
   DevBuf<float> d_surf_field;
   DevBuf<int> d_surf_map, d_surf_wg, d_surf_out;
   // a path-traced frame (mdh_path_frame_begin, ..): three fp32 sums a pixel, rows top first, used on the query stream alone,
   // and what mdh_path_frame_begin fixed -- the size, the camera as it stood, seed, bounces, jitter -- with the samples so far
   DevBuf<float> d_path_frame;
   struct PathFrame {
      bool open = false;
      int W = 0, H = 0, bounces = 0, jitter = 0;
      uint32_t seed = 0;
      int32_t samples = 0;
      KCamera cam;
      // an adaptive one (mdh_path_frame_begin_adaptive): the rule's parameters; samples is then the largest count a pixel can hold
      bool adaptive = false;
      int min_samples = 0, max_samples = 0;
      float tolerance = 0.0f, floor = 0.0f;
   } pf;
   // ... and an adaptive frame's further state (mdh_path_frame_adaptive.h), on the query stream alone: n a pixel; (m1, m2) a pixel;
   // the list of running pixels, a slot each, with the workgroups' totals and the grand total behind it; mdh_path_frame_stats' two words
   DevBuf<int> d_path_count, d_path_list;
   DevBuf<float> d_path_moments;
   DevBuf<long long> d_path_totals;
   int opt_pf_compact = 0; // MDH_OPT_PATH_FRAME_COMPACT (0: the value that wins in front of the obj_mesh, DESIGN.md section 4, "An adaptive path-traced frame")
   QueryBridge bridge; // every query's events to the caller's stream and to the frames (query_enqueue; created by the first that needs one)
   int opt_rq_refill = MDH_RAY_STREAM_REFILL_DEFAULT; // MDH_OPT_RAY_STREAM_REFILL
   int opt_rq_groups = 0;                             // MDH_OPT_RAY_STREAM_GROUPS (0: as many workgroups as are resident)
   // Two sets of probe atlases.  `last` is the set the most recent frame wrote: every read, write and
   // single pass works on it in place.  A pipelined mdh_render (frame overlap, see mdh_render) writes the
   // other set while the previous frame's screen pass still reads this one, then flips.
   // (MDH_ATLAS_SETS of them, three since round 3: with two, the probe passes of frame N + 1 write the set the screen pass of
   //  frame N - 1 still reads and wait for it -- the chain screen (N - 1) -> probes (N + 1) -> screen (N + 1) bound the frame
   //  rate of pipelined frames; with three they wait for the screen pass of frame N - 2, long gone)
   static const int NSETS = MDH_ATLAS_SETS;
   DevBuf<> d_rad2[NSETS], d_irr2[NSETS];
   DevBuf<> d_rad_mips[NSETS]; // MDH_OPT_RADIANCE_MIPS: levels 1 .. radiance_lods of each set's radiance atlas, one behind the other
   int opt_mips = 0;
   int n_cus = 0;                          // compute units of the device
   // RadOrder (mdh_kernels.h): every ray's primary-march steps, the rays sorted by them, the sort's histograms
   DevBuf<float> d_irr_taps;     // k_irradiance's scratch: the taps of the pass's probes (mdh_kernels.h)
   DevBuf<unsigned char> d_rad_steps;      // one group, sized for d_rad_steps.cap rays (pass_radiance)
   DevBuf<unsigned> d_rad_order, d_rad_hist;
   ResortClock<RadOrderOf> rad_order;      // when they are sorted again, and what the stored order is of (pass_radiance)
   unsigned long geometry_edits = 0;       // primitives set or added so far
   int opt_rad_order = MDH_RAD_ORDER_DEFAULT;
   // MDH_OPT_RADIANCE_REPLAY (mdh_march.h: RayRecord): one record per probe ray of the slice, indexed by the ray.
   // ONE buffer serves all three atlas sets: a record holds nothing of an atlas, and it is written and read by radiance
   // passes only.  Those run on the probe stream, one behind the other, or on the main stream after the join that orders a
   // single pass against the frames in flight (join_main; the probe stream is ordered after the main stream's work when
   // frames go in flight again) -- the order that d_rad_order relies on between the pass that sorts and the pass that reads.
   // It is allocated, grown and freed like d_rad_steps / d_rad_order: with both streams drained.
   DevBuf<RayRecord> d_rad_rec;            // (its capacity: rays)
   ReplaySchedule<RadRecKey> rad_replay;   // march, record or replay (rad_replay_pick chooses, pass_radiance reports)
   unsigned long march_inputs = 0;         // edits besides geometry_edits that change what a march kernel reads or which one runs (options, partition builds)
   int opt_rad_replay = 1;
   // MDH_OPT_SCREEN_REPLAY (mdh_march.h: PixelRecord): one record per pixel of the rank's tiles, indexed by the pixel
   // (mdh_kernels.h: screen_record_index).  ONE buffer: a record holds nothing of an atlas, a framebuffer or a light.  Screen
   // passes of frames in flight alternate between the main and the alternate stream and nothing else orders them against each
   // other, so the buffer carries its own order: every pass that reads it marks its stream (scr_rec_reads), the pass
   // that writes it retires the readers on the other streams and signals scr_rec_written, and a reader on a stream that
   // has not seen the latest write waits for that.  Allocated, grown and freed with every stream drained.
   DevBuf<PixelRecord> d_scr_rec;          // (its capacity: pixels, own tiles * 64)
   Fence scr_rec_written;                  // one group, created with the first records (pass_screen)
   RingUse<1> scr_rec_reads;
   ReplaySchedule<ScrRecKey> scr_replay;   // march, record or replay (scr_replay_pick chooses, pass_screen reports); alone in surviving a failed allocation of its records
   unsigned long reflect_edits = 0;
   int opt_scr_replay = 0;
   // MDH_OPT_SCREEN_ORDER (ScreenArgs, mdh_kernels.h): the screen pass's tiles in the order of their wavefronts' durations
   // (the three buffers and the two events are one group, created by the first pass that sorts: pass_screen)
   DevBuf<unsigned char> d_scr_cost;             // [tiles] sort keys, written by the pass that is followed by a sort
   DevBuf<unsigned> d_scr_order[2];              // [tiles] two buffers: passes in flight keep reading the one they were launched with
   DevBuf<unsigned> d_scr_hist;
   ResortClock<ScrOrderOf> scr_order;            // when they are sorted again, and what the stored order is of (pass_screen, screen_sort_tiles)
   Fence scr_sorted;                             // the last sort
   Event ev_scr_other;
   int opt_scr_order = 1;
   int opt_scr_split = MDH_SCREEN_SPLIT_DEFAULT; // MDH_OPT_SCREEN_SPLIT: the wavefronts a split screen launch may have (0: never split)
   std::map<std::pair<const void *, size_t>, int> resident; // workgroups per CU of (kernel, LDS bytes): rad_first_round
   int last = 0;
   int opt_overlap = 2;
   int opt_irr_all = 1; // MDH_OPT_IRRADIANCE_ALL
   int opt_residency = 0; // MDH_OPT_TABLE_RESIDENCY as set: 1 = global residency forced, 0 = chosen by the table's size (commit_scene)
   int residency = 0;     // ... of the committed scene: 0 = the whole table in LDS, 1 = geometry and material ids read from its image in memory
   int opt_tri_bvh = 0;   // MDH_OPT_TRIANGLE_BVH as set
   bool bvh_active = false; // ... and of the committed scene: the option is on and a Triangle kind is declared (global residency, the MDH_PF_BVH kernels)
   BvhImage bvh;            // the hierarchy over bvh_tris, the triangles it was built from (commit_scene rebuilds it when they change)
   std::vector<float> bvh_tris;
   bool bvh_built = false;
   int opt_jit = 1; // user-defined kinds: 1 = compile the MDH_X programs with hiprtc, 0 = interpret them (MDH_OPT_JIT)
   std::string jit_kinds; // mdh_jit_kinds.h of this scene (generated once)
   hipStream_t probe_stream = nullptr;   // radiance + irradiance passes of pipelined frames
   hipStream_t alt_stream = nullptr;     // screen pass of every other pipelined frame
   Event ev_screen[NSETS], ev_probe[NSETS], ev_join, ev_join_alt;
   Event ev_vol[NSETS]; // the camera-only volumetric passes of a pipelined frame (on vol_stream, beside its probe passes)
   bool ev_screen_valid[NSETS] = {false};
   bool alt_pending = false; // work on alt_stream that `stream` has not been ordered after yet
   // an open frame (mdh_frame_begin .. mdh_frame_end)
   bool in_frame = false, frame_pipelined = false;
   bool in_frame_passes = false; // run_pass is called for the passes that end an open frame (frame_end_passes)
   bool fuse_scat_march = false; // the frame's visibility launch also marches the scattering texels' camera rays (k_visibility)
   int frame_cur = 0;
   int scr_parity = 0; // which screen stream / framebuffer the last pipelined frame drew on
   bool main_dirty = true; // work went to `stream` outside a pipelined frame since the probe stream last joined it
   // froxel and scattering textures, one per atlas set: the volumetric passes of a pipelined frame run on the
   // probe stream into the set that frame produces
   DevBuf<float> d_vis2[NSETS];
   DevBuf<float4> d_scat2[NSETS];
   DevBuf<float4> d_fb2[2]; // two framebuffers: consecutive pipelined frames draw on two streams
   int fb_last = 0;                       // the one the most recent frame drew
   // mdh_swap_buffers: a ring of RGBA8 copies of a framebuffer, each a device buffer (written on the stream that
   // drew the frame) and a pinned host buffer (filled on a stream of its own, so no screen pass queues behind a copy)
   static constexpr int FRONT_RING = 3;
   DevBuf<unsigned> d_front[FRONT_RING];
   PinnedBuf<unsigned char> h_front[FRONT_RING];
   Event ev_front[FRONT_RING]; // slot's host copy done
   Event ev_packed;
   hipStream_t copy_stream = nullptr;
   // MDH_OPT_WINDOW: the screen pass itself stores the RGBA8 pixels into a ring of pinned host buffers (over PCIe,
   // no copy and no extra kernel); a swap then only marks the last one with an event
   static constexpr int WIN_RING = 4;
   int opt_window = 2; // MDH_OPT_WINDOW: 0 never, 1 always, 2 from the first mdh_swap_buffers on
   PinnedBuf<unsigned> h_win[WIN_RING];
   Event ev_win[WIN_RING];
   long long win_passes = 0; // screen passes that wrote a window slot; the last one wrote slot (win_passes - 1) % WIN_RING
   bool win_valid = false;   // the last screen pass wrote a window slot
   int win_owner[2] = {0, 1};
   // what mdh_front_buffer returns: set by mdh_swap_buffers
   const unsigned char *front_ptr = nullptr;
   hipEvent_t front_ev = nullptr; // (borrowed: the ev_win or ev_front of that slot)
   long long swaps = 0; // mdh_swap_buffers calls so far; the last one went to slot (swaps - 1) % FRONT_RING
   // (rank, world) whose tiles are the only non-zero pixels of a framebuffer; {0, 1}: every pixel may be set
   int fb_owner[2][2] = {{-1, -1}, {-1, -1}};
   // geometry buffer: [which framebuffer] x {index, t, steps} (int32 / float / int32 per pixel)
   DevBuf<> d_gb2[2][3];
   KScene ks{};
   // timing: event pairs recorded around every pass, resolved lazily (no host sync per pass)
   struct Pending { int pass; hipEvent_t e0, e1; };
   std::vector<Pending> pending;
   std::vector<hipEvent_t> free_events;
   double pass_ms[MDH_PASS_COUNT] = {0};
   long long pass_n[MDH_PASS_COUNT] = {0};
   hipStream_t own_stream = nullptr;
#ifdef MDH_DIAG
   unsigned long long work[MDH_PASS_COUNT][4] = {{0}}; // g_work of the last run of each pass (mdh_diag_work)
   int32_t variant[MDH_PASS_COUNT][2] = {{0}};          // pick_kernel's pfk and pow2 at the last run of each pass (mdh_diag_variant)
#endif
   // the communicator of a sharded run (mdh_comm_init): one rank per process and GPU.  With it mdh_render runs the
   // exchange of the atlas slices itself, on the probe stream, between the probe passes.
   ncclComm_t comm = nullptr;
   // mdh_comm_abort may come from a watchdog thread while the owning thread is inside a collective: the
   // watchdog then only aborts (ncclCommAbort, once) and raises the flag; the owning thread forgets the handle when its
   // call returns.  With nobody inside, the aborting thread owns the state and drops everything itself.
   std::atomic<bool> comm_aborted{false};
   std::atomic<int> comm_busy{0};
   DevBuf<double> d_comm_scratch; // barrier / max reductions
   struct PeerState *peer = nullptr; // the peer exchange (mdh_peer_init): the same sharded frame, its exchange as copies
   bool irr_lds_granted = false; // k_irradiance may use up to 160 KiB of dynamic LDS on this renderer's device
   // MDH_OPT_PROBE_SETTLE (mdh_host.h: SettleTracker): the frames' irradiance passes report whether they changed a texel; once
   // MDH_SETTLE_PASSES of them in a row did not, under inputs that still hold, frames leave their probe passes out.
   // (the slots and the counters are one group, created by the first tracked pass: settle_args)
   SettleTracker settle;
   PinnedBuf<SettleSlot> h_settle; // its slots
   DevBuf<unsigned long long> d_settle; // k_irradiance's counter: workgroups done | texels changed << 32
   bool settle_no_memory = false;  // their allocation failed: passes run untracked
   int opt_settle = 1;
   int frame_probe_seq = 0;        // the open frame's probe passes so far: 0 none, 1 one radiance pass, 2 radiance then irradiance, -1 anything else
   long long settle_skipped = 0;   // probe passes of frames that were not launched
};
// Something a probe pass reads or writes may have changed: every entry point calls this except the few that provably touch
// none of it ("Exact work elimination", item 13 lists them).  The next frame runs its probe passes.
static void settle_bump(mdh_renderer *r) { if (r) r->settle.bump(); }
// a frame of a single rank in screen mode 0: the only kind whose probe passes may be left out (collectives stay matched across ranks)
static bool settle_eligible(const mdh_renderer *r) { return MDH_PROBE_SETTLE && r->opt_mode == 0 && !r->comm && !r->peer && r->opt_world == 1; }

// Order `stream` after everything pipelined frames put on the alternate screen stream (which
// itself waited for the probe stream): called before any operation outside a pipelined frame.
static int join_main(mdh_renderer *r)
{
   if (!r->alt_pending) return MDH_OK;
   HIP_TRY(hipEventRecord(r->ev_join_alt.ev, r->alt_stream));
   HIP_TRY(hipStreamWaitEvent(r->stream, r->ev_join_alt.ev, 0));
   r->alt_pending = false;
   return MDH_OK;
}
// Host wait for a set of this renderer's streams: bit si of `mask` is the stream that stream_index calls si (those that
// do not exist yet are skipped), SYNC_OWN the renderer's own main stream while the caller has supplied another.
enum : unsigned { SYNC_MAIN = 1, SYNC_PROBE = 2, SYNC_ALT = 4, SYNC_QUERY = 8, SYNC_VOL = 16, SYNC_OWN = 32, SYNC_ALL = 63 };
static int sync_streams(mdh_renderer *r, unsigned mask)
{
   const hipStream_t sts[] = {r->stream, r->probe_stream, r->alt_stream, r->query_stream, r->vol_stream, r->own_stream != r->stream ? r->own_stream : nullptr};
   for (int si = 0; si < 6; ++si)
      if ((mask >> si & 1u) && sts[si]) HIP_TRY(hipStreamSynchronize(sts[si]));
   return MDH_OK;
}
// host wait for everything this renderer has enqueued anywhere (its own streams only: other renderers of the process run on)
static int drain_streams(mdh_renderer *r) { return sync_streams(r, SYNC_ALL); }
static hipEvent_t get_event(mdh_renderer *r)
{
   if (!r->free_events.empty()) { hipEvent_t e = r->free_events.back(); r->free_events.pop_back(); return e; }
   hipEvent_t e = nullptr;
   if (hipEventCreate(&e) != hipSuccess) return nullptr;
   return e;
}
// Fold event pairs into the per-pass totals.  wait = true: after every stream a pass can run on has drained, all of
// them; wait = false (the bound on the pending list, at a frame boundary): only the pairs whose end event has already
// completed, the rest stay pending.  Entries leave the list as they are folded, so an error half way leaves no pair behind
// whose events were already handed back.
static int resolve_timing(mdh_renderer *r, bool wait = true)
{
   if (r->pending.empty()) return MDH_OK;
   if (wait) {
      { int jr = join_main(r); if (jr != MDH_OK) return jr; }
      { int sr = sync_streams(r, SYNC_MAIN | SYNC_PROBE | SYNC_ALT | SYNC_VOL | SYNC_OWN); if (sr != MDH_OK) return sr; } // (SYNC_VOL: timed volumetric passes of pipelined frames)
   }
   int rc = MDH_OK;
   size_t keep = 0;
   for (size_t i = 0; i < r->pending.size(); ++i) {
      const mdh_renderer::Pending p = r->pending[i];
      float ms = 0.0f;
      hipError_t e = rc != MDH_OK ? hipErrorNotReady : ((wait || hipEventQuery(p.e1) == hipSuccess) ? hipEventElapsedTime(&ms, p.e0, p.e1) : hipErrorNotReady);
      if (e == hipSuccess) {
         r->pass_ms[p.pass] += ms;
         r->pass_n[p.pass] += 1;
         r->free_events.push_back(p.e0);
         r->free_events.push_back(p.e1);
         continue;
      }
      if (e != hipErrorNotReady || wait) {
         if (rc == MDH_OK) { snprintf(g_err, sizeof g_err, "hipEventElapsedTime failed: %s", hipGetErrorString(e)); rc = MDH_E_DEVICE; }
      }
      r->pending[keep++] = p;
   }
   r->pending.resize(keep);
   if (!wait) (void)hipGetLastError(); // (a hipErrorNotReady of the queries is no error of the next launch)
   return rc;
}
// the bound on the pending list, applied where no frame is open
static int bound_timing(mdh_renderer *r) { return r->pending.size() >= 4096 ? resolve_timing(r, false) : MDH_OK; }

static int probe_total(const mdh_renderer *r) { return r->probes.probe_count[0] * r->probes.probe_count[1]; }
static size_t texel_bytes(const mdh_renderer *r) { return r->opt_atlas == 0 ? 4 : 16; }
static size_t atlas_bytes(const mdh_renderer *r, int tex)
{
   int res = tex == MDH_TEX_RADIANCE ? r->probes.radiance_resolution : r->probes.irradiance_resolution;
   return (size_t)probe_total(r) * res * res * texel_bytes(r);
}
static void own_probes(const mdh_renderer *r, int *b, int *e)
{
   long long P = probe_total(r);
   const long long rank = r->opt_rank < r->opt_world ? r->opt_rank : r->opt_world - 1; // (rank >= world is refused where a slice is used)
   *b = (int)(P * rank / r->opt_world);
   *e = (int)(P * (rank + 1) / r->opt_world);
}

// the partition table of a renderer: [cell][kinds + Index_Count] ints (what the reference's SSBO holds, mdh_read_partitioning),
// then the same candidate sets as bits, [cell][words] (partitioning_closest_bits, mdh_device.h)
// (the bits start on a 16-byte boundary and are a whole number of float4: workgroups stage them into LDS 16 bytes at a time)
static size_t part_table_ints(const mdh_renderer *r) { return ((size_t)r->part_cells * (r->npk + r->part.index_count) + 3) / 4 * 4; }
static int part_mask_words(const mdh_renderer *r)
{
   int declared = 0;
   for (int k = 0; k < r->npk; ++k) declared += r->pk[k].max_count;
   return declared > 32 ? (declared + 31) / 32 : 2; // (at least two: scenes of up to 64 primitives read a cell's bits as one 8-byte pair)
}
static size_t part_bits_ints(const mdh_renderer *r) { return ((size_t)r->part_cells * part_mask_words(r) + 3) / 4 * 4; }
static size_t part_buffer_ints(const mdh_renderer *r) { return part_table_ints(r) + part_bits_ints(r); }
// The cells' bits are read from memory (L1 / L2), never staged into LDS (KScene::part_bits_f4 = 0).  (measured: staged, the
// 16 KB of the reference's simple_scene, 2000 cells x 2 words, leave room for five workgroups per CU instead of seven and its
// screen pass takes 0.78 instead of 0.70 ms, although no march step reads memory any more)
static float rd_f(const mdh_renderer *r, int off) { float f; memcpy(&f, r->scene_ubo.data() + off, 4); return f; }
static int rd_i(const mdh_renderer *r, int off) { int32_t i; memcpy(&i, r->scene_ubo.data() + off, 4); return i; }
static float4 mk4(float x, float y, float z, float w) { float4 v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
static float4 rd_v3w(const mdh_renderer *r, int off, float w) { return mk4(rd_f(r, off), rd_f(r, off + 4), rd_f(r, off + 8), w); }
static float i_as_f(int i) { float f; memcpy(&f, &i, 4); return f; }
static int f_as_i(float f) { int i; memcpy(&i, &f, 4); return i; }

// Repack the std140 images into the float4 table the kernels stage into LDS
// (layout in mdh_device.h) and refresh the SGPR header.
static int stream_index(const mdh_renderer *r, hipStream_t st) { return st == r->probe_stream ? 1 : (st == r->alt_stream ? 2 : (st == r->query_stream ? 3 : (st == r->vol_stream ? 4 : 0))); }
// before a kernel that stages the table is launched on `st`: order `st` after the table's upload
static int table_acquire(mdh_renderer *r, hipStream_t st)
{
   const int si = stream_index(r, st);
   HIP_TRY(r->table_fence.wait(st, si));
   if (r->part.enable) HIP_TRY(r->part_fence.wait(st, si)); // ... and after the build of the partition table
   return MDH_OK;
}
// after it: the table buffer is in use on `st` until this point of the stream
static int table_release(mdh_renderer *r, hipStream_t st)
{
   const int si = stream_index(r, st);
   HIP_TRY(r->tab_use.mark(r->tab_slot, st, si));
   if (r->part.enable) HIP_TRY(r->part_use.mark(r->part_slot, st, si));
   return MDH_OK;
}

static bool has_custom_kinds(const mdh_renderer *r)
{
   bool c = false;
   for (int k = 0; k < r->npk; ++k) c = c || r->pk[k].type == PK_CUSTOM;
   for (int k = 0; k < r->nlk; ++k) c = c || r->lk[k].type == LK_CUSTOM;
   return c;
}

static int commit_scene(mdh_renderer *r, hipStream_t up)
{
   KScene &s = r->ks;
   s.max_dist = r->max_dist;
   std::vector<float4> &t = r->table_host;
   t.clear();
   int H[H_INTS] = {0};
   t.resize(H_INTS / 4); // the int header, filled in at the end
   H[H_NK] = r->npk;
   H[H_NL] = r->nlk;
   for (int ty = 0; ty < 4; ++ty) { s.tcount[ty] = 0; s.tslot[ty] = 0; }
   // geometry: kind by kind, the elements below the runtime count
   for (int k = 0; k < r->npk; ++k) {
      const Kind &kd = r->pk[k];
      int n = rd_i(r, kd.count_off);
      if (n < 0) n = 0;
      if (n > kd.max_count) n = kd.max_count;
      H[H_KTYPE + k] = kd.type; H[H_KCOUNT + k] = n; H[H_KBASE + k] = r->prim_base[k]; H[H_KMAX + k] = kd.max_count; H[H_KSLOT + k] = (int)t.size();
      if (kd.type == PK_CUSTOM) { // instances packed as MDH_X_COMP addresses them: components in order, vec3 = 3 floats
         const int stride = (kd.inst_floats + 3) / 4;
         H[H_KSTRIDE + k] = stride;
         for (int i = 0; i < n; ++i) {
            const int b = kd.array_off + kd.stride * i;
            float buf[32] = {0};
            int f = 0;
            for (int c = 0; c < kd.ncomp; ++c) {
               const int nf = kd.comp_kind[c] == MDH_VEC3 ? 3 : 1;
               memcpy(buf + f, r->scene_ubo.data() + b + kd.comp_off[c], 4 * nf); // ints travel as raw bits
               f += nf;
            }
            for (int q = 0; q < stride; ++q) t.push_back(mk4(buf[4 * q], buf[4 * q + 1], buf[4 * q + 2], buf[4 * q + 3]));
         }
         continue;
      }
      H[H_KSTRIDE + k] = kd.type == PK_TRIANGLE ? 3 : (kd.type == PK_BOX ? 2 : 1);
      s.tcount[kd.type] = n; s.tslot[kd.type] = (int)t.size();
      for (int i = 0; i < n; ++i) {
         int b = kd.array_off + kd.stride * i;
         switch (kd.type) {
         case PK_SPHERE: t.push_back(rd_v3w(r, b + kd.f_a, rd_f(r, b + kd.f_b))); break;
         case PK_PLANE: t.push_back(rd_v3w(r, b + kd.f_a, rd_f(r, b + kd.f_b))); break;
         case PK_BOX: t.push_back(rd_v3w(r, b + kd.f_a, 0.0f)); t.push_back(rd_v3w(r, b + kd.f_b, 0.0f)); break;
         default: t.push_back(rd_v3w(r, b + kd.f_a, 0.0f)); t.push_back(rd_v3w(r, b + kd.f_b, 0.0f)); t.push_back(rd_v3w(r, b + kd.f_c, 0.0f)); break;
         }
      }
   }
   // axis-aligned planes fold into six offsets; the others are repeated as "general planes"
   // for closest_primitive (the per-kind copy above stays complete for the arg-min / normals)
   {
      const float inf = INFINITY;
      for (int g = 0; g < 6; ++g) { s.axis_off[g] = inf; H[H_AXIS_IDX + g] = -1; }
      int per_dir[6] = {0, 0, 0, 0, 0, 0};
      s.n_axis = 0;
      s.gplane_slot = (int)t.size();
      s.gplane_count = 0;
      for (int k = 0; k < r->npk; ++k) {
         const Kind &kd = r->pk[k];
         if (kd.type != PK_PLANE) continue;
         for (int i = 0; i < H[H_KCOUNT + k]; ++i) {
            int b = kd.array_off + kd.stride * i;
            float n[3] = {rd_f(r, b + kd.f_a), rd_f(r, b + kd.f_a + 4), rd_f(r, b + kd.f_a + 8)};
            float o = rd_f(r, b + kd.f_b);
            int axis = -1, nz = 0;
            for (int c = 0; c < 3; ++c)
               if (n[c] != 0.0f) { ++nz; axis = c; }
            if (nz == 1 && (n[axis] == 1.0f || n[axis] == -1.0f) && o == o) {
               int g = 2 * axis + (n[axis] < 0.0f ? 1 : 0);
               if (o < s.axis_off[g]) { s.axis_off[g] = o; H[H_AXIS_IDX + g] = r->prim_base[k] + i; }
               ++per_dir[g];
               ++s.n_axis;
            } else {
               t.push_back(mk4(n[0], n[1], n[2], o));
               ++s.gplane_count;
            }
         }
      }
      // the typed arg-min of closest_primitive_info needs every plane to be one of the six folded ones
      // (two planes of one direction can tie after rounding, and the tie goes to the lower index)
      H[H_FASTINFO] = s.gplane_count == 0;
      for (int g = 0; g < 6; ++g)
         if (per_dir[g] > 1) H[H_FASTINFO] = 0;
      for (int ty = 0; ty < 4; ++ty) H[H_TBASE + ty] = 0;
      for (int k = 0; k < r->npk; ++k) {
         if (r->pk[k].type == PK_CUSTOM) H[H_FASTINFO] = 0;
         else H[H_TBASE + r->pk[k].type] = r->prim_base[k];
      }
   }
   // segment_clear's threshold EPS + delta and its coordinate bound lim (mdh_device.h, where the argument is): delta =
   // 2^-12 (1 + lim) with lim = 2 (M + 1), M the largest magnitude the scan reads -- coordinates, offsets, radii, half-sizes.
   // Off (0) for scenes the bound does not cover: triangles, user-defined kinds, negative radii or half-sizes, non-finite
   // values, and a max_dist (every SDF value is at most that) not above the threshold.
   {
      bool on = s.tcount[PK_TRIANGLE] == 0;
      for (int k = 0; k < r->npk; ++k) on = on && r->pk[k].type != PK_CUSTOM;
      float M = 0.0f;
      auto see = [&](float v) { if (std::isfinite(v)) M = std::max(M, std::fabs(v)); else on = false; };
      for (int g = 0; g < 6; ++g)
         if (s.axis_off[g] != INFINITY) see(s.axis_off[g]);
      for (int i = 0; i < s.gplane_count; ++i) { const float4 p = t[s.gplane_slot + i]; see(p.x); see(p.y); see(p.z); see(p.w); }
      for (int i = 0; i < s.tcount[PK_SPHERE]; ++i) {
         const float4 a = t[s.tslot[PK_SPHERE] + i];
         see(a.x); see(a.y); see(a.z); see(a.w);
         on = on && a.w >= 0.0f;
      }
      for (int i = 0; i < s.tcount[PK_BOX]; ++i) {
         const float4 c = t[s.tslot[PK_BOX] + 2 * i], e = t[s.tslot[PK_BOX] + 2 * i + 1];
         see(c.x); see(c.y); see(c.z); see(e.x); see(e.y); see(e.z);
         on = on && e.x >= 0.0f && e.y >= 0.0f && e.z >= 0.0f;
      }
      const float lim = 2.0f * (M + 1.0f);
      const float thr = 0.001f + std::ldexp(1.0f + lim, -12); // (MDH_EPS + delta)
      on = on && std::isfinite(lim) && std::isfinite(thr) && s.max_dist > thr;
      H[H_VCLEAR] = f_as_i(on ? thr : 0.0f);
      H[H_VCLEAR_LIM] = f_as_i(lim);
   }
   // material ids (int32), 4 per float4
   // the MDH_X programs of the user-defined kinds (ints, read through hdr ())
   for (int k = 0; k < r->npk; ++k) {
      const Kind &kd = r->pk[k];
      if (kd.type != PK_CUSTOM) continue;
      const std::vector<int32_t> *progs[3] = {&kd.x_dist, &kd.x_nrm, &kd.x_mat};
      const int hs[3] = {H_XDIST, H_XNRM, H_XMAT}, hn[3] = {H_XDISTN, H_XNRMN, H_XMATN};
      for (int q = 0; q < 3; ++q) {
         H[hs[q] + k] = (int)t.size() * 4;
         H[hn[q] + k] = (int)progs[q]->size();
         for (size_t w0 = 0; w0 < progs[q]->size(); w0 += 4) {
            float m[4] = {0, 0, 0, 0};
            for (size_t j = 0; j < 4 && w0 + j < progs[q]->size(); ++j) m[j] = i_as_f((*progs[q])[w0 + j]);
            t.push_back(mk4(m[0], m[1], m[2], m[3]));
         }
      }
   }
   for (int k = 0; k < r->npk; ++k) {
      const Kind &kd = r->pk[k];
      if (kd.type == PK_CUSTOM) continue;
      H[H_KMAT + k] = (int)t.size() * 4;
      for (int i0 = 0; i0 < H[H_KCOUNT + k]; i0 += 4) {
         float m[4] = {0, 0, 0, 0};
         for (int j = 0; j < 4 && i0 + j < H[H_KCOUNT + k]; ++j) m[j] = i_as_f(rd_i(r, kd.array_off + kd.stride * (i0 + j) + kd.f_d));
         t.push_back(mk4(m[0], m[1], m[2], m[3]));
      }
   }
   const size_t geo_begin = H_INTS / 4, geo_end = t.size(); // geometry, general planes, programs, material ids: what global residency leaves in memory
   for (int k = 0; k < r->nlk; ++k) {
      const Kind &kd = r->lk[k];
      int n = rd_i(r, kd.count_off);
      if (n < 0) n = 0;
      if (n > kd.max_count) n = kd.max_count;
      H[H_LTYPE + k] = kd.type; H[H_LCOUNT + k] = n; H[H_LSLOT + k] = (int)t.size();
      if (kd.type == LK_CUSTOM) { // instance floats as MDH_X_COMP addresses them, then the two programs
         const int stride = (kd.inst_floats + 3) / 4;
         H[H_LSTRIDE + k] = stride;
         for (int i = 0; i < n; ++i) {
            const int b = kd.array_off + kd.stride * i;
            float buf[32] = {0};
            int f = 0;
            for (int c = 0; c < kd.ncomp; ++c) {
               const int nf = kd.comp_kind[c] == MDH_VEC3 ? 3 : 1;
               memcpy(buf + f, r->scene_ubo.data() + b + kd.comp_off[c], 4 * nf);
               f += nf;
            }
            for (int q = 0; q < stride; ++q) t.push_back(mk4(buf[4 * q], buf[4 * q + 1], buf[4 * q + 2], buf[4 * q + 3]));
         }
         const std::vector<int32_t> *progs[2] = {&kd.x_dist, &kd.x_nrm};
         const int hs[2] = {H_XLSAMPLE, H_XLPOS}, hn[2] = {H_XLSAMPLEN, H_XLPOSN};
         for (int q = 0; q < 2; ++q) {
            H[hs[q] + k] = (int)t.size() * 4;
            H[hn[q] + k] = (int)progs[q]->size();
            for (size_t w0 = 0; w0 < progs[q]->size(); w0 += 4) {
               float m4[4] = {0, 0, 0, 0};
               for (size_t j = 0; j < 4 && w0 + j < progs[q]->size(); ++j) m4[j] = i_as_f((*progs[q])[w0 + j]);
               t.push_back(mk4(m4[0], m4[1], m4[2], m4[3]));
            }
         }
         continue;
      }
      for (int i = 0; i < n; ++i) {
         int b = kd.array_off + kd.stride * i;
         if (kd.type == LK_POINT) { t.push_back(rd_v3w(r, b + kd.f_a, 0.0f)); t.push_back(rd_v3w(r, b + kd.f_b, 0.0f)); }
         else { t.push_back(rd_v3w(r, b + kd.f_a, rd_f(r, b + kd.f_c))); t.push_back(rd_v3w(r, b + kd.f_b, 0.0f)); t.push_back(rd_v3w(r, b + kd.f_d, 0.0f)); }
      }
   }
   s.total_lights = rd_i(r, r->total_light_off);
   s.mat_slot = (int)t.size();
   for (int m = 0; m < MAX_MATERIALS; ++m) {
      float f[5];
      memcpy(f, r->materials_ubo + 16 + 32 * m, 20);
      t.push_back(mk4(f[0], f[1], f[2], f[3]));
      t.push_back(mk4(f[4], 0, 0, 0));
   }
   s.u8_slot = -1; // (RGB8 texels are decoded in registers: u8_unorm, mdh_device.h)
   // RESIDENCY (mdh_device.h: Geo).  A table that fits the LDS budget is staged whole, as it is laid out above.  One that does
   // not -- or any, under MDH_OPT_TABLE_RESIDENCY 1 -- is laid out with its resident part first: header ints, lights, materials,
   // the k / 255 table, then everything the kernels read from the image in memory; every workgroup stages the first
   // table_f4 float4 only.  User-defined kinds interpret their instances out of LDS: they keep the whole table there.
   // (the march kernels park MDH_PARK_DWORDS floats per thread behind the table, lds_bytes_march)
   {
      const size_t park = (size_t)MDH_SCR_PARK_ROWS * MDH_BLOCK * sizeof(float), budget = MDH_LDS_WORKGROUP_BUDGET;
      const size_t n_geo = geo_end - geo_begin, n_res = t.size() - n_geo;
      const bool has_custom = has_custom_kinds(r);
      const bool fits = t.size() * 16 + park <= budget;
      if (fits && r->opt_residency == 1 && has_custom)
         return seterr(MDH_E_INVALID, "MDH_OPT_TABLE_RESIDENCY 1: scenes with user-defined kinds keep their table in LDS");
      if (!fits && (has_custom || n_res * 16 + park > budget))
         return seterr(MDH_E_INVALID, "scene tables exceed the 64 KiB LDS budget of a workgroup");
      // MDH_OPT_TRIANGLE_BVH: the walk reads nodes and triangles from the image -- global residency, whatever the size
      int tri_kinds = 0;
      for (int k = 0; k < r->npk; ++k) tri_kinds += r->pk[k].type == PK_TRIANGLE;
      r->bvh_active = r->opt_tri_bvh != 0 && tri_kinds == 1 && !has_custom && r->part.enable == 0;
      r->residency = !fits || r->opt_residency == 1 || r->bvh_active ? 1 : 0;
      s.table_f4 = (int)t.size();
      if (r->residency) {
         std::rotate(t.begin() + geo_begin, t.begin() + geo_end, t.end());
         const int up = (int)(n_res - geo_begin), down = (int)n_geo; // float4 the memory part moves up, the resident part down
         for (int k = 0; k < r->npk; ++k) { H[H_KSLOT + k] += up; H[H_KMAT + k] += 4 * up; }
         for (int ty = 0; ty < 4; ++ty) if (s.tslot[ty]) s.tslot[ty] += up; // (0: no kind of that type)
         s.gplane_slot += up;
         for (int k = 0; k < r->nlk; ++k) H[H_LSLOT + k] -= down;
         s.mat_slot -= down;
         if (s.u8_slot >= 0) s.u8_slot -= down;
         H[H_VCLEAR] = 0; // (segment_clear reads its geometry from LDS: off, as it is for every scene with triangles or a partition)
         s.table_f4 = (int)n_res;
         t.push_back(mk4(0, 0, 0, 0)); t.push_back(mk4(0, 0, 0, 0)); // (the first-sphere / first-box reads of a scene without any stay inside the image)
      }
   }
   if (r->bvh_active) { // the hierarchy behind everything else of the image: nodes, then the permutation (rebuilt when a triangle or their count changed)
      const int n = s.tcount[PK_TRIANGLE];
      std::vector<float> tris(9 * (size_t)n);
      for (int i = 0; i < 3 * n; ++i) { const float4 v = t[s.tslot[PK_TRIANGLE] + i]; tris[3 * (size_t)i] = v.x; tris[3 * (size_t)i + 1] = v.y; tris[3 * (size_t)i + 2] = v.z; }
      if (!r->bvh_built || tris.size() != r->bvh_tris.size() || (n > 0 && memcmp(tris.data(), r->bvh_tris.data(), tris.size() * 4) != 0)) {
         bvh_build(tris.data(), n, r->bvh);
         r->bvh_tris.swap(tris);
         r->bvh_built = true;
      }
      H[H_BVH_NODES] = (int)t.size();
      H[H_BVH_COUNT] = (int)r->bvh.nodes.size() / 2;
      H[H_BVH_ALWAYS] = r->bvh.n_always;
      H[H_BVH_DELTA] = f_as_i(r->bvh.delta);
      t.insert(t.end(), r->bvh.nodes.begin(), r->bvh.nodes.end());
      for (int i0 = 0; i0 < n; i0 += 4) {
         float m[4] = {0, 0, 0, 0};
         for (int j = 0; j < 4 && i0 + j < n; ++j) m[j] = i_as_f(r->bvh.perm[i0 + j]);
         t.push_back(mk4(m[0], m[1], m[2], m[3]));
      }
   }
   for (int k = 0; k < r->npk; ++k) { H[H_KQUAD + 4 * k] = H[H_KTYPE + k]; H[H_KQUAD + 4 * k + 1] = H[H_KSLOT + k]; H[H_KQUAD + 4 * k + 2] = H[H_KBASE + k]; H[H_KQUAD + 4 * k + 3] = H[H_KMAX + k]; }
   memcpy(t.data(), H, sizeof H);

   if (t.size() > r->table_cap) { // grow the whole ring (rare: the table only grows with the primitive counts)
      { int dr = drain_streams(r); if (dr != MDH_OK) return dr; }
      r->tab_use.forget();
      for (int q = 0; q < mdh_renderer::TAB_RING; ++q) {
         HIP_TRY(r->d_table_ring[q].grow(t.size() + 256));
         HIP_TRY(r->h_table_ring[q].grow(t.size() + 256));
      }
      r->table_cap = t.size() + 256; // (last: after a failure the next commit grows the rest)
   }
   const int ns = (r->tab_slot + 1) % mdh_renderer::TAB_RING;
   HIP_TRY(r->tab_use.retire_on_host(ns));
   memcpy(r->h_table_ring[ns].ptr, t.data(), t.size() * sizeof(float4));
   HIP_TRY(hipMemcpyAsync(r->d_table_ring[ns].ptr, r->h_table_ring[ns].ptr, t.size() * sizeof(float4), hipMemcpyHostToDevice, up));
   HIP_TRY(r->table_fence.signal(up, stream_index(r, up)));
   r->tab_slot = ns;
   s.table = r->d_table_ring[ns].ptr;
   s.part_enable = r->part.enable;
   s.part_border = r->part.border_behavior;
   s.part_index_count = r->part.index_count;
   s.part_cells = r->part_cells;
   for (int a = 0; a < 3; ++a) { s.part_dims[a] = r->part.grid_dimensions[a]; s.part_sp[a] = r->pg_spacing[a]; s.part_off[a] = r->pg_offset[a]; }
   s.part_sp_pow2 = 1;
   for (int a = 0; a < 3; ++a) {
      int e = 0;
      const float mant = frexpf(r->pg_spacing[a], &e);
      const bool pow2 = mant == 0.5f && e > -100 && e < 100; // 2^(e-1), well inside the normal range
      s.part_inv_sp[a] = pow2 ? 1.0f / r->pg_spacing[a] : 0.0f;
      if (!pow2) s.part_sp_pow2 = 0;
   }
   // the grid's dimensions as the fp32 values the cell index is computed with (uniform conversions the kernels would repeat at every march step)
   for (int a = 0; a < 3; ++a) s.part_fdims[a] = (float)r->part.grid_dimensions[a];
   s.part_fyz = (float)(r->part.grid_dimensions[1] * r->part.grid_dimensions[2]);
   s.part_table = r->d_part_ring[r->part_slot].ptr;
   s.part_mask_off = (int)part_table_ints(r);
   s.part_mask_words = part_mask_words(r);
   s.part_bits_f4 = 0; // (the bits are never staged into LDS: mdh_device.h, KScene::part_bits_f4)
   { // KScene::part_small: one 8-byte load per lookup, a shift and a mask per built-in type
      int declared = 0;
      bool small = r->part.enable != 0;
      for (int ty = 0; ty < 4; ++ty) { s.part_tbit[ty] = 0u; s.part_tmask[ty] = 0u; }
      for (int k = 0; k < r->npk; ++k) {
         const Kind &kd = r->pk[k];
         if (kd.type == PK_CUSTOM || kd.max_count > 32) small = false;
         else if (kd.max_count > 0 && s.part_tmask[kd.type]) small = false; // (two kinds of one built-in type: one shift and mask cannot name both)
         else if (kd.max_count > 0) { s.part_tbit[kd.type] = (unsigned)r->prim_base[k]; s.part_tmask[kd.type] = kd.max_count == 32 ? 0xffffffffu : ((1u << kd.max_count) - 1u); }
         declared += kd.max_count;
      }
      s.part_small = small && declared <= 64 && part_mask_words(r) == 2 ? 1 : 0;
   }
   r->table_dirty = false;
   return MDH_OK;
}

static KProbes make_probes(const mdh_renderer *r)
{
   KProbes p;
   p.pcx = r->probes.probe_count[0]; p.pcy = r->probes.probe_count[1];
   p.gx = r->probes.grid_dimensions[0]; p.gy = r->probes.grid_dimensions[1]; p.gz = r->probes.grid_dimensions[2];
   p.sx = r->probes.grid_spacing[0]; p.sy = r->probes.grid_spacing[1]; p.sz = r->probes.grid_spacing[2];
   p.rres = r->probes.radiance_resolution; p.ires = r->probes.irradiance_resolution;
   p.fmt = r->opt_atlas;
   auto log2_or_neg = [](int v) { int s = 0; while ((1 << s) < v) ++s; return (1 << s) == v ? s : -1; };
   p.rshift = log2_or_neg(p.rres); p.ishift = log2_or_neg(p.ires); p.pcx_shift = log2_or_neg(p.pcx);
   p.inv_pcx = log2_or_neg(p.pcx) >= 0 ? 1.0f / (float)p.pcx : 0.0f;
   p.inv_pcy = log2_or_neg(p.pcy) >= 0 ? 1.0f / (float)p.pcy : 0.0f;
   p.rad = r->d_rad2[r->last].ptr; p.irr = r->d_irr2[r->last].ptr;
   own_probes(r, &p.probe_begin, &p.probe_end);
   // the uniform fp32 values of the atlas taps: the kernels' own expressions, evaluated here once (IEEE, one rounding each)
   p.irr_lo = 0.5f / (float)p.ires; p.irr_hi = 1.0f - p.irr_lo;
   p.rad_lo = 0.5f / (float)p.rres; p.rad_hi = 1.0f - p.rad_lo;
   p.irr_w = (float)(p.pcx * p.ires); p.irr_h = (float)(p.pcy * p.ires);
   p.rad_w = (float)(p.pcx * p.rres); p.rad_h = (float)(p.pcy * p.rres);
   p.fpcx = (float)p.pcx; p.fpcy = (float)p.pcy;
   p.rad_lods = 0;
   while ((2 << p.rad_lods) <= p.rres) ++p.rad_lods;
   // div_magic: exact for numerators below 65536 -- texel coordinates of an atlas image, probe ids
   auto magic = [](int d) { return (unsigned)((1ull << 32) / (unsigned long long)d + 1ull); };
   const bool small = (long long)p.pcx * p.rres < 65536 && (long long)p.pcy * p.rres < 65536 && (long long)p.pcx * p.ires < 65536 &&
                      (long long)p.pcy * p.ires < 65536 && (long long)p.pcx * p.pcy < 65536;
   p.m_rres = small && p.rres > 1 ? magic(p.rres) : 0u;
   p.m_ires = small && p.ires > 1 ? magic(p.ires) : 0u;
   p.m_pcx = small && p.pcx > 1 ? magic(p.pcx) : 0u;
   p.rad_mips = nullptr; // (the screen pass sets it: pass_screen)
   return p;
}
static KCamera make_camera(const mdh_renderer *r)
{
   KCamera c;
   c.px = r->cam_pos[0]; c.py = r->cam_pos[1]; c.pz = r->cam_pos[2];
   memcpy(c.m, r->cam_m, sizeof c.m);
   return c;
}
static KVolumetrics make_vol(const mdh_renderer *r, bool enabled, int set)
{
   KVolumetrics v;
   v.enabled = enabled ? 1 : 0;
   v.vw = r->vol.visibility_resolution[0]; v.vh = r->vol.visibility_resolution[1]; v.vz = r->vol.visibility_resolution[2];
   v.sw = r->vol.scattering_resolution[0]; v.sh = r->vol.scattering_resolution[1];
   v.vstep = r->vstep; v.sstep = r->sstep;
   v.vis = r->d_vis2[set].ptr; v.scat = r->d_scat2[set].ptr;
   return v;
}

static int alloc_atlases(mdh_renderer *r)
{
   for (int s = 0; s < mdh_renderer::NSETS; ++s) {
      HIP_TRY(r->d_rad2[s].release()); // (released, not only grown: the other format's atlases are smaller or larger)
      HIP_TRY(r->d_irr2[s].release());
      HIP_TRY(r->d_rad2[s].grow(atlas_bytes(r, MDH_TEX_RADIANCE)));
      HIP_TRY(r->d_irr2[s].grow(atlas_bytes(r, MDH_TEX_IRRADIANCE)));
      // Load_Empty_Texture (render_passes.adb:115-116): contents start as zeros here
      HIP_TRY(hipMemsetAsync(r->d_rad2[s].ptr, 0, atlas_bytes(r, MDH_TEX_RADIANCE), r->stream));
      HIP_TRY(hipMemsetAsync(r->d_irr2[s].ptr, 0, atlas_bytes(r, MDH_TEX_IRRADIANCE), r->stream));
   }
   r->main_dirty = true;
   return MDH_OK;
}

// MDH_OPT_RADIANCE_MIPS: texels of levels 1 .. radiance_lods together (a third of level 0 at most)
static size_t rad_mips_texels(const mdh_renderer *r)
{
   size_t n = 0;
   for (int res = r->probes.radiance_resolution >> 1; res >= 1; res >>= 1) n += (size_t)probe_total(r) * res * res;
   return n;
}
static int alloc_rad_mips(mdh_renderer *r)
{
   for (int s = 0; s < mdh_renderer::NSETS; ++s) {
      HIP_TRY(r->d_rad_mips[s].release());
      if (r->opt_mips) HIP_TRY(r->d_rad_mips[s].grow(rad_mips_texels(r) * texel_bytes(r))); // (no texels: stays empty)
   }
   return MDH_OK;
}
// the levels of set `set`'s radiance atlas on stream st (before the screen pass that reads them)
static int build_rad_mips(mdh_renderer *r, int set, hipStream_t st)
{
   const char *src = (const char *)r->d_rad2[set].ptr;
   char *dst = (char *)r->d_rad_mips[set].ptr;
   for (int res = r->probes.radiance_resolution >> 1; res >= 1; res >>= 1) {
      const long n = (long)probe_total(r) * res * res;
      hipLaunchKernelGGL(k_radiance_mips, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const void *)src, (void *)dst, r->opt_atlas, res, (int)n);
      src = dst;
      dst += (size_t)n * texel_bytes(r);
   }
   HIP_TRY(hipGetLastError());
   return MDH_OK;
}

static int rccl_api_destroy(ncclComm_t c); // (mdh_comm_* below)
static void peer_drop(mdh_renderer *r);      // (mdh_peer_* below)
static bool peer_active(const mdh_renderer *r);
static int peer_check(mdh_renderer *r);
extern "C" int32_t mdh_destroy(mdh_renderer *r)
{
   if (!r) return MDH_OK;
   (void)hipSetDevice(r->device);
   (void)sync_streams(r, SYNC_MAIN | SYNC_PROBE | SYNC_ALT | SYNC_QUERY | SYNC_VOL);
   if (r->copy_stream) (void)hipStreamSynchronize(r->copy_stream);
   if (r->comm) { ncclComm_t c = r->comm; r->comm = nullptr; (void)rccl_api_destroy(c); }
   peer_drop(r);
   for (auto &p : r->pending) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
   if (r->rq_e0) r->free_events.push_back(r->rq_e0);
   if (r->rq_e1) r->free_events.push_back(r->rq_e1);
   for (auto e : r->free_events) (void)hipEventDestroy(e);
   // the members release what they own; the streams go last, behind every event that was recorded on one
   const hipStream_t streams[] = {r->query_stream, r->vol_stream, r->copy_stream, r->probe_stream, r->alt_stream, r->own_stream};
   delete r;
   for (hipStream_t st : streams)
      if (st) (void)hipStreamDestroy(st);
   return MDH_OK;
}

// Renderers.Create (renderers.adb:91-300) + Scenes.Compile (scenes.adb:1378-1421)
extern "C" int32_t mdh_create(int32_t width, int32_t height, const mdh_scene_desc *scene, const mdh_probe_settings *probes,
                              const mdh_volumetrics *vol, int32_t device, mdh_renderer **out)
{
   if (!scene || !probes || !vol || !out || width <= 0 || height <= 0) return seterr(MDH_E_INVALID, "bad argument");
   if (scene->n_prim_kinds < 0 || scene->n_prim_kinds > MDH_MAX_KINDS || scene->n_light_kinds < 0 || scene->n_light_kinds > MDH_MAX_LIGHT_KINDS)
      return seterr(MDH_E_INVALID, "too many kinds");
   // Setup_Probe_Layout, renderers.adb:54-65
   if (probes->grid_dimensions[0] * probes->grid_dimensions[1] * probes->grid_dimensions[2] != probes->probe_count[0] * probes->probe_count[1])
      return seterr(MDH_E_PROBE_MISMATCH, "Probe_Count should match grid dimensions.");
   if (probes->radiance_resolution < 1 || probes->irradiance_resolution < 1 || probes->probe_count[0] < 1 || probes->probe_count[1] < 1)
      return seterr(MDH_E_INVALID, "bad probe settings");
   mdh_renderer *r = new mdh_renderer();
   r->W = width; r->H = height; r->device = device;
   r->npk = scene->n_prim_kinds; r->nlk = scene->n_light_kinds;
   // Compute_Scene_GPU_Type (scenes.adb:1268-1345)
   int off = 0, base = 0;
   for (int k = 0; k < r->npk; ++k) {
      if (!resolve_kind(r->pk[k], scene->prim_kinds[k], false)) { delete r; return seterr(MDH_E_UNSUPPORTED_KIND, "primitive kind is neither one of Sphere, Plane, Box, Triangle with their components nor a user-defined kind with three valid MDH_X programs"); }
      off = pad_to(off, 4); r->pk[k].count_off = off; off += 4;
      off = pad_to(off, 16); r->pk[k].array_off = off; off += r->pk[k].stride * r->pk[k].max_count;
      r->prim_base[k] = base; base += r->pk[k].max_count;
      if (r->pk[k].max_count > 4095) { delete r; return seterr(MDH_E_INVALID, "declared primitive count above 4095"); }
   }
   for (int k = 0; k < r->npk; ++k)
      for (int j = 0; j < k; ++j)
         if (r->pk[k].type != PK_CUSTOM && r->pk[k].type == r->pk[j].type) { delete r; return seterr(MDH_E_INVALID, "a built-in primitive kind is declared twice"); }
   for (int k = 0; k < r->nlk; ++k) {
      if (!resolve_kind(r->lk[k], scene->light_kinds[k], true)) { delete r; return seterr(MDH_E_UNSUPPORTED_KIND, "light kind is neither PointLight or SpotLight with their components nor a user-defined kind with valid Sample and Position programs"); }
      off = pad_to(off, 4); r->lk[k].count_off = off; off += 4;
      off = pad_to(off, 16); r->lk[k].array_off = off; off += r->lk[k].stride * r->lk[k].max_count;
   }
   off = pad_to(off, 4); r->total_light_off = off; off += 4;
   r->scene_ubo.assign((size_t)off, 0);
   r->max_dist = image_roundtrip(scene->max_dist);
   r->part = scene->partitioning;
   r->probes = *probes;
   r->vol = *vol;
   r->vstep = image_roundtrip(vol->visibility_step_size);
   r->sstep = image_roundtrip(vol->scattering_step_size);
   if (r->part.enable) {
      if (r->part.index_count < 1 || r->part.grid_dimensions[0] < 1 || r->part.grid_dimensions[1] < 1 || r->part.grid_dimensions[2] < 1) { delete r; return seterr(MDH_E_INVALID, "bad partitioning settings"); }
      for (int a = 0; a < 3; ++a) { r->pg_spacing[a] = image_roundtrip(r->part.grid_spacing[a]); r->pg_offset[a] = image_roundtrip(r->part.grid_offset[a]); }
      r->part_cells = r->part.grid_dimensions[0] * r->part.grid_dimensions[1] * r->part.grid_dimensions[2];
      float sx = r->part.grid_spacing[0], sy = r->part.grid_spacing[1], sz = r->part.grid_spacing[2];
      r->part_gpu_diag = image_roundtrip(sqrtf((sx * sx + sy * sy) + sz * sz));
   }
   // ---- device
   int ndev = 0;
   if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { delete r; return seterr(MDH_E_NO_DEVICE, "no HIP device visible; libmadarch_hip has no CPU path"); }
   if (device < 0 || device >= ndev) { delete r; return seterr(MDH_E_NO_DEVICE, "device ordinal out of range"); }
   hipDeviceProp_t prop;
   if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) { delete r; return seterr(MDH_E_NO_DEVICE, "device is not gfx950 (MI355X); the kernels are built for gfx950 only"); }
   r->n_cus = prop.multiProcessorCount;
   int rc = MDH_OK;
   auto fail = [&](int code) { mdh_destroy(r); return code; };
#define TRY_OR_FAIL(expr)                                                                                          \
   do {                                                                                                            \
      hipError_t e_ = (expr);                                                                                      \
      if (e_ != hipSuccess) {                                                                                      \
         snprintf(g_err, sizeof g_err, "%s failed: %s", #expr, hipGetErrorString(e_));                             \
         return fail(MDH_E_DEVICE);                                                                                \
      }                                                                                                            \
   } while (0)
   TRY_OR_FAIL(hipSetDevice(device));
   TRY_OR_FAIL(hipStreamCreateWithFlags(&r->own_stream, hipStreamNonBlocking));
   r->stream = r->own_stream;
   {
      int lo = 0, hi = 0; // numerically lower = higher priority
      TRY_OR_FAIL(hipDeviceGetStreamPriorityRange(&lo, &hi));
      // the probe passes are the head of each frame's dependency chain: high priority (measured on MI355X:
      // 3340 vs 3300 Mpix/s at BASELINE config 3)
      TRY_OR_FAIL(hipStreamCreateWithPriority(&r->probe_stream, hipStreamNonBlocking, hi));
      TRY_OR_FAIL(hipStreamCreateWithFlags(&r->alt_stream, hipStreamNonBlocking));
      TRY_OR_FAIL(create_all(r->ev_join, r->ev_join_alt, r->table_fence));
      for (int q = 0; q < mdh_renderer::NSETS; ++q) TRY_OR_FAIL(create_all(r->ev_screen[q], r->ev_probe[q], r->ev_vol[q]));
      // (HIP maps a process's streams onto a few hardware queues, four by default: a fifth stream shares one with another
      //  and their work serialises -- measured: light_shafts lost a fifth of its frame rate.  So the volumetric stream exists
      //  only with volumetrics, and the query stream from the first Eval_Distance_To on.)
      if (vol->enabled) TRY_OR_FAIL(hipStreamCreateWithFlags(&r->vol_stream, hipStreamNonBlocking));
      TRY_OR_FAIL(create_all(r->part_fence, r->ev_warn, r->tab_use, r->part_use));
   }
   if ((rc = alloc_atlases(r)) != MDH_OK) return fail(rc);
   size_t px = (size_t)width * height;
   for (int s = 0; s < 2; ++s) {
      TRY_OR_FAIL(r->d_fb2[s].grow(px));
      TRY_OR_FAIL(hipMemsetAsync(r->d_fb2[s].ptr, 0, px * sizeof(float4), r->stream));
   }
   for (int s = 0; s < 2; ++s)
      for (int q = 0; q < 3; ++q) TRY_OR_FAIL(r->d_gb2[s][q].grow(px * 4));
   TRY_OR_FAIL(r->d_warn.grow(1));
   TRY_OR_FAIL(r->h_warn.grow(1));
   *r->h_warn.ptr = 0;
   size_t vis_n = (size_t)vol->visibility_resolution[0] * vol->visibility_resolution[1] * vol->visibility_resolution[2] * 3;
   size_t scat_n = (size_t)vol->scattering_resolution[0] * vol->scattering_resolution[1];
   if (vis_n / 3 >= (1ull << 32) || scat_n >= (1ull << 32)) { seterr(MDH_E_INVALID, "a volumetrics texture of 2^32 texels or more"); return fail(MDH_E_INVALID); } // (tex_sample: 32-bit texel index)
   for (int s = 0; s < mdh_renderer::NSETS; ++s) {
      TRY_OR_FAIL(r->d_vis2[s].grow(vis_n ? vis_n : 1));
      TRY_OR_FAIL(hipMemsetAsync(r->d_vis2[s].ptr, 0, (vis_n ? vis_n : 1) * 4, r->stream));
      TRY_OR_FAIL(r->d_scat2[s].grow(scat_n ? scat_n : 1));
      TRY_OR_FAIL(hipMemsetAsync(r->d_scat2[s].ptr, 0, (scat_n ? scat_n : 1) * sizeof(float4), r->stream));
   }
   if (r->part.enable) {
      if (part_buffer_ints(r) >= (1ull << 31)) { seterr(MDH_E_INVALID, "a partition table of 2^31 ints or more"); return fail(MDH_E_INVALID); }
      size_t n = part_buffer_ints(r);
      for (int q = 0; q < mdh_renderer::PART_RING; ++q) {
         TRY_OR_FAIL(r->d_part_ring[q].grow(n));
         TRY_OR_FAIL(hipMemsetAsync(r->d_part_ring[q].ptr, 0, n * 4, r->stream));
      }
   }
   TRY_OR_FAIL(hipStreamSynchronize(r->stream));
#undef TRY_OR_FAIL
   *out = r;
   return MDH_OK;
}

extern "C" int32_t mdh_set_option(mdh_renderer *r, int32_t option, int32_t value)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   switch (option) { // (the options no probe pass reads: everything else, known or not, counts as an edit)
   case MDH_OPT_TIMING: case MDH_OPT_SCREEN_ORDER: case MDH_OPT_SCREEN_SPLIT: case MDH_OPT_SCREEN_REPLAY: case MDH_OPT_GBUFFER:
   case MDH_OPT_WINDOW: case MDH_OPT_AO_STEPS: case MDH_OPT_INDIRECT_SPECULAR: case MDH_OPT_PROBE_SETTLE: break;
   case MDH_OPT_RAY_STREAM_REFILL: case MDH_OPT_RAY_STREAM_GROUPS: case MDH_OPT_PATH_FRAME_COMPACT: break; // (the device-array ray queries' schedule, an adaptive path-traced frame's mapping: no pass reads it)
   default: settle_bump(r);
   }
   // what an open frame has latched (its atlas set, slice, streams and screen mode) cannot change under it
   if (r->in_frame && (option == MDH_OPT_ATLAS_FORMAT || option == MDH_OPT_RANK || option == MDH_OPT_WORLD || option == MDH_OPT_FRAME_OVERLAP ||
                       option == MDH_OPT_SCREEN_MODE))
      return seterr(MDH_E_STATE, "a frame is open");
   if ((r->comm || peer_active(r)) && (option == MDH_OPT_RANK || option == MDH_OPT_WORLD)) return seterr(MDH_E_STATE, "rank and world belong to the communicator (mdh_comm_init / mdh_peer_init)");
   if (peer_active(r) && option == MDH_OPT_IRRADIANCE_ALL && !value) return seterr(MDH_E_STATE, "the peer exchange moves radiance slices only: MDH_OPT_IRRADIANCE_ALL stays on");
   switch (option) {
   case MDH_OPT_ATLAS_FORMAT:
      if (value != 0 && value != 1) return seterr(MDH_E_INVALID, "atlas format is 0 (RGB8) or 1 (fp32)");
      if (value != r->opt_atlas) {
         if (r->peer) return seterr(MDH_E_STATE, "the peers hold handles of this renderer's atlases (mdh_peer_export): leave first (mdh_comm_destroy)");
         HIP_TRY(hipSetDevice(r->device));
         { int jr = join_main(r); if (jr != MDH_OK) return jr; }
         HIP_TRY(hipStreamSynchronize(r->stream));
         r->opt_atlas = value;
         int rc = alloc_atlases(r);
         if (rc != MDH_OK) return rc;
         if ((rc = alloc_rad_mips(r)) != MDH_OK) return rc;
      }
      break;
   case MDH_OPT_SCREEN_MODE: if (value < 0 || value > 2) return seterr(MDH_E_INVALID, "screen mode is 0, 1 or 2"); r->opt_mode = value; break;
   case MDH_OPT_AO_STEPS: r->opt_ao = value; break;
   case MDH_OPT_GBUFFER: r->opt_gbuffer = value ? 1 : 0; break;
   case MDH_OPT_RANK: if (value < 0) return seterr(MDH_E_INVALID, "rank < 0"); r->opt_rank = value; break;
   case MDH_OPT_WORLD: if (value < 1) return seterr(MDH_E_INVALID, "world < 1"); r->opt_world = value; break;
   case MDH_OPT_TIMING: r->opt_timing = value ? 1 : 0; break;
   case MDH_OPT_ADA_EVAL_DIV: r->opt_ada_div = value ? 1 : 0; break;
   case MDH_OPT_JIT: r->opt_jit = value ? 1 : 0; ++r->march_inputs; break;
   case MDH_OPT_IRRADIANCE_ALL: r->opt_irr_all = value ? 1 : 0; break;
   case MDH_OPT_WINDOW:
      if (value < 0 || value > 2) return seterr(MDH_E_INVALID, "bad value");
      r->opt_window = value; r->win_valid = false;
      break;
   case MDH_OPT_FRAME_OVERLAP:
      if (value < 0 || value > 2) return seterr(MDH_E_INVALID, "frame overlap is 0, 1 or 2");
      if ((value != 0) != (r->opt_overlap != 0)) r->scr_order.force(); // (how much of the screen pass is sorted follows the schedule: sort again)
      r->opt_overlap = value;
      break;
   case MDH_OPT_INDIRECT_SPECULAR: if (value < 0 || value > 3) return seterr(MDH_E_INVALID, "indirect specular mode is 0 .. 3"); r->opt_spec = value; break;
   case MDH_OPT_HYSTERESIS_PERMILLE: if (value < 0 || value > 999) return seterr(MDH_E_INVALID, "hysteresis is 0 .. 999 per mille"); r->opt_hyst = value; break;
   case MDH_OPT_RADIANCE_ORDER: r->opt_rad_order = value ? 1 : 0; r->rad_order.forget(); break;
   case MDH_OPT_SCREEN_ORDER: r->opt_scr_order = value ? 1 : 0; r->scr_order.forget(); break;
   case MDH_OPT_SCREEN_SPLIT: if (value < 0) return seterr(MDH_E_INVALID, "MDH_OPT_SCREEN_SPLIT: a number of wavefronts"); r->opt_scr_split = value; break;
   case MDH_OPT_NUMERICS: if (value != (MDH_FAST_NUMERICS ? 1 : (MDH_HYBRID_NUMERICS ? 2 : 0))) return seterr(MDH_E_STATE, "the numerics are a property of the library build (make fast builds the experiment)"); break;
   case MDH_OPT_TABLE_RESIDENCY:
      if (value != 0 && value != 1) return seterr(MDH_E_INVALID, "table residency is 0 (by size) or 1 (global, forced)");
      if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
      if (value != r->opt_residency) { r->opt_residency = value; r->table_dirty = true; ++r->march_inputs; } // (the next commit lays the table out again)
      break;
   case MDH_OPT_TRIANGLE_BVH: {
      if (value != 0 && value != 1) return seterr(MDH_E_INVALID, "the triangle BVH is 0 (off) or 1 (on)");
      if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
      int tri_kinds = 0;
      for (int k = 0; k < r->npk; ++k) tri_kinds += r->pk[k].type == PK_TRIANGLE;
      if (value && (r->part.enable != 0 || has_custom_kinds(r) || tri_kinds > 1))
         return seterr(MDH_E_STATE, "MDH_OPT_TRIANGLE_BVH: scenes without a space partition, without user-defined kinds and with one Triangle kind only");
      if (value != r->opt_tri_bvh) { r->opt_tri_bvh = value; r->table_dirty = true; ++r->march_inputs; } // (the next commit lays the table out again)
      break;
   }
   case MDH_OPT_RADIANCE_MIPS: {
      const int res = r->probes.radiance_resolution;
      if (value && (res & (res - 1)) != 0) return seterr(MDH_E_INVALID, "radiance mips need a power-of-two radiance resolution");
      if ((value != 0) != (r->opt_mips != 0)) {
         HIP_TRY(hipSetDevice(r->device));
         { int dr = drain_streams(r); if (dr != MDH_OK) return dr; }
         r->opt_mips = value ? 1 : 0;
         int rc = alloc_rad_mips(r);
         if (rc != MDH_OK) return rc;
      }
      break;
   }
   case MDH_OPT_RADIANCE_REPLAY:
      r->opt_rad_replay = value ? 1 : 0;
      r->rad_replay.option_set(r->opt_rad_replay != 0, false); // (the previous pass stays seen: a key that stands is recorded by the first pass after the option comes back on)
      if (!r->opt_rad_replay) { // the records are dropped (the buffer itself with the streams drained: never under an open frame)
         if (r->d_rad_rec.ptr && !r->in_frame) {
            HIP_TRY(hipSetDevice(r->device));
            { int sr = sync_streams(r, SYNC_PROBE | SYNC_MAIN); if (sr != MDH_OK) return sr; }
            HIP_TRY(r->d_rad_rec.release());
         }
      }
      break;
   case MDH_OPT_SCREEN_REPLAY:
      r->opt_scr_replay = value ? 1 : 0;
      r->scr_replay.option_set(r->opt_scr_replay != 0, true); // (off forgets the previous pass too: the first pass after the option comes back on marches plainly)
      if (!r->opt_scr_replay) { // the records are dropped (the buffer itself with the streams drained: never under an open frame)
         if (r->d_scr_rec.ptr && !r->in_frame) {
            HIP_TRY(hipSetDevice(r->device));
            int drc = drain_streams(r);
            if (drc != MDH_OK) return drc;
            r->scr_rec_reads.forget();
            HIP_TRY(r->d_scr_rec.release());
         }
      }
      break;
   case MDH_OPT_PROBE_SETTLE: r->opt_settle = value ? 1 : 0; r->settle.set_enabled(r->opt_settle != 0); break; // (0 forgets the run)
   case MDH_OPT_RAY_STREAM_REFILL:
      if (value < MDH_RS_REFILL_MIN || value > MDH_RS_REFILL_MAX) return seterr(MDH_E_INVALID, "MDH_OPT_RAY_STREAM_REFILL: 1 .. 64 idle lanes");
      r->opt_rq_refill = value;
      break;
   case MDH_OPT_RAY_STREAM_GROUPS: if (value < 0) return seterr(MDH_E_INVALID, "MDH_OPT_RAY_STREAM_GROUPS: a number of workgroups, 0 = as many as are resident"); r->opt_rq_groups = value; break;
   case MDH_OPT_PATH_FRAME_COMPACT: r->opt_pf_compact = value ? 1 : 0; break; // (read where a round is enqueued: the same bits)
   default: return seterr(MDH_E_INVALID, "unknown option");
   }
   return MDH_OK;
}
extern "C" int32_t mdh_get_option(mdh_renderer *r, int32_t option, int32_t *value)
{
   if (!r || !value) return seterr(MDH_E_INVALID, "bad argument");
   switch (option) {
   case MDH_OPT_ATLAS_FORMAT: *value = r->opt_atlas; break;
   case MDH_OPT_SCREEN_MODE: *value = r->opt_mode; break;
   case MDH_OPT_AO_STEPS: *value = r->opt_ao; break;
   case MDH_OPT_GBUFFER: *value = r->opt_gbuffer; break;
   case MDH_OPT_RANK: *value = r->opt_rank; break;
   case MDH_OPT_WORLD: *value = r->opt_world; break;
   case MDH_OPT_TIMING: *value = r->opt_timing; break;
   case MDH_OPT_ADA_EVAL_DIV: *value = r->opt_ada_div; break;
   case MDH_OPT_FRAME_OVERLAP: *value = r->opt_overlap; break;
   case MDH_OPT_JIT: *value = r->opt_jit; break;
   case MDH_OPT_IRRADIANCE_ALL: *value = r->opt_irr_all; break;
   case MDH_OPT_WINDOW: *value = r->opt_window; break;
   case MDH_OPT_INDIRECT_SPECULAR: *value = r->opt_spec; break;
   case MDH_OPT_HYSTERESIS_PERMILLE: *value = r->opt_hyst; break;
   case MDH_OPT_RADIANCE_ORDER: *value = r->opt_rad_order; break;
   case MDH_OPT_RADIANCE_REPLAY: *value = r->opt_rad_replay; break;
   case MDH_OPT_SCREEN_REPLAY: *value = r->opt_scr_replay; break;
   case MDH_OPT_SCREEN_ORDER: *value = r->opt_scr_order; break;
   case MDH_OPT_SCREEN_SPLIT: *value = r->opt_scr_split; break;
   case MDH_OPT_NUMERICS: *value = MDH_FAST_NUMERICS ? 1 : (MDH_HYBRID_NUMERICS ? 2 : 0); break; // 0 exact (shipped), 1 / 2 the labelled experiments
   case MDH_OPT_RADIANCE_MIPS: *value = r->opt_mips; break;
   case MDH_OPT_TRIANGLE_BVH: *value = r->opt_tri_bvh; break;
   case MDH_OPT_PROBE_SETTLE: *value = r->opt_settle; break;
   case MDH_OPT_RAY_STREAM_REFILL: *value = r->opt_rq_refill; break;
   case MDH_OPT_RAY_STREAM_GROUPS: *value = r->opt_rq_groups; break;
   case MDH_OPT_PATH_FRAME_COMPACT: *value = r->opt_pf_compact; break;
   case MDH_OPT_TABLE_RESIDENCY: { // of the committed scene: edits since the last commit are committed first
      if (r->table_dirty && !r->in_frame) {
         HIP_TRY(hipSetDevice(r->device));
         const int rc = commit_scene(r, r->stream);
         if (rc != MDH_OK) return rc;
      }
      *value = r->residency;
      break;
   }
   default: return seterr(MDH_E_INVALID, "unknown option");
   }
   return MDH_OK;
}

// Set_Material (renderers.adb:349-367)
extern "C" int32_t mdh_set_material(mdh_renderer *r, int32_t id0, const float albedo[3], float metallic, float roughness)
{
   settle_bump(r);
   if (!r || !albedo) return seterr(MDH_E_INVALID, "bad argument");
   if (id0 < 0 || id0 >= MAX_MATERIALS) return seterr(MDH_E_INDEX, "material index out of range");
   uint8_t *p = r->materials_ubo + 16 + 32 * id0;
   { // MDH_OPT_SCREEN_REPLAY: a pixel's reflection ray is traced when its material's roughness is below 0.75
     // (render_probes.glsl:262).  The replaying kernel tests the live roughness as the marching one does and traces only
     // what the record also traced: a material that turns rough switches its reflections off in both kernels alike, a
     // material in use that turns smooth needs rays no record holds and ends the replay.  Any other edit of it does not.
      float was;
      memcpy(&was, p + 16, 4);
      if (id0 < r->last_material_index && !(was < 0.75f) && roughness < 0.75f) ++r->reflect_edits;
   }
   memcpy(p, albedo, 12);
   memcpy(p + 12, &metallic, 4);
   memcpy(p + 16, &roughness, 4);
   if (id0 >= r->last_material_index) r->last_material_index = id0 + 1;
   r->table_dirty = true;
   return MDH_OK;
}
// Add_Material (renderers.adb:369-377)
extern "C" int32_t mdh_add_material(mdh_renderer *r, const float albedo[3], float metallic, float roughness, int32_t *out_id0)
{
   settle_bump(r);
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   int id = r->last_material_index;
   int rc = mdh_set_material(r, id, albedo, metallic, roughness);
   if (rc == MDH_OK && out_id0) *out_id0 = id;
   return rc;
}
// Write_Entity (renderers.adb:335-347) of a whole element
static int write_entity(mdh_renderer *r, const Kind &k, int index1, const void *blob, int nbytes)
{
   if (!blob || nbytes != k.elem_size) return seterr(MDH_E_INVALID, "blob size does not match the std140 element size");
   if (index1 < 1 || index1 > k.max_count) return seterr(MDH_E_INDEX, "index out of the declared range");
   memcpy(r->scene_ubo.data() + k.array_off + k.stride * (index1 - 1), blob, (size_t)nbytes);
   r->table_dirty = true;
   return MDH_OK;
}
// Set_Primitive (renderers.adb:379-398)
extern "C" int32_t mdh_set_primitive(mdh_renderer *r, int32_t kind_ix, int32_t index1, const void *blob, int32_t nbytes)
{
   settle_bump(r);
   if (!r || kind_ix < 0 || kind_ix >= r->npk) return seterr(MDH_E_INVALID, "bad kind index");
   if (index1 < 1 || index1 > r->host_count[kind_ix]) return seterr(MDH_E_INDEX, "index past the primitives added");
   ++r->geometry_edits;
   return write_entity(r, r->pk[kind_ix], index1, blob, nbytes);
}
// Add_Primitive (renderers.adb:435-456)
extern "C" int32_t mdh_add_primitive(mdh_renderer *r, int32_t kind_ix, const void *blob, int32_t nbytes, int32_t *out_count)
{
   settle_bump(r);
   if (!r || kind_ix < 0 || kind_ix >= r->npk) return seterr(MDH_E_INVALID, "bad kind index");
   int count = r->host_count[kind_ix] + 1;
   ++r->geometry_edits;
   int rc = write_entity(r, r->pk[kind_ix], count, blob, nbytes);
   if (rc != MDH_OK) return rc;
   r->host_count[kind_ix] = count;
   int32_t c = count;
   memcpy(r->scene_ubo.data() + r->pk[kind_ix].count_off, &c, 4);
   if (out_count) *out_count = count;
   return MDH_OK;
}
// Set_Light (renderers.adb:458-483)
extern "C" int32_t mdh_set_light(mdh_renderer *r, int32_t index1, int32_t light_kind_ix, const void *blob, int32_t nbytes)
{
   settle_bump(r);
   if (!r || light_kind_ix < 0 || light_kind_ix >= r->nlk) return seterr(MDH_E_INVALID, "bad light kind index");
   int rc = write_entity(r, r->lk[light_kind_ix], index1, blob, nbytes);
   if (rc != MDH_OK) return rc;
   int32_t c = index1;
   memcpy(r->scene_ubo.data() + r->lk[light_kind_ix].count_off, &c, 4);
   memcpy(r->scene_ubo.data() + r->total_light_off, &c, 4);
   return MDH_OK;
}
extern "C" int32_t mdh_set_camera_position(mdh_renderer *r, const float p[3])
{
   if (!r || !p) return seterr(MDH_E_INVALID, "bad argument");
   memcpy(r->cam_pos, p, 12);
   return MDH_OK;
}
extern "C" int32_t mdh_set_camera_orientation(mdh_renderer *r, const float m[9])
{
   if (!r || !m) return seterr(MDH_E_INVALID, "bad argument");
   memcpy(r->cam_m, m, 36);
   return MDH_OK;
}

// `up`: the stream the new table is uploaded on (the one that uses it first); nullptr = the main stream
static int ensure_committed(mdh_renderer *r, hipStream_t up = nullptr)
{
   HIP_TRY(hipSetDevice(r->device));
   if (r->table_dirty) return commit_scene(r, up ? up : r->stream);
   return MDH_OK;
}
static size_t lds_bytes(const mdh_renderer *r) { return (size_t)(r->ks.table_f4 + r->ks.part_bits_f4) * sizeof(float4); }
// the march kernels park MDH_PARK_DWORDS floats per thread behind the table (mdh_march.h)
static size_t lds_bytes_march(const mdh_renderer *r) { return lds_bytes(r) + (size_t)MDH_PARK_DWORDS * MDH_BLOCK * sizeof(float); }
// the screen pass runs without the visibility queue, whose entries, first steps and result words are the park
// slots from 15 up: 3 KiB less per workgroup, room for one more workgroup of a neighbouring pass on the CU
// (`mode`: the screen mode of the launch -- the renderer's for its screen pass, the call's for mdh_shade_rays)
static size_t lds_bytes_screen_mode(const mdh_renderer *r, int mode)
{
   // (scenes with a space partition: three more rows, the second shaded point's normal across its visibility marches, MDH_PARK_VD_ROW)
   const int rows = mode == 2 ? MDH_DIRECT_PARK_ROWS : (r->part.enable ? std::max(MDH_SCR_PARK_ROWS, MDH_PARK_VD_ROW + 3) : MDH_SCR_PARK_ROWS);
   return lds_bytes(r) + (size_t)rows * MDH_BLOCK * sizeof(float);
}
static size_t lds_bytes_screen(const mdh_renderer *r) { return lds_bytes_screen_mode(r, r->opt_mode); }

// ------------------------------------------------------------------ hiprtc build of user-defined kinds
// MDH_OPT_JIT: instead of interpreting the MDH_X programs, compile them.  Every program becomes a
// straight-line function (one statement per instruction, the same operations in the same order, so
// the results are those of the interpreter bit for bit), mdh_jit_kinds.h dispatches on the kind, and
// the kernels of this library are compiled again around it with hiprtc -- the analogue of the
// reference's runtime glCompileShader of its generated GLSL.  Modules are cached per process by their
// generated source.
// A Distance program whose result is  sqrt (A) - R,  sqrt (A) + S  or  sqrt (A)  itself (a sphere, a torus, a capsule, a rounded
// anything: most distance functions end that way) can take part in the wave-level culling of the built-in spheres
// (mdh_device.h: closest_primitive): inside  closest = min (closest, d)  the root is not taken when, in every lane of the
// wavefront, A already proves d >= closest -- the same rule, the same margins, the same proof (rounding is monotone), and the
// same operations on the same values whenever the root IS taken.  jit_min_form finds the two instructions: the root S whose
// only reader is the final operation F, and F whose value (through moves) is the program's r0.
struct JitMinForm { int pc_sqrt = -1, pc_final = -1, kind = 0; }; // kind: 1 = sqrt - r[b], 2 = sqrt + r[b], 3 = r[a] + sqrt, 4 = sqrt
static int jit_op_reads(int op) // registers an instruction reads (SEL: three, see below)
{
   switch (op) {
   case MDH_X_LIT: case MDH_X_COMP: case MDH_X_POINT: return 0;
   case MDH_X_MOV: case MDH_X_NEG: case MDH_X_ABS: case MDH_X_FLOOR: case MDH_X_SIGN: case MDH_X_SQRT: case MDH_X_ITOF:
   case MDH_X_ACOS: case MDH_X_SIN: case MDH_X_COS: case MDH_X_TAN: case MDH_X_ASIN: case MDH_X_ATAN: return 1;
   case MDH_X_SEL: return 3;
   default: return 2;
   }
}
static JitMinForm jit_min_form(const std::vector<int32_t> &code)
{
   JitMinForm none, f;
   struct Val { int pc, op, a, b; int readers; };
   std::vector<Val> vals; // value 0: "never written" (registers start as 0.0f)
   vals.push_back({-1, -1, 0, 0, 0});
   int id[MDH_X_REGS];
   for (int i = 0; i < MDH_X_REGS; ++i) id[i] = 0;
   for (size_t pc = 0; pc < code.size(); ++pc) {
      const uint32_t w = (uint32_t)code[pc];
      const int op = w & 255, d = (w >> 8) & 63, a = (w >> 16) & 255, b = (w >> 24) & 63, ra = a & 63;
      const int reads = jit_op_reads(op);
      int c = 0;
      if (op == MDH_X_LIT) ++pc;
      if (op == MDH_X_SEL) c = code[++pc] & 63;
      if (op == MDH_X_MOV) { id[d] = id[ra]; continue; } // (a move hands the value on)
      if (reads >= 1) ++vals[id[ra]].readers;
      if (reads >= 2) ++vals[id[b]].readers;
      if (reads >= 3) ++vals[id[c]].readers;
      vals.push_back({(int)pc - (op == MDH_X_LIT || op == MDH_X_SEL ? 1 : 0), op, reads >= 1 ? id[ra] : 0, reads >= 2 ? id[b] : 0, 0});
      id[d] = (int)vals.size() - 1;
   }
   const Val &F = vals[id[0]];
   if (F.pc < 0) return none;
   auto is_root = [&](int v) { return v > 0 && vals[v].op == MDH_X_SQRT && vals[v].readers == 1; };
   if (F.op == MDH_X_SQRT && F.readers == 0) { f.pc_sqrt = f.pc_final = F.pc; f.kind = 4; return f; }
   if (F.op == MDH_X_SUB && is_root(F.a) && F.b != F.a) { f.pc_sqrt = vals[F.a].pc; f.pc_final = F.pc; f.kind = 1; return f; }
   if (F.op == MDH_X_ADD && is_root(F.a) && F.b != F.a) { f.pc_sqrt = vals[F.a].pc; f.pc_final = F.pc; f.kind = 2; return f; }
   if (F.op == MDH_X_ADD && is_root(F.b) && F.b != F.a) { f.pc_sqrt = vals[F.b].pc; f.pc_final = F.pc; f.kind = 3; return f; }
   return none;
}
// min_form: emit  float NAME (int ent, f3 x, float closest)  =  min (closest, the program's distance)  with the root culled
static void jit_emit_program(std::string &out, const char *name, const std::vector<int32_t> &code, const JitMinForm *min_form = nullptr)
{
   char buf[512];
   bool used[MDH_X_REGS] = {false};
   std::string body;
   static const char *ARG[10] = {"x.x", "x.y", "x.z", "nrm.x", "nrm.y", "nrm.z", "dir.x", "dir.y", "dir.z", "dist"};
   for (size_t pc = 0; pc < code.size(); ++pc) {
      const uint32_t w = (uint32_t)code[pc];
      const int op = w & 255, d = (w >> 8) & 63, a = (w >> 16) & 255, b = (w >> 24) & 63, ra = a & 63;
      if (min_form && (int)pc == min_form->pc_final) { // the final operation: cull, or take the root and finish as the program does
         used[ra] = used[b] = true;
         char rr[32], fin[64];
         switch (min_form->kind) {
         case 1: snprintf(rr, sizeof rr, "r%d", b); snprintf(fin, sizeof fin, "sqrt_(d2_) - r%d", b); break;
         case 2: snprintf(rr, sizeof rr, "-r%d", b); snprintf(fin, sizeof fin, "sqrt_(d2_) + r%d", b); break;
         case 3: snprintf(rr, sizeof rr, "-r%d", ra); snprintf(fin, sizeof fin, "r%d + sqrt_(d2_)", ra); break;
         default: snprintf(rr, sizeof rr, "0.0f"); snprintf(fin, sizeof fin, "sqrt_(d2_)"); break;
         }
         if (min_form->kind == 4) { snprintf(buf, sizeof buf, "   const float d2_ = r%d;\n", ra); body += buf; }
         snprintf(buf, sizeof buf,
                  "   const float tsum_ = closest + (%s);\n"
                  "   const bool need_ = !(tsum_ < 0.0f) && !(d2_ > (tsum_ * tsum_) * 1.000001f);\n"
                  "   if (__ballot(need_) != 0ull) closest = min_raw(closest, %s);\n"
                  "   return closest;\n", rr, fin);
         body += buf;
         break;
      }
      if (min_form && (int)pc == min_form->pc_sqrt) { // the root waits (its register is read by the final operation only)
         used[ra] = true;
         snprintf(buf, sizeof buf, "   const float d2_ = r%d;\n", ra); body += buf;
         continue;
      }
      used[d] = true;
      const char *fmt = nullptr;
      switch (op) {
      case MDH_X_LIT: snprintf(buf, sizeof buf, "   r%d = __builtin_bit_cast(float, (int)0x%08xu);\n", d, (unsigned)code[++pc]); body += buf; continue;
      case MDH_X_COMP: snprintf(buf, sizeof buf, "   r%d = tab_float(ent + %d);\n", d, a); body += buf; continue;
      case MDH_X_POINT: snprintf(buf, sizeof buf, "   r%d = %s;\n", d, ARG[a < 10 ? a : 9]); body += buf; continue;
      case MDH_X_SEL: {
         const int c = code[++pc] & 63;
         used[ra] = used[b] = used[c] = true;
         snprintf(buf, sizeof buf, "   r%d = r%d != 0.0f ? r%d : r%d;\n", d, ra, b, c); body += buf; continue;
      }
      case MDH_X_MOV: fmt = "   r%d = r%d;\n"; break;
      case MDH_X_ADD: fmt = "   r%d = r%d + r%d;\n"; break;
      case MDH_X_SUB: fmt = "   r%d = r%d - r%d;\n"; break;
      case MDH_X_MUL: fmt = "   r%d = r%d * r%d;\n"; break;
      case MDH_X_DIV: fmt = "   r%d = r%d / r%d;\n"; break;
      case MDH_X_DIVF: fmt = "   r%d = ADA_DIV ? r%2$d + r%3$d : r%2$d / r%3$d;\n"; break;
      case MDH_X_NEG: fmt = "   r%d = -r%d;\n"; break;
      case MDH_X_ABS: fmt = "   r%d = __builtin_fabsf(r%d);\n"; break;
      case MDH_X_FLOOR: fmt = "   r%d = __builtin_floorf(r%d);\n"; break;
      case MDH_X_SIGN: fmt = "   r%d = sign_(r%d);\n"; break;
      case MDH_X_MIN: fmt = "   r%d = min_(r%d, r%d);\n"; break;
      case MDH_X_MAX: fmt = "   r%d = max_(r%d, r%d);\n"; break;
      case MDH_X_SQRT: fmt = "   r%d = sqrt_(r%d);\n"; break;
      case MDH_X_POW: fmt = "   r%d = pow_(r%d, r%d);\n"; break;
      case MDH_X_LT: fmt = "   r%d = r%d < r%d ? 1.0f : 0.0f;\n"; break;
      case MDH_X_GT: fmt = "   r%d = r%d > r%d ? 1.0f : 0.0f;\n"; break;
      case MDH_X_LE: fmt = "   r%d = r%d <= r%d ? 1.0f : 0.0f;\n"; break;
      case MDH_X_GE: fmt = "   r%d = r%d >= r%d ? 1.0f : 0.0f;\n"; break;
      case MDH_X_ITOF: fmt = "   r%d = (float)__builtin_bit_cast(int, r%d);\n"; break;
      case MDH_X_ACOS: fmt = "   r%d = acos_(r%d);\n"; break;
      case MDH_X_SIN: fmt = "   r%d = sin_(r%d);\n"; break;
      case MDH_X_COS: fmt = "   r%d = cos_(r%d);\n"; break;
      case MDH_X_TAN: fmt = "   r%d = tan_(r%d);\n"; break;
      case MDH_X_ASIN: fmt = "   r%d = asin_(r%d);\n"; break;
      case MDH_X_ATAN: fmt = "   r%d = atan_(r%d);\n"; break;
      default: fmt = "   r%d = 0.0f;\n"; break;
      }
      used[ra] = used[b] = true;
      if (op == MDH_X_DIVF) snprintf(buf, sizeof buf, "   r%d = ADA_DIV ? r%d + r%d : r%d / r%d;\n", d, ra, b, ra, b);
      else snprintf(buf, sizeof buf, fmt, d, ra, b);
      body += buf;
   }
   used[0] = used[1] = used[2] = true;
   if (min_form) {
      out += "MDH_DEV float ";
      out += name;
      out += "(int ent, f3 x, float closest)\n{\n   constexpr bool ADA_DIV = false;\n   float";
   } else {
      out += "template <bool ADA_DIV> MDH_DEV f3 ";
      out += name;
      out += "(int ent, f3 x, f3 nrm, f3 dir, float dist)\n{\n   float";
   }
   bool first = true;
   for (int i = 0; i < MDH_X_REGS; ++i)
      if (used[i]) { snprintf(buf, sizeof buf, "%s r%d = 0.0f", first ? "" : ",", i); out += buf; first = false; }
   out += ";\n" + body + (min_form ? "}\n" : "   return F3(r0, r1, r2);\n}\n");
}
// mdh_jit_kinds.h of a scene: the programs as functions and the two dispatchers mdh_device.h calls
static std::string jit_kinds_header(const mdh_renderer *r)
{
   std::string s = "// generated by libmadarch_hip (mdh_api.hip: jit_kinds_header)\n", prim_cases, light_cases, closest_all;
   char name[64], buf[512];
   for (int k = 0; k < r->npk; ++k) {
      if (r->pk[k].type != PK_CUSTOM) continue;
      const std::vector<int32_t> *progs[3] = {&r->pk[k].x_dist, &r->pk[k].x_nrm, &r->pk[k].x_mat};
      { // closest_primitive's loop over this kind's instances, the kind a constant; Distance in its min form where it has one
         const JitMinForm mf = jit_min_form(r->pk[k].x_dist);
         snprintf(name, sizeof name, "jit_p%d_min", k);
         if (mf.kind) jit_emit_program(s, name, r->pk[k].x_dist, &mf);
         snprintf(buf, sizeof buf,
                  "   {\n      const int n = hdr(H_KCOUNT + %d), stride = hdr(H_KSTRIDE + %d) * 4;\n      int ent = hdr(H_KSLOT + %d) * 4;\n"
                  "#pragma unroll 1\n      for (int i = 0; i < n; ++i, ent += stride) closest = %s;\n   }\n", k, k, k,
                  mf.kind ? (std::string(name) + "(ent, x, closest)").c_str()
                          : ("min_raw(closest, jit_p" + std::to_string(k) + "_0<false>(ent, x, F3(0.0f, 0.0f, 0.0f), F3(0.0f, 0.0f, 0.0f), 0.0f).x)").c_str());
         closest_all += buf;
      }
      for (int q = 0; q < 3; ++q) {
         snprintf(name, sizeof name, "jit_p%d_%d", k, q);
         jit_emit_program(s, name, *progs[q]);
         snprintf(buf, sizeof buf, "   case %d: return %s<ADA_DIV>(ent, x, F3(0.0f, 0.0f, 0.0f), F3(0.0f, 0.0f, 0.0f), 0.0f);\n", q * 8 + k, name);
         prim_cases += buf;
      }
   }
   for (int k = 0; k < r->nlk; ++k) {
      if (r->lk[k].type != LK_CUSTOM) continue;
      const std::vector<int32_t> *progs[2] = {&r->lk[k].x_dist, &r->lk[k].x_nrm};
      for (int q = 0; q < 2; ++q) {
         snprintf(name, sizeof name, "jit_l%d_%d", k, q);
         jit_emit_program(s, name, *progs[q]);
         snprintf(buf, sizeof buf, "   case %d: return %s<false>(ent, pos, nrm, dir, dist);\n", q * 4 + k, name);
         light_cases += buf;
      }
   }
   s += "// closest_primitive over every instance of every user-defined kind (scenes.adb:602-629)\n"
        "#define MDH_JIT_CLOSEST_ALL 1\nMDH_DEV float jit_closest_all(f3 x, float closest)\n{\n" + closest_all + "   return closest;\n}\n";
   s += "// which: 0 Distance, 1 Normal, 2 Material; k: the kind (wave-uniform)\n"
        "template <bool ADA_DIV> MDH_DEV f3 jit_prim(int which, int k, int ent, f3 x)\n{\n   switch (which * 8 + k) {\n" + prim_cases +
        "   default: break;\n   }\n   return F3(0.0f, 0.0f, 0.0f);\n}\n"
        "// which: 0 Sample, 1 Position\n"
        "MDH_DEV f3 jit_light(int which, int k, int ent, f3 pos, f3 nrm, f3 dir, float dist)\n{\n   switch (which * 4 + k) {\n" + light_cases +
        "   default: break;\n   }\n   return F3(0.0f, 0.0f, 0.0f);\n}\n";
   return s;
}

// hiprtc is loaded when the first user-defined kind is compiled; a box without it falls back to the interpreter
struct HiprtcApi {
   decltype(&hiprtcCreateProgram) CreateProgram = nullptr;
   decltype(&hiprtcDestroyProgram) DestroyProgram = nullptr;
   decltype(&hiprtcAddNameExpression) AddNameExpression = nullptr;
   decltype(&hiprtcCompileProgram) CompileProgram = nullptr;
   decltype(&hiprtcGetCodeSize) GetCodeSize = nullptr;
   decltype(&hiprtcGetCode) GetCode = nullptr;
   decltype(&hiprtcGetLoweredName) GetLoweredName = nullptr;
   decltype(&hiprtcGetProgramLogSize) GetProgramLogSize = nullptr;
   decltype(&hiprtcGetProgramLog) GetProgramLog = nullptr;
   decltype(&hiprtcGetErrorString) GetErrorString = nullptr;
   bool ok = false;
};
static const HiprtcApi &hiprtc_api()
{
   static HiprtcApi api;
   static bool tried = false;
   if (tried) return api;
   tried = true;
   void *h = nullptr;
   for (const char *name : {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
   if (!h) return api;
#define MDH_RTC_SYM(field, sym) api.field = (decltype(api.field))dlsym(h, #sym)
   MDH_RTC_SYM(CreateProgram, hiprtcCreateProgram); MDH_RTC_SYM(DestroyProgram, hiprtcDestroyProgram);
   MDH_RTC_SYM(AddNameExpression, hiprtcAddNameExpression); MDH_RTC_SYM(CompileProgram, hiprtcCompileProgram);
   MDH_RTC_SYM(GetCodeSize, hiprtcGetCodeSize); MDH_RTC_SYM(GetCode, hiprtcGetCode); MDH_RTC_SYM(GetLoweredName, hiprtcGetLoweredName);
   MDH_RTC_SYM(GetProgramLogSize, hiprtcGetProgramLogSize); MDH_RTC_SYM(GetProgramLog, hiprtcGetProgramLog);
   MDH_RTC_SYM(GetErrorString, hiprtcGetErrorString);
#undef MDH_RTC_SYM
   api.ok = api.CreateProgram && api.DestroyProgram && api.AddNameExpression && api.CompileProgram && api.GetCodeSize && api.GetCode &&
            api.GetLoweredName && api.GetProgramLogSize && api.GetProgramLog && api.GetErrorString;
   return api;
}

struct JitModule {
   hipModule_t mod = nullptr;
   std::map<std::string, hipFunction_t> fn;
};
static std::mutex g_jit_mutex;
static std::map<std::string, JitModule *> g_jit_cache;

// Compile the kernels named by `exprs` (template-ids) around this scene's mdh_jit_kinds.h.
static JitModule *jit_module(mdh_renderer *r, const std::vector<std::string> &exprs)
{
   const HiprtcApi &rtc = hiprtc_api();
   if (!rtc.ok) { seterr(MDH_E_DEVICE, "libhiprtc.so cannot be loaded: user-defined kinds are interpreted"); return nullptr; }
   if (r->jit_kinds.empty()) {
      r->jit_kinds = jit_kinds_header(r);
      if (const char *dump = getenv("MADARCH_HIP_JIT_DUMP")) // (diagnostic: the generated mdh_jit_kinds.h of the scene)
         if (FILE *f = fopen(dump, "w")) { fputs(r->jit_kinds.c_str(), f); fclose(f); }
   }
   std::string key = "device " + std::to_string(r->device) + "\n" + r->jit_kinds; // (a module and its functions belong to the device they were loaded on)
   for (auto &e : exprs) key += "|" + e;
   std::lock_guard<std::mutex> lock(g_jit_mutex);
   auto it = g_jit_cache.find(key);
   if (it != g_jit_cache.end()) return it->second;
   const char *headers[4] = {MDH_SRC_DEVICE, MDH_SRC_MARCH, MDH_SRC_KERNELS, r->jit_kinds.c_str()};
   const char *names[4] = {"mdh_device.h", "mdh_march.h", "mdh_kernels.h", "mdh_jit_kinds.h"};
   hiprtcProgram prog = nullptr;
   auto fail = [&](const char *what, hiprtcResult e) -> JitModule * {
      std::string log;
      size_t n = 0;
      if (prog && rtc.GetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) { log.resize(n); rtc.GetProgramLog(prog, &log[0]); }
      snprintf(g_err, sizeof g_err, "hiprtc %s failed (%s): %.380s", what, rtc.GetErrorString(e), log.c_str());
      if (prog) rtc.DestroyProgram(&prog);
      return nullptr;
   };
   hiprtcResult e = rtc.CreateProgram(&prog, "#define MDH_JIT 1\n#include \"mdh_kernels.h\"\n", "mdh_jit.hip", 4, headers, names);
   if (e != HIPRTC_SUCCESS) return fail("create", e);
   for (auto &x : exprs)
      if ((e = rtc.AddNameExpression(prog, x.c_str())) != HIPRTC_SUCCESS) return fail("name expression", e);
   // the flags of the Makefile: one IEEE operation per source operation, no vectorizers
   const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero", "-fno-vectorize", "-fno-slp-vectorize"};
   if ((e = rtc.CompileProgram(prog, (int)(sizeof opts / sizeof opts[0]), opts)) != HIPRTC_SUCCESS) return fail("compile", e);
   size_t size = 0;
   if ((e = rtc.GetCodeSize(prog, &size)) != HIPRTC_SUCCESS) return fail("code size", e);
   std::vector<char> code(size);
   if ((e = rtc.GetCode(prog, code.data())) != HIPRTC_SUCCESS) return fail("code", e);
   JitModule *m = new JitModule();
   if (hipModuleLoadData(&m->mod, code.data()) != hipSuccess) { delete m; return fail("module load", HIPRTC_ERROR_INTERNAL_ERROR); }
   for (auto &x : exprs) {
      const char *lowered = nullptr;
      if ((e = rtc.GetLoweredName(prog, x.c_str(), &lowered)) != HIPRTC_SUCCESS) { delete m; return fail("lowered name", e); }
      hipFunction_t f = nullptr;
      if (hipModuleGetFunction(&f, m->mod, lowered) != hipSuccess) { delete m; return fail("module function", HIPRTC_ERROR_INTERNAL_ERROR); }
      m->fn[x] = f;
   }
   rtc.DestroyProgram(&prog);
   g_jit_cache[key] = m;
   return m;
}
// Does the radiance pass of this renderer's slice leave most wavefront slots empty (k_radiance's SMALL variant)?
static bool rad_small_launch(const mdh_renderer *r)
{
   const KProbes p = make_probes(r);
   const long waves = ((long)(p.probe_end - p.probe_begin) * p.rres * p.rres + 63) / 64;
   return waves <= (long)r->n_cus * 4 * MDH_RAD_SMALL_WAVES_PER_SIMD;
}
// The workgroups of the radiance pass the chip holds at once, when the launch is that and a remainder smaller than
// it (k_radiance, mdh_kernels.h: the remainder runs at a raised issue priority); 0 otherwise.
static int rad_first_round(mdh_renderer *r, const void *kernel, hipFunction_t fn, size_t lds, int blocks)
{
   const void *key = kernel ? kernel : (const void *)fn;
   auto it = r->resident.find({key, lds});
   if (it == r->resident.end()) {
      int per_cu = 0;
      const hipError_t e = kernel ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, MDH_BLOCK, lds)
                                  : hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, MDH_BLOCK, lds);
      if (e != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
      it = r->resident.insert({{key, lds}, per_cu}).first;
   }
   const long first = (long)it->second * r->n_cus;
   return first > 0 && blocks > first && blocks < 2 * first ? (int)first : 0;
}
// launch a function of a JIT module: the arguments are the kernel's by-value structs, laid out as the
// kernarg segment lays them out (each at its natural alignment = a struct of them)
template <typename Args> static int jit_launch(hipFunction_t f, int blocks, int block, size_t lds, hipStream_t st, Args &args)
{
   size_t size = sizeof(Args);
   void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
   HIP_TRY(hipModuleLaunchKernel(f, blocks, 1, 1, block, 1, 1, (unsigned)lds, st, nullptr, extra));
   return MDH_OK;
}

// Every kernel template is named in ONE function at the end of this file, kernel_ptr, and launched through the pointer it
// returns: a kernel template is instantiated where it is first named, and the code object keeps that order -- the passes of
// frames in flight share their CUs' instruction caches (measured: the same kernels at other addresses, each as fast by itself,
// the headline with frames in flight 0.5 % slower).  The kernels of global residency (MDH_PF_GTAB, mdh_device.h: Geo) come
// last there: behind everything else they move nothing.
enum { GK_k_visibility, GK_k_scat_march, GK_k_scattering, GK_k_radiance, GK_k_screen, GK_k_partition_build, GK_k_eval_distance, GK_k_diag_segments, GK_k_ray_query, GK_k_ray_stream, GK_k_ray_shade, GK_k_camera_rays, GK_k_point_shade, GK_k_path_trace, GK_k_point_inscatter, GK_k_ray_inscatter, GK_k_listed, GK_k_surface_field, GK_k_surface_vertices, GK_k_surface_field_listed, GK_k_surface_vertices_listed, GK_k_path_frame, GK_k_path_frame_rays, GK_k_path_frame_resolve,
       GK_k_path_frame_adaptive, GK_k_path_adapt_count, GK_k_path_adapt_scan, GK_k_path_adapt_compact, GK_k_path_adapt_stats, GK_k_path_frame_resolve_adaptive };
// WHICH KERNEL A PASS RUNS ("One place that picks a pass's kernel"): every template argument of the
// pass's kernel, computed once by pick_kernel; kernel_name and kernel_ptr turn the same description into the name hiprtc
// instantiates and into the kernel of this library.
struct PassKernel {
   int family = -1; // GK_*
   int pf = 0;      // the kernel's MDH_PF_* word
   int mode = 0;    // k_screen, k_ray_shade: the screen mode (k_point_shade: 0, 2, or 3 for the irradiance alone), ...
   bool gbuf = false, alt = false; // ... the geometry buffer, the variant of the optional specular bodies
   bool small = false;             // k_radiance: SMALL
   int rec = 0;                    // k_radiance, k_screen: REC (0 marches, 1 marches and records, 2 replays the records: rad_replay_pick, scr_replay_pick)
   int what = 0;                   // k_ray_query, k_ray_stream, k_listed: WHAT (MDH_RQ_*); k_path_frame: REUSE (1: no jitter); k_path_adapt_compact: COMPACT
   bool ada_div = false;           // k_eval_distance: MDH_OPT_ADA_DIVISION
   bool jit = false; // a function of the scene's hiprtc module (user-defined kinds under MDH_OPT_JIT), not a kernel of this library
   int pfk = 0;      // the variant by the scene's census, before the pass's own choices, and the power-of-two addressing
   bool pow2 = false; // ... of the atlases: what mdh_diag_variant reports
};
static const void *kernel_ptr(const PassKernel &k);
template <typename... A> static int launch_kernel_ptr(const void *kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... a)
{
   if (!kernel) return seterr(MDH_E_INVALID, "no kernel built for this variant"); // (kernel_ptr lists no such instantiation)
   void *args[] = {(void *)&a...}; // (by value, in the kernel's parameter types: the call sites pass exactly those)
   (void)hipLaunchKernel(kernel, grid, block, args, lds, st); // (errors surface in hipGetLastError, as after hipLaunchKernelGGL)
   return MDH_OK;
}
// the kernels outside the passes that stage the scene table (the partition's builder, the distance query), by its residency
static const void *table_kernel(const mdh_renderer *r, int family, int what = 0)
{
   PassKernel k;
   k.family = family;
   k.pf = r->residency ? MDH_PF_GTAB : 0;
   k.ada_div = r->opt_ada_div != 0;
   // the distance query walks the triangle BVH too -- unless it divides as Madarch.Values."/" does (L + R: no distance, no bound)
   if (family == GK_k_eval_distance && r->bvh_active && !k.ada_div) k.pf |= MDH_PF_BVH;
   // the ray queries march as the passes do: through the space partition (its border as a variant of its own) or the triangle
   // BVH where the scene has one -- the general variants, whose bits the census variants share (pick_kernel)
   if (family == GK_k_ray_query || family == GK_k_ray_stream || family == GK_k_ray_shade || family == GK_k_point_shade || family == GK_k_path_trace ||
       family == GK_k_point_inscatter || family == GK_k_ray_inscatter || family == GK_k_surface_field || family == GK_k_surface_vertices ||
       family == GK_k_path_frame || family == GK_k_path_frame_adaptive) {
      k.what = what;
      if (family == GK_k_ray_shade || family == GK_k_point_shade) { k.what = 0; k.mode = what; } // (mdh_shade_rays, mdh_shade_points: `what` is the call's mode)
      if (r->part.enable) k.pf |= MDH_PF_PART | (r->part.border_behavior != 0 ? MDH_PF_FALLBACK : 0);
      if (r->bvh_active) k.pf |= MDH_PF_BVH;
   }
   if (family == GK_k_listed) k.what = what; // (the exact scan of listed kinds: the table's residency alone)
   return kernel_ptr(k);
}

// Update_Partitioning (renderers.adb:757-775): all three methods build the table on the device
extern "C" int32_t mdh_update_partitioning(mdh_renderer *r, int32_t method)
{
   settle_bump(r);
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!r->part.enable) return MDH_OK; // renderers.adb:763-765
   if (method < 0 || method > 2) return seterr(MDH_E_INVALID, "bad method");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   // The build goes where the table is used first -- the probe stream when frames are kept in flight -- into the
   // next buffer of the ring, and nothing waits on the host: frames in flight keep their buffer, later launches
   // on any stream are ordered after part_fence (table_acquire).
   const bool piped = r->opt_overlap && r->stream == r->own_stream && r->opt_mode == 0;
   hipStream_t up = piped ? r->probe_stream : r->stream;
   int rc = ensure_committed(r, up);
   if (rc != MDH_OK) return rc;
   if (!piped) {
      if ((rc = join_main(r)) != MDH_OK) return rc;
      r->main_dirty = true;
   }
   const int sup = stream_index(r, up);
   const int ns = (r->part_slot + 1) % mdh_renderer::PART_RING;
   HIP_TRY(r->part_use.retire_on_stream(ns, up, sup)); // the last kernels that read that buffer (four builds ago)
   // the warning counter is shared by consecutive builds: behind the previous build and its read-back
   if (r->part_fence.version && r->part_fence.by != up) HIP_TRY(hipStreamWaitEvent(up, r->ev_warn.ev, 0));
   PartBuildArgs a;
   a.method = method;
   const int *d = r->part.grid_dimensions;
   if (method == 2) { a.gx = 2 * (d[0] / 2); a.gy = 2 * (d[1] / 2); a.gz = 2 * (d[2] / 2); }
   else { a.gx = d[0]; a.gy = d[1]; a.gz = d[2]; }
   for (int i = 0; i < 3; ++i) {
      // the CPU builders read the settings record, the compute shader the GLSL text
      a.sp[i] = method == 2 ? r->pg_spacing[i] : r->part.grid_spacing[i];
      a.off[i] = method == 2 ? r->pg_offset[i] : r->part.grid_offset[i];
   }
   a.gpu_diag = r->part_gpu_diag;
   a.table = r->d_part_ring[ns].ptr;
   a.warnings = r->d_warn.ptr;
   // The builders write a cell's counts and the candidates it found, nothing else: entries behind them and cells
   // outside the builder's grid (GPU_Fast on odd dimensions) keep what the table held before, in the
   // reference's single buffer.  So the next buffer starts as a copy of the current one (tens of KiB).
   const size_t total = part_buffer_ints(r); // (the lists and their bits)
   const int cells = a.gx * a.gy * a.gz;
   if ((rc = table_acquire(r, up)) != MDH_OK) return rc; // (also orders `up` after the previous build)
   HIP_TRY(hipMemcpyAsync(r->d_part_ring[ns].ptr, r->d_part_ring[r->part_slot].ptr, total * 4, hipMemcpyDeviceToDevice, up));
   HIP_TRY(hipMemsetAsync(r->d_warn.ptr, 0, 4, up));
   if (cells > 0) {
      if ((rc = launch_kernel_ptr(table_kernel(r, GK_k_partition_build), dim3(cells), dim3(64), lds_bytes(r), up, r->ks, a)) != MDH_OK) return rc; // one wavefront per cell
      HIP_TRY(hipGetLastError());
   }
   // the lists once more as bits, for every cell (cells the builder left alone keep their lists, and so their bits)
   hipLaunchKernelGGL(k_partition_bits, dim3((r->part_cells + 63) / 64), dim3(64), lds_bytes(r), up, r->ks, r->d_part_ring[ns].ptr);
   HIP_TRY(hipGetLastError());
   if ((rc = table_release(r, up)) != MDH_OK) return rc; // (the copy read the current buffer)
   HIP_TRY(hipMemcpyAsync(r->h_warn.ptr, r->d_warn.ptr, 4, hipMemcpyDeviceToHost, up));
   HIP_TRY(hipEventRecord(r->ev_warn.ev, up));
   r->warn_pending = true;
   HIP_TRY(r->part_fence.signal(up, sup));
   ++r->march_inputs; // (the partition variants march through the new table: any record of their rays would be stale)
   r->part_slot = ns;
   r->ks.part_table = r->d_part_ring[ns].ptr;
   return MDH_OK;
}

// MDH_OPT_WINDOW: the pinned host buffer the next screen pass stores the window's pixels in.  A ring: the pixels
// of a frame stay untouched until WIN_RING - 1 further screen passes have been enqueued.
static int window_slot(mdh_renderer *r, int rank, int world, unsigned **out)
{
   const size_t bytes = (size_t)r->W * r->H * 4;
   const bool owner_changed = r->win_owner[0] != rank || r->win_owner[1] != world;
   if (owner_changed) { // other ranks' tiles read 0, as in the framebuffer: clear every slot once nothing writes them any more
      { int sr = sync_streams(r, SYNC_PROBE | SYNC_ALT | SYNC_MAIN); if (sr != MDH_OK) return sr; }
      for (int q = 0; q < mdh_renderer::WIN_RING; ++q)
         if (r->h_win[q].ptr) memset(r->h_win[q].ptr, 0, bytes);
      r->win_owner[0] = rank; r->win_owner[1] = world;
   }
   const int slot = (int)(r->win_passes % mdh_renderer::WIN_RING);
   if (!r->h_win[slot].ptr) {
      HIP_TRY(r->h_win[slot].grow(bytes / 4));
      memset(r->h_win[slot].ptr, 0, bytes);
   }
   r->win_passes += 1;
   r->win_valid = true;
   *out = r->h_win[slot].ptr;
   return MDH_OK;
}

// the census of the reference's rooms (MDH_PF_ROOM) among the scenes without partition or user-defined kinds (pick_kernel)
static bool room_census(const mdh_renderer *r)
{
   return r->ks.n_axis > 0 && r->ks.gplane_count == 0 && r->ks.tcount[PK_SPHERE] == 1 && r->ks.tcount[PK_BOX] == 1 &&
          r->ks.tcount[PK_TRIANGLE] == 0;
}
// MDH_OPT_RADIANCE_MIPS: does the screen pass over atlas set `set` read the levels of its radiance atlas (KProbes::rad_mips)?
static bool rad_mips_used(const mdh_renderer *r, int set) { return r->opt_mips && r->opt_mode == 0 && r->opt_spec != 0 && r->d_rad_mips[set].ptr; }

// MDH_OPT_RADIANCE_REPLAY.  The variants built with record and replay kernels: the brute-force scan and the census of the rooms,
// with and without power-of-two atlases (kernel_ptr).  The partition, global-residency / BVH and user-defined-kind variants
// keep marching.
#define MDH_RAD_REPLAY_BUILT (MDH_RAD_REPLAY && MDH_RAD_QVIS && MDH_SHARE_FIRST_STEP)
static bool rad_replay_built(const PassKernel &k) { return MDH_RAD_REPLAY_BUILT && !k.jit && (k.pf & ~(MDH_PF_ROOM | MDH_PF_POW2)) == 0; }
// everything the marches of this renderer's probe rays read, and the kernel that runs them
static RadRecKey rad_rec_key(const mdh_renderer *r, const PassKernel &k)
{
   RadRecKey q = {};
   const KProbes p = make_probes(r);
   q.geometry = r->geometry_edits; q.inputs = r->march_inputs; q.part_version = r->part_fence.version;
   q.grid[0] = p.gx; q.grid[1] = p.gy; q.grid[2] = p.gz;
   q.spacing[0] = p.sx; q.spacing[1] = p.sy; q.spacing[2] = p.sz;
   q.res[0] = p.rres; q.res[1] = p.ires; q.pc[0] = p.pcx; q.pc[1] = p.pcy;
   q.probe_begin = p.probe_begin; q.probe_end = p.probe_end;
   q.rays = (long)(p.probe_end - p.probe_begin) * p.rres * p.rres;
   q.max_dist = r->ks.max_dist;
   q.pf = k.pf; q.small = k.small ? 1 : 0; q.jit = k.jit ? 1 : 0; q.residency = r->residency; q.bvh = r->bvh_active ? 1 : 0;
   q.table_f4 = r->ks.table_f4; q.part_bits_f4 = r->ks.part_bits_f4;
   return q;
}
// The schedule is ReplaySchedule's (mdh_host.h); here, what makes the recording kernel admissible.
static int rad_replay_pick(const mdh_renderer *r, const PassKernel &k)
{
   const RadRecKey now = rad_rec_key(r, k);
   // (the recording kernel parks five rows more than the marching one: a table that commit_scene fitted into the workgroup's LDS
   //  budget beside MDH_PARK_DWORDS rows may not fit beside these -- such a scene keeps marching, and the counters say so)
   const bool admissible = now.rays > 0 && now.rays < (1l << 31) &&
                           lds_bytes(r) + (size_t)MDH_RECORD_PARK_ROWS * MDH_BLOCK * sizeof(float) <= MDH_LDS_WORKGROUP_BUDGET;
   return r->rad_replay.choose(now, r->opt_rad_replay && rad_replay_built(k), r->d_rad_rec.ptr != nullptr, admissible);
}

// MDH_OPT_SCREEN_REPLAY ("Exact work elimination", item 12).  The variants built with record and replay
// kernels: the fixed mode (mode 0, no optional specular body) over the brute-force scan and the census of the rooms, for
// and without power-of-two atlases, with and without the geometry buffer (kernel_ptr: sixteen kernels; the build time is in
// DESIGN.md).  Everything else keeps marching.
#define MDH_SCR_REPLAY_BUILT (MDH_SCR_REPLAY && MDH_SHARE_FIRST_STEP && MDH_REUSE_FOLDED)
static bool scr_replay_built(const PassKernel &k) { return MDH_SCR_REPLAY_BUILT && !k.jit && k.mode == 0 && !k.alt && (k.pf & ~(MDH_PF_ROOM | MDH_PF_POW2)) == 0; }
// What the key holds, and what every entry point does to it:
//   mdh_set_primitive, mdh_add_primitive                 geometry_edits                       end the replay
//   mdh_update_partitioning, MDH_OPT_JIT, _TABLE_RESIDENCY, _TRIANGLE_BVH   march_inputs / part_fence.version   end it (and pick a variant that only marches)
//   mdh_set_camera_position / _orientation               cam, by value                        a new value ends it, the held value does not
//   MDH_OPT_RANK, _WORLD, _SCREEN_MODE, _INDIRECT_SPECULAR, _AO_STEPS, _GBUFFER, _WINDOW, _SCREEN_SPLIT   by value   a new value ends it
//   mdh_set_material                                     reflect_edits                        only when a material in use goes below roughness 0.75
//   mdh_add_material, mdh_set_light, mdh_write_texture, mdh_write_atlas_slice, MDH_OPT_ATLAS_FORMAT, _HYSTERESIS_PERMILLE,
//   _SCREEN_ORDER, _FRAME_OVERLAP, _TIMING, _RADIANCE_*   nothing: a record holds nothing they change
// (width, height, probe grid, spacing, resolutions and max_dist are fixed at mdh_create; the key holds them all the same)
static ScrRecKey scr_rec_key(const mdh_renderer *r, const PassKernel &k)
{
   ScrRecKey q = {};
   q.march = rad_rec_key(r, k);
   q.march.small = k.gbuf ? 1 : 0; // (k_radiance's SMALL has no meaning here: the kernel's other template argument)
   q.march.probe_begin = q.march.probe_end = 0; q.march.rays = 0; // (the radiance pass's slice: a screen march reads every probe's place, none of its rays)
   memcpy(q.cam, r->cam_pos, 12); memcpy(q.cam + 3, r->cam_m, 36);
   q.W = r->W; q.H = r->H; q.rank = r->opt_rank; q.world = r->opt_world;
   q.mode = r->opt_mode; q.spec = r->opt_spec; q.ao = r->opt_ao; q.gbuffer = r->opt_gbuffer; q.window = r->opt_window; q.split = r->opt_scr_split;
   q.reflect_edits = r->reflect_edits;
   return q;
}
static long scr_rec_pixels(const mdh_renderer *r)
{
   const long tiles = (long)((r->W + 7) / 8) * ((r->H + 7) / 8);
   return r->opt_rank < r->opt_world ? (tiles - r->opt_rank + r->opt_world - 1) / r->opt_world * 64 : 0;
}
// The schedule is ReplaySchedule's (mdh_host.h); here, what makes the recording kernel admissible.
static int scr_replay_pick(const mdh_renderer *r, const PassKernel &k)
{
   // (the recording kernel parks eleven rows more than the marching one: a table that commit_scene fitted into the workgroup's
   //  LDS budget beside MDH_PARK_DWORDS rows may not fit beside these -- such a scene keeps marching, and the counters say so;
   //  the second point's arg-min index shares a word: tables of 2^22 entries and more keep marching too)
   const bool admissible = scr_rec_pixels(r) > 0 && r->ks.table_f4 < (int)MDH_REC2_INDEX_MASK &&
                           lds_bytes(r) + (size_t)MDH_SCR_RECORD_PARK_ROWS * MDH_BLOCK * sizeof(float) <= MDH_LDS_WORKGROUP_BUDGET;
   return r->scr_replay.choose(scr_rec_key(r, k), r->opt_scr_replay && scr_replay_built(k), r->d_scr_rec.ptr != nullptr, admissible);
}

static PassKernel pick_kernel(const mdh_renderer *r, int pass, int set)
{
   PassKernel k;
   const bool custom = has_custom_kinds(r);
   // bit 0 = space partition, bit 1 = user-defined kinds, bit 3 = the partition's border falls back to the full scan
   // (built-in kinds: a variant of its own; with user-defined kinds the kernels test the setting at run time)
   const int pf = (r->part.enable != 0 ? MDH_PF_PART : 0) | (custom ? MDH_PF_CUSTOM : 0) |
                  (r->part.enable != 0 && r->part.border_behavior != 0 && !custom ? MDH_PF_FALLBACK : 0);
   // bit 6 = global residency of the scene table (mdh_device.h: Geo; commit_scene chose it, never with user-defined kinds):
   // the general variants only -- no census, no power-of-two atlases
   const bool gtab = r->residency != 0;
   // bit 4 = the census of the reference's rooms (mdh_device.h: closest_primitive): every plane folded into the axis offsets,
   // one sphere, one box, nothing else, no partition -- the scan's loops as straight-line code
   const bool room = pf == 0 && room_census(r) && !gtab;
   // bit 5 = the partition's small form with its census (mdh_device.h: partitioning_closest_bits)
   const bool psmall = pf == MDH_PF_PART && r->ks.part_small && r->ks.part_tmask[PK_TRIANGLE] == 0 && r->ks.part_sp_pow2 && r->ks.part_cells < (1 << 24) && !gtab;
   // bit 7 = the triangle BVH (MDH_OPT_TRIANGLE_BVH; commit_scene: global residency, no partition, no user-defined kinds)
   k.pfk = gtab ? (pf | MDH_PF_GTAB | (r->bvh_active ? MDH_PF_BVH : 0)) : room ? MDH_PF_ROOM : (psmall ? (MDH_PF_PART | MDH_PF_PSMALL) : pf);
   // bit 2: the probe-sampling kernels (radiance, mode-0 screen) have a variant for atlases whose every dimension is a power
   // of two (and small enough for what it assumes besides: probe ids within 24-bit products, RGBA8 byte offsets within 32
   // bits -- mdh_device.h: grid_to_probe_id, atlas_rgba8)
   auto is_pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
   const long long pcount = (long long)r->probes.probe_count[0] * r->probes.probe_count[1];
   const long long rres = r->probes.radiance_resolution, ires = r->probes.irradiance_resolution;
   k.pow2 = is_pow2(r->probes.probe_count[0]) && is_pow2(r->probes.probe_count[1]) && is_pow2(r->probes.radiance_resolution) &&
            is_pow2(r->probes.irradiance_resolution) && pcount < 65536 && pcount * rres * rres <= (1ll << 30) && pcount * ires * ires <= (1ll << 30);
   // user-defined kinds compiled into the kernels (MDH_OPT_JIT), or interpreted by the kernels of this library -- which are
   // built without the power-of-two variant for them: scenes with user-defined kinds get it from hiprtc only
   k.jit = custom && r->opt_jit && pass != MDH_PASS_IRRADIANCE;
   const bool p2 = k.pow2 && !gtab && (!custom || k.jit);
   k.pf = k.pfk;
   switch (pass) {
   case MDH_PASS_RADIANCE:
      k.family = GK_k_radiance;
      if (p2) k.pf |= MDH_PF_POW2;
      k.small = rad_small_launch(r);
      k.rec = rad_replay_pick(r, k);
      break;
   case MDH_PASS_VISIBILITY: k.family = GK_k_visibility; break;
   case MDH_PASS_SCATTERING: k.family = MDH_SCAT_SPLIT ? GK_k_scat_march : GK_k_scattering; break;
   case MDH_PASS_SCREEN: {
      k.family = GK_k_screen;
      k.mode = r->opt_mode;
      k.gbuf = r->opt_gbuffer != 0;
      // the other two bodies of render_probes.glsl:264-272, and mode 2 over a mip chain that really exists: a variant of their own
      k.alt = k.mode == 0 && (r->opt_spec == 1 || r->opt_spec == 3 || (r->opt_spec == 2 && rad_mips_used(r, set)));
      // the census variants are built for the renderer's own pixel program (mode 0 without the optional bodies) and, the
      // partition's, for simple_scene's direct light + occlusion (mode 2, BASELINE config 2): everything else runs the general scan
      const int census = k.pf & (MDH_PF_ROOM | MDH_PF_PSMALL);
      if (!((k.mode == 0 && !k.alt) || ((census & MDH_PF_PSMALL) && k.mode == 2))) k.pf &= ~census;
      if (p2 && k.mode == 0 && !k.alt) k.pf |= MDH_PF_POW2;
      k.rec = scr_replay_pick(r, k);
      break;
   }
   default: break; // (the irradiance pass has one kernel)
   }
   return k;
}
// the name hiprtc instantiates for a scene's module
static std::string kernel_name(const PassKernel &k)
{
   char s[64] = "";
   switch (k.family) {
   case GK_k_radiance: snprintf(s, sizeof s, "k_radiance<%d, %s>", k.pf, k.small ? "true" : "false"); break;
   case GK_k_visibility: snprintf(s, sizeof s, "k_visibility<%d>", k.pf); break;
   case GK_k_scat_march: snprintf(s, sizeof s, "k_scat_march<%d>", k.pf); break;
   case GK_k_scattering: snprintf(s, sizeof s, "k_scattering<%d>", k.pf); break;
   case GK_k_screen: snprintf(s, sizeof s, "k_screen<%d, %d, %s, %s>", k.pf, k.mode, k.gbuf ? "true" : "false", k.alt ? "true" : "false"); break;
   default: break;
   }
   return s;
}

// One pass on stream `st`.  The radiance pass reads the irradiance atlas of set `src` and writes the
// radiance atlas of set `dst`; every other pass works on set `dst` (in place: src == dst == r->last).
struct PassRun {
   mdh_renderer *r;
   int pass;
   hipStream_t st;
   int src, dst, fbix;
   PassKernel k;
   const void *kernel = nullptr; // the kernel of this library, or ...
   hipFunction_t fn = nullptr;   // ... the function of the scene's hiprtc module (k.jit)
   KProbes pr;
   KCamera cam;
   hipEvent_t e0 = nullptr, e1 = nullptr; // MDH_OPT_TIMING
};
// A pass's kernel with its by-value arguments `a`.  Args is the struct of the kernel's parameters in their order: the kernel
// argument segment, as the function of a hiprtc module takes it (jit_launch).
template <typename Args, typename... A> static int launch_pass(const PassRun &p, int blocks, size_t lds, A... a)
{
   if (p.fn) {
      Args args = {a...};
      return jit_launch(p.fn, blocks, MDH_BLOCK, lds, p.st, args);
   }
   return launch_kernel_ptr(p.kernel, dim3(blocks), dim3(MDH_BLOCK), lds, p.st, a...);
}

static int pass_begin(PassRun &p)
{
   mdh_renderer *r = p.r;
   if (p.fbix < 0) p.fbix = r->fb_last;
   p.pr = make_probes(r);
   p.pr.rad = r->d_rad2[p.dst].ptr;
   p.pr.irr = r->d_irr2[p.pass == MDH_PASS_RADIANCE ? p.src : p.dst].ptr;
   p.cam = make_camera(r);
   p.k = pick_kernel(r, p.pass, p.dst);
   if (p.k.jit) { // a scene hiprtc cannot build falls back to the interpreter for good (the reason stays in mdh_last_error, MDH_OPT_JIT reads 0 afterwards)
      const std::string name = kernel_name(p.k);
      if (JitModule *jm = jit_module(r, {name})) p.fn = jm->fn[name];
      else { r->opt_jit = 0; settle_bump(r); p.k = pick_kernel(r, p.pass, p.dst); }
   }
   if (!p.k.jit && p.pass != MDH_PASS_IRRADIANCE && !(p.kernel = kernel_ptr(p.k))) return seterr(MDH_E_INVALID, "no kernel built for this pass's variant"); // (before anything is acquired)
   if (p.pass != MDH_PASS_IRRADIANCE) { // (the irradiance pass does not stage the scene table)
      int trc = table_acquire(r, p.st);
      if (trc != MDH_OK) return trc;
   }
#ifdef MDH_DIAG
   r->variant[p.pass][0] = p.k.pfk;
   r->variant[p.pass][1] = p.k.pow2 ? 1 : 0;
#endif
   if (r->opt_timing) {
      p.e0 = get_event(r);
      p.e1 = get_event(r);
      if (!p.e0 || !p.e1) return seterr(MDH_E_DEVICE, "hipEventCreate failed");
      HIP_TRY(hipEventRecord(p.e0, p.st));
   }
   return MDH_OK;
}
static int pass_end(PassRun &p)
{
   mdh_renderer *r = p.r;
   HIP_TRY(hipGetLastError());
   if (p.pass != MDH_PASS_IRRADIANCE) {
      int trc = table_release(r, p.st);
      if (trc != MDH_OK) return trc;
   }
   if (r->opt_timing && p.e1) {
      HIP_TRY(hipEventRecord(p.e1, p.st));
      r->pending.push_back({p.pass, p.e0, p.e1}); // (folded at frame boundaries: bound_timing)
   }
#ifdef MDH_DIAG
   { // the diagnostic build waits for every pass and takes its work counters
      HIP_TRY(hipStreamSynchronize(p.st));
      HIP_TRY(hipMemcpyFromSymbol(r->work[p.pass], HIP_SYMBOL(g_work), sizeof r->work[p.pass]));
      unsigned long long z[4] = {0, 0, 0, 0};
      HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_work), z, sizeof z));
   }
#endif
   return MDH_OK;
}

static int pass_radiance(PassRun &p)
{
   mdh_renderer *r = p.r;
   const KProbes &pr = p.pr;
   hipStream_t st = p.st;
   const long rays = (long)(pr.probe_end - pr.probe_begin) * pr.rres * pr.rres;
   long n = rays;
   {
      const int G = MDH_RAD_PROBES_PER_WAVE, T = (G == 1) ? 8 : (G == 4) ? 4 : (G == 16) ? 2 : 1;
      if (pr.rres % T == 0) n = (long)((pr.probe_end - pr.probe_begin + G - 1) / G) * G * pr.rres * pr.rres;
   }
   if (n <= 0) return MDH_OK;
   // the rays in the order of the previous pass's primary-march lengths (RadOrder, mdh_kernels.h)
   RadOrder ro = {nullptr, nullptr, (int)rays, nullptr};
   // MDH_OPT_RADIANCE_REPLAY: the pass that writes the rays' records, or reads them (pick_kernel chose: p.k.rec)
   if (p.k.rec == 1 && (size_t)rays > r->d_rad_rec.cap) { // (the buffer is only ever used by radiance passes, on the probe stream or the main stream)
      { int sr = sync_streams(r, SYNC_PROBE | SYNC_MAIN); if (sr != MDH_OK) return sr; }
      r->rad_replay.records_gone();
      HIP_TRY(r->d_rad_rec.grow((size_t)rays));
   }
   if (p.k.rec) ro.rec = r->d_rad_rec.ptr;
   // (chunks of whole workgroup strides, at most MDH_RO_MAX_CHUNKS of them)
   const long ro_chunk = std::max(2048l, ((rays + MDH_RO_MAX_CHUNKS - 1) / MDH_RO_MAX_CHUNKS + 1023) / 1024 * 1024);
   const int ro_chunks = (int)((rays + ro_chunk - 1) / ro_chunk);
   if (r->opt_rad_order && rays >= 8192 && rays < (1l << 31)) {
      if ((size_t)rays > r->d_rad_steps.cap) {
         // (the buffers are only ever used by radiance passes, on the probe stream or the main stream)
         { int sr = sync_streams(r, SYNC_PROBE | SYNC_MAIN); if (sr != MDH_OK) return sr; }
         r->rad_order.forget();
         HIP_TRY(create_all(r->d_rad_steps.sized((size_t)rays), r->d_rad_order.sized((size_t)rays), r->d_rad_hist.sized(256 * MDH_RO_MAX_CHUNKS)));
      }
      const bool have = r->rad_order.ordered && r->rad_order.of.rays == rays && r->rad_order.of.begin == pr.probe_begin;
      if (have) { ro.order = r->d_rad_order.ptr; n = rays; }
      // A probe ray's march changes with the scene's geometry, not with time, lights or materials: the rays are sorted
      // again when primitives were set or added since (at most every MDH_RAD_RESORT_MOVING passes: a stale order costs
      // speed only, and three more launches per frame cost the host of a 0.4 ms frame 10 %) and every MDH_RAD_RESORT
      // passes besides -- the sort kernels (20 us) are out of almost every frame.
      if (r->rad_order.due(have, r->rad_order.of.scene != r->geometry_edits)) ro.steps = r->d_rad_steps.ptr;
   }
   n = (n + 63) / 64 * 64;
   const int blocks = (int)((n + MDH_BLOCK - 1) / MDH_BLOCK);
   const size_t lds = p.k.rec == 2 ? lds_bytes(r) + (size_t)MDH_REPLAY_PARK_ROWS * MDH_BLOCK * sizeof(float)
                    : p.k.rec == 1 ? lds_bytes(r) + (size_t)MDH_RECORD_PARK_ROWS * MDH_BLOCK * sizeof(float) : lds_bytes_march(r);
   struct Args { KScene sc; KProbes pr; int first_round; RadOrder ro; };
   const int rc = launch_pass<Args>(p, blocks, lds, r->ks, pr, rad_first_round(r, p.kernel, p.fn, lds, blocks), ro);
   if (rc != MDH_OK) return rc;
   r->rad_replay.ran(p.k.rec, rad_rec_key(r, p.k), true); // what this pass marched through (or replayed), for the next pass's choice
   if (ro.steps) { // the next pass's order from this pass's step counts
      hipLaunchKernelGGL(k_rad_hist, dim3(ro_chunks), dim3(256), 0, st, (const unsigned char *)r->d_rad_steps.ptr, (int)rays, (int)ro_chunk, r->d_rad_hist.ptr);
      hipLaunchKernelGGL(k_rad_scan, dim3(1), dim3(256), 0, st, r->d_rad_hist.ptr, ro_chunks);
      hipLaunchKernelGGL(k_rad_scatter, dim3(ro_chunks), dim3(256), 0, st, (const unsigned char *)r->d_rad_steps.ptr, (int)rays, (int)ro_chunk, (const unsigned *)r->d_rad_hist.ptr, r->d_rad_order.ptr);
      r->rad_order.of = {rays, pr.probe_begin, r->geometry_edits};
      r->rad_order.sorted();
   } else if (!ro.order)
      r->rad_order.forget();
   return MDH_OK;
}

// MDH_OPT_PROBE_SETTLE: the irradiance pass of an open frame is numbered, and tracked when it is the frame's one irradiance
// pass behind its one radiance pass (any other pattern breaks the run: SettleTracker::enqueue)
static int settle_args(PassRun &p, int n, SettleArgs &sa)
{
   mdh_renderer *r = p.r;
   const bool regular = r->frame_probe_seq == 1 && n > 0;
   r->frame_probe_seq = regular ? 2 : -1;
   bool trackable = regular && r->opt_settle && settle_eligible(r) && !r->settle_no_memory;
   if (trackable && !r->d_settle.ptr) { // (zeroed once per renderer, here: every pass that finishes clears its own counter)
      if (create_all(r->h_settle.sized(SettleTracker::RING), r->d_settle.sized(1)) != hipSuccess) {
         (void)hipGetLastError();
         r->settle_no_memory = true; // (the feature is an optimisation: without its few bytes every pass runs)
         trackable = false;
      } else {
         memset(r->h_settle.ptr, 0, SettleTracker::RING * sizeof(SettleSlot));
         r->settle.slots = r->h_settle.ptr;
         HIP_TRY(hipMemsetAsync(r->d_settle.ptr, 0, sizeof(unsigned long long), p.st));
      }
   }
   SettleSlot *slot = nullptr;
   sa.seq = r->settle.enqueue(trackable, r->frame_pipelined ? 1 : 0, &slot);
   if (sa.seq) { sa.ctr = r->d_settle.ptr; sa.slot = (unsigned long long *)(void *)slot; }
   return MDH_OK;
}
static int pass_irradiance(PassRun &p)
{
   mdh_renderer *r = p.r;
   KProbes &pr = p.pr;
   if (r->opt_world > 1 && r->opt_irr_all) { pr.probe_begin = 0; pr.probe_end = probe_total(r); } // every rank, every probe
   int n = pr.probe_end - pr.probe_begin; // one workgroup per probe, its taps staged in LDS
   size_t lds = (size_t)2 * pr.rres * pr.rres * sizeof(float4);
   float *tap_planes = nullptr;
#if MDH_FAST_NUMERICS
   if (pr.ires * pr.ires <= 64) lds += (size_t)4 * 64 * sizeof(float4); // (the experiment's fold: all taps staged, four partial sums per texel)
   else
#endif
   if (pr.ires * pr.ires <= 64 && MDH_IRR_BLOCK == 256 && n > 0) { // (k_irradiance: a channel per wavefront, the taps through device memory)
      const size_t need = (size_t)n * 6 * MDH_IRR_CHANNELS_PLANE(pr.rres * pr.rres);
      if (need > r->d_irr_taps.cap) { // (the scratch of irradiance passes only, which follow one another on their stream)
         { int sr = sync_streams(r, SYNC_PROBE | SYNC_MAIN); if (sr != MDH_OK) return sr; }
         HIP_TRY(r->d_irr_taps.grow(need));
      }
      tap_planes = r->d_irr_taps.ptr;
      lds = MDH_IRR_CHANNELS_LDS;
   } else
   if (pr.ires * pr.ires <= 64 && lds > (size_t)4 * MDH_IRR_CHUNK * sizeof(float4)) lds = (size_t)4 * MDH_IRR_CHUNK * sizeof(float4); // two chunk buffers
   if (lds > 64 * 1024) { // radiance tiles beyond 45 x 45 texels: up to the whole 160 KiB of a CU (70 x 70)
      if (lds > 160 * 1024) return seterr(MDH_E_INVALID, "radiance resolution too large for the irradiance pass (160 KiB of LDS: at most 70)");
      if (!r->irr_lds_granted) { // (the attribute belongs to the function on THIS device: kept per renderer, not per process)
         HIP_TRY(hipFuncSetAttribute((const void *)k_irradiance, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
         r->irr_lds_granted = true;
      }
   }
   SettleArgs sa = {nullptr, nullptr, 0u};
   if (r->in_frame) { int src = settle_args(p, n, sa); if (src != MDH_OK) return src; }
   // (hysteresis: the previous frame's irradiance is set `src` -- the same set when the pass runs in place)
   if (n > 0) hipLaunchKernelGGL(k_irradiance, dim3(n), dim3(MDH_IRR_BLOCK), lds, p.st, pr, (const void *)r->d_irr2[p.src].ptr, (float)r->opt_hyst / 1000.0f, tap_planes, sa);
   return MDH_OK;
}

static int pass_visibility(PassRun &p)
{
   mdh_renderer *r = p.r;
   KVolumetrics vol = make_vol(r, true, p.dst);
   const long n = (long)vol.vw * vol.vh * vol.vz;
   if (n <= 0) return MDH_OK;
   // inside a frame the launch also marches the scattering texels' camera rays (k_visibility's second part, mdh_kernels.h)
   const int vis_blocks = (int)((n + MDH_BLOCK - 1) / MDH_BLOCK);
   int blocks = vis_blocks;
   if (MDH_SCAT_SPLIT && r->fuse_scat_march) blocks += (int)(((long)vol.sw * vol.sh + MDH_BLOCK - 1) / MDH_BLOCK);
   struct Args { KScene sc; KVolumetrics vol; KCamera cam; int vis_blocks; };
   return launch_pass<Args>(p, blocks, lds_bytes(r), r->ks, vol, p.cam, vis_blocks);
}

static int pass_scattering(PassRun &p)
{
   mdh_renderer *r = p.r;
   KVolumetrics vol = make_vol(r, true, p.dst);
   const long n = (long)vol.sw * vol.sh;
   if (n <= 0) return MDH_OK;
   const int blocks = (int)((n + MDH_BLOCK - 1) / MDH_BLOCK);
   struct Args { KScene sc; KVolumetrics vol; KCamera cam; };
   if (!(MDH_SCAT_SPLIT && r->fuse_scat_march)) { // (inside a frame the visibility pass's launch has marched them)
      const int rc = launch_pass<Args>(p, blocks, lds_bytes(r), r->ks, vol, p.cam);
      if (rc != MDH_OK) return rc;
   }
#if MDH_SCAT_SPLIT
   // the texels' lengths are in place: their steps, spread over lanes and folded in step order (k_scat_fold, mdh_kernels.h)
   HIP_TRY(hipGetLastError());
   hipLaunchKernelGGL(k_scat_fold, dim3((unsigned)((n + MDH_SCAT_TEXELS - 1) / MDH_SCAT_TEXELS)), dim3(MDH_SCAT_BLOCK), 0, p.st, vol);
#endif
   return MDH_OK;
}

// later screen passes' tile order from this pass's durations (ScreenArgs::cost), into the buffer no pass in flight reads
static int screen_sort_tiles(PassRun &p, const ScreenArgs &a)
{
   mdh_renderer *r = p.r;
   hipStream_t st = p.st;
   const KProbes &pr = p.pr;
   const int own_tiles = a.n_own, si_st = stream_index(r, st);
   HIP_TRY(hipGetLastError());
   if (r->opt_timing && p.e1) { // (the sort is no part of the pass's time: ADVICE r03)
      HIP_TRY(hipEventRecord(p.e1, st));
      r->pending.push_back({p.pass, p.e0, p.e1});
      p.e0 = p.e1 = nullptr;
   }
   ScrOrderOf &of = r->scr_order.of;
   const int nb = r->scr_order.ordered && of.buf == 0 ? 1 : 0;
   // (passes that read that buffer were launched before the previous sort; on the other screen stream nothing
   //  orders them against this stream when no probe passes run: wait for what that stream holds)
   hipStream_t other = st == r->alt_stream ? r->stream : r->alt_stream;
   if (other && other != st && r->scr_order.ordered) {
      HIP_TRY(hipEventRecord(r->ev_scr_other.ev, other));
      HIP_TRY(hipStreamWaitEvent(st, r->ev_scr_other.ev, 0));
   }
   const long chunk = std::max(2048l, (((long)own_tiles + MDH_RO_MAX_CHUNKS - 1) / MDH_RO_MAX_CHUNKS + 1023) / 1024 * 1024);
   const int chunks = (int)((own_tiles + chunk - 1) / chunk);
   // Sorted as a whole every screen pass measured is faster on its own (BASELINE config 3: +4.5 %, config 2: +59 %,
   // config 5's frame on one GPU: +7 %) and, with frames in flight, every frame but one kind: where the probe passes
   // are a large share of the frame (config 3 at 1080p: 524 288 probe rays for 2 M pixels), a screen pass that
   // holds every wavefront slot to its very end keeps the NEXT frame's probe passes -- the head of that frame's
   // dependency chain -- waiting for slots that the thin tail of an image-order pass hands over early: -3 %.
   // There only the tiles that took twice the median and more go to the front (the ones that make the tail) and
   // all others keep their place: +-0 in flight (profiles/r03_x_screen_tile_order.log).
   const long probe_rays = r->opt_mode == 0 ? (long)(pr.probe_end - pr.probe_begin) * pr.rres * pr.rres : 0;
   const bool probe_heavy = probe_rays * 10 >= (long)own_tiles * 64;
   const int floor_permille = r->frame_pipelined && r->in_frame_passes && probe_heavy ? 2000 : 0; // (thousandths of the median)
   hipLaunchKernelGGL(k_rad_hist, dim3(chunks), dim3(256), 0, st, (const unsigned char *)r->d_scr_cost.ptr, own_tiles, (int)chunk, r->d_scr_hist.ptr);
   if (floor_permille > 0) {
      hipLaunchKernelGGL(k_order_floor, dim3(chunks), dim3(256), 0, st, r->d_scr_cost.ptr, own_tiles, (int)chunk, (const unsigned *)r->d_scr_hist.ptr, chunks, floor_permille);
      hipLaunchKernelGGL(k_rad_hist, dim3(chunks), dim3(256), 0, st, (const unsigned char *)r->d_scr_cost.ptr, own_tiles, (int)chunk, r->d_scr_hist.ptr);
   }
   hipLaunchKernelGGL(k_rad_scan, dim3(1), dim3(256), 0, st, r->d_scr_hist.ptr, chunks);
   hipLaunchKernelGGL(k_order_scatter_stable, dim3(chunks), dim3(256), 0, st, (const unsigned char *)r->d_scr_cost.ptr, own_tiles, (int)chunk, (const unsigned *)r->d_scr_hist.ptr, r->d_scr_order[nb].ptr);
   HIP_TRY(hipGetLastError());
   HIP_TRY(r->scr_sorted.signal(st, si_st));
   of.buf = nb; of.n = own_tiles; of.rank = a.rank; of.world = a.world;
   of.geom = r->geometry_edits; // (the camera was stamped when the sort was decided: pass_screen)
   r->scr_order.sorted();
   return MDH_OK;
}

static int pass_screen(PassRun &p)
{
   mdh_renderer *r = p.r;
   hipStream_t st = p.st;
   KProbes &pr = p.pr;
   const int fbix = p.fbix;
   KVolumetrics vol = make_vol(r, r->vol.enabled != 0 && r->opt_mode == 0, p.dst);
   ScreenArgs a;
   a.W = r->W; a.H = r->H;
   a.tiles_x = (r->W + 7) / 8;
   a.n_tiles = a.tiles_x * ((r->H + 7) / 8);
   a.rank = r->opt_rank; a.world = r->opt_world;
   a.ao_steps = r->opt_ao;
   a.spec_mode = r->opt_spec;
   if (rad_mips_used(r, p.dst)) { // MDH_OPT_RADIANCE_MIPS: the levels of the atlas this pass reads
      int mrc = build_rad_mips(r, p.dst, st);
      if (mrc != MDH_OK) return mrc;
      pr.rad_mips = r->d_rad_mips[p.dst].ptr;
   }
   a.fb = r->d_fb2[fbix].ptr; a.gb_index = (int *)r->d_gb2[fbix][0].ptr; a.gb_t = (float *)r->d_gb2[fbix][1].ptr; a.gb_steps = (int *)r->d_gb2[fbix][2].ptr;
   a.window = nullptr;
   if (r->opt_window == 1 || (r->opt_window == 2 && r->swaps > 0)) { // the window's pixels straight into pinned host memory (mdh_swap_buffers)
      int wrc = window_slot(r, a.rank, a.world, &a.window);
      if (wrc != MDH_OK) return wrc;
   }
   // other ranks' tiles read 0: cleared when the buffer last held another rank's (or a whole) frame, not every frame
   if (a.world > 1 && (r->fb_owner[fbix][0] != a.rank || r->fb_owner[fbix][1] != a.world))
      HIP_TRY(hipMemsetAsync(r->d_fb2[fbix].ptr, 0, (size_t)r->W * r->H * sizeof(float4), st));
   r->fb_owner[fbix][0] = a.rank; r->fb_owner[fbix][1] = a.world;
   const int own_tiles = (a.n_tiles - a.rank + a.world - 1) / a.world;
   a.n_own = own_tiles;
   a.order = nullptr;
   a.cost = nullptr;
   // MDH_OPT_SCREEN_ORDER: the tiles in the order of an earlier pass's wavefront durations, slowest first
   bool sort_after = false;
   if (r->opt_scr_order && own_tiles >= 2048) {
      const int si_st = stream_index(r, st);
      if (!r->d_scr_cost.ptr)
         HIP_TRY(create_all(r->d_scr_cost.sized(a.n_tiles), r->d_scr_order[0].sized(a.n_tiles), r->d_scr_order[1].sized(a.n_tiles),
                            r->d_scr_hist.sized(256 * MDH_RO_MAX_CHUNKS), r->scr_sorted, r->ev_scr_other));
      float cam_now[12];
      memcpy(cam_now, r->cam_pos, 12); memcpy(cam_now + 3, r->cam_m, 36);
      ScrOrderOf &of = r->scr_order.of;
      const bool have = r->scr_order.ordered && of.n == own_tiles && of.rank == a.rank && of.world == a.world;
      if (have) {
         a.order = r->d_scr_order[of.buf].ptr;
         HIP_TRY(r->scr_sorted.wait(st, si_st)); // (the sort may have run on another stream)
      }
      // which tiles are slow follows the camera and the geometry: sorted again when either changed since (at most every
      // MDH_RAD_RESORT_MOVING passes: a stale order costs speed only) and every MDH_RAD_RESORT passes besides
      const bool moved = memcmp(cam_now, of.cam, sizeof cam_now) != 0 || of.geom != r->geometry_edits;
      if (r->scr_order.due(have, moved)) {
         sort_after = true;
         a.cost = r->d_scr_cost.ptr;
         memcpy(of.cam, cam_now, sizeof cam_now);
      }
   } else
      r->scr_order.forget();
   // MDH_OPT_SCREEN_SPLIT (ScreenArgs::split): launches that leave most of the chip's wavefront slots empty give a tile to
   // two or four wavefronts; never with a tile order (launches of 2 048 tiles and more)
   a.split = 0;
   if (!a.order && !a.cost && r->opt_scr_split > 0 && a.world == 1) { // (a rank's scattered tiles of a sharded frame: measured 1 - 3 % slower split, profiles/r04_x_split_tiles.log)
      if ((long)own_tiles * 4 <= r->opt_scr_split) a.split = 2;
      else if ((long)own_tiles * 2 <= r->opt_scr_split) a.split = 1;
   }
   // MDH_OPT_SCREEN_REPLAY: the pass that writes the pixels' records, or reads them (pick_kernel chose: p.k.rec)
   a.rec = nullptr;
   if (own_tiles <= 0) p.k.rec = 0;
   if (p.k.rec == 1 && (size_t)own_tiles * 64 > r->d_scr_rec.cap) {
      int drc = drain_streams(r);
      if (drc != MDH_OK) return drc;
      r->scr_replay.records_gone();
      r->scr_rec_reads.forget();
      HIP_TRY(create_all(r->scr_rec_written, r->scr_rec_reads)); // (only with the first records: events are scarce, mdh_create)
      if (r->d_scr_rec.grow((size_t)own_tiles * 64) != hipSuccess) { // no memory for the records: the renderer keeps marching, and the counters say so
         r->scr_replay.allocation_failed();
         (void)hipGetLastError();
         p.k.rec = 0;
         if (!(p.kernel = kernel_ptr(p.k))) return seterr(MDH_E_INVALID, "no kernel built for this pass's variant");
      }
   }
   if (p.k.rec) {
      const int si_st = stream_index(r, st);
      a.rec = r->d_scr_rec.ptr;
      HIP_TRY(r->scr_rec_written.wait(st, si_st)); // (the records may have been written on another stream)
      if (p.k.rec == 1) HIP_TRY(r->scr_rec_reads.retire_on_stream(0, st, si_st)); // ... and may still be read on another
   }
   if (own_tiles > 0) {
      const long waves = (long)own_tiles << a.split;
      const int blocks = (int)((waves + (MDH_BLOCK / 64) - 1) / (MDH_BLOCK / 64));
      struct Args { KScene sc; KProbes pr; KVolumetrics vol; KCamera cam; ScreenArgs a; };
      const size_t lds = p.k.rec == 1 ? lds_bytes(r) + (size_t)MDH_SCR_RECORD_PARK_ROWS * MDH_BLOCK * sizeof(float) : lds_bytes_screen(r);
      const int rc = launch_pass<Args>(p, blocks, lds, r->ks, pr, vol, p.cam, a);
      if (rc != MDH_OK) return rc;
   }
   { // what this pass marched through (or replayed), for the next pass's choice
      const int si_st = stream_index(r, st);
      if (p.k.rec == 1) HIP_TRY(r->scr_rec_written.signal(st, si_st));
      else if (p.k.rec == 2) HIP_TRY(r->scr_rec_reads.mark(0, st, si_st));
      r->scr_replay.ran(p.k.rec, scr_rec_key(r, p.k), r->opt_scr_replay != 0); // (with the option off the next pass marches plainly whatever its key)
   }
   return sort_after ? screen_sort_tiles(p, a) : MDH_OK;
}

static int run_pass(mdh_renderer *r, int pass, hipStream_t st, int src, int dst, int fbix = -1)
{
   if (pass < MDH_PASS_RADIANCE || pass > MDH_PASS_SCREEN) return seterr(MDH_E_INVALID, "bad pass");
   PassRun p = {r, pass, st, src, dst, fbix};
   int rc = pass_begin(p);
   if (rc != MDH_OK) return rc;
   switch (pass) {
   case MDH_PASS_RADIANCE: rc = pass_radiance(p); break;
   case MDH_PASS_IRRADIANCE: rc = pass_irradiance(p); break;
   case MDH_PASS_VISIBILITY: rc = pass_visibility(p); break;
   case MDH_PASS_SCATTERING: rc = pass_scattering(p); break;
   default: rc = pass_screen(p); break;
   }
   return rc != MDH_OK ? rc : pass_end(p);
}

extern "C" int32_t mdh_render_pass(mdh_renderer *r, int32_t pass)
{
   settle_bump(r);
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open: use mdh_frame_probe_pass / mdh_frame_end");
   if (r->opt_rank >= r->opt_world) return seterr(MDH_E_STATE, "MDH_OPT_RANK is not below MDH_OPT_WORLD");
   int rc = ensure_committed(r);
   if (rc != MDH_OK) return rc;
   if ((rc = join_main(r)) != MDH_OK) return rc;
   r->main_dirty = true;
   if ((rc = run_pass(r, pass, r->stream, r->last, r->last)) != MDH_OK) return rc;
   return bound_timing(r);
}
// Render (renderers.adb:302-321).
//
// Frame overlap (MDH_OPT_FRAME_OVERLAP, on by default, single-GPU renderers on their own stream).
// The probe passes of frame N+1 do not depend on the screen pass of frame N -- they need the
// irradiance atlas frame N produced and nothing else -- and the screen passes of two frames are
// independent of each other.  Every kernel of a frame ends in a tail of a few slow wavefronts
// (the radiance pass spends more than half of its time below 20 % occupancy; the irradiance pass
// fills a fraction of the chip), so serial frames leave the chip idle a good part of the time.
// Pipelined frames use three HIP streams (four with volumetrics), MDH_ATLAS_SETS = 3 atlas sets and two framebuffers;
// frame N works on set c = N mod 3 and reads the irradiance of set `last` = (N - 1) mod 3, its screen pass draws on
// stream and framebuffer p = N mod 2:
//    probe stream: wait screen(N-3) (the last reader of atlas set c)
//                  -> radiance(irr[last] -> rad[c]) -> [exchange] -> irradiance(rad[c] -> irr[c]) -> ev_probe[c]
//    volumetric stream (renderers with volumetrics): wait screen(N-3) -> visibility, scattering of set c -> ev_vol[c]
//    screen stream p (main / alternate): wait ev_probe[c] (and ev_vol[c]) -> screen(atlas set c -> framebuffer p)
// so that screen(N+1) starts while screen(N) drains and the probe passes of N+2 fill in behind.  Anything outside a pipelined frame first orders the main stream after the others
// (join_main), and the next pipelined frame orders the others after the main stream: results are
// those of the serial order bit for bit.
// A frame in three steps, for callers that put work of their own between the passes (the
// one-process-per-GPU runs all-gather the atlas slices after each probe pass, on the stream
// mdh_probe_stream names): begin -> probe passes -> end.  mdh_render is exactly
// begin, radiance, irradiance, end.
static hipStream_t frame_probe_stream(const mdh_renderer *r) { return r->frame_pipelined ? r->probe_stream : r->stream; }
extern "C" int32_t mdh_frame_begin(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is already open");
   if (r->opt_rank >= r->opt_world) return seterr(MDH_E_STATE, "MDH_OPT_RANK is not below MDH_OPT_WORLD");
   r->frame_pipelined = r->opt_overlap && r->stream == r->own_stream; // (modes 1 and 2 have no probe passes: their screen passes still alternate streams)
   // an edited scene goes up on the stream that uses it first; frames in flight keep the table buffers they were launched with
   int rc = ensure_committed(r, r->frame_pipelined && r->opt_mode == 0 ? r->probe_stream : nullptr);
   if (rc != MDH_OK) return rc;
   if (!r->frame_pipelined) {
      if ((rc = join_main(r)) != MDH_OK) return rc;
      r->main_dirty = true;
      r->frame_cur = r->last;
   } else {
      // modes 1 and 2 run no probe passes: the atlas sets stay as they are (their screen passes still alternate)
      const int cur = r->opt_mode == 0 ? (r->last + 1) % mdh_renderer::NSETS : r->last;
      if (r->main_dirty) { // the other streams have to see everything that went to the main stream meanwhile
         if ((rc = join_main(r)) != MDH_OK) return rc;
         HIP_TRY(hipEventRecord(r->ev_join.ev, r->stream));
         HIP_TRY(hipStreamWaitEvent(r->probe_stream, r->ev_join.ev, 0));
         HIP_TRY(hipStreamWaitEvent(r->alt_stream, r->ev_join.ev, 0));
         if (r->vol_stream) HIP_TRY(hipStreamWaitEvent(r->vol_stream, r->ev_join.ev, 0)); // (the volumetric passes of pipelined frames: frame_end_passes)
         r->main_dirty = false;
      } else if (r->opt_mode == 0 && r->ev_screen_valid[cur]) { // the last screen pass that read atlas set cur
         HIP_TRY(hipStreamWaitEvent(r->probe_stream, r->ev_screen[cur].ev, 0));
         if (r->vol_stream) HIP_TRY(hipStreamWaitEvent(r->vol_stream, r->ev_screen[cur].ev, 0)); // (it read the froxels of set cur as well)
      }
      r->frame_cur = cur;
   }
   r->in_frame = true;
   // MDH_OPT_PROBE_SETTLE: the slots that have arrived are read (no wait), and the frame's probe passes are left out when the
   // atlases have stopped changing -- the sets rotate, the events are recorded and every other pass runs as ever
   r->frame_probe_seq = 0;
   (void)r->settle.frame_begin(settle_eligible(r), r->frame_pipelined ? 1 : 0);
   return MDH_OK;
}
// a pass of an open frame failed: close the frame and make the next one re-join every stream (the work already
// enqueued on the probe stream is ordered against nothing else)
static int abandon_frame(mdh_renderer *r, int rc)
{
   r->in_frame = false;
   r->main_dirty = true;
   r->settle.reset();
   if (r->probe_stream) (void)hipStreamSynchronize(r->probe_stream);
   if (r->vol_stream) (void)hipStreamSynchronize(r->vol_stream);
   return rc;
}
extern "C" int32_t mdh_frame_probe_pass(mdh_renderer *r, int32_t pass)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!r->in_frame) return seterr(MDH_E_STATE, "no open frame");
   if (pass != MDH_PASS_RADIANCE && pass != MDH_PASS_IRRADIANCE) return seterr(MDH_E_INVALID, "not a probe pass");
   if (r->opt_mode != 0) return MDH_OK; // modes 1 and 2 draw without probes (renderers.adb:302-321 runs them anyway; nothing reads them)
   if (r->settle.skip_pass()) { // the pass would store the bits its set already holds (all sets hold them): not launched
      ++r->settle_skipped;
      if (r->opt_timing) { // (mdh_pass_time counts the passes of frames, run or settled: this one's time is what lies between its two events)
         HIP_TRY(hipSetDevice(r->device));
         hipEvent_t e0 = get_event(r), e1 = get_event(r);
         if (!e0 || !e1) return seterr(MDH_E_DEVICE, "hipEventCreate failed");
         HIP_TRY(hipEventRecord(e0, frame_probe_stream(r)));
         HIP_TRY(hipEventRecord(e1, frame_probe_stream(r)));
         r->pending.push_back({pass, e0, e1});
      }
      return MDH_OK;
   }
   if (pass == MDH_PASS_RADIANCE) {
      if (r->frame_probe_seq == 0) r->frame_probe_seq = 1;
      else { r->frame_probe_seq = -1; r->settle.untracked_pass(); }
   }
   return run_pass(r, pass, frame_probe_stream(r), r->last, r->frame_cur);
}
static int frame_end_passes(mdh_renderer *r);
extern "C" int32_t mdh_frame_end(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!r->in_frame) return seterr(MDH_E_STATE, "no open frame");
   r->in_frame = false;
   r->in_frame_passes = true;
   const int rc = frame_end_passes(r);
   r->in_frame_passes = false;
   return rc == MDH_OK ? bound_timing(r) : abandon_frame(r, rc);
}
static int frame_end_passes(mdh_renderer *r)
{
   int rc;
   const int cur = r->frame_cur;
   if (!r->frame_pipelined) {
      if (r->opt_mode == 0 && r->vol.enabled) {
         r->fuse_scat_march = true; // (both passes follow each other: the first one's launch marches the second one's camera rays)
         rc = run_pass(r, MDH_PASS_VISIBILITY, r->stream, cur, cur);
         if (rc == MDH_OK) rc = run_pass(r, MDH_PASS_SCATTERING, r->stream, cur, cur);
         r->fuse_scat_march = false;
         if (rc != MDH_OK) return rc;
      }
      return run_pass(r, MDH_PASS_SCREEN, r->stream, cur, cur);
   }
   const bool dual = r->opt_overlap > 1;
   // (level 1: all screen passes on the main stream, after whatever the alternate stream still holds)
   if (!dual && r->alt_pending && (rc = join_main(r)) != MDH_OK) return rc;
   // framebuffer 1 is only ever written from the alternate stream and framebuffer 0 from the main stream, so
   // each buffer's writes are ordered by its stream; frames that cannot alternate draw on (main, 0)
   r->scr_parity = dual ? r->scr_parity ^ 1 : 0;
   hipStream_t screen_stream = r->scr_parity ? r->alt_stream : r->stream;
   const int fbix = r->scr_parity;
   if (r->opt_mode == 0 && r->vol.enabled) {
      // camera-only passes into this frame's set: on a stream of their own, beside this frame's probe
      // passes and the previous screen pass -- they are a few hundred wavefronts each and wait for nothing the probes make
      hipStream_t vs = r->vol_stream ? r->vol_stream : r->probe_stream;
      r->fuse_scat_march = true;
      rc = run_pass(r, MDH_PASS_VISIBILITY, vs, cur, cur);
      if (rc == MDH_OK) rc = run_pass(r, MDH_PASS_SCATTERING, vs, cur, cur);
      r->fuse_scat_march = false;
      if (rc != MDH_OK) return rc;
      if (vs != r->probe_stream) {
         HIP_TRY(hipEventRecord(r->ev_vol[cur].ev, vs));
         HIP_TRY(hipStreamWaitEvent(screen_stream, r->ev_vol[cur].ev, 0));
      }
   }
   HIP_TRY(hipEventRecord(r->ev_probe[cur].ev, r->probe_stream));
   HIP_TRY(hipStreamWaitEvent(screen_stream, r->ev_probe[cur].ev, 0));
   if ((rc = run_pass(r, MDH_PASS_SCREEN, screen_stream, cur, cur, fbix)) != MDH_OK) return rc;
   HIP_TRY(hipEventRecord(r->ev_screen[cur].ev, screen_stream));
   r->ev_screen_valid[cur] = true;
   r->last = cur;
   r->fb_last = fbix;
   if (screen_stream == r->alt_stream) r->alt_pending = true;
   return MDH_OK;
}
extern "C" int32_t mdh_render(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   int rc;
   if ((rc = mdh_frame_begin(r)) != MDH_OK) return rc;
   // (with a communicator: the exchanges of the sharded schedule between the probe passes, mdh_frame_exchange)
   if ((rc = mdh_frame_probe_pass(r, MDH_PASS_RADIANCE)) != MDH_OK || (rc = mdh_frame_exchange(r, MDH_TEX_RADIANCE)) != MDH_OK ||
       (rc = mdh_frame_probe_pass(r, MDH_PASS_IRRADIANCE)) != MDH_OK ||
       (!r->opt_irr_all && (rc = mdh_frame_exchange(r, MDH_TEX_IRRADIANCE)) != MDH_OK))
      return abandon_frame(r, rc);
   return mdh_frame_end(r);
}

// ------------------------------------------------------------------ one frame on N GPUs: the communicator
// One process per GPU; the processes' renderers join an RCCL communicator and mdh_render of every rank is then one
// frame of the sharded schedule (include/madarch_hip.h "one frame on the N GPUs of a node").  librccl is opened on
// first use: a process that already holds one (a PyTorch process: the wheel carries its own, same SONAME) gets that
// one, any other the system's.
struct RcclApi {
   decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
   decltype(&ncclCommInitRank) CommInitRank = nullptr;
   decltype(&ncclCommDestroy) CommDestroy = nullptr;
   decltype(&ncclCommAbort) CommAbort = nullptr;
   decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;
   decltype(&ncclAllGather) AllGather = nullptr;
   decltype(&ncclBroadcast) Broadcast = nullptr;
   decltype(&ncclAllReduce) AllReduce = nullptr;
   decltype(&ncclReduce) Reduce = nullptr;
   decltype(&ncclGroupStart) GroupStart = nullptr;
   decltype(&ncclGroupEnd) GroupEnd = nullptr;
   decltype(&ncclGetErrorString) GetErrorString = nullptr;
   bool ok = false;
};
static const RcclApi &rccl_api()
{
   static RcclApi api;
   static std::once_flag once;
   std::call_once(once, [] {
      void *h = nullptr;
      const char *env = getenv("MADARCH_HIP_RCCL_LIBRARY");
      if (env && *env) h = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
      for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
         if (!h) h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (!h) return;
#define MDH_RCCL_SYM(field, sym) api.field = (decltype(api.field))dlsym(h, #sym)
      MDH_RCCL_SYM(GetUniqueId, ncclGetUniqueId); MDH_RCCL_SYM(CommInitRank, ncclCommInitRank); MDH_RCCL_SYM(CommDestroy, ncclCommDestroy);
      MDH_RCCL_SYM(CommAbort, ncclCommAbort); MDH_RCCL_SYM(CommGetAsyncError, ncclCommGetAsyncError); MDH_RCCL_SYM(AllGather, ncclAllGather);
      MDH_RCCL_SYM(Broadcast, ncclBroadcast); MDH_RCCL_SYM(AllReduce, ncclAllReduce); MDH_RCCL_SYM(Reduce, ncclReduce);
      MDH_RCCL_SYM(GroupStart, ncclGroupStart); MDH_RCCL_SYM(GroupEnd, ncclGroupEnd); MDH_RCCL_SYM(GetErrorString, ncclGetErrorString);
#undef MDH_RCCL_SYM
      api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.CommAbort && api.CommGetAsyncError && api.AllGather && api.Broadcast &&
               api.AllReduce && api.Reduce && api.GroupStart && api.GroupEnd && api.GetErrorString;
   });
   return api;
}
#define RCCL_TRY(expr)                                                                                             \
   do {                                                                                                            \
      ncclResult_t e_ = (expr);                                                                                    \
      if (e_ != ncclSuccess) {                                                                                     \
         snprintf(g_err, sizeof g_err, "%s failed: %s (%s:%d)", #expr, rccl_api().GetErrorString(e_), __FILE__, __LINE__); \
         return MDH_E_COMM;                                                                                        \
      }                                                                                                            \
   } while (0)
static int rccl_api_destroy(ncclComm_t c) { return rccl_api().ok && rccl_api().CommDestroy(c) == ncclSuccess ? MDH_OK : MDH_E_COMM; }
static int rccl_ready()
{
   return rccl_api().ok ? MDH_OK : seterr(MDH_E_COMM, "librccl.so.1 cannot be loaded (or lacks a symbol): no communicator; MADARCH_HIP_RCCL_LIBRARY names another file");
}

// ------------------------------------------------------------------ the peer exchange (include/madarch_hip.h)
// The sharded frame's exchange as device-to-device COPIES between processes of one node, ordered ON THE DEVICE.  What a rank
// shares: its radiance atlases (one hipIpcMemHandle per atlas set) and a block of FRAME NUMBERS in device memory, one per
// set.  Behind its radiance pass a rank stores the frame's number into its own block (k_peer_publish, on the probe stream);
// a rank that needs a peer's slice enqueues k_peer_wait -- one wavefront that polls the peer's number through the mapped
// handle until it has reached this frame's (system-scope loads; bounded: a peer that never arrives ends the wait with an
// error word in host memory instead of a hung queue) -- and behind it the copy of the slice out of the peer's atlas into
// its own (hipMemcpyAsync, device to device).  No host of any rank waits for anything: frames stay in flight, the screen
// pass of the previous frame runs beside the exchange.
// (Round 4 first used interprocess EVENTS for the ordering.  They work -- tests of 4 frames passed -- and fail: after some
// tens of frames hipStreamWaitEvent on a peer's event returned hipErrorInvalidValue, and HIP implements such waits as host
// callbacks.  hipStreamWaitValue32 enqueued before the peer's write stalled the peer's first HIP call in the probe
// (scripts/probes/ipc_probe.cpp, mode 2).  A polling wavefront needs nothing but memory.)
//
// Why reading a peer's slice is safe against the peer's NEXT radiance pass into the same set (three frames on): that
// pass comes behind the peer's irradiance pass of the frame before it, which waited for this rank's slice of that
// frame, which this rank's probe stream produced behind this copy.
struct PeerBlob { // MDH_PEER_BLOB_BYTES on the wire
   uint32_t magic, version;
   int32_t pid, device, nsets;
   uint64_t rad_bytes;
   hipIpcMemHandle_t rad[MDH_ATLAS_SETS];
   hipIpcMemHandle_t flags;
   uint64_t serial; // (of this export: a blob of an earlier session of the same process is refused)
};
static_assert(sizeof(PeerBlob) <= MDH_PEER_BLOB_BYTES, "MDH_PEER_BLOB_BYTES holds a rank's handles");
struct PeerState {
   bool active = false;
   int rank = 0, world = 1;
   bool exported = false;
   uint64_t serial = 0;
   unsigned *d_flags = nullptr;         // [MDH_ATLAS_SETS] the number of the last frame whose slice of set s is complete (device memory, shared)
   unsigned seq[MDH_ATLAS_SETS] = {0};
   unsigned *h_err = nullptr;           // pinned host word: a wait gave up
   struct Peer {
      void *rad[MDH_ATLAS_SETS] = {nullptr};
      unsigned *flags = nullptr;
   };
   std::vector<Peer> peers;
};
#ifndef MDH_PEER_SPIN_LIMIT
#define MDH_PEER_SPIN_LIMIT (1u << 23) // polls of k_peer_wait, about a microsecond each
#endif
__global__ void k_peer_publish(unsigned *flag, unsigned n)
{
   __hip_atomic_store(flag, n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_peer_wait(const unsigned *flag, unsigned n, unsigned *err)
{
   if (threadIdx.x != 0) return;
   for (unsigned spin = 0; spin < MDH_PEER_SPIN_LIMIT; ++spin) {
      // (frame numbers only grow; the difference as a signed number survives the counter's wrap)
      if ((int)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - n) >= 0) return;
      __builtin_amdgcn_s_sleep(32);
   }
   __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); // the copy behind this wait reads a stale slice: the host is told
}
static bool peer_active(const mdh_renderer *r) { return r->peer && r->peer->active; }
static void peer_close_peers(PeerState *p)
{
   for (auto &q : p->peers) {
      for (int s = 0; s < MDH_ATLAS_SETS; ++s) {
         if (q.rad[s]) (void)hipIpcCloseMemHandle(q.rad[s]);
         q.rad[s] = nullptr;
      }
      if (q.flags) (void)hipIpcCloseMemHandle(q.flags);
      q.flags = nullptr;
   }
   p->peers.clear();
}
// leave the exchange: the peers' handles are closed, this rank is rank 0 of 1 again (its own exports stay valid until mdh_destroy)
static void peer_leave(mdh_renderer *r)
{
   PeerState *p = r->peer;
   if (!p) return;
   peer_close_peers(p);
   if (p->active) {
      p->active = false;
      r->opt_rank = 0;
      r->opt_world = 1;
      r->rad_order.forget();
      r->fb_owner[0][0] = r->fb_owner[1][0] = -1;
   }
}
static void peer_abort(mdh_renderer *r) { (void)r; } // (nothing on the host waits: a wait on the device ends by itself, MDH_PEER_SPIN_LIMIT)
static void peer_drop(mdh_renderer *r)
{
   PeerState *p = r->peer;
   if (!p) return;
   peer_leave(r);
   if (p->d_flags) (void)hipFree(p->d_flags);
   if (p->h_err) (void)hipHostFree(p->h_err);
   delete p;
   r->peer = nullptr;
}
// a wait that gave up: reported once, by the next call that looks
static int peer_check(mdh_renderer *r)
{
   PeerState *p = r->peer;
   if (p && p->h_err && *(volatile unsigned *)p->h_err) {
      *(volatile unsigned *)p->h_err = 0u;
      return seterr(MDH_E_COMM, "a peer's radiance slice did not arrive in time (its frame number never came): the atlases of the frames since are not the whole frame's");
   }
   return MDH_OK;
}
extern "C" int32_t mdh_peer_export(mdh_renderer *r, uint8_t blob_out[MDH_PEER_BLOB_BYTES])
{
   settle_bump(r);
   if (!r || !blob_out) return seterr(MDH_E_INVALID, "bad argument");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   if (r->comm || peer_active(r)) return seterr(MDH_E_STATE, "the renderer has a communicator");
   HIP_TRY(hipSetDevice(r->device));
   { int dr = drain_streams(r); if (dr != MDH_OK) return dr; }
   if (!r->peer) r->peer = new PeerState();
   PeerState *p = r->peer;
   if (!p->d_flags) HIP_TRY(hipMalloc((void **)&p->d_flags, 4096));
   if (!p->h_err) { HIP_TRY(hipHostMalloc((void **)&p->h_err, 64, hipHostMallocDefault)); *p->h_err = 0u; }
   // a new session starts at frame 0: nobody must take an earlier session's numbers for this one's
   HIP_TRY(hipMemset(p->d_flags, 0, 4096));
   for (int s = 0; s < MDH_ATLAS_SETS; ++s) p->seq[s] = 0u;
   static uint64_t serial = 0;
   p->serial = ++serial;
   p->exported = true;
   PeerBlob b;
   memset(&b, 0, sizeof b);
   b.magic = 0x5045484du; b.version = 2;
   b.pid = (int32_t)getpid(); b.device = r->device; b.nsets = MDH_ATLAS_SETS;
   b.rad_bytes = atlas_bytes(r, MDH_TEX_RADIANCE);
   b.serial = p->serial;
   for (int s = 0; s < MDH_ATLAS_SETS; ++s) HIP_TRY(hipIpcGetMemHandle(&b.rad[s], r->d_rad2[s].ptr));
   HIP_TRY(hipIpcGetMemHandle(&b.flags, p->d_flags));
   memset(blob_out, 0, MDH_PEER_BLOB_BYTES);
   memcpy(blob_out, &b, sizeof b);
   return MDH_OK;
}
extern "C" int32_t mdh_peer_init(mdh_renderer *r, const uint8_t *blobs, int32_t rank, int32_t world)
{
   settle_bump(r);
   if (!r || !blobs) return seterr(MDH_E_INVALID, "bad argument");
   if (world < 1 || rank < 0 || rank >= world) return seterr(MDH_E_INVALID, "rank is not below world");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   if (r->comm || peer_active(r)) return seterr(MDH_E_STATE, "the renderer already has a communicator");
   PeerState *p = r->peer;
   if (!p || !p->exported) return seterr(MDH_E_STATE, "mdh_peer_export comes first");
   if (!r->opt_irr_all) return seterr(MDH_E_STATE, "the peer exchange moves radiance slices only: MDH_OPT_IRRADIANCE_ALL must be on");
   HIP_TRY(hipSetDevice(r->device));
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   HIP_TRY(hipStreamSynchronize(r->stream));
   p->peers.assign((size_t)world, PeerState::Peer());
   for (int q = 0; q < world; ++q) {
      PeerBlob b;
      memcpy(&b, blobs + (size_t)q * MDH_PEER_BLOB_BYTES, sizeof b);
      if (b.magic != 0x5045484du || b.version != 2 || b.nsets != MDH_ATLAS_SETS) { peer_close_peers(p); return seterr(MDH_E_INVALID, "not a peer blob of this library"); }
      if (b.rad_bytes != atlas_bytes(r, MDH_TEX_RADIANCE)) { peer_close_peers(p); return seterr(MDH_E_INVALID, "a peer's radiance atlas has another size: the ranks' probe settings and atlas formats must agree"); }
      if (q == rank) {
         if (b.pid != (int32_t)getpid() || b.serial != p->serial) { peer_close_peers(p); return seterr(MDH_E_INVALID, "the blob at this rank's place is not this renderer's latest export"); }
         continue;
      }
      if (b.pid == (int32_t)getpid()) { peer_close_peers(p); return seterr(MDH_E_INVALID, "two ranks of a peer exchange in one process: a process cannot open its own interprocess handles"); }
      PeerState::Peer &pe = p->peers[(size_t)q];
      for (int s = 0; s < MDH_ATLAS_SETS; ++s)
         if (hipIpcOpenMemHandle(&pe.rad[s], b.rad[s], hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); peer_close_peers(p); return seterr(MDH_E_COMM, "hipIpcOpenMemHandle failed on a peer's radiance atlas"); }
      if (hipIpcOpenMemHandle((void **)&pe.flags, b.flags, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); peer_close_peers(p); return seterr(MDH_E_COMM, "hipIpcOpenMemHandle failed on a peer's frame numbers"); }
   }
   *p->h_err = 0u;
   p->rank = rank; p->world = world;
   p->active = true;
   r->opt_rank = rank;
   r->opt_world = world;
   r->rad_order.forget();
   return MDH_OK;
}
static int peer_exchange(mdh_renderer *r, int tex)
{
   PeerState *p = r->peer;
   if (tex != MDH_TEX_RADIANCE) return r->opt_irr_all ? MDH_OK : seterr(MDH_E_STATE, "the peer exchange moves radiance slices only: MDH_OPT_IRRADIANCE_ALL must be on");
   { int pc = peer_check(r); if (pc != MDH_OK) return pc; }
   hipStream_t st = frame_probe_stream(r);
   const int s = r->frame_cur;
   const size_t per = (size_t)r->probes.radiance_resolution * r->probes.radiance_resolution * texel_bytes(r);
   const long long P = probe_total(r), world = p->world;
   hipEvent_t e0 = nullptr, e1 = nullptr;
   if (r->opt_timing) {
      e0 = get_event(r);
      e1 = get_event(r);
      if (!e0 || !e1) return seterr(MDH_E_DEVICE, "hipEventCreate failed");
      HIP_TRY(hipEventRecord(e0, st));
   }
   // my slice of set s is complete behind everything the probe stream holds: its frame number says so
   const unsigned n = ++p->seq[s];
   hipLaunchKernelGGL(k_peer_publish, dim3(1), dim3(1), 0, st, p->d_flags + s, n);
   HIP_TRY(hipGetLastError());
   char *mine = (char *)r->d_rad2[s].ptr;
   for (long long k = 1; k < world; ++k) { // (peers in a rotated order: the ranks do not all read the same peer at once)
      const long long q = (p->rank + k) % world;
      const long long b = P * q / world, e = P * (q + 1) / world; // own_probes () of rank q
      if (e <= b) continue;
      PeerState::Peer &pe = p->peers[(size_t)q];
      hipLaunchKernelGGL(k_peer_wait, dim3(1), dim3(64), 0, st, (const unsigned *)(pe.flags + s), n, p->h_err);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(mine + per * (size_t)b, (const char *)pe.rad[s] + per * (size_t)b, per * (size_t)(e - b), hipMemcpyDeviceToDevice, st));
   }
   if (r->opt_timing) {
      HIP_TRY(hipEventRecord(e1, st));
      r->pending.push_back({MDH_PASS_EXCHANGE, e0, e1});
   }
   return MDH_OK;
}

extern "C" int32_t mdh_comm_available(void) { return rccl_ready(); }
extern "C" int32_t mdh_comm_unique_id(uint8_t id_out[MDH_COMM_ID_BYTES])
{
   static_assert(sizeof(ncclUniqueId) == MDH_COMM_ID_BYTES, "MDH_COMM_ID_BYTES is the size of ncclUniqueId");
   if (!id_out) return seterr(MDH_E_INVALID, "bad argument");
   int rc = rccl_ready();
   if (rc != MDH_OK) return rc;
   ncclUniqueId id;
   RCCL_TRY(rccl_api().GetUniqueId(&id));
   memcpy(id_out, &id, sizeof id);
   return MDH_OK;
}
extern "C" int32_t mdh_comm_init(mdh_renderer *r, const uint8_t id_in[MDH_COMM_ID_BYTES], int32_t rank, int32_t world)
{
   settle_bump(r);
   if (!r || !id_in) return seterr(MDH_E_INVALID, "bad argument");
   if (world < 1 || rank < 0 || rank >= world) return seterr(MDH_E_INVALID, "rank is not below world");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   if (r->comm || peer_active(r)) return seterr(MDH_E_STATE, "the renderer already has a communicator");
   int rc = rccl_ready();
   if (rc != MDH_OK) return rc;
   HIP_TRY(hipSetDevice(r->device)); // (the communicator binds to the current device)
   if ((rc = join_main(r)) != MDH_OK) return rc;
   ncclUniqueId id;
   memcpy(&id, id_in, sizeof id);
   ncclComm_t comm = nullptr;
   RCCL_TRY(rccl_api().CommInitRank(&comm, world, id, rank));
   if (r->d_comm_scratch.grow(2) != hipSuccess) {
      (void)rccl_api().CommAbort(comm);
      return seterr(MDH_E_DEVICE, "hipMalloc failed");
   }
   r->comm = comm;
   r->opt_rank = rank;
   r->opt_world = world;
   r->rad_order.forget(); // (the stored ray order is of another slice)
   return MDH_OK;
}
// the renderer is rank 0 of 1 again (the handle itself is the caller's business)
static void comm_forget(mdh_renderer *r)
{
   settle_bump(r);
   r->comm = nullptr;
   r->comm_aborted = false;
   r->opt_rank = 0;
   r->opt_world = 1;
   r->rad_order.forget();
   r->fb_owner[0][0] = r->fb_owner[1][0] = -1; // (the framebuffers hold a rank's tiles: cleared before they are drawn whole)
}
static int comm_drop(mdh_renderer *r, bool abort)
{
   if (!r->comm) return MDH_OK;
   ncclComm_t c = r->comm;
   if (r->comm_aborted) { comm_forget(r); return MDH_OK; } // (a watchdog has aborted -- and thereby freed -- it already)
   if (abort) { comm_forget(r); RCCL_TRY(rccl_api().CommAbort(c)); return MDH_OK; }
   RCCL_TRY(rccl_api().CommDestroy(c)); // (a failed destroy keeps the handle: the caller may abort it)
   comm_forget(r);
   return MDH_OK;
}
// the owning thread's view of a watchdog's abort: the handle is gone
static int comm_gone(mdh_renderer *r)
{
   comm_forget(r);
   if (r->in_frame) { r->in_frame = false; r->main_dirty = true; }
   return seterr(MDH_E_COMM, "the communicator was aborted (mdh_comm_abort)");
}
struct CommBusy { // the owning thread is inside RCCL with r->comm
   mdh_renderer *r;
   explicit CommBusy(mdh_renderer *r_) : r(r_) { ++r->comm_busy; }
   ~CommBusy() { --r->comm_busy; }
};
extern "C" int32_t mdh_comm_destroy(mdh_renderer *r)
{
   settle_bump(r);
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   HIP_TRY(hipSetDevice(r->device));
   { int dr = drain_streams(r); if (dr != MDH_OK) return dr; } // collectives in flight end first
   if (r->peer) { peer_leave(r); return MDH_OK; }
   return comm_drop(r, false);
}
// what a watchdog of the host calls (from any thread) when a collective never returns: no wait for anything
extern "C" int32_t mdh_comm_abort(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   (void)hipSetDevice(r->device);
   if (r->peer && !r->comm) { peer_abort(r); if (r->in_frame) { r->in_frame = false; r->main_dirty = true; } return MDH_OK; }
   ncclComm_t c = r->comm;
   if (!c) return MDH_OK;
   if (r->comm_busy.load() > 0) { // another thread is inside a collective: abort only, that thread forgets the handle when its call returns
      if (!r->comm_aborted.exchange(true)) RCCL_TRY(rccl_api().CommAbort(c));
      return MDH_OK;
   }
   if (r->in_frame) { r->in_frame = false; r->main_dirty = true; }
   return comm_drop(r, true);
}
// an asynchronous failure of the communicator (a peer died, a transport error) surfaces here
static int comm_check(mdh_renderer *r)
{
   if (r->comm_aborted) return comm_gone(r);
   ncclResult_t ae = ncclSuccess;
   RCCL_TRY(rccl_api().CommGetAsyncError(r->comm, &ae));
   if (ae != ncclSuccess && ae != ncclInProgress) {
      snprintf(g_err, sizeof g_err, "the communicator reports an asynchronous error: %s", rccl_api().GetErrorString(ae));
      return MDH_E_COMM;
   }
   return MDH_OK;
}
// The exchange step of an open frame: every rank's slice of the atlas the open frame is producing goes to every other
// rank, in place (the atlases are probe-major: a slice is one byte range, and a rank's input is its slice where it
// lies in the output -- the in-place form of ncclAllGather, no staging copy), on the stream of the frame's probe
// passes: the screen pass of the previous frame keeps running beside it.  Probe counts the world size does not
// divide (the reference's default 36 probes on 8 ranks) go as one group of broadcasts, a slice each, which RCCL
// fuses into one launch as well.
extern "C" int32_t mdh_frame_exchange(mdh_renderer *r, int32_t tex)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (tex != MDH_TEX_RADIANCE && tex != MDH_TEX_IRRADIANCE) return seterr(MDH_E_INVALID, "not an atlas");
   if (!r->in_frame) return seterr(MDH_E_STATE, "no open frame");
   if (peer_active(r)) return r->opt_mode != 0 ? MDH_OK : peer_exchange(r, tex);
   if (!r->comm || r->opt_mode != 0) return MDH_OK;
   if (r->comm_aborted) return comm_gone(r);
   CommBusy busy(r);
   const RcclApi &n = rccl_api();
   hipStream_t st = frame_probe_stream(r);
   char *buf = (char *)(tex == MDH_TEX_RADIANCE ? r->d_rad2[r->frame_cur].ptr : r->d_irr2[r->frame_cur].ptr);
   const int res = tex == MDH_TEX_RADIANCE ? r->probes.radiance_resolution : r->probes.irradiance_resolution;
   const size_t per = (size_t)res * res * texel_bytes(r);
   const long long P = probe_total(r), world = r->opt_world;
   hipEvent_t e0 = nullptr, e1 = nullptr;
   if (r->opt_timing) {
      e0 = get_event(r);
      e1 = get_event(r);
      if (!e0 || !e1) return seterr(MDH_E_DEVICE, "hipEventCreate failed");
      HIP_TRY(hipEventRecord(e0, st));
   }
   static const bool force_bcast = [] { const char *e = getenv("MADARCH_HIP_EXCHANGE"); return e && strcmp(e, "broadcast") == 0; }();
   // (a failed collective hands its timing events back: ADVICE r03)
   auto failed = [&](const char *what, ncclResult_t e) {
      if (e0) r->free_events.push_back(e0);
      if (e1) r->free_events.push_back(e1);
      snprintf(g_err, sizeof g_err, "%s failed: %s", what, n.GetErrorString(e));
      return r->comm_aborted ? comm_gone(r) : (int)MDH_E_COMM;
   };
   if (P % world == 0 && !force_bcast) {
      const size_t count = per * (size_t)(P / world);
      const ncclResult_t ar = n.AllGather(buf + count * (size_t)r->opt_rank, buf, count, ncclChar, r->comm, st);
      if (ar != ncclSuccess) return failed("ncclAllGather", ar);
   } else {
      ncclResult_t gr = n.GroupStart();
      if (gr != ncclSuccess) return failed("ncclGroupStart", gr);
      for (long long q = 0; q < world; ++q) {
         const long long b = P * q / world, e = P * (q + 1) / world; // own_probes () of rank q
         if (e > b) {
            ncclResult_t br = n.Broadcast(buf + per * (size_t)b, buf + per * (size_t)b, per * (size_t)(e - b), ncclChar, (int)q, r->comm, st);
            if (br != ncclSuccess) { (void)n.GroupEnd(); return failed("ncclBroadcast", br); }
         }
      }
      if ((gr = n.GroupEnd()) != ncclSuccess) return failed("ncclGroupEnd", gr);
   }
   if (r->comm_aborted) { if (e0) r->free_events.push_back(e0); if (e1) r->free_events.push_back(e1); return comm_gone(r); }
   if (r->opt_timing) {
      HIP_TRY(hipEventRecord(e1, st));
      r->pending.push_back({MDH_PASS_EXCHANGE, e0, e1});
   }
   return MDH_OK;
}
extern "C" int32_t mdh_comm_barrier(mdh_renderer *r)
{
   settle_bump(r);
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   int rc = mdh_finish(r);
   if (rc == MDH_OK && peer_active(r)) return seterr(MDH_E_STATE, "the peer exchange has no collectives: the host's own channel is the barrier");
   if (rc != MDH_OK || !r->comm) return rc;
   if (r->comm_aborted) return comm_gone(r);
   CommBusy busy(r);
   HIP_TRY(hipMemsetAsync(r->d_comm_scratch.ptr, 0, sizeof(double), r->stream));
   RCCL_TRY(rccl_api().AllReduce(r->d_comm_scratch.ptr, r->d_comm_scratch.ptr, 1, ncclFloat64, ncclSum, r->comm, r->stream));
   HIP_TRY(hipStreamSynchronize(r->stream));
   return comm_check(r);
}
extern "C" int32_t mdh_comm_max_f64(mdh_renderer *r, double *value)
{
   settle_bump(r);
   if (!r || !value) return seterr(MDH_E_INVALID, "bad argument");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   if (peer_active(r)) return seterr(MDH_E_STATE, "the peer exchange has no collectives");
   if (!r->comm) return MDH_OK;
   if (r->comm_aborted) return comm_gone(r);
   CommBusy busy(r);
   HIP_TRY(hipSetDevice(r->device));
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   HIP_TRY(hipMemcpyAsync(r->d_comm_scratch.ptr + 1, value, sizeof(double), hipMemcpyHostToDevice, r->stream));
   RCCL_TRY(rccl_api().AllReduce(r->d_comm_scratch.ptr + 1, r->d_comm_scratch.ptr + 1, 1, ncclFloat64, ncclMax, r->comm, r->stream));
   HIP_TRY(hipMemcpyAsync(value, r->d_comm_scratch.ptr + 1, sizeof(double), hipMemcpyDeviceToHost, r->stream));
   HIP_TRY(hipStreamSynchronize(r->stream));
   return comm_check(r);
}
extern "C" int32_t mdh_comm_reduce_framebuffer(mdh_renderer *r, int32_t root)
{
   settle_bump(r);
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   if (peer_active(r)) return seterr(MDH_E_STATE, "the peer exchange has no collectives: read every rank's framebuffer and add them");
   if (!r->comm) return MDH_OK;
   if (root < 0 || root >= r->opt_world) return seterr(MDH_E_INVALID, "root is not a rank");
   if (r->comm_aborted) return comm_gone(r);
   CommBusy busy(r);
   HIP_TRY(hipSetDevice(r->device));
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   r->main_dirty = true;
   float4 *fb = r->d_fb2[r->fb_last].ptr;
   RCCL_TRY(rccl_api().Reduce(fb, fb, (size_t)r->W * r->H * 4, ncclFloat32, ncclSum, root, r->comm, r->stream));
   // the root's buffer now holds every rank's tiles: its next sharded screen pass clears it first
   if (r->opt_rank == root) r->fb_owner[r->fb_last][0] = -1;
   HIP_TRY(hipStreamSynchronize(r->stream));
   return comm_check(r);
}

// the stream the probe passes of the open frame run on (what a caller's collectives must be ordered on)
extern "C" int32_t mdh_probe_stream(mdh_renderer *r, void **stream)
{
   if (!r || !stream) return seterr(MDH_E_INVALID, "bad argument");
   if (r->in_frame) *stream = (void *)frame_probe_stream(r);
   else *stream = (void *)((r->opt_overlap && r->stream == r->own_stream) ? r->probe_stream : r->stream);
   return MDH_OK;
}
extern "C" int32_t mdh_finish(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   HIP_TRY(hipSetDevice(r->device));
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   HIP_TRY(hipStreamSynchronize(r->stream));
   { int pc = peer_check(r); if (pc != MDH_OK) return pc; }
   return resolve_timing(r);
}

extern "C" int32_t mdh_read_framebuffer(mdh_renderer *r, float *rgb_out)
{
   if (!r || !rgb_out) return seterr(MDH_E_INVALID, "bad argument");
   HIP_TRY(hipSetDevice(r->device));
   size_t px = (size_t)r->W * r->H;
   std::vector<float4> tmp(px);
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   HIP_TRY(hipMemcpyAsync(tmp.data(), r->d_fb2[r->fb_last].ptr, px * sizeof(float4), hipMemcpyDeviceToHost, r->stream));
   HIP_TRY(hipStreamSynchronize(r->stream));
   for (size_t i = 0; i < px; ++i) { rgb_out[3 * i] = tmp[i].x; rgb_out[3 * i + 1] = tmp[i].y; rgb_out[3 * i + 2] = tmp[i].z; }
   return MDH_OK;
}
// Swap_Buffers (renderers.adb:320): the last frame as the window's RGBA8 pixels in pinned host memory, without a
// host wait, so that frames stay in flight.
//  - MDH_OPT_WINDOW = 1: the screen pass has already stored them there itself (64 lanes x 4 bytes over PCIe beside
//    its float4 store); the swap only records an event behind it.
//  - otherwise: k_present converts the framebuffer on the stream that drew it and a copy stream takes the result
//    to the host beside the passes of the next frame.
extern "C" int32_t mdh_swap_buffers(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   HIP_TRY(hipSetDevice(r->device));
   const size_t px = (size_t)r->W * r->H;
   // framebuffer 1 is written from the alternate stream only; once the main stream has been ordered after it
   // (join_main) the main stream holds its latest contents as well
   const bool on_alt = r->fb_last == 1 && r->alt_pending;
   hipStream_t st = on_alt ? r->alt_stream : r->stream;
   if (r->opt_window && r->win_valid) {
      const int slot = (int)((r->win_passes - 1) % mdh_renderer::WIN_RING);
      HIP_TRY(r->ev_win[slot].create());
      HIP_TRY(hipEventRecord(r->ev_win[slot].ev, st));
      r->front_ptr = (const unsigned char *)r->h_win[slot].ptr;
      r->front_ev = r->ev_win[slot].ev;
      r->swaps += 1;
      return MDH_OK;
   }
   const int slot = (int)(r->swaps % mdh_renderer::FRONT_RING);
   if (!r->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&r->copy_stream, hipStreamNonBlocking));
   HIP_TRY(r->ev_packed.create());
   HIP_TRY(r->d_front[slot].grow(px));
   HIP_TRY(r->h_front[slot].grow(px * 4));
   if (!r->ev_front[slot].ev) HIP_TRY(r->ev_front[slot].create());
   else HIP_TRY(hipStreamWaitEvent(st, r->ev_front[slot].ev, 0)); // the copy that read this slot's device buffer three swaps ago
   hipLaunchKernelGGL(k_present, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, r->d_fb2[r->fb_last].ptr, r->d_front[slot].ptr, (int)px);
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipEventRecord(r->ev_packed.ev, st));
   HIP_TRY(hipStreamWaitEvent(r->copy_stream, r->ev_packed.ev, 0));
   HIP_TRY(hipMemcpyAsync(r->h_front[slot].ptr, r->d_front[slot].ptr, px * 4, hipMemcpyDeviceToHost, r->copy_stream));
   HIP_TRY(hipEventRecord(r->ev_front[slot].ev, r->copy_stream));
   // framebuffer 1 read from the main stream: its next writer (the alternate stream) has to come after this
   if (r->fb_last == 1 && !on_alt) r->main_dirty = true;
   r->front_ptr = r->h_front[slot].ptr;
   r->front_ev = r->ev_front[slot].ev;
   r->swaps += 1;
   return MDH_OK;
}
extern "C" int32_t mdh_front_buffer(mdh_renderer *r, const uint8_t **rgba, int64_t *swap_count)
{
   if (!r || !rgba) return seterr(MDH_E_INVALID, "bad argument");
   if (r->swaps == 0) return seterr(MDH_E_STATE, "no mdh_swap_buffers yet");
   HIP_TRY(hipSetDevice(r->device));
   HIP_TRY(hipEventSynchronize(r->front_ev));
   *rgba = r->front_ptr;
   if (swap_count) *swap_count = r->swaps;
   return MDH_OK;
}
extern "C" int32_t mdh_read_gbuffer(mdh_renderer *r, int32_t *index_out, float *t_out, int32_t *steps_out)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   HIP_TRY(hipSetDevice(r->device));
   size_t n = (size_t)r->W * r->H * 4;
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   if (index_out) HIP_TRY(hipMemcpyAsync(index_out, r->d_gb2[r->fb_last][0].ptr, n, hipMemcpyDeviceToHost, r->stream));
   if (t_out) HIP_TRY(hipMemcpyAsync(t_out, r->d_gb2[r->fb_last][1].ptr, n, hipMemcpyDeviceToHost, r->stream));
   if (steps_out) HIP_TRY(hipMemcpyAsync(steps_out, r->d_gb2[r->fb_last][2].ptr, n, hipMemcpyDeviceToHost, r->stream));
   HIP_TRY(hipStreamSynchronize(r->stream));
   return MDH_OK;
}

// The atlas set and the stream reads, writes and device pointers refer to: inside an open frame the
// set that frame is producing, on the stream its probe passes run on; otherwise the last frame's
// set on the main stream.
static int atlas_set(const mdh_renderer *r) { return r->in_frame ? r->frame_cur : r->last; }
static hipStream_t atlas_stream(const mdh_renderer *r) { return r->in_frame ? frame_probe_stream(r) : r->stream; }
// host copies of the probe-major atlases as float RGB per texel
// (texels [first, first + n) of the probe-major atlas; n = 0: all of it)
static int atlas_to_host(mdh_renderer *r, int tex, std::vector<float> &rgb, size_t first = 0, size_t n = 0)
{
   int res = tex == MDH_TEX_RADIANCE ? r->probes.radiance_resolution : r->probes.irradiance_resolution;
   if (n == 0 && first == 0) n = (size_t)probe_total(r) * res * res;
   const char *src = (const char *)(tex == MDH_TEX_RADIANCE ? r->d_rad2[atlas_set(r)].ptr : r->d_irr2[atlas_set(r)].ptr) + first * texel_bytes(r);
   if (n == 0) { rgb.clear(); return MDH_OK; }
   hipStream_t st = atlas_stream(r);
   if (!r->in_frame) { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   rgb.resize(n * 3);
   if (r->opt_atlas == 0) {
      std::vector<uchar4> tmp(n);
      HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (size_t i = 0; i < n; ++i) { rgb[3 * i] = (float)tmp[i].x / 255.0f; rgb[3 * i + 1] = (float)tmp[i].y / 255.0f; rgb[3 * i + 2] = (float)tmp[i].z / 255.0f; }
   } else {
      std::vector<float4> tmp(n);
      HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * 16, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (size_t i = 0; i < n; ++i) { rgb[3 * i] = tmp[i].x; rgb[3 * i + 1] = tmp[i].y; rgb[3 * i + 2] = tmp[i].z; }
   }
   return MDH_OK;
}
static float unorm8_host(float x)
{
   if (x != x) return 0.0f;
   float c = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
   return rintf(c * 255.0f);
}
// upload texels [first, first + n) of a probe-major atlas from float RGB
static int atlas_from_host(mdh_renderer *r, int tex, size_t first, size_t n, const float *rgb)
{
   void *dst = tex == MDH_TEX_RADIANCE ? r->d_rad2[atlas_set(r)].ptr : r->d_irr2[atlas_set(r)].ptr;
   hipStream_t st = atlas_stream(r);
   if (!r->in_frame) {
      int jr = join_main(r);
      if (jr != MDH_OK) return jr;
      r->main_dirty = true;
   }
   if (r->opt_atlas == 0) {
      std::vector<uchar4> tmp(n);
      for (size_t i = 0; i < n; ++i) {
         tmp[i].x = (unsigned char)unorm8_host(rgb[3 * i]); tmp[i].y = (unsigned char)unorm8_host(rgb[3 * i + 1]);
         tmp[i].z = (unsigned char)unorm8_host(rgb[3 * i + 2]); tmp[i].w = 255;
      }
      HIP_TRY(hipMemcpyAsync((uchar4 *)dst + first, tmp.data(), n * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
   } else {
      std::vector<float4> tmp(n);
      for (size_t i = 0; i < n; ++i) {
         float a = rgb[3 * i], b = rgb[3 * i + 1], c = rgb[3 * i + 2];
         tmp[i] = mk4(a != a ? 0.0f : a, b != b ? 0.0f : b, c != c ? 0.0f : c, 1.0f);
      }
      HIP_TRY(hipMemcpyAsync((float4 *)dst + first, tmp.data(), n * 16, hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
   }
   return MDH_OK;
}

extern "C" int32_t mdh_read_texture(mdh_renderer *r, int32_t tex, float *out, int32_t *w, int32_t *h, int32_t *c)
{
   if (r && tex > MDH_TEX_RADIANCE_MIP0 && tex <= MDH_TEX_RADIANCE_MIP0 + 15) { // level l of the radiance atlas, built now from the current atlas
      const int l = tex - MDH_TEX_RADIANCE_MIP0, res = r->probes.radiance_resolution >> l, pcx = r->probes.probe_count[0];
      if (!r->opt_mips || res < 1) return seterr(MDH_E_INVALID, "no such level (MDH_OPT_RADIANCE_MIPS)");
      HIP_TRY(hipSetDevice(r->device));
      { int jr = join_main(r); if (jr != MDH_OK) return jr; }
      const int set = atlas_set(r), W = res * pcx, H = res * r->probes.probe_count[1];
      if (out) {
         int rc = build_rad_mips(r, set, r->stream);
         if (rc != MDH_OK) return rc;
         size_t off = 0;
         for (int k = 1; k < l; ++k) off += (size_t)probe_total(r) * (r->probes.radiance_resolution >> k) * (r->probes.radiance_resolution >> k);
         const size_t n = (size_t)probe_total(r) * res * res;
         std::vector<float> rgb(n * 3);
         const char *src = (const char *)r->d_rad_mips[set].ptr + off * texel_bytes(r);
         if (r->opt_atlas == 0) {
            std::vector<uchar4> tmp(n);
            HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * 4, hipMemcpyDeviceToHost, r->stream));
            HIP_TRY(hipStreamSynchronize(r->stream));
            for (size_t i = 0; i < n; ++i) { rgb[3 * i] = (float)tmp[i].x / 255.0f; rgb[3 * i + 1] = (float)tmp[i].y / 255.0f; rgb[3 * i + 2] = (float)tmp[i].z / 255.0f; }
         } else {
            std::vector<float4> tmp(n);
            HIP_TRY(hipMemcpyAsync(tmp.data(), src, n * 16, hipMemcpyDeviceToHost, r->stream));
            HIP_TRY(hipStreamSynchronize(r->stream));
            for (size_t i = 0; i < n; ++i) { rgb[3 * i] = tmp[i].x; rgb[3 * i + 1] = tmp[i].y; rgb[3 * i + 2] = tmp[i].z; }
         }
         for (int Y = 0; Y < H; ++Y)
            for (int X = 0; X < W; ++X) {
               const int tx = X / res, ty = Y / res;
               const size_t idx = ((size_t)(ty * pcx + tx) * res + (Y - ty * res)) * res + (X - tx * res);
               memcpy(out + ((size_t)Y * W + X) * 3, &rgb[idx * 3], 12);
            }
      }
      if (w) *w = W;
      if (h) *h = H;
      if (c) *c = 3;
      return MDH_OK;
   }
   if (!r || tex < 0 || tex > 3) return seterr(MDH_E_INVALID, "bad argument");
   HIP_TRY(hipSetDevice(r->device));
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   int W, H, C;
   if (tex == MDH_TEX_RADIANCE || tex == MDH_TEX_IRRADIANCE) {
      int res = tex == MDH_TEX_RADIANCE ? r->probes.radiance_resolution : r->probes.irradiance_resolution;
      W = res * r->probes.probe_count[0]; H = res * r->probes.probe_count[1]; C = 3;
      if (out) {
         std::vector<float> rgb;
         int rc = atlas_to_host(r, tex, rgb);
         if (rc != MDH_OK) return rc;
         int pcx = r->probes.probe_count[0];
         for (int Y = 0; Y < H; ++Y)
            for (int X = 0; X < W; ++X) {
               int tx = X / res, ty = Y / res;
               size_t idx = ((size_t)(ty * pcx + tx) * res + (Y - ty * res)) * res + (X - tx * res);
               memcpy(out + ((size_t)Y * W + X) * 3, &rgb[idx * 3], 12);
            }
      }
   } else if (tex == MDH_TEX_VISIBILITY) {
      W = r->vol.visibility_resolution[0]; H = r->vol.visibility_resolution[1] * r->vol.visibility_resolution[2]; C = 3;
      if (out) { HIP_TRY(hipMemcpyAsync(out, r->d_vis2[atlas_set(r)].ptr, (size_t)W * H * 12, hipMemcpyDeviceToHost, r->stream)); HIP_TRY(hipStreamSynchronize(r->stream)); }
   } else {
      W = r->vol.scattering_resolution[0]; H = r->vol.scattering_resolution[1]; C = 4;
      if (out) { HIP_TRY(hipMemcpyAsync(out, r->d_scat2[atlas_set(r)].ptr, (size_t)W * H * 16, hipMemcpyDeviceToHost, r->stream)); HIP_TRY(hipStreamSynchronize(r->stream)); }
   }
   if (w) *w = W;
   if (h) *h = H;
   if (c) *c = C;
   return MDH_OK;
}
extern "C" int32_t mdh_write_texture(mdh_renderer *r, int32_t tex, const float *in, int32_t w, int32_t h, int32_t c)
{
   settle_bump(r);
   if (!r || tex < 0 || tex > 3 || !in) return seterr(MDH_E_INVALID, "bad argument");
   HIP_TRY(hipSetDevice(r->device));
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   r->main_dirty = true;
   int W, H, C;
   int rc = mdh_read_texture(r, tex, nullptr, &W, &H, &C);
   if (rc != MDH_OK) return rc;
   if (w != W || h != H || c != C) return seterr(MDH_E_INVALID, "texture shape mismatch");
   if (tex == MDH_TEX_RADIANCE || tex == MDH_TEX_IRRADIANCE) {
      int res = tex == MDH_TEX_RADIANCE ? r->probes.radiance_resolution : r->probes.irradiance_resolution;
      int pcx = r->probes.probe_count[0];
      std::vector<float> rgb((size_t)W * H * 3);
      for (int Y = 0; Y < H; ++Y)
         for (int X = 0; X < W; ++X) {
            int tx = X / res, ty = Y / res;
            size_t idx = ((size_t)(ty * pcx + tx) * res + (Y - ty * res)) * res + (X - tx * res);
            memcpy(&rgb[idx * 3], in + ((size_t)Y * W + X) * 3, 12);
         }
      return atlas_from_host(r, tex, 0, (size_t)W * H, rgb.data());
   }
   void *dst = tex == MDH_TEX_VISIBILITY ? (void *)r->d_vis2[atlas_set(r)].ptr : (void *)r->d_scat2[atlas_set(r)].ptr;
   HIP_TRY(hipMemcpyAsync(dst, in, (size_t)W * H * C * 4, hipMemcpyHostToDevice, r->stream));
   HIP_TRY(hipStreamSynchronize(r->stream));
   return MDH_OK;
}
extern "C" int32_t mdh_read_atlas_slice(mdh_renderer *r, int32_t tex, int32_t probe_begin, int32_t n_probes, float *out)
{
   if (!r || (tex != MDH_TEX_RADIANCE && tex != MDH_TEX_IRRADIANCE) || !out) return seterr(MDH_E_INVALID, "bad argument");
   if (probe_begin < 0 || n_probes < 0 || probe_begin + n_probes > probe_total(r)) return seterr(MDH_E_INDEX, "probe range");
   HIP_TRY(hipSetDevice(r->device));
   if (n_probes == 0) return MDH_OK;
   // the slice only: one device-to-host copy of its bytes (a sharded run's host exchange reads its own slice every frame)
   int res = tex == MDH_TEX_RADIANCE ? r->probes.radiance_resolution : r->probes.irradiance_resolution;
   std::vector<float> rgb;
   int rc = atlas_to_host(r, tex, rgb, (size_t)probe_begin * res * res, (size_t)n_probes * res * res);
   if (rc != MDH_OK) return rc;
   memcpy(out, rgb.data(), rgb.size() * sizeof(float));
   return MDH_OK;
}
extern "C" int32_t mdh_write_atlas_slice(mdh_renderer *r, int32_t tex, int32_t probe_begin, int32_t n_probes, const float *in)
{
   settle_bump(r);
   if (!r || (tex != MDH_TEX_RADIANCE && tex != MDH_TEX_IRRADIANCE) || !in) return seterr(MDH_E_INVALID, "bad argument");
   if (probe_begin < 0 || n_probes < 0 || probe_begin + n_probes > probe_total(r)) return seterr(MDH_E_INDEX, "probe range");
   HIP_TRY(hipSetDevice(r->device));
   int res = tex == MDH_TEX_RADIANCE ? r->probes.radiance_resolution : r->probes.irradiance_resolution;
   return atlas_from_host(r, tex, (size_t)probe_begin * res * res, (size_t)n_probes * res * res, in);
}
extern "C" int32_t mdh_atlas_device_ptr(mdh_renderer *r, int32_t tex, void **dptr, int64_t *total_bytes, int64_t *own_offset, int64_t *own_bytes)
{
   settle_bump(r);
   if (!r || (tex != MDH_TEX_RADIANCE && tex != MDH_TEX_IRRADIANCE)) return seterr(MDH_E_INVALID, "bad argument");
   if (r->opt_rank >= r->opt_world) return seterr(MDH_E_STATE, "MDH_OPT_RANK is not below MDH_OPT_WORLD");
   int res = tex == MDH_TEX_RADIANCE ? r->probes.radiance_resolution : r->probes.irradiance_resolution;
   int b, e;
   own_probes(r, &b, &e);
   int64_t per = (int64_t)res * res * (int64_t)texel_bytes(r);
   if (!r->in_frame) { // (inside a frame the caller works on the probe stream, which the frame orders)
      int jr = join_main(r);
      if (jr != MDH_OK) return jr;
      r->main_dirty = true; // the caller may write through the pointer
   }
   if (dptr) *dptr = tex == MDH_TEX_RADIANCE ? r->d_rad2[atlas_set(r)].ptr : r->d_irr2[atlas_set(r)].ptr;
   if (total_bytes) *total_bytes = (int64_t)atlas_bytes(r, tex);
   if (own_offset) *own_offset = per * b;
   if (own_bytes) *own_bytes = per * (e - b);
   return MDH_OK;
}
extern "C" int32_t mdh_stream(mdh_renderer *r, void **stream)
{
   if (!r || !stream) return seterr(MDH_E_INVALID, "bad argument");
   { int jr = join_main(r); if (jr != MDH_OK) return jr; } // the stream handed out is ordered after all work so far
   *stream = (void *)r->stream;
   return MDH_OK;
}
extern "C" int32_t mdh_set_stream(mdh_renderer *r, void *stream)
{
   settle_bump(r);
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   HIP_TRY(hipSetDevice(r->device));
   { int jr = join_main(r); if (jr != MDH_OK) return jr; }
   r->main_dirty = true;
   HIP_TRY(hipStreamSynchronize(r->stream));
   int rc = resolve_timing(r);
   if (rc != MDH_OK) return rc;
   if ((rc = sync_streams(r, SYNC_PROBE | SYNC_ALT | SYNC_QUERY | SYNC_VOL)) != MDH_OK) return rc;
   r->stream = stream ? (hipStream_t)stream : r->own_stream;
   // the new main stream has not waited for anything: uploads and earlier work are complete (synchronised above)
   r->table_fence.mark_all_seen();
   r->part_fence.mark_all_seen();
   return MDH_OK;
}

// the query stream, created by the first call that needs it (device_set: the caller has made the device current)
static int query_stream_get(mdh_renderer *r, hipStream_t *qs, bool device_set = false)
{
   if (!device_set) HIP_TRY(hipSetDevice(r->device));
   if (!r->query_stream) HIP_TRY(hipStreamCreateWithFlags(&r->query_stream, hipStreamNonBlocking));
   *qs = r->query_stream;
   return MDH_OK;
}
// Eval_Distance_To (renderers.adb:499-526), batched on the device
extern "C" int32_t mdh_eval_distance_to(mdh_renderer *r, int32_t n, const float *pts, const int32_t *kind_ixs, int32_t n_kinds,
                                        float *normals_out, float *dist_out)
{
   settle_bump(r);
   if (!r || !pts || !kind_ixs || !dist_out || n < 0 || n_kinds < 0 || n_kinds > MDH_MAX_KINDS) return seterr(MDH_E_INVALID, "bad argument");
   for (int i = 0; i < n_kinds; ++i)
      if (kind_ixs[i] < 0 || kind_ixs[i] >= r->npk) return seterr(MDH_E_INVALID, "bad kind index");
   if (n == 0) return MDH_OK;
   // on a stream of its own: the query waits for the table it reads, not for the frames in flight
   hipStream_t qs = nullptr;
   int rc = query_stream_get(r, &qs);
   if (rc != MDH_OK || (rc = ensure_committed(r, qs)) != MDH_OK) return rc;
   const size_t want = ((size_t)n < 256 ? 256 : (size_t)n) * 7; // 7 floats per query: point, normal, distance
   if (want > r->d_query.cap) {
      if (r->d_query.ptr) HIP_TRY(hipStreamSynchronize(qs));
      HIP_TRY(r->d_query.grow(want));
   }
   const size_t query_cap = r->d_query.cap / 7;
   float *d_pts = r->d_query.ptr, *d_n = d_pts + 3 * query_cap, *d_d = d_n + 3 * query_cap;
   HIP_TRY(hipMemcpyAsync(d_pts, pts, (size_t)n * 12, hipMemcpyHostToDevice, qs));
   EvalArgs a;
   a.n = n; a.n_kinds = n_kinds;
   for (int i = 0; i < MDH_MAX_KINDS; ++i) { a.kinds[i] = i < n_kinds ? kind_ixs[i] : 0; a.host_count[i] = r->host_count[i]; }
   a.pts = d_pts; a.normals = d_n; a.dist = d_d;
   if ((rc = table_acquire(r, qs)) != MDH_OK) return rc;
   if ((rc = launch_kernel_ptr(table_kernel(r, GK_k_eval_distance), dim3((n + 63) / 64), dim3(64), lds_bytes(r), qs, r->ks, a)) != MDH_OK) return rc;
   HIP_TRY(hipGetLastError());
   if ((rc = table_release(r, qs)) != MDH_OK) return rc;
   HIP_TRY(hipMemcpyAsync(dist_out, d_d, (size_t)n * 4, hipMemcpyDeviceToHost, qs));
   if (normals_out) HIP_TRY(hipMemcpyAsync(normals_out, d_n, (size_t)n * 12, hipMemcpyDeviceToHost, qs));
   HIP_TRY(hipStreamSynchronize(qs));
   return MDH_OK;
}

// ------------------------------------------------------------------ the query path
// What every query of the host's own rays and points shares ("The query path"): the query stream, the staging of
// host arrays in d_rays, the check of device arrays, and query_enqueue -- the one order in which a query's kernel is tied
// to the frames, to the caller's stream, to the scene's table and to the timing pair.  A family below is its checks, its
// args struct's filler and its kernel.
// d_rays: MDH_RAY_WORDS words a ray, each array at its slot's offset times the buffer's capacity in rays
#define MDH_RAY_WORDS 18
constexpr int RAY_SLOT_WORDS[] = {3, 3, 1, 1, 1, 1, 1, 3, 3, 1};
constexpr int ray_slot(int i) { int at = 0; for (int k = 0; k < i; ++k) at += RAY_SLOT_WORDS[k]; return at; }
enum RaySlot : int {
   SLOT_ORG = ray_slot(0), SLOT_DIR = ray_slot(1), SLOT_TMAX = ray_slot(2),                                   // what a ray brings
   SLOT_HIT = ray_slot(3), SLOT_INDEX = ray_slot(4), SLOT_T = ray_slot(5), SLOT_STEPS = ray_slot(6),          // its answers: t, or the visibility / shadow value
   SLOT_POS = ray_slot(7), SLOT_NORMAL = ray_slot(8), SLOT_RADIUS = ray_slot(9),                              // ... and a swept sphere's radius
   SLOT_VIEW = SLOT_TMAX, SLOT_MATERIAL = SLOT_T, // a point's view direction (3 words, over tmax, hit and index: a point has none) and material id
   SLOT_F = SLOT_TMAX, SLOT_LEN = SLOT_T,         // in-scattering: a point's distance along its ray, a ray's length
   SLOT_RGB = SLOT_POS,                           // a shaded or traced ray's, a point's colour
};
static_assert(SLOT_ORG == 0 && SLOT_DIR == 3 && SLOT_TMAX == 6 && SLOT_HIT == 7 && SLOT_INDEX == 8 && SLOT_T == 9 && SLOT_STEPS == 10 && SLOT_POS == 11 &&
              SLOT_NORMAL == 14 && SLOT_RADIUS == 17, "the places the kernels' arrays have always had");
static_assert(ray_slot(sizeof RAY_SLOT_WORDS / sizeof *RAY_SLOT_WORDS) == MDH_RAY_WORDS, "the slots fill a ray's words");
// n rays' room in d_rays on the query stream.  up and down copy `words` words a ray between a host array and a slot, skip a
// null array, and yield the slot's place; the first copy that fails is kept in err, and nothing is enqueued behind it.
struct RayStage {
   float *base = nullptr;
   size_t cap = 0, n = 0;
   hipStream_t qs = nullptr;
   hipError_t err = hipSuccess;
   template <class T = float> T *at(int slot) const { return (T *)(base + (size_t)slot * cap); }
   template <class T> T *up(int slot, const T *host, int words)
   {
      if (host && err == hipSuccess) err = hipMemcpyAsync(at(slot), host, n * words * 4, hipMemcpyHostToDevice, qs);
      return at<T>(slot);
   }
   template <class T> T *down(T *host, int slot, int words)
   {
      if (host && err == hipSuccess) err = hipMemcpyAsync(host, at(slot), n * words * 4, hipMemcpyDeviceToHost, qs);
      return at<T>(slot);
   }
};
// the only place that grows d_rays: at least 256 rays; whatever the query stream still does with the old memory is drained
static int rays_stage(mdh_renderer *r, size_t n, hipStream_t qs, RayStage &st)
{
   const size_t want = (n < 256 ? 256 : n) * MDH_RAY_WORDS;
   if (want > r->d_rays.cap) {
      if (r->d_rays.ptr) HIP_TRY(hipStreamSynchronize(qs));
      HIP_TRY(r->d_rays.grow(want));
   }
   st.base = r->d_rays.ptr; st.cap = r->d_rays.cap / MDH_RAY_WORDS; st.n = n; st.qs = qs;
   return MDH_OK;
}
// a host form's first steps behind its last refusal: the query stream, the committed scene, room for its n rays
static int host_query_begin(mdh_renderer *r, int32_t n, RayStage &st)
{
   hipStream_t qs = nullptr;
   int rc = query_stream_get(r, &qs);
   if (rc != MDH_OK || (rc = ensure_committed(r, qs)) != MDH_OK) return rc;
   return rays_stage(r, (size_t)n, qs, st);
}
// a device form's, behind ray_arrays_check
static int device_query_begin(mdh_renderer *r, hipStream_t *qs)
{
   const int rc = query_stream_get(r, qs, true);
   return rc != MDH_OK ? rc : ensure_committed(r, *qs);
}

// Arrays the device addresses: nothing is copied, and the rays are validated by the lanes that take them.  What the host can
// check -- and must, a pointer the device cannot address is a fault inside the kernel -- is where the arrays live.
struct RayArray { const void *p; size_t bytes; const char *what; };
// is [p, p + bytes) memory this renderer's device addresses?  Memory of the device itself, page-locked host memory or
// managed memory, as hipPointerGetAttributes knows it; pageable host memory is unregistered (or, to older runtimes, an
// invalid value: the sticky error is cleared).  Where the runtime names the allocation's range, the array has to end inside it.
static int ray_array_check(const mdh_renderer *r, const RayArray &a)
{
   if (!a.p) return MDH_OK; // (an optional output that was not asked for; required ones were looked at before)
   hipPointerAttribute_t at;
   memset(&at, 0, sizeof at);
   const hipError_t e = hipPointerGetAttributes(&at, a.p);
   if (e != hipSuccess) {
      (void)hipGetLastError();
      snprintf(g_err, sizeof g_err, "%s: not memory the device can address (%s)", a.what, hipGetErrorString(e));
      return MDH_E_INVALID;
   }
   const bool ok = (at.type == hipMemoryTypeDevice && at.device == r->device) || at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged;
   if (!ok) {
      snprintf(g_err, sizeof g_err, "%s: not memory the device can address (%s)", a.what, at.type == hipMemoryTypeDevice ? "another device's" : "pageable host memory");
      return MDH_E_INVALID;
   }
   if (at.type == hipMemoryTypeDevice) {
      hipDeviceptr_t base = nullptr;
      size_t size = 0;
      if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)a.p) != hipSuccess) (void)hipGetLastError(); // (no range known: the caller's word)
      else if ((const char *)a.p < (const char *)base || (size_t)((const char *)a.p - (const char *)base) + a.bytes > size) {
         snprintf(g_err, sizeof g_err, "%s: %zu bytes from this address end outside its allocation", a.what, a.bytes);
         return MDH_E_INVALID;
      }
   }
   return MDH_OK;
}
// the workgroups of `kernel` with `lds` bytes of dynamic LDS the device holds at once (0: the runtime does not say)
static long resident_groups(mdh_renderer *r, const void *kernel, size_t lds)
{
   auto it = r->resident.find({kernel, lds});
   if (it == r->resident.end()) {
      int per_cu = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, MDH_BLOCK, lds) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
      it = r->resident.insert({{kernel, lds}, per_cu}).first;
   }
   return (long)it->second * r->n_cus;
}
// every array of a device form (the device is made current for the look)
template <size_t N> static int ray_arrays_check(const mdh_renderer *r, const RayArray (&arrays)[N])
{
   HIP_TRY(hipSetDevice(r->device));
   for (const RayArray &ra : arrays) {
      const int rc = ray_array_check(r, ra);
      if (rc != MDH_OK) return rc;
   }
   return MDH_OK;
}
// the workgroups of a streamed query of n rays: no more than are resident, or than MDH_OPT_RAY_STREAM_GROUPS allows
static unsigned stream_groups(mdh_renderer *r, const void *kernel, size_t lds, int32_t n)
{
   long groups = ((long)n + MDH_BLOCK - 1) / MDH_BLOCK;
   if (kernel) { // (none: launch_kernel_ptr says so)
      const long resident = resident_groups(r, kernel, lds);
      if (resident > 0 && groups > resident) groups = resident;
   }
   if (r->opt_rq_groups > 0 && groups > r->opt_rq_groups) groups = r->opt_rq_groups;
   return (unsigned)groups;
}
// One query on the query stream qs.  `framed`: it reads what the frames write (an atlas set) or keeps a place among them, so
// it is tied to the main stream as a screen pass is by running there -- join_main, qs behind the main stream, and behind the
// kernel the main stream behind qs with main_dirty set, so that the next frame orders its probe, volumetric and alternate
// streams behind the query before any of them rewrites a set.  `caller`: the stream device arrays are ordered with, or qs
// itself (host arrays: the copies around this call are on qs).  `launch` enqueues the kernel, and nothing else: under
// MDH_OPT_TIMING the pair rq_e0 / rq_e1 around it is what mdh_ray_query_time reports.
template <typename Launch> static int query_enqueue(mdh_renderer *r, hipStream_t qs, hipStream_t caller, bool framed, Launch launch)
{
   int rc;
   if (framed) {
      if ((rc = join_main(r)) != MDH_OK) return rc;
      r->main_dirty = true;
   }
   const hipStream_t *main = framed ? &r->stream : nullptr;
   if (main || caller != qs) HIP_TRY(r->bridge.create());
   HIP_TRY(r->bridge.enter(qs, caller, main));
   if ((rc = table_acquire(r, qs)) != MDH_OK) return rc;
   const bool timed = r->opt_timing && (r->rq_e0 || (r->rq_e0 = get_event(r))) && (r->rq_e1 || (r->rq_e1 = get_event(r)));
   if (timed) HIP_TRY(hipEventRecord(r->rq_e0, qs));
   if ((rc = launch()) != MDH_OK) return rc;
   HIP_TRY(hipGetLastError());
   if (timed) HIP_TRY(hipEventRecord(r->rq_e1, qs));
   r->rq_timed = timed; // (pending for a device form: mdh_ray_query_wait or mdh_ray_query_time reads the pair)
   if ((rc = table_release(r, qs)) != MDH_OK) return rc;
   HIP_TRY(r->bridge.leave(qs, caller, main));
   return MDH_OK;
}
// ... of a kernel that takes the scene and `a`, a lane per ray; a variant nobody built is refused before anything is enqueued
template <typename... A> static int query_kernel(mdh_renderer *r, const void *kernel, unsigned blocks, size_t lds, hipStream_t qs, hipStream_t caller, bool framed, A... a)
{
   if (!kernel) return seterr(MDH_E_INVALID, "no kernel built for this variant");
   return query_enqueue(r, qs, caller, framed, [&] { return launch_kernel_ptr(kernel, dim3(blocks), dim3(MDH_BLOCK), lds, qs, r->ks, a...); });
}
static unsigned lane_blocks(int32_t n) { return (unsigned)(((size_t)n + MDH_BLOCK - 1) / MDH_BLOCK); }
// the scene's half of the bound that stands in for a stall guard (mdh_ray_stream.h: rs_shade_ray_valid has the ray's), for
// `who` ("shaded rays", "traced paths"); `probes`: the query reads the probe grid
static int scene_extent_check(const mdh_renderer *r, const char *who, bool probes)
{
   const char *what = nullptr;
   if (!rs_shade_extent_valid(r->max_dist)) what = "a max_dist of at most 1024";
   for (int k = 0; k < r->nlk && !what; ++k) {
      const Kind &kd = r->lk[k];
      int n = rd_i(r, kd.count_off);
      if (n > kd.max_count) n = kd.max_count;
      for (int i = 0; i < n; ++i)
         for (int c = 0; c < 3; ++c)
            if (!rs_shade_extent_valid(rd_f(r, kd.array_off + kd.stride * i + kd.f_a + 4 * c))) what = "every light within 1024 of the origin along every axis";
   }
   for (int c = 0; c < 3 && probes && !what; ++c)
      if (!rs_shade_extent_valid((float)(r->probes.grid_dimensions[c] - 1) * r->probes.grid_spacing[c])) what = "the probe grid's far corner within 1024 of the origin along every axis";
   if (!what) return MDH_OK;
   snprintf(g_err, sizeof g_err, "%s need %s", who, what);
   return MDH_E_STATE;
}
static int shade_scene_check(const mdh_renderer *r) { return scene_extent_check(r, "shaded rays", true); } // (rays and points alike)

// the host's wait for a query's results; under MDH_OPT_TIMING the kernel's own time is read off its two events
static int ray_query_wait(mdh_renderer *r)
{
   HIP_TRY(hipStreamSynchronize(r->query_stream));
   if (r->rq_timed) {
      float ms = 0.0f;
      HIP_TRY(hipEventElapsedTime(&ms, r->rq_e0, r->rq_e1));
      r->rq_ms = ms;
      r->rq_timed = false;
   }
   return MDH_OK;
}
extern "C" int32_t mdh_ray_query_time(mdh_renderer *r, double *kernel_ms)
{
   if (!r || !kernel_ms) return seterr(MDH_E_INVALID, "bad argument");
   if (r->rq_timed) { // a device query nobody has waited for yet: for its end event, not for the stream
      float ms = 0.0f;
      HIP_TRY(hipSetDevice(r->device));
      HIP_TRY(hipEventSynchronize(r->rq_e1));
      HIP_TRY(hipEventElapsedTime(&ms, r->rq_e0, r->rq_e1));
      r->rq_ms = ms;
      r->rq_timed = false;
   }
   *kernel_ms = r->rq_ms;
   return MDH_OK;
}
// the host's wait for every device query enqueued so far (callers that order their own stream need none)
extern "C" int32_t mdh_ray_query_wait(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!r->query_stream) return MDH_OK; // (no query yet)
   HIP_TRY(hipSetDevice(r->device));
   return ray_query_wait(r);
}

// ------------------------------------------------------------------ ray queries
// raycast, raycast_visibility and softshadows (raymarching.glsl:4-56) for n rays of the host's, on the query stream beside the
// frames in flight (k_ray_query, mdh_kernels.h).  They read the committed scene and edit nothing: no settle_bump, no counter
// of the replays' keys moves -- the probe-settle run, the radiance replay and the screen replay go on across them (pending
// edits are committed first, and have made their own marks).
static bool all_finite(const float *v, size_t n)
{
   bool ok = true;
   for (size_t i = 0; i < n; ++i) ok = ok && rs_finite(v[i]); // (mdh_ray_stream.h: the predicate the device-array queries apply per lane)
   return ok;
}
// the checks all three share, before anything is launched; tmax is null for mdh_raycast
static int ray_query_check(const mdh_renderer *r, int32_t n, const float *org, const float *dir, const float *tmax)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!org || !dir || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   if (!all_finite(org, 3 * (size_t)n) || !all_finite(dir, 3 * (size_t)n)) return seterr(MDH_E_INVALID, "a ray is not finite");
   if (tmax) {
      bool ok = true;
      for (int32_t i = 0; i < n; ++i) ok = ok && rs_tmax_valid(tmax[i], r->max_dist);
      if (!ok) return seterr(MDH_E_INVALID, "a ray's length is not finite or exceeds the scene's max_dist");
   }
   return MDH_OK;
}
// the family's args: the queries here, the device-array forms and the sweeps below all fill them in this one place
static RayQueryArgs ray_query_args(int32_t n, float tmin, float k, const float *org, const float *dir, const float *tmax, const float *radius, int *hit, int *index,
                                   float *t, int *steps, float *pos, float *normal, float *out)
{
   RayQueryArgs a;
   a.n = n; a.tmin = tmin; a.k = k;
   a.org = org; a.dir = dir; a.tmax = tmax; a.radius = radius;
   a.hit = hit; a.index = index; a.steps = steps;
   a.t = t; a.pos = pos; a.normal = normal;
   a.out = out;
   return a;
}
// ... with the answers' places in d_rays (no normal asked for: the kernel leaves primitive_info out)
static RayQueryArgs ray_query_staged(const RayStage &st, float tmin, float k, const float *org, const float *dir, const float *tmax, const float *radius, bool normals, float *out)
{
   return ray_query_args((int32_t)st.n, tmin, k, org, dir, tmax, radius, st.at<int>(SLOT_HIT), st.at<int>(SLOT_INDEX), st.at(SLOT_T), st.at<int>(SLOT_STEPS),
                         st.at(SLOT_POS), normals ? st.at(SLOT_NORMAL) : nullptr, out);
}
// a raycast's or a sweep's answers, from d_rays to the arrays the host asked for
static void ray_query_down(RayStage &st, int32_t *hit_out, int32_t *index_out, float *t_out, int32_t *steps_out, float *pos_out, float *normal_out)
{
   st.down(hit_out, SLOT_HIT, 1); st.down(index_out, SLOT_INDEX, 1); st.down(t_out, SLOT_T, 1); st.down(steps_out, SLOT_STEPS, 1);
   st.down(pos_out, SLOT_POS, 3); st.down(normal_out, SLOT_NORMAL, 3);
}
// enqueues the family's kernel for `a`: k_listed<.., what> (n_kinds > 0: the exact minimum over the kinds listed), k_ray_stream
// <.., what> (`streamed`: device arrays, lanes refilled as rays end) or k_ray_query<.., what>
static int ray_query_enqueue(mdh_renderer *r, int what, const RayQueryArgs &a, const int32_t *kind_ixs, int32_t n_kinds, bool streamed, hipStream_t qs, hipStream_t caller)
{
   const size_t lds = lds_bytes(r);
   const dim3 block(MDH_BLOCK);
   if (n_kinds > 0) {
      ListedArgs la;
      la.q = a; la.n_kinds = n_kinds;
      for (int i = 0; i < MDH_MAX_KINDS; ++i) { la.kinds[i] = i < n_kinds ? kind_ixs[i] : 0; la.host_count[i] = r->host_count[i]; }
      const void *kernel = table_kernel(r, GK_k_listed, what);
      return query_enqueue(r, qs, caller, false, [&] { return launch_kernel_ptr(kernel, dim3(lane_blocks(a.n)), block, lds, qs, r->ks, la); });
   }
   if (streamed) {
      const void *kernel = table_kernel(r, GK_k_ray_stream, what);
      const unsigned groups = stream_groups(r, kernel, lds, a.n);
      HIP_TRY(r->d_rq_next.grow(1)); // (created by the first streamed query)
      RayStreamArgs sa;
      sa.q = a; sa.next = r->d_rq_next.ptr; sa.refill = r->opt_rq_refill;
      HIP_TRY(hipMemsetAsync(r->d_rq_next.ptr, 0, sizeof(unsigned), qs));
      return query_enqueue(r, qs, caller, false, [&] { return launch_kernel_ptr(kernel, dim3(groups), block, lds, qs, r->ks, sa); });
   }
   const void *kernel = table_kernel(r, GK_k_ray_query, what);
   return query_enqueue(r, qs, caller, false, [&] { return launch_kernel_ptr(kernel, dim3(lane_blocks(a.n)), block, lds, qs, r->ks, a); });
}
// host arrays: uploads the rays, launches k_ray_query<.., what> and leaves the results in d_rays (a.out: beside t)
static int ray_query_run(mdh_renderer *r, int what, int32_t n, const float *org, const float *dir, const float *tmax, float tmin, float k, bool normals, RayStage &st)
{
   const int rc = host_query_begin(r, n, st);
   if (rc != MDH_OK) return rc;
   const float *d_org = st.up(SLOT_ORG, org, 3), *d_dir = st.up(SLOT_DIR, dir, 3), *d_tmax = st.up(SLOT_TMAX, tmax, 1);
   HIP_TRY(st.err);
   return ray_query_enqueue(r, what, ray_query_staged(st, tmin, k, d_org, d_dir, d_tmax, nullptr, normals, st.at(SLOT_T)), nullptr, 0, false, st.qs, st.qs);
}
// a scalar per ray (the visibility, the shadow value) back to the host
static int32_t ray_query_scalar(mdh_renderer *r, int what, int32_t n, const float *org, const float *dir, const float *tmax, float tmin, float k, float *out)
{
   RayStage st;
   const int rc = ray_query_run(r, what, n, org, dir, tmax, tmin, k, false, st);
   if (rc != MDH_OK) return rc;
   st.down(out, SLOT_T, 1);
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_raycast(mdh_renderer *r, int32_t n, const float *org, const float *dir, int32_t *hit_out, int32_t *index_out,
                               float *t_out, int32_t *steps_out, float *pos_out, float *normal_out)
{
   int rc = ray_query_check(r, n, org, dir, nullptr);
   if (rc != MDH_OK) return rc;
   if (!hit_out) return seterr(MDH_E_INVALID, "bad argument");
   if (n == 0) return MDH_OK;
   RayStage st;
   if ((rc = ray_query_run(r, MDH_RQ_RAYCAST, n, org, dir, nullptr, 0.0f, 0.0f, normal_out != nullptr, st)) != MDH_OK) return rc;
   ray_query_down(st, hit_out, index_out, t_out, steps_out, pos_out, normal_out);
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_raycast_visibility(mdh_renderer *r, int32_t n, const float *org, const float *dir, const float *tmax, float *vis_out)
{
   if (r && (!tmax || !vis_out)) return seterr(MDH_E_INVALID, "bad argument");
   const int rc = ray_query_check(r, n, org, dir, tmax);
   if (rc != MDH_OK || n == 0) return rc;
   return ray_query_scalar(r, MDH_RQ_VISIBILITY, n, org, dir, tmax, 0.0f, 0.0f, vis_out);
}
extern "C" int32_t mdh_softshadows(mdh_renderer *r, int32_t n, const float *org, const float *dir, float tmin, const float *tmax, float k, float *out)
{
   if (r && (!tmax || !out)) return seterr(MDH_E_INVALID, "bad argument");
   if (r && (!std::isfinite(tmin) || !std::isfinite(k) || tmin < 0.0f)) return seterr(MDH_E_INVALID, "min_dist is negative, or min_dist or k is not finite");
   const int rc = ray_query_check(r, n, org, dir, tmax);
   if (rc != MDH_OK || n == 0) return rc;
   return ray_query_scalar(r, MDH_RQ_SOFTSHADOW, n, org, dir, tmax, tmin, k, out);
}

// ------------------------------------------------------------------ ray queries on device arrays
// mdh_raycast_device, mdh_raycast_visibility_device, mdh_softshadows_device: the same three queries for arrays the device
// addresses, asynchronous and ordered with a stream of the caller's.  The kernel (k_ray_stream, mdh_kernels.h) still runs
// on the query stream, so that the scene's commit and the table's fences are used as they are; the bridge's events order it
// with the caller's stream (query_enqueue).  Nothing is copied and the host waits for nothing.
// where the arrays live, then the family's kernel between the caller's stream's events; `arrays`: every array of the call
template <size_t N>
static int ray_query_device(mdh_renderer *r, int what, const RayArray (&arrays)[N], const RayQueryArgs &a, const int32_t *kind_ixs, int32_t n_kinds, bool streamed, void *stream)
{
   int rc = ray_arrays_check(r, arrays);
   if (rc != MDH_OK || a.n == 0) return rc;
   hipStream_t qs = nullptr;
   if ((rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   return ray_query_enqueue(r, what, a, kind_ixs, n_kinds, streamed, qs, (hipStream_t)stream);
}
extern "C" int32_t mdh_raycast_device(mdh_renderer *r, int32_t n, const float *org, const float *dir, int32_t *hit_out, int32_t *index_out,
                                      float *t_out, int32_t *steps_out, float *pos_out, float *normal_out, void *stream)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!org || !dir || !hit_out || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   const size_t w = (size_t)n * 4;
   const RayArray arrays[] = {{org, 3 * w, "origins"}, {dir, 3 * w, "directions"}, {hit_out, w, "hit"}, {index_out, w, "index"}, {t_out, w, "t"},
                              {steps_out, w, "steps"}, {pos_out, 3 * w, "positions"}, {normal_out, 3 * w, "normals"}};
   const RayQueryArgs a = ray_query_args(n, 0.0f, 0.0f, org, dir, nullptr, nullptr, hit_out, index_out, t_out, steps_out, pos_out, normal_out, nullptr);
   return ray_query_device(r, MDH_RQ_RAYCAST, arrays, a, nullptr, 0, true, stream);
}
static int32_t ray_stream_scalar(mdh_renderer *r, int what, int32_t n, const float *org, const float *dir, float tmin, const float *tmax, float k, float *out, void *stream)
{
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   const size_t w = (size_t)n * 4;
   const RayArray arrays[] = {{org, 3 * w, "origins"}, {dir, 3 * w, "directions"}, {tmax, w, "tmax"}, {out, w, "results"}};
   const RayQueryArgs a = ray_query_args(n, tmin, k, org, dir, tmax, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out);
   return ray_query_device(r, what, arrays, a, nullptr, 0, true, stream);
}
extern "C" int32_t mdh_raycast_visibility_device(mdh_renderer *r, int32_t n, const float *org, const float *dir, const float *tmax, float *vis_out, void *stream)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!org || !dir || !tmax || !vis_out || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   return ray_stream_scalar(r, MDH_RQ_VISIBILITY, n, org, dir, 0.0f, tmax, 0.0f, vis_out, stream);
}
extern "C" int32_t mdh_softshadows_device(mdh_renderer *r, int32_t n, const float *org, const float *dir, float tmin, const float *tmax, float k, float *out, void *stream)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!org || !dir || !tmax || !out || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   if (!std::isfinite(tmin) || !std::isfinite(k) || tmin < 0.0f) return seterr(MDH_E_INVALID, "min_dist is negative, or min_dist or k is not finite");
   return ray_stream_scalar(r, MDH_RQ_SOFTSHADOW, n, org, dir, tmin, tmax, k, out, stream);
}

// ------------------------------------------------------------------ sweeping a host's spheres
// mdh_spherecast, mdh_contacts and their _device forms: a sphere swept along each ray to its first contact, and one evaluation
// at each centre, against the scene as every pass sees it (n_kinds = 0: k_ray_query / k_ray_stream with MDH_RQ_SPHERECAST,
// k_ray_query with MDH_RQ_CONTACT) or against the exact minimum over the kinds listed (k_listed, mdh_kernels.h).  The contract
// is the ray queries', through the query path: pending edits seen, nothing edited and no settle_bump.  MDH_OPT_ADA_EVAL_DIV
// is not consulted: a march needs a distance.
static int sweep_kinds_check(const mdh_renderer *r, const int32_t *kind_ixs, int32_t n_kinds)
{
   if (n_kinds < 0 || n_kinds > MDH_MAX_KINDS || (n_kinds > 0 && !kind_ixs)) return seterr(MDH_E_INVALID, "bad argument");
   for (int i = 0; i < n_kinds; ++i)
      if (kind_ixs[i] < 0 || kind_ixs[i] >= r->npk) return seterr(MDH_E_INVALID, "bad kind index");
   return MDH_OK;
}
// what the host can say of host arrays before anything is launched (dir and tmax: null for contacts)
static int sweep_host_check(const mdh_renderer *r, int32_t n, const float *org, const float *dir, const float *radius, const float *tmax)
{
   if (!all_finite(org, 3 * (size_t)n) || (dir && !all_finite(dir, 3 * (size_t)n))) return seterr(MDH_E_INVALID, dir ? "a ray is not finite" : "a centre is not finite");
   bool ok = true;
   if (radius) for (int32_t i = 0; i < n; ++i) ok = ok && rs_sweep_radius_valid(radius[i], r->max_dist);
   if (!ok) return seterr(MDH_E_INVALID, "a radius is not finite, negative or exceeds the scene's max_dist");
   if (tmax) for (int32_t i = 0; i < n; ++i) ok = ok && rs_sweep_tmax_valid(tmax[i], r->max_dist);
   if (!ok) return seterr(MDH_E_INVALID, "a ray's length is not finite, negative or exceeds the scene's max_dist");
   return MDH_OK;
}
// host arrays: uploads what the call brings into d_rays (dir and tmax: null for contacts), launches, and leaves the results there
static int sweep_host_run(mdh_renderer *r, int what, int32_t n, const float *org, const float *dir, const float *radius, const float *tmax,
                          const int32_t *kind_ixs, int32_t n_kinds, bool normals, RayStage &st)
{
   const int rc = host_query_begin(r, n, st);
   if (rc != MDH_OK) return rc;
   const float *d_org = st.up(SLOT_ORG, org, 3), *d_dir = st.up(SLOT_DIR, dir, 3), *d_tmax = st.up(SLOT_TMAX, tmax, 1), *d_radius = st.up(SLOT_RADIUS, radius, 1);
   HIP_TRY(st.err);
   const RayQueryArgs a = ray_query_staged(st, 0.0f, 0.0f, d_org, dir ? d_dir : nullptr, tmax ? d_tmax : nullptr, radius ? d_radius : nullptr, normals, nullptr);
   return ray_query_enqueue(r, what, a, kind_ixs, n_kinds, false, st.qs, st.qs);
}
// what all four refuse before they look at their arrays
static int sweep_check(const mdh_renderer *r, int32_t n, bool arrays, const int32_t *kind_ixs, int32_t n_kinds)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!arrays || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   return sweep_kinds_check(r, kind_ixs, n_kinds); // (the kind list is the host's, wherever the arrays live)
}
extern "C" int32_t mdh_spherecast(mdh_renderer *r, int32_t n, const float *org, const float *dir, const float *radius, const float *tmax,
                                  const int32_t *kind_ixs, int32_t n_kinds, int32_t *hit_out, int32_t *index_out, float *t_out, int32_t *steps_out,
                                  float *pos_out, float *normal_out)
{
   int rc = sweep_check(r, n, org && dir && hit_out, kind_ixs, n_kinds);
   if (rc != MDH_OK || (rc = sweep_host_check(r, n, org, dir, radius, tmax)) != MDH_OK) return rc;
   if (n == 0) return MDH_OK;
   RayStage st;
   if ((rc = sweep_host_run(r, MDH_RQ_SPHERECAST, n, org, dir, radius, tmax, kind_ixs, n_kinds, normal_out != nullptr, st)) != MDH_OK) return rc;
   ray_query_down(st, hit_out, index_out, t_out, steps_out, pos_out, normal_out);
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_spherecast_device(mdh_renderer *r, int32_t n, const float *org, const float *dir, const float *radius, const float *tmax,
                                         const int32_t *kind_ixs, int32_t n_kinds, int32_t *hit_out, int32_t *index_out, float *t_out, int32_t *steps_out,
                                         float *pos_out, float *normal_out, void *stream)
{
   const int rc = sweep_check(r, n, org && dir && hit_out, kind_ixs, n_kinds);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)n * 4;
   const RayArray arrays[] = {{org, 3 * w, "origins"}, {dir, 3 * w, "directions"}, {radius, w, "radii"}, {tmax, w, "tmax"}, {hit_out, w, "hit"}, {index_out, w, "index"},
                              {t_out, w, "t"}, {steps_out, w, "steps"}, {pos_out, 3 * w, "positions"}, {normal_out, 3 * w, "normals"}};
   const RayQueryArgs a = ray_query_args(n, 0.0f, 0.0f, org, dir, tmax, radius, hit_out, index_out, t_out, steps_out, pos_out, normal_out, nullptr);
   return ray_query_device(r, MDH_RQ_SPHERECAST, arrays, a, kind_ixs, n_kinds, true, stream);
}
extern "C" int32_t mdh_contacts(mdh_renderer *r, int32_t n, const float *centre, const float *radius, const int32_t *kind_ixs, int32_t n_kinds,
                                float *dist_out, int32_t *index_out, float *normal_out)
{
   int rc = sweep_check(r, n, centre && dist_out, kind_ixs, n_kinds);
   if (rc != MDH_OK || (rc = sweep_host_check(r, n, centre, nullptr, radius, nullptr)) != MDH_OK) return rc;
   if (n == 0) return MDH_OK;
   RayStage st;
   if ((rc = sweep_host_run(r, MDH_RQ_CONTACT, n, centre, nullptr, radius, nullptr, kind_ixs, n_kinds, normal_out != nullptr, st)) != MDH_OK) return rc;
   ray_query_down(st, nullptr, index_out, dist_out, nullptr, nullptr, normal_out); // (a contact's distance: where a ray's t is)
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_contacts_device(mdh_renderer *r, int32_t n, const float *centre, const float *radius, const int32_t *kind_ixs, int32_t n_kinds,
                                       float *dist_out, int32_t *index_out, float *normal_out, void *stream)
{
   const int rc = sweep_check(r, n, centre && dist_out, kind_ixs, n_kinds);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)n * 4;
   const RayArray arrays[] = {{centre, 3 * w, "centres"}, {radius, w, "radii"}, {dist_out, w, "distances"}, {index_out, w, "index"}, {normal_out, 3 * w, "normals"}};
   const RayQueryArgs a = ray_query_args(n, 0.0f, 0.0f, centre, nullptr, nullptr, radius, nullptr, index_out, dist_out, nullptr, nullptr, normal_out, nullptr);
   return ray_query_device(r, MDH_RQ_CONTACT, arrays, a, kind_ixs, n_kinds, false, stream);
}

// ------------------------------------------------------------------ meshing the scene's surface
// mdh_surface_mesh, mdh_surface_mesh_device: surface nets over a regular grid of the scene's distance (mdh_surface.h has the
// definition and the five kernels), by the query path -- the query stream, the committed scene, one bridge enter / leave and
// one table acquire / release round all launches, whose first and last mdh_ray_query_time's events enclose.  No settle_bump:
// nothing is edited.  The scratch is the renderer's and grows on demand; only the query stream uses it, and is drained
// before a buffer is replaced.
struct SurfaceGrid { int nc, ncell, nblocks; }; // corners, cells, workgroups of k_surface_count
static int surface_check(const mdh_renderer *r, const float *origin, float h, const int32_t *cells, float iso, const int32_t *kind_ixs, int32_t n_kinds, int32_t vcap,
                         int32_t qcap, const void *pos, const void *nrm, const void *idx, const void *quads, const void *counts, SurfaceGrid &g)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!origin || !cells || !counts) return seterr(MDH_E_INVALID, "bad argument");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   int rc = sweep_kinds_check(r, kind_ixs, n_kinds);
   if (rc != MDH_OK) return rc;
   if (cells[0] < 1 || cells[1] < 1 || cells[2] < 1) return seterr(MDH_E_INVALID, "a grid has at least one cell along every axis");
   if (!all_finite(origin, 3) || !rs_finite(h) || !rs_finite(iso) || !(h > 0.0f)) return seterr(MDH_E_INVALID, "the grid's origin, spacing or level is not finite, or the spacing is not positive");
   if (std::fabs(iso) > r->max_dist) return seterr(MDH_E_INVALID, "the level exceeds the scene's max_dist");
   long long nc = 1;
   for (int c = 0; c < 3; ++c) {
      if (cells[c] >= MDH_SURFACE_MAX_CORNERS) return seterr(MDH_E_INVALID, "the grid has more than MDH_SURFACE_MAX_CORNERS corners");
      nc *= (long long)cells[c] + 1; // (below 2^72 / 2^48 / 2^24 in turn: no overflow)
      if (nc > MDH_SURFACE_MAX_CORNERS) return seterr(MDH_E_INVALID, "the grid has more than MDH_SURFACE_MAX_CORNERS corners");
      const float far = origin[c] + (float)cells[c] * h; // (the last corner as the lanes compute it; the corners between lie between)
      if (!(std::fabs(origin[c]) <= 1024.0f) || !(std::fabs(far) <= 1024.0f)) return seterr(MDH_E_INVALID, "a grid corner lies outside +-1024");
   }
   if (vcap < 0 || qcap < 0) return seterr(MDH_E_INVALID, "a negative capacity");
   if (vcap == 0 ? (pos || nrm || idx) : (!pos && !nrm && !idx)) return seterr(MDH_E_INVALID, "vertex arrays and vertex_capacity: both or neither");
   if ((qcap == 0) != (quads == nullptr)) return seterr(MDH_E_INVALID, "quads_out and quad_capacity: both or neither");
   g.nc = (int)nc;
   g.ncell = cells[0] * cells[1] * cells[2];
   g.nblocks = (g.nc + MDH_BLOCK - 1) / MDH_BLOCK;
   return MDH_OK;
}
// room for n elements in a buffer only the query stream uses
template <class T> static int surface_room(DevBuf<T> &b, size_t n, hipStream_t qs)
{
   if (n <= b.cap) return MDH_OK;
   if (b.ptr) HIP_TRY(hipStreamSynchronize(qs));
   HIP_TRY(b.grow(n));
   return MDH_OK;
}
// the launches for outputs the device addresses (a: the grid, the capacities and the outputs are filled in)
static int surface_enqueue(mdh_renderer *r, SurfaceArgs a, const SurfaceGrid &g, const int32_t *kind_ixs, int32_t n_kinds, hipStream_t qs, hipStream_t caller)
{
   int rc;
   if ((rc = surface_room(r->d_surf_field, (size_t)g.nc, qs)) != MDH_OK || (rc = surface_room(r->d_surf_map, (size_t)g.ncell, qs)) != MDH_OK ||
       (rc = surface_room(r->d_surf_wg, 2 * (size_t)g.nblocks, qs)) != MDH_OK)
      return rc;
   a.nblocks = g.nblocks;
   a.field = r->d_surf_field.ptr; a.map = r->d_surf_map.ptr; a.wg = r->d_surf_wg.ptr;
   ListedArgs la;
   la.q = RayQueryArgs();
   la.n_kinds = n_kinds;
   for (int i = 0; i < MDH_MAX_KINDS; ++i) { la.kinds[i] = i < n_kinds ? kind_ixs[i] : 0; la.host_count[i] = r->host_count[i]; }
   const bool listed = n_kinds > 0;
   const void *field = table_kernel(r, listed ? GK_k_surface_field_listed : GK_k_surface_field);
   const void *vertices = table_kernel(r, listed ? GK_k_surface_vertices_listed : GK_k_surface_vertices);
   if (!field || !vertices) return seterr(MDH_E_INVALID, "no kernel built for this variant");
   const size_t lds = lds_bytes(r);
   const dim3 block(MDH_BLOCK);
   const long waves = (long)((a.cx + 4) / 4) * ((a.cy + 4) / 4) * ((a.cz + 4) / 4); // 4 x 4 x 4 blocks of the cx + 1, .. corners
   const unsigned field_groups = (unsigned)((waves + MDH_BLOCK / 64 - 1) / (MDH_BLOCK / 64)), cell_groups = (unsigned)((g.ncell + MDH_BLOCK - 1) / MDH_BLOCK);
   return query_enqueue(r, qs, caller, false, [&] {
      int rc = listed ? launch_kernel_ptr(field, dim3(field_groups), block, lds, qs, r->ks, a, la) : launch_kernel_ptr(field, dim3(field_groups), block, lds, qs, r->ks, a);
      if (rc == MDH_OK) rc = launch_kernel_ptr((const void *)k_surface_count, dim3((unsigned)g.nblocks), block, 0, qs, a);
      if (rc == MDH_OK) rc = launch_kernel_ptr((const void *)k_surface_scan, dim3(1), block, 0, qs, a);
      if (rc == MDH_OK && (a.vcap > 0 || a.qcap > 0)) // (the quads read the cells' vertices)
         rc = listed ? launch_kernel_ptr(vertices, dim3(cell_groups), block, lds, qs, r->ks, a, la) : launch_kernel_ptr(vertices, dim3(cell_groups), block, lds, qs, r->ks, a);
      if (rc == MDH_OK && a.qcap > 0) rc = launch_kernel_ptr((const void *)k_surface_quads, dim3((unsigned)g.nblocks), block, 0, qs, a);
      return rc;
   });
}
static SurfaceArgs surface_args(const float *origin, float h, const int32_t *cells, float iso, int32_t vcap, int32_t qcap)
{
   SurfaceArgs a;
   memset(&a, 0, sizeof a);
   a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2]; a.h = h; a.iso = iso;
   a.cx = cells[0]; a.cy = cells[1]; a.cz = cells[2];
   a.vcap = vcap; a.qcap = qcap;
   return a;
}
extern "C" int32_t mdh_surface_mesh(mdh_renderer *r, const float *origin, float spacing, const int32_t *cells, float iso, const int32_t *kind_ixs, int32_t n_kinds,
                                    int32_t vcap, int32_t qcap, float *pos_out, float *normal_out, int32_t *index_out, int32_t *quads_out, float *field_out, int32_t *counts_out)
{
   SurfaceGrid g;
   int rc = surface_check(r, origin, spacing, cells, iso, kind_ixs, n_kinds, vcap, qcap, pos_out, normal_out, index_out, quads_out, counts_out, g);
   if (rc != MDH_OK) return rc;
   hipStream_t qs = nullptr;
   if ((rc = query_stream_get(r, &qs)) != MDH_OK || (rc = ensure_committed(r, qs)) != MDH_OK) return rc;
   // the results' places in d_surf_out: the counts, then what was asked for
   const size_t v = (size_t)vcap, q = (size_t)qcap;
   const size_t at_pos = 2, at_nrm = at_pos + (pos_out ? 3 * v : 0), at_idx = at_nrm + (normal_out ? 3 * v : 0), at_quads = at_idx + (index_out ? v : 0), words = at_quads + 4 * q;
   if ((rc = surface_room(r->d_surf_out, words, qs)) != MDH_OK) return rc;
   int *out = r->d_surf_out.ptr;
   SurfaceArgs a = surface_args(origin, spacing, cells, iso, vcap, qcap);
   a.counts = out;
   a.positions = pos_out ? (float *)(out + at_pos) : nullptr;
   a.normals = normal_out ? (float *)(out + at_nrm) : nullptr;
   a.index = index_out ? out + at_idx : nullptr;
   a.quads = quads_out ? out + at_quads : nullptr;
   if ((rc = surface_enqueue(r, a, g, kind_ixs, n_kinds, qs, qs)) != MDH_OK) return rc;
   int32_t found[2] = {0, 0};
   HIP_TRY(hipMemcpyAsync(found, out, sizeof found, hipMemcpyDeviceToHost, qs));
   HIP_TRY(hipStreamSynchronize(qs));
   const size_t nv = (size_t)std::min(found[0], vcap), nq = (size_t)std::min(found[1], qcap); // (nothing behind them is written)
   if (pos_out && nv) HIP_TRY(hipMemcpyAsync(pos_out, a.positions, nv * 12, hipMemcpyDeviceToHost, qs));
   if (normal_out && nv) HIP_TRY(hipMemcpyAsync(normal_out, a.normals, nv * 12, hipMemcpyDeviceToHost, qs));
   if (index_out && nv) HIP_TRY(hipMemcpyAsync(index_out, a.index, nv * 4, hipMemcpyDeviceToHost, qs));
   if (quads_out && nq) HIP_TRY(hipMemcpyAsync(quads_out, a.quads, nq * 16, hipMemcpyDeviceToHost, qs));
   if (field_out) HIP_TRY(hipMemcpyAsync(field_out, r->d_surf_field.ptr, (size_t)g.nc * 4, hipMemcpyDeviceToHost, qs));
   if ((rc = ray_query_wait(r)) != MDH_OK) return rc;
   counts_out[0] = found[0]; counts_out[1] = found[1];
   return MDH_OK;
}
extern "C" int32_t mdh_surface_mesh_device(mdh_renderer *r, const float *origin, float spacing, const int32_t *cells, float iso, const int32_t *kind_ixs, int32_t n_kinds,
                                           int32_t vcap, int32_t qcap, float *pos_out, float *normal_out, int32_t *index_out, int32_t *quads_out, float *field_out,
                                           int32_t *counts_out, void *stream)
{
   SurfaceGrid g;
   int rc = surface_check(r, origin, spacing, cells, iso, kind_ixs, n_kinds, vcap, qcap, pos_out, normal_out, index_out, quads_out, counts_out, g);
   if (rc != MDH_OK) return rc;
   const size_t v = (size_t)vcap * 4, q = (size_t)qcap * 4;
   const RayArray arrays[] = {{pos_out, 3 * v, "positions"}, {normal_out, 3 * v, "normals"}, {index_out, v, "index"}, {quads_out, 4 * q, "quads"},
                              {field_out, (size_t)g.nc * 4, "field"}, {counts_out, 8, "counts"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK) return rc;
   hipStream_t qs = nullptr;
   if ((rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   SurfaceArgs a = surface_args(origin, spacing, cells, iso, vcap, qcap);
   a.positions = pos_out; a.normals = normal_out; a.index = index_out; a.quads = quads_out; a.field_out = field_out; a.counts = counts_out;
   return surface_enqueue(r, a, g, kind_ixs, n_kinds, qs, (hipStream_t)stream);
}

// ------------------------------------------------------------------ shading a host's rays
// mdh_shade_rays, mdh_shade_rays_device: pixel_color_probes (render_probes.glsl:246-291) along n rays of the host's, through
// the pixel program the screen pass runs (k_ray_shade, mdh_kernels.h), by the query path.  No settle_bump: nothing is edited.
// WHICH ATLASES, AND WHEN.  The query is a mdh_render_pass (MDH_PASS_SCREEN) that runs on the query stream: it reads set
// `last` at its place among the frames (query_enqueue, `framed`): behind every screen pass of a frame up to `last`, hence
// every probe pass of those frames, and in front of whatever a later frame rewrites.
// everything both calls refuse before they look at their arrays
static int shade_rays_check(const mdh_renderer *r, int32_t n, const float *org, const float *dir, int32_t mode, const float *rgb)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!org || !dir || !rgb || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   if (mode != 0 && mode != 2) return seterr(MDH_E_INVALID, "rays are shaded in mode 0 or 2 (mode 1, the normal, is mdh_raycast's)");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   // (the ALT variant of the screen pass, pick_kernel: not built for rays)
   if (r->opt_spec == 1 || r->opt_spec == 3 || (r->opt_spec == 2 && r->opt_mips && r->d_rad_mips[r->last].ptr))
      return seterr(MDH_E_STATE, "rays are shaded with MDH_OPT_INDIRECT_SPECULAR 0 or 2, the latter without MDH_OPT_RADIANCE_MIPS");
   return shade_scene_check(r);
}
static RayShadeArgs ray_shade_args(const mdh_renderer *r, int32_t n, int32_t tone_map, const float *org, const float *dir, float *rgb, int *hit, int *index, float *t, int *steps)
{
   RayShadeArgs a;
   a.n = n; a.tone_map = tone_map ? 1 : 0; a.ao_steps = r->opt_ao; a.spec_mode = r->opt_spec;
   a.org = org; a.dir = dir; a.rgb = rgb;
   a.hit = hit; a.index = index; a.t = t; a.steps = steps;
   return a;
}
// k_ray_shade with the screen pass's rows and the probes of set `last`, at its place among the frames
static int shade_rays_run(mdh_renderer *r, int32_t mode, const RayShadeArgs &a, hipStream_t qs, hipStream_t caller)
{
   return query_kernel(r, table_kernel(r, GK_k_ray_shade, mode), lane_blocks(a.n), lds_bytes_screen_mode(r, mode), qs, caller, true, make_probes(r), a);
}
extern "C" int32_t mdh_shade_rays(mdh_renderer *r, int32_t n, const float *org, const float *dir, int32_t mode, int32_t tone_map, float *rgb_out,
                                  int32_t *hit_out, int32_t *index_out, float *t_out, int32_t *steps_out)
{
   int rc = shade_rays_check(r, n, org, dir, mode, rgb_out);
   if (rc != MDH_OK) return rc;
   {
      bool ok = true;
      for (size_t i = 0; i < (size_t)n; ++i) ok = ok && rs_shade_ray_valid(org[3 * i], org[3 * i + 1], org[3 * i + 2], dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]); // (the lanes' predicate)
      if (!ok) return seterr(MDH_E_INVALID, "a ray is not finite, starts beyond 1024 or has a direction component beyond 2");
   }
   if (n == 0) return MDH_OK;
   RayStage st;
   if ((rc = host_query_begin(r, n, st)) != MDH_OK) return rc;
   const float *d_org = st.up(SLOT_ORG, org, 3), *d_dir = st.up(SLOT_DIR, dir, 3);
   HIP_TRY(st.err);
   const RayShadeArgs a = ray_shade_args(r, n, tone_map, d_org, d_dir, st.at(SLOT_RGB), st.at<int>(SLOT_HIT), st.at<int>(SLOT_INDEX), st.at(SLOT_T), st.at<int>(SLOT_STEPS));
   if ((rc = shade_rays_run(r, mode, a, st.qs, st.qs)) != MDH_OK) return rc;
   st.down(rgb_out, SLOT_RGB, 3); st.down(hit_out, SLOT_HIT, 1); st.down(index_out, SLOT_INDEX, 1); st.down(t_out, SLOT_T, 1); st.down(steps_out, SLOT_STEPS, 1);
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_shade_rays_device(mdh_renderer *r, int32_t n, const float *org, const float *dir, int32_t mode, int32_t tone_map, float *rgb_out,
                                         int32_t *hit_out, int32_t *index_out, float *t_out, int32_t *steps_out, void *stream)
{
   int rc = shade_rays_check(r, n, org, dir, mode, rgb_out);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)n * 4;
   const RayArray arrays[] = {{org, 3 * w, "origins"}, {dir, 3 * w, "directions"}, {rgb_out, 3 * w, "colours"}, {hit_out, w, "hit"},
                              {index_out, w, "index"}, {t_out, w, "t"}, {steps_out, w, "steps"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK || n == 0) return rc;
   hipStream_t qs = nullptr;
   if ((rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   return shade_rays_run(r, mode, ray_shade_args(r, n, tone_map, org, dir, rgb_out, hit_out, index_out, t_out, steps_out), qs, (hipStream_t)stream);
}

// ------------------------------------------------------------------ path tracing a host's rays
// mdh_path_trace, mdh_path_trace_device: the estimator of k_path_trace (mdh_kernels.h) along n rays of the host's, samples
// sample_first .. sample_first + sample_count - 1 added to rgb_accum, by the query path at a shaded ray's place among the
// frames (no atlas is read, but the query keeps that call's place).  No settle_bump: nothing is edited.
// MDH_OPT_AO_STEPS and MDH_OPT_INDIRECT_SPECULAR do not enter.  Every refusal happens before a launch.
// everything both calls refuse before they look at their arrays
static int path_trace_check(const mdh_renderer *r, int32_t n, const float *org, const float *dir, int32_t sample_first, int32_t sample_count, int32_t bounces, const float *rgb)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!org || !dir || !rgb || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   if (sample_first < 0 || sample_count < 0 || sample_count > INT32_MAX - sample_first) return seterr(MDH_E_INVALID, "the samples are sample_first .. sample_first + sample_count - 1, both at least 0 and their sum below 2^31");
   if (!path_bounces_valid(bounces)) return seterr(MDH_E_INVALID, "paths take 0 to 6 bounces");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   return scene_extent_check(r, "traced paths", false); // (no path reads the probe grid)
}
static PathTraceArgs path_trace_args(int32_t n, uint32_t seed, uint32_t id_first, int32_t sample_first, int32_t sample_count, int32_t bounces, const float *org,
                                     const float *dir, float *rgb, int *hit, int *index, float *t)
{
   PathTraceArgs a;
   a.n = n; a.bounces = bounces; a.seed = seed; a.id_first = id_first; a.sample_first = sample_first; a.sample_count = sample_count;
   a.org = org; a.dir = dir; a.rgb = rgb;
   a.hit = hit; a.index = index; a.t = t;
   return a;
}
// k_path_trace (no park rows) at the place among the frames a shaded ray's kernel has: no atlas is read, the place is kept
static int path_trace_run(mdh_renderer *r, const PathTraceArgs &a, hipStream_t qs, hipStream_t caller)
{
   return query_kernel(r, table_kernel(r, GK_k_path_trace), lane_blocks(a.n), lds_bytes(r), qs, caller, true, a);
}
extern "C" int32_t mdh_path_trace(mdh_renderer *r, int32_t n, const float *org, const float *dir, uint32_t seed, uint32_t id_first, int32_t sample_first,
                                  int32_t sample_count, int32_t bounces, float *rgb_accum, int32_t *hit_out, int32_t *index_out, float *t_out)
{
   int rc = path_trace_check(r, n, org, dir, sample_first, sample_count, bounces, rgb_accum);
   if (rc != MDH_OK) return rc;
   {
      bool ok = true;
      for (size_t i = 0; i < (size_t)n; ++i) ok = ok && path_ray_valid(org[3 * i], org[3 * i + 1], org[3 * i + 2], dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]); // (the lanes' predicate)
      if (!ok) return seterr(MDH_E_INVALID, "a ray is not finite, starts beyond 1024, has a direction component beyond 2 or a direction of zero");
   }
   if (n == 0 || sample_count == 0) return MDH_OK;
   RayStage st;
   if ((rc = host_query_begin(r, n, st)) != MDH_OK) return rc;
   const float *d_org = st.up(SLOT_ORG, org, 3), *d_dir = st.up(SLOT_DIR, dir, 3);
   float *d_rgb = st.up(SLOT_RGB, rgb_accum, 3); // (the sums so far)
   HIP_TRY(st.err);
   const PathTraceArgs a = path_trace_args(n, seed, id_first, sample_first, sample_count, bounces, d_org, d_dir, d_rgb, st.at<int>(SLOT_HIT), st.at<int>(SLOT_INDEX), st.at(SLOT_T));
   if ((rc = path_trace_run(r, a, st.qs, st.qs)) != MDH_OK) return rc;
   st.down(rgb_accum, SLOT_RGB, 3); st.down(hit_out, SLOT_HIT, 1); st.down(index_out, SLOT_INDEX, 1); st.down(t_out, SLOT_T, 1);
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_path_trace_device(mdh_renderer *r, int32_t n, const float *org, const float *dir, uint32_t seed, uint32_t id_first, int32_t sample_first,
                                         int32_t sample_count, int32_t bounces, float *rgb_accum, int32_t *hit_out, int32_t *index_out, float *t_out, void *stream)
{
   int rc = path_trace_check(r, n, org, dir, sample_first, sample_count, bounces, rgb_accum);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)n * 4;
   const RayArray arrays[] = {{org, 3 * w, "origins"}, {dir, 3 * w, "directions"}, {rgb_accum, 3 * w, "colour sums"}, {hit_out, w, "hit"},
                              {index_out, w, "index"}, {t_out, w, "t"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK || n == 0 || sample_count == 0) return rc;
   hipStream_t qs = nullptr;
   if ((rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   return path_trace_run(r, path_trace_args(n, seed, id_first, sample_first, sample_count, bounces, org, dir, rgb_accum, hit_out, index_out, t_out), qs, (hipStream_t)stream);
}
// the sampler by itself, on the host over the functions the lanes call (mdh_path.h): no launch, no renderer
extern "C" int32_t mdh_path_scatter(int32_t n, const float *dir, const float *normal, const float *roughness, uint32_t seed, uint32_t id_first, int32_t sample,
                                    int32_t bounce, float *dir_out)
{
   if (n < 0 || sample < 0 || bounce < 0 || (n > 0 && (!dir || !normal || !roughness || !dir_out))) return seterr(MDH_E_INVALID, "bad argument");
   for (size_t i = 0; i < (size_t)n; ++i)
      path_scatter_at(dir + 3 * i, normal + 3 * i, roughness[i], seed, id_first + (uint32_t)i, (uint32_t)sample, (uint32_t)bounce, dir_out + 3 * i);
   return MDH_OK;
}
// ------------------------------------------------------------------ in-scattering along a host's rays and at its points
// mdh_inscatter_points, mdh_inscatter_rays and their _device forms: the lights' fog at n points and along n rays of the host's
// (k_point_inscatter, k_ray_inscatter, mdh_kernels.h), by the query path as the RAY QUERIES take it, not the shade queries:
// nothing here reads an atlas, so there is no ordering against the frame's passes.  No settle_bump: nothing is edited.  Every
// refusal happens before a launch.
// what both forms of both calls refuse before they look at their arrays (the points' calls have neither march nor step)
static int inscatter_check(const mdh_renderer *r, int32_t n, bool arrays, bool rays, int32_t march, float step)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!arrays || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   if (rays && march != 0 && march != 1) return seterr(MDH_E_INVALID, "march is 0 or 1");
   if (rays && !rs_inscatter_step_valid(step, r->max_dist)) return seterr(MDH_E_INVALID, "the step is not finite, not above 0, or more than 4096 of it fit into the scene's max_dist");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   return MDH_OK;
}
static InscatterPointArgs inscatter_point_args(int32_t n, const float *pos, const float *dir, const float *f, float *rgb)
{
   InscatterPointArgs a;
   a.n = n;
   a.pos = pos; a.dir = dir; a.f = f;
   a.rgb = rgb;
   return a;
}
static InscatterRayArgs inscatter_ray_args(int32_t n, int32_t march, float step, const float *org, const float *dir, const float *tmax, float *rgb, float *len, int *steps)
{
   InscatterRayArgs a;
   a.n = n; a.march = march; a.step = step;
   a.org = org; a.dir = dir; a.tmax = tmax;
   a.rgb = rgb; a.len = len; a.steps = steps;
   return a;
}
// a lane per point; a wavefront per ray.  No atlas is read: neither kernel has a place among the frames
static int inscatter_points_run(mdh_renderer *r, const InscatterPointArgs &a, hipStream_t qs, hipStream_t caller)
{
   return query_kernel(r, table_kernel(r, GK_k_point_inscatter), lane_blocks(a.n), lds_bytes(r), qs, caller, false, a);
}
static int inscatter_rays_run(mdh_renderer *r, const InscatterRayArgs &a, hipStream_t qs, hipStream_t caller)
{
   const unsigned blocks = (unsigned)(((size_t)a.n + MDH_BLOCK / MDH_RS_WAVE - 1) / (MDH_BLOCK / MDH_RS_WAVE));
   return query_kernel(r, table_kernel(r, GK_k_ray_inscatter), blocks, lds_bytes(r), qs, caller, false, a);
}
extern "C" int32_t mdh_inscatter_points(mdh_renderer *r, int32_t n, const float *pos, const float *dir, const float *f, float *rgb_out)
{
   int rc = inscatter_check(r, n, pos && dir && rgb_out, false, 0, 0.0f);
   if (rc != MDH_OK) return rc;
   if (!all_finite(pos, 3 * (size_t)n) || !all_finite(dir, 3 * (size_t)n)) return seterr(MDH_E_INVALID, "a point or direction is not finite");
   if (f) {
      bool ok = true;
      for (int32_t i = 0; i < n; ++i) ok = ok && rs_inscatter_f_valid(f[i]); // (the lanes' predicate)
      if (!ok) return seterr(MDH_E_INVALID, "a distance along the ray is not finite");
   }
   if (n == 0) return MDH_OK;
   RayStage st;
   if ((rc = host_query_begin(r, n, st)) != MDH_OK) return rc;
   const float *d_pos = st.up(SLOT_ORG, pos, 3), *d_dir = st.up(SLOT_DIR, dir, 3), *d_f = st.up(SLOT_F, f, 1);
   HIP_TRY(st.err);
   if ((rc = inscatter_points_run(r, inscatter_point_args(n, d_pos, d_dir, f ? d_f : nullptr, st.at(SLOT_RGB)), st.qs, st.qs)) != MDH_OK) return rc;
   st.down(rgb_out, SLOT_RGB, 3);
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_inscatter_points_device(mdh_renderer *r, int32_t n, const float *pos, const float *dir, const float *f, float *rgb_out, void *stream)
{
   int rc = inscatter_check(r, n, pos && dir && rgb_out, false, 0, 0.0f);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)n * 4;
   const RayArray arrays[] = {{pos, 3 * w, "positions"}, {dir, 3 * w, "directions"}, {f, w, "distances"}, {rgb_out, 3 * w, "colours"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK || n == 0) return rc;
   hipStream_t qs = nullptr;
   if ((rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   return inscatter_points_run(r, inscatter_point_args(n, pos, dir, f, rgb_out), qs, (hipStream_t)stream);
}
extern "C" int32_t mdh_inscatter_rays(mdh_renderer *r, int32_t n, const float *org, const float *dir, const float *tmax, int32_t march, float step,
                                      float *rgb_out, float *len_out, int32_t *steps_out)
{
   int rc = inscatter_check(r, n, org && dir && tmax && rgb_out, true, march, step);
   if (rc != MDH_OK) return rc;
   if (!all_finite(org, 3 * (size_t)n) || !all_finite(dir, 3 * (size_t)n)) return seterr(MDH_E_INVALID, "a ray is not finite");
   {
      bool ok = true;
      for (int32_t i = 0; i < n; ++i) ok = ok && rs_inscatter_tmax_valid(tmax[i], r->max_dist); // (the wavefronts' predicate)
      if (!ok) return seterr(MDH_E_INVALID, "a ray's length is not finite, is negative or exceeds the scene's max_dist");
   }
   if (n == 0) return MDH_OK;
   RayStage st;
   if ((rc = host_query_begin(r, n, st)) != MDH_OK) return rc;
   const float *d_org = st.up(SLOT_ORG, org, 3), *d_dir = st.up(SLOT_DIR, dir, 3), *d_tmax = st.up(SLOT_TMAX, tmax, 1);
   HIP_TRY(st.err);
   const InscatterRayArgs a = inscatter_ray_args(n, march, step, d_org, d_dir, d_tmax, st.at(SLOT_RGB), st.at(SLOT_LEN), st.at<int>(SLOT_STEPS));
   if ((rc = inscatter_rays_run(r, a, st.qs, st.qs)) != MDH_OK) return rc;
   st.down(rgb_out, SLOT_RGB, 3); st.down(len_out, SLOT_LEN, 1); st.down(steps_out, SLOT_STEPS, 1);
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_inscatter_rays_device(mdh_renderer *r, int32_t n, const float *org, const float *dir, const float *tmax, int32_t march, float step,
                                             float *rgb_out, float *len_out, int32_t *steps_out, void *stream)
{
   int rc = inscatter_check(r, n, org && dir && tmax && rgb_out, true, march, step);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)n * 4;
   const RayArray arrays[] = {{org, 3 * w, "origins"}, {dir, 3 * w, "directions"}, {tmax, w, "tmax"}, {rgb_out, 3 * w, "colours"},
                              {len_out, w, "lengths"}, {steps_out, w, "steps"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK || n == 0) return rc;
   hipStream_t qs = nullptr;
   if ((rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   return inscatter_rays_run(r, inscatter_ray_args(n, march, step, org, dir, tmax, rgb_out, len_out, steps_out), qs, (hipStream_t)stream);
}

// ------------------------------------------------------------------ lighting a host's points
// mdh_shade_points, mdh_shade_points_device: the light that arrives at n points of the host's -- pixel_color_probes from the
// hit on (mode 0), direct light times occlusion (mode 2), or sample_irradiance alone (mode 3) -- through k_point_shade
// (mdh_kernels.h), by the query path at a shaded ray's place among the frames, under shade_scene_check.  Nothing is edited.
static int shade_points_check(const mdh_renderer *r, int32_t n, const float *pos, const float *normal, const float *view, const int32_t *material,
                              int32_t mode, int32_t tone_map, const float *rgb)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!pos || !normal || !rgb || n < 0) return seterr(MDH_E_INVALID, "bad argument");
   if (mode != 0 && mode != 2 && mode != MDH_POINT_IRRADIANCE) return seterr(MDH_E_INVALID, "points are shaded in mode 0, 2 or 3 (the irradiance alone)");
   if (mode == MDH_POINT_IRRADIANCE && tone_map != 0) return seterr(MDH_E_INVALID, "the irradiance of mode 3 is not tone-mapped");
   if (mode != MDH_POINT_IRRADIANCE && (!view || !material)) return seterr(MDH_E_INVALID, "modes 0 and 2 need a view direction and a material id per point");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "point queries answer scenes of built-in kinds only");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   // (the ALT variant of the screen pass, pick_kernel: not built for points either; mode 3 has no reflection)
   if (mode != MDH_POINT_IRRADIANCE && (r->opt_spec == 1 || r->opt_spec == 3 || (r->opt_spec == 2 && r->opt_mips && r->d_rad_mips[r->last].ptr)))
      return seterr(MDH_E_STATE, "points are shaded with MDH_OPT_INDIRECT_SPECULAR 0 or 2, the latter without MDH_OPT_RADIANCE_MIPS");
   return shade_scene_check(r);
}
static PointShadeArgs shade_points_args(const mdh_renderer *r, int32_t n, int32_t tone_map, const float *pos, const float *normal, const float *view, const int32_t *material, float *rgb)
{
   PointShadeArgs a;
   a.n = n; a.tone_map = tone_map ? 1 : 0; a.ao_steps = r->opt_ao; a.spec_mode = r->opt_spec; a.n_materials = MAX_MATERIALS; a.pad_ = 0;
   a.pos = pos; a.normal = normal; a.view = view; a.material = material; a.rgb = rgb;
   return a;
}
// k_point_shade with its own rows (mode 3 parks nothing), at a shaded ray's place among the frames
static int shade_points_run(mdh_renderer *r, int32_t mode, const PointShadeArgs &a, hipStream_t qs, hipStream_t caller)
{
   const size_t lds = mode == MDH_POINT_IRRADIANCE ? lds_bytes(r) : lds_bytes_screen_mode(r, mode);
   return query_kernel(r, table_kernel(r, GK_k_point_shade, mode), lane_blocks(a.n), lds, qs, caller, true, make_probes(r), a);
}
extern "C" int32_t mdh_shade_points(mdh_renderer *r, int32_t n, const float *pos, const float *normal, const float *view, const int32_t *material,
                                    int32_t mode, int32_t tone_map, float *rgb_out)
{
   int rc = shade_points_check(r, n, pos, normal, view, material, mode, tone_map, rgb_out);
   if (rc != MDH_OK) return rc;
   const bool full = mode != MDH_POINT_IRRADIANCE; // (mode 3 reads neither view directions nor material ids: not looked at)
   {
      bool ok = true;
      for (size_t i = 0; i < (size_t)n; ++i) // (the lanes' predicate)
         ok = ok && rs_shade_point_valid(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], full ? view[3 * i] : 0.0f,
                                         full ? view[3 * i + 1] : 0.0f, full ? view[3 * i + 2] : 0.0f, full ? material[i] : 0, full ? MAX_MATERIALS : 1);
      if (!ok) return seterr(MDH_E_INVALID, "a point is not finite, lies beyond 1024, has a normal or view component beyond 1, or names no material");
   }
   if (n == 0) return MDH_OK;
   RayStage st;
   if ((rc = host_query_begin(r, n, st)) != MDH_OK) return rc;
   const float *d_pos = st.up(SLOT_ORG, pos, 3), *d_normal = st.up(SLOT_DIR, normal, 3), *d_view = st.up(SLOT_VIEW, full ? view : nullptr, 3);
   const int32_t *d_material = st.up(SLOT_MATERIAL, full ? material : nullptr, 1);
   HIP_TRY(st.err);
   if ((rc = shade_points_run(r, mode, shade_points_args(r, n, tone_map, d_pos, d_normal, d_view, d_material, st.at(SLOT_RGB)), st.qs, st.qs)) != MDH_OK) return rc;
   st.down(rgb_out, SLOT_RGB, 3);
   HIP_TRY(st.err);
   return ray_query_wait(r);
}
extern "C" int32_t mdh_shade_points_device(mdh_renderer *r, int32_t n, const float *pos, const float *normal, const float *view, const int32_t *material,
                                           int32_t mode, int32_t tone_map, float *rgb_out, void *stream)
{
   int rc = shade_points_check(r, n, pos, normal, view, material, mode, tone_map, rgb_out);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)n * 4;
   if (mode == MDH_POINT_IRRADIANCE) { view = nullptr; material = nullptr; } // (mode 3 reads neither: not looked at, not passed on)
   const RayArray arrays[] = {{pos, 3 * w, "positions"}, {normal, 3 * w, "normals"}, {view, 3 * w, "view directions"}, {material, w, "material ids"}, {rgb_out, 3 * w, "colours"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK || n == 0) return rc;
   hipStream_t qs = nullptr;
   if ((rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   return shade_points_run(r, mode, shade_points_args(r, n, tone_map, pos, normal, view, material, rgb_out), qs, (hipStream_t)stream);
}
// the material id of primitive `index` (the numbering of mdh_read_gbuffer and mdh_raycast: the kinds in their declared order,
// each with its declared count) as the scene's table holds it now, pending edits included; -1 for -1 and for an index no
// primitive has.  A lookup on the host: what primitive_info (mdh_device.h) reads, without a launch.
extern "C" int32_t mdh_primitive_material(mdh_renderer *r, int32_t n, const int32_t *index, int32_t *material_out)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (n < 0 || (n > 0 && (!index || !material_out))) return seterr(MDH_E_INVALID, "bad argument");
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "a user-defined kind's material is a program's result: built-in kinds only");
   for (int32_t q = 0; q < n; ++q) {
      int32_t m = -1;
      long rest = index[q];
      for (int k = 0; k < r->npk && rest >= 0; ++k) {
         const Kind &kd = r->pk[k];
         if (rest < kd.max_count) {
            int count = rd_i(r, kd.count_off);
            if (count > kd.max_count) count = kd.max_count;
            if (rest < count) m = rd_i(r, kd.array_off + kd.stride * (int)rest + kd.f_d);
            break;
         }
         rest -= kd.max_count;
      }
      material_out[q] = m;
   }
   return MDH_OK;
}

// mdh_camera_rays, mdh_camera_rays_device: the rays of a width x height frame of the current camera (draw_screen.glsl:20-24),
// computed on the device by the screen kernel's own functions (k_camera_rays, mdh_kernels.h).  They read the camera, by value,
// and nothing else of the renderer.
static int camera_rays_check(const mdh_renderer *r, int32_t width, int32_t height, const float *org, const float *dir)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!org || !dir || width <= 0 || height <= 0 || (long long)width * height > (1ll << 28)) return seterr(MDH_E_INVALID, "bad argument");
   return MDH_OK;
}
static int camera_rays_launch(mdh_renderer *r, int32_t width, int32_t height, float *d_org, float *d_dir, hipStream_t st)
{
   PassKernel k;
   k.family = GK_k_camera_rays;
   CameraRayArgs a = {width, height, d_org, d_dir};
   const long n = (long)width * height;
   const int rc = launch_kernel_ptr(kernel_ptr(k), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, make_camera(r), a);
   if (rc != MDH_OK) return rc;
   HIP_TRY(hipGetLastError());
   return MDH_OK;
}
extern "C" int32_t mdh_camera_rays(mdh_renderer *r, int32_t width, int32_t height, float *org_out, float *dir_out)
{
   int rc = camera_rays_check(r, width, height, org_out, dir_out);
   if (rc != MDH_OK) return rc;
   hipStream_t qs = nullptr;
   RayStage st;
   if ((rc = query_stream_get(r, &qs)) != MDH_OK || (rc = rays_stage(r, (size_t)width * height, qs, st)) != MDH_OK) return rc;
   if ((rc = camera_rays_launch(r, width, height, st.at(SLOT_ORG), st.at(SLOT_DIR), qs)) != MDH_OK) return rc;
   st.down(org_out, SLOT_ORG, 3); st.down(dir_out, SLOT_DIR, 3);
   HIP_TRY(st.err);
   HIP_TRY(hipStreamSynchronize(qs));
   return MDH_OK;
}
extern "C" int32_t mdh_camera_rays_device(mdh_renderer *r, int32_t width, int32_t height, float *org_out, float *dir_out, void *stream)
{
   int rc = camera_rays_check(r, width, height, org_out, dir_out);
   if (rc != MDH_OK) return rc;
   const size_t bytes = (size_t)width * height * 12;
   const RayArray arrays[] = {{org_out, bytes, "origins"}, {dir_out, bytes, "directions"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK) return rc;
   return camera_rays_launch(r, width, height, org_out, dir_out, (hipStream_t)stream); // (on the caller's stream itself: ordered with it by being there)
}

// ------------------------------------------------------------------ a path-traced frame
// mdh_path_frame_begin, .._accumulate, .._read, .._rays, .._info, .._end and mdh_path_pixel_uv: the path tracer's estimator over the
// pixels of a frame, with the sums in the renderer's own memory (d_path_frame) from call to call (mdh_path_frame.h: the
// kernels).  mdh_path_frame_accumulate goes the query path at mdh_path_trace's place among the frames and is what
// mdh_ray_query_time times; the rays and the resolve read no scene and take neither the scene's table nor the timing pair.
// No settle_bump anywhere: nothing is edited.  Every refusal happens before a launch or an allocation.
// mdh_path_frame_begin_adaptive opens the same accumulator with a count and two moments a pixel and a stopping rule (mdh_path.h:
// path_pixel_active; mdh_path_frame_adaptive.h: the kernels): accumulate is then one round of four launches in one query_enqueue,
// the resolve divides by the pixel's count, and mdh_path_frame_stats / mdh_path_pixel_active hand out the state and the rule.
// what begin and accumulate refuse of the renderer's state: mdh_path_trace's list
static int path_frame_state_check(const mdh_renderer *r)
{
   if (has_custom_kinds(r)) return seterr(MDH_E_STATE, "ray queries answer scenes of built-in kinds only");
   if (r->in_frame) return seterr(MDH_E_STATE, "a frame is open");
   return scene_extent_check(r, "traced paths", false);
}
static int path_frame_open_check(const mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!r->pf.open) return seterr(MDH_E_STATE, "no path-traced frame is open (mdh_path_frame_begin)");
   return MDH_OK;
}
// a frame's slots (mdh_path_frame_adaptive.h): 64 a tile of 8 x 8 pixels, and the workgroups of 256 of them
static int path_frame_tiles(int W, int H) { return ((W + 7) / 8) * ((H + 7) / 8); } // (at most 2^23, a frame one pixel wide: 2^29 slots)
// mdh_path_frame_begin and mdh_path_frame_begin_adaptive (rule: the four parameters, or null for a plain frame)
struct PathRule { int min_samples, max_samples; float tolerance, floor; };
static int path_frame_open(mdh_renderer *r, int32_t width, int32_t height, uint32_t seed, int32_t bounces, int32_t jitter, const PathRule *rule)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!path_frame_size_valid(width, height)) return seterr(MDH_E_INVALID, "a path-traced frame has 1 to 2^26 pixels");
   if (!path_bounces_valid(bounces)) return seterr(MDH_E_INVALID, "paths take 0 to 6 bounces");
   if (jitter != 0 && jitter != 1) return seterr(MDH_E_INVALID, "jitter is 0 or 1");
   int rc = path_frame_state_check(r);
   if (rc != MDH_OK) return rc;
   hipStream_t qs = nullptr;
   if ((rc = query_stream_get(r, &qs)) != MDH_OK) return rc;
   const size_t pixels = (size_t)width * height, words = pixels * 3;
   r->pf.open = false; // (a failure below leaves no accumulator)
   if ((rc = surface_room(r->d_path_frame, words, qs)) != MDH_OK) return rc;
   if (rule) { // the count, the moments, the list with the workgroups' totals and the grand total behind it, the statistics' two words
      const size_t slots = (size_t)path_frame_tiles(width, height) * 64, groups = (slots + MDH_BLOCK - 1) / MDH_BLOCK;
      if ((rc = surface_room(r->d_path_count, pixels, qs)) != MDH_OK || (rc = surface_room(r->d_path_moments, 2 * pixels, qs)) != MDH_OK ||
          (rc = surface_room(r->d_path_list, slots + groups + 1, qs)) != MDH_OK || (rc = surface_room(r->d_path_totals, 2, qs)) != MDH_OK)
         return rc;
      HIP_TRY(hipMemsetAsync(r->d_path_count.ptr, 0, pixels * 4, qs));
      HIP_TRY(hipMemsetAsync(r->d_path_moments.ptr, 0, pixels * 8, qs));
   }
   HIP_TRY(hipMemsetAsync(r->d_path_frame.ptr, 0, words * 4, qs));
   r->pf.W = width; r->pf.H = height; r->pf.bounces = bounces; r->pf.jitter = jitter; r->pf.seed = seed;
   r->pf.samples = 0;
   r->pf.adaptive = rule != nullptr;
   if (rule) { r->pf.min_samples = rule->min_samples; r->pf.max_samples = rule->max_samples; r->pf.tolerance = rule->tolerance; r->pf.floor = rule->floor; }
   r->pf.cam = make_camera(r); // as it stands: later setters do not smear a running accumulation
   r->pf.open = true;
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_begin(mdh_renderer *r, int32_t width, int32_t height, uint32_t seed, int32_t bounces, int32_t jitter)
{
   return path_frame_open(r, width, height, seed, bounces, jitter, nullptr);
}
extern "C" int32_t mdh_path_frame_begin_adaptive(mdh_renderer *r, int32_t width, int32_t height, uint32_t seed, int32_t bounces, int32_t jitter, int32_t min_samples,
                                                 int32_t max_samples, float tolerance, float floor)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (!path_adaptive_valid(min_samples, max_samples, tolerance, floor))
      return seterr(MDH_E_INVALID, "1 <= min_samples <= max_samples <= 2^24, a tolerance and a floor that are finite and at least 0");
   const PathRule rule = {min_samples, max_samples, tolerance, floor};
   return path_frame_open(r, width, height, seed, bounces, jitter, &rule);
}
// the kernels' description of the open adaptive frame
static PathAdaptArgs path_adapt_args(const mdh_renderer *r)
{
   PathAdaptArgs a;
   memset(&a, 0, sizeof a);
   a.W = r->pf.W; a.H = r->pf.H;
   a.tiles_x = (a.W + 7) / 8; a.n_tiles = path_frame_tiles(a.W, a.H);
   a.n_slots = a.n_tiles * 64; a.nblocks = (a.n_slots + MDH_BLOCK - 1) / MDH_BLOCK;
   a.bounces = r->pf.bounces; a.seed = r->pf.seed; a.jitter = r->pf.jitter;
   a.min_samples = r->pf.min_samples; a.max_samples = r->pf.max_samples; a.tolerance = r->pf.tolerance; a.floor = r->pf.floor;
   a.compact = r->opt_pf_compact;
   a.sums = r->d_path_frame.ptr; a.count = r->d_path_count.ptr; a.moments = r->d_path_moments.ptr;
   a.list = r->d_path_list.ptr; a.wg = a.list + a.n_slots;
   return a;
}
static const void *adapt_kernel(int family, int what = 0)
{
   PassKernel k;
   k.family = family; k.what = what;
   return kernel_ptr(k);
}
// one round of an adaptive frame: the pixels active under the rule now take min (sample_count, max_samples - n) more samples.
// Four launches on the query stream inside one query_enqueue (what mdh_ray_query_time then times); the host learns no count
static int path_frame_round(mdh_renderer *r, int32_t sample_count)
{
   int rc;
   hipStream_t qs = nullptr;
   if ((rc = query_stream_get(r, &qs)) != MDH_OK || (rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   PathAdaptArgs a = path_adapt_args(r);
   a.sample_count = sample_count;
   const void *kernel = table_kernel(r, GK_k_path_frame_adaptive);
   if (!kernel) return seterr(MDH_E_INVALID, "no kernel built for this variant");
   const KCamera cam = r->pf.cam;
   const dim3 grid((unsigned)a.nblocks), block(MDH_BLOCK);
   rc = query_enqueue(r, qs, qs, true, [&] {
      int lrc = launch_kernel_ptr(adapt_kernel(GK_k_path_adapt_count), grid, block, 0, qs, a);
      if (lrc == MDH_OK) lrc = launch_kernel_ptr(adapt_kernel(GK_k_path_adapt_scan), dim3(1), block, 0, qs, a);
      if (lrc == MDH_OK) lrc = launch_kernel_ptr(adapt_kernel(GK_k_path_adapt_compact, a.compact), grid, block, 0, qs, a);
      if (lrc == MDH_OK) lrc = launch_kernel_ptr(kernel, grid, block, lds_bytes(r), qs, r->ks, cam, a);
      return lrc;
   });
   if (rc != MDH_OK) return rc;
   const int32_t left = r->pf.max_samples - r->pf.samples;
   r->pf.samples += sample_count < left ? sample_count : left; // (the largest count a pixel can hold)
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_accumulate(mdh_renderer *r, int32_t sample_count)
{
   int rc = path_frame_open_check(r);
   if (rc != MDH_OK) return rc;
   if (sample_count < 0 || sample_count > INT32_MAX - r->pf.samples) return seterr(MDH_E_INVALID, "a sample count of at least 0, the samples so far and it below 2^31");
   if ((rc = path_frame_state_check(r)) != MDH_OK || sample_count == 0) return rc;
   if (r->pf.adaptive) return path_frame_round(r, sample_count);
   hipStream_t qs = nullptr;
   if ((rc = query_stream_get(r, &qs)) != MDH_OK || (rc = device_query_begin(r, &qs)) != MDH_OK) return rc;
   PathFrameArgs a;
   a.W = r->pf.W; a.H = r->pf.H;
   a.tiles_x = (a.W + 7) / 8; a.n_tiles = a.tiles_x * ((a.H + 7) / 8);
   a.bounces = r->pf.bounces; a.seed = r->pf.seed; a.jitter = r->pf.jitter;
   a.sample_first = r->pf.samples; a.sample_count = sample_count;
   a.sums = r->d_path_frame.ptr;
   // the recorded primary segment where it can be used again: without jitter, in a launch of more than one sample (one sample
   // has nothing to reuse and the record's registers cost it time: DESIGN.md section 4, "A path-traced frame"; the same bits)
   const void *kernel = table_kernel(r, GK_k_path_frame, !r->pf.jitter && sample_count > 1 ? 1 : 0);
   if (!kernel) return seterr(MDH_E_INVALID, "no kernel built for this variant");
   const KCamera cam = r->pf.cam;
   const unsigned blocks = (unsigned)((a.n_tiles + MDH_BLOCK / 64 - 1) / (MDH_BLOCK / 64));
   if ((rc = query_enqueue(r, qs, qs, true, [&] { return launch_kernel_ptr(kernel, dim3(blocks), dim3(MDH_BLOCK), lds_bytes(r), qs, r->ks, cam, a); })) != MDH_OK) return rc;
   r->pf.samples += sample_count;
   return MDH_OK; // (nothing to copy: nothing waits)
}
static int path_frame_read_check(const mdh_renderer *r, int32_t tone_map)
{
   const int rc = path_frame_open_check(r);
   if (rc != MDH_OK) return rc;
   if (tone_map != 0 && tone_map != 1) return seterr(MDH_E_INVALID, "tone_map is 0 or 1");
   if (r->pf.samples == 0) return seterr(MDH_E_STATE, "no sample has been accumulated: there is no 0 / 0 image");
   return MDH_OK;
}
// the resolve on the query stream, where the sums are written, for arrays `caller`'s stream holds
static int path_frame_resolve(mdh_renderer *r, int32_t tone_map, float *rgb, unsigned *rgba8, float *sums, hipStream_t qs, hipStream_t caller)
{
   if (!rgb && !rgba8 && !sums) return MDH_OK;
   PathFrameResolveArgs a;
   a.n = r->pf.W * r->pf.H; a.samples = r->pf.samples; a.tone_map = tone_map;
   a.sums = r->d_path_frame.ptr; a.rgb = rgb; a.rgba8 = rgba8; a.sums_out = sums;
   PassKernel k;
   k.family = r->pf.adaptive ? GK_k_path_frame_resolve_adaptive : GK_k_path_frame_resolve;
   if (caller != qs) HIP_TRY(r->bridge.create());
   HIP_TRY(r->bridge.enter(qs, caller, nullptr));
   const dim3 grid((unsigned)(((size_t)a.n + 255) / 256));
   const int *count = r->d_path_count.ptr; // (an adaptive frame: rgb = sum / (float) n of the pixel)
   const int rc = r->pf.adaptive ? launch_kernel_ptr(kernel_ptr(k), grid, dim3(256), 0, qs, a, count) : launch_kernel_ptr(kernel_ptr(k), grid, dim3(256), 0, qs, a);
   if (rc != MDH_OK) return rc;
   HIP_TRY(hipGetLastError());
   HIP_TRY(r->bridge.leave(qs, caller, nullptr));
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_read(mdh_renderer *r, int32_t tone_map, float *rgb_out, uint32_t *rgba8_out, float *sums_out, int32_t *samples_out)
{
   int rc = path_frame_read_check(r, tone_map);
   if (rc != MDH_OK) return rc;
   hipStream_t qs = nullptr;
   RayStage st;
   const size_t n = (size_t)r->pf.W * r->pf.H;
   if ((rc = query_stream_get(r, &qs)) != MDH_OK || (rc = rays_stage(r, n, qs, st)) != MDH_OK) return rc;
   if ((rc = path_frame_resolve(r, tone_map, rgb_out ? st.at(SLOT_RGB) : nullptr, rgba8_out ? st.at<unsigned>(SLOT_HIT) : nullptr, nullptr, qs, qs)) != MDH_OK) return rc;
   st.down(rgb_out, SLOT_RGB, 3); st.down(rgba8_out, SLOT_HIT, 1);
   HIP_TRY(st.err);
   if (sums_out) HIP_TRY(hipMemcpyAsync(sums_out, r->d_path_frame.ptr, n * 12, hipMemcpyDeviceToHost, qs)); // (the raw sums: no kernel)
   if ((rc = ray_query_wait(r)) != MDH_OK) return rc;
   if (samples_out) *samples_out = r->pf.samples;
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_read_device(mdh_renderer *r, int32_t tone_map, float *rgb_out, uint32_t *rgba8_out, float *sums_out, int32_t *samples_out,
                                              void *stream)
{
   int rc = path_frame_read_check(r, tone_map);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)r->pf.W * r->pf.H * 4;
   const RayArray arrays[] = {{rgb_out, 3 * w, "colours"}, {rgba8_out, w, "rgba8"}, {sums_out, 3 * w, "colour sums"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK) return rc;
   hipStream_t qs = nullptr;
   if ((rc = query_stream_get(r, &qs, true)) != MDH_OK) return rc;
   if ((rc = path_frame_resolve(r, tone_map, rgb_out, rgba8_out, sums_out, qs, (hipStream_t)stream)) != MDH_OK) return rc;
   if (samples_out) *samples_out = r->pf.samples; // (the host's: the count is no result of the device)
   return MDH_OK;
}
static int path_frame_rays_check(const mdh_renderer *r, int32_t sample, const float *org, const float *dir)
{
   const int rc = path_frame_open_check(r);
   if (rc != MDH_OK) return rc;
   if (sample < 0 || !org || !dir) return seterr(MDH_E_INVALID, "bad argument");
   return MDH_OK;
}
static int path_frame_rays_launch(mdh_renderer *r, int32_t sample, float *d_org, float *d_dir, hipStream_t st)
{
   PassKernel k;
   k.family = GK_k_path_frame_rays;
   PathFrameRayArgs a = {r->pf.W, r->pf.H, r->pf.seed, sample, r->pf.jitter, d_org, d_dir};
   const size_t n = (size_t)r->pf.W * r->pf.H;
   const int rc = launch_kernel_ptr(kernel_ptr(k), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r->pf.cam, a);
   if (rc != MDH_OK) return rc;
   HIP_TRY(hipGetLastError());
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_rays(mdh_renderer *r, int32_t sample, float *org_out, float *dir_out)
{
   int rc = path_frame_rays_check(r, sample, org_out, dir_out);
   if (rc != MDH_OK) return rc;
   hipStream_t qs = nullptr;
   RayStage st;
   if ((rc = query_stream_get(r, &qs)) != MDH_OK || (rc = rays_stage(r, (size_t)r->pf.W * r->pf.H, qs, st)) != MDH_OK) return rc;
   if ((rc = path_frame_rays_launch(r, sample, st.at(SLOT_ORG), st.at(SLOT_DIR), qs)) != MDH_OK) return rc;
   st.down(org_out, SLOT_ORG, 3); st.down(dir_out, SLOT_DIR, 3);
   HIP_TRY(st.err);
   HIP_TRY(hipStreamSynchronize(qs));
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_rays_device(mdh_renderer *r, int32_t sample, float *org_out, float *dir_out, void *stream)
{
   int rc = path_frame_rays_check(r, sample, org_out, dir_out);
   if (rc != MDH_OK) return rc;
   const size_t bytes = (size_t)r->pf.W * r->pf.H * 12;
   const RayArray arrays[] = {{org_out, bytes, "origins"}, {dir_out, bytes, "directions"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK) return rc;
   return path_frame_rays_launch(r, sample, org_out, dir_out, (hipStream_t)stream); // (on the caller's stream itself, as mdh_camera_rays_device)
}
extern "C" int32_t mdh_path_frame_info(mdh_renderer *r, int32_t *width, int32_t *height, int32_t *samples, int32_t *bounces, int32_t *jitter)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   const bool open = r->pf.open; // (none open: zeros)
   if (width) *width = open ? r->pf.W : 0;
   if (height) *height = open ? r->pf.H : 0;
   if (samples) *samples = open ? r->pf.samples : 0;
   if (bounces) *bounces = open ? r->pf.bounces : 0;
   if (jitter) *jitter = open ? r->pf.jitter : 0;
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_end(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   r->pf.open = false;
   r->pf.samples = 0;
   if (!r->d_path_frame.ptr) return MDH_OK;
   HIP_TRY(hipSetDevice(r->device));
   if (r->query_stream) HIP_TRY(hipStreamSynchronize(r->query_stream)); // (whatever still reads or writes the sums)
   HIP_TRY(r->d_path_frame.release());
   HIP_TRY(r->d_path_count.release()); HIP_TRY(r->d_path_moments.release()); HIP_TRY(r->d_path_list.release()); HIP_TRY(r->d_path_totals.release());
   return MDH_OK;
}
// mdh_path_frame_stats, mdh_path_frame_stats_device: an adaptive frame's counts and moments, the pixels active under the rule now and
// the samples taken.  The two scalars come from one workgroup's kernel on the query stream (no scene, no timing pair).
static int path_frame_stats_check(const mdh_renderer *r)
{
   const int rc = path_frame_open_check(r);
   if (rc != MDH_OK) return rc;
   if (!r->pf.adaptive) return seterr(MDH_E_STATE, "the open path-traced frame is a plain one (mdh_path_frame_begin_adaptive)");
   return MDH_OK;
}
static int path_frame_stats_enqueue(mdh_renderer *r, int32_t *count, float *moments, long long *active, long long *total, hipMemcpyKind kind, hipStream_t qs, hipStream_t caller)
{
   if (!count && !moments && !active && !total) return MDH_OK;
   const size_t n = (size_t)r->pf.W * r->pf.H;
   if (caller != qs) HIP_TRY(r->bridge.create());
   HIP_TRY(r->bridge.enter(qs, caller, nullptr));
   if (active || total) {
      PathAdaptArgs a = path_adapt_args(r);
      a.active_out = active; a.total_out = total;
      const int rc = launch_kernel_ptr(adapt_kernel(GK_k_path_adapt_stats), dim3(1), dim3(MDH_BLOCK), 0, qs, a);
      if (rc != MDH_OK) return rc;
      HIP_TRY(hipGetLastError());
   }
   if (count) HIP_TRY(hipMemcpyAsync(count, r->d_path_count.ptr, n * 4, kind, qs));
   if (moments) HIP_TRY(hipMemcpyAsync(moments, r->d_path_moments.ptr, n * 8, kind, qs));
   HIP_TRY(r->bridge.leave(qs, caller, nullptr));
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_stats(mdh_renderer *r, int32_t *count_out, float *moments_out, int64_t *active, int64_t *total_samples)
{
   int rc = path_frame_stats_check(r);
   if (rc != MDH_OK) return rc;
   hipStream_t qs = nullptr;
   if ((rc = query_stream_get(r, &qs)) != MDH_OK) return rc;
   long long *d = r->d_path_totals.ptr;
   if ((rc = path_frame_stats_enqueue(r, count_out, moments_out, active ? d : nullptr, total_samples ? d + 1 : nullptr, hipMemcpyDeviceToHost, qs, qs)) != MDH_OK) return rc;
   long long both[2] = {0, 0};
   if (active || total_samples) HIP_TRY(hipMemcpyAsync(both, d, sizeof both, hipMemcpyDeviceToHost, qs));
   if ((rc = ray_query_wait(r)) != MDH_OK) return rc;
   if (active) *active = both[0];
   if (total_samples) *total_samples = both[1];
   return MDH_OK;
}
extern "C" int32_t mdh_path_frame_stats_device(mdh_renderer *r, int32_t *count_out, float *moments_out, int64_t *active, int64_t *total_samples, void *stream)
{
   int rc = path_frame_stats_check(r);
   if (rc != MDH_OK) return rc;
   const size_t w = (size_t)r->pf.W * r->pf.H * 4;
   const RayArray arrays[] = {{count_out, w, "counts"}, {moments_out, 2 * w, "moments"}, {active, 8, "the active count"}, {total_samples, 8, "the samples' total"}};
   if ((rc = ray_arrays_check(r, arrays)) != MDH_OK) return rc;
   if ((active && ((uintptr_t)active & 7)) || (total_samples && ((uintptr_t)total_samples & 7))) return seterr(MDH_E_INVALID, "the two 64-bit words are aligned to 8 bytes");
   hipStream_t qs = nullptr;
   if ((rc = query_stream_get(r, &qs, true)) != MDH_OK) return rc;
   return path_frame_stats_enqueue(r, count_out, moments_out, (long long *)active, (long long *)total_samples, hipMemcpyDeviceToDevice, qs, (hipStream_t)stream);
}
// the rule by itself, on the host over the function the lanes call (mdh_path.h): no launch, no renderer
extern "C" int32_t mdh_path_pixel_active(int32_t n_pixels, const int32_t *count, const float *m1, const float *m2, int32_t min_samples, int32_t max_samples, float tolerance,
                                         float floor, uint8_t *active_out)
{
   if (n_pixels < 0 || !path_adaptive_valid(min_samples, max_samples, tolerance, floor) || (n_pixels > 0 && (!count || !m1 || !m2 || !active_out)))
      return seterr(MDH_E_INVALID, "bad argument");
   for (size_t q = 0; q < (size_t)n_pixels; ++q) active_out[q] = path_pixel_active(count[q], m1[q], m2[q], min_samples, max_samples, tolerance, floor) ? 1 : 0;
   return MDH_OK;
}
// the jitter by itself, on the host over the functions the lanes call (mdh_path.h): no launch, no renderer
extern "C" int32_t mdh_path_pixel_uv(int32_t width, int32_t height, uint32_t seed, uint32_t id_first, int32_t n, int32_t sample, int32_t jitter, float *uv_out)
{
   if (!path_frame_size_valid(width, height) || n < 0 || sample < 0 || (jitter != 0 && jitter != 1) || (n > 0 && !uv_out)) return seterr(MDH_E_INVALID, "bad argument");
   if ((uint64_t)id_first + (uint64_t)n > (uint64_t)width * (uint64_t)height) return seterr(MDH_E_INVALID, "the ids id_first .. id_first + n - 1 are pixels of the frame");
   for (size_t q = 0; q < (size_t)n; ++q) {
      const uint32_t id = id_first + (uint32_t)q;
      path_pixel_uv((int)(id % (uint32_t)width), (int)(id / (uint32_t)width), width, height, seed, (uint32_t)sample, jitter != 0, uv_out[2 * q], uv_out[2 * q + 1]);
   }
   return MDH_OK;
}


// the hierarchy of the committed scene (pending edits are committed first): its nodes, leaves, depth and the length of the
// always-evaluated list; all 0 while MDH_OPT_TRIANGLE_BVH is off or the scene declares no triangles
extern "C" int32_t mdh_triangle_bvh_info(mdh_renderer *r, int32_t *nodes, int32_t *leaves, int32_t *depth, int32_t *always)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (r->table_dirty && !r->in_frame) {
      HIP_TRY(hipSetDevice(r->device));
      const int rc = commit_scene(r, r->stream);
      if (rc != MDH_OK) return rc;
   }
   const bool on = r->bvh_active;
   if (nodes) *nodes = on ? (int32_t)r->bvh.nodes.size() / 2 : 0;
   if (leaves) *leaves = on ? r->bvh.leaves : 0;
   if (depth) *depth = on ? r->bvh.depth : 0;
   if (always) *always = on ? r->bvh.n_always : 0;
   return MDH_OK;
}
#ifdef MDH_BVH_STATS
// the counter build: node visits and skipped nodes (wavefronts) since the last call
extern "C" int32_t mdh_diag_bvh(unsigned long long *out2)
{
   if (hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_bvh_stats), sizeof(unsigned long long) * 2) != hipSuccess) return MDH_E_DEVICE;
   unsigned long long z[2] = {0, 0};
   if (hipMemcpyToSymbol(HIP_SYMBOL(g_bvh_stats), z, sizeof z) != hipSuccess) return MDH_E_DEVICE;
   return MDH_OK;
}
#endif

#ifdef MDH_BEST_STATS
// the counter build: the best-first probe search's wave-rounds, winning lanes, fallback wavefronts and fallback lanes since the last call
extern "C" int32_t mdh_diag_best_first(unsigned long long *out4)
{
   if (!out4) return MDH_E_INVALID;
   if (hipDeviceSynchronize() != hipSuccess) return MDH_E_DEVICE;
   if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_best_stats), sizeof(unsigned long long) * 4) != hipSuccess) return MDH_E_DEVICE;
   unsigned long long z[4] = {0, 0, 0, 0};
   if (hipMemcpyToSymbol(HIP_SYMBOL(g_best_stats), z, sizeof z) != hipSuccess) return MDH_E_DEVICE;
   return MDH_OK;
}
// ... and of its first round's approximate ranking (MDH_BEST_APPROX): lanes it gave a winner, lanes it gave no candidate, lanes it
// left undecided, wavefronts that ran the exact scan because of them, since the last call
extern "C" int32_t mdh_diag_best_approx(unsigned long long *out4)
{
   if (!out4) return MDH_E_INVALID;
   if (hipDeviceSynchronize() != hipSuccess) return MDH_E_DEVICE;
   if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_best_approx_stats), sizeof(unsigned long long) * 4) != hipSuccess) return MDH_E_DEVICE;
   unsigned long long z[4] = {0, 0, 0, 0};
   if (hipMemcpyToSymbol(HIP_SYMBOL(g_best_approx_stats), z, sizeof z) != hipSuccess) return MDH_E_DEVICE;
   return MDH_OK;
}
#endif

// MDH_OPT_SCREEN_REPLAY: screen passes launched since creation that marched, marched and recorded, replayed
extern "C" int32_t mdh_screen_replay_stats(mdh_renderer *r, int64_t *plain, int64_t *recording, int64_t *replaying)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (plain) *plain = r->scr_replay.stats[0];
   if (recording) *recording = r->scr_replay.stats[1];
   if (replaying) *replaying = r->scr_replay.stats[2];
   return MDH_OK;
}
// the size of a pixel's record (tests/test_screen_replay_host.py holds DESIGN.md's figure against it)
extern "C" int32_t mdh_screen_record_bytes(void) { return (int32_t)sizeof(PixelRecord); }
// MDH_OPT_PROBE_SETTLE: the run of unchanged irradiance passes under the inputs that hold now, probe passes not launched
// since creation, texels the newest observed pass changed.  Reads the slots that have arrived; waits for nothing.
extern "C" int32_t mdh_probe_settle_stats(mdh_renderer *r, int64_t *run, int64_t *skipped, int64_t *last_changed_texels)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (r->settle.slots) r->settle.poll();
   if (run) *run = r->settle.current_run();
   if (skipped) *skipped = r->settle_skipped;
   if (last_changed_texels) *last_changed_texels = r->settle.last_changed;
   return MDH_OK;
}
// MDH_OPT_RADIANCE_REPLAY: radiance passes launched since creation that marched, marched and recorded, replayed
extern "C" int32_t mdh_radiance_replay_stats(mdh_renderer *r, int64_t *plain, int64_t *recording, int64_t *replaying)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (plain) *plain = r->rad_replay.stats[0];
   if (recording) *recording = r->rad_replay.stats[1];
   if (replaying) *replaying = r->rad_replay.stats[2];
   return MDH_OK;
}
extern "C" int32_t mdh_pass_time(mdh_renderer *r, int32_t pass, double *ms, int64_t *launches)
{
   if (!r || pass < 0 || pass >= MDH_PASS_COUNT) return seterr(MDH_E_INVALID, "bad argument");
   HIP_TRY(hipSetDevice(r->device));
   int rc = resolve_timing(r);
   if (rc != MDH_OK) return rc;
   if (ms) *ms = r->pass_ms[pass];
   if (launches) *launches = r->pass_n[pass];
   return MDH_OK;
}
extern "C" int32_t mdh_reset_pass_times(mdh_renderer *r)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   HIP_TRY(hipSetDevice(r->device));
   int rc = resolve_timing(r);
   if (rc != MDH_OK) return rc;
   for (int i = 0; i < MDH_PASS_COUNT; ++i) { r->pass_ms[i] = 0; r->pass_n[i] = 0; }
   return MDH_OK;
}

// Scenes.Get_Primitives_Location / Get_Lights_Location (scenes.adb:1435-1462)
extern "C" int32_t mdh_scene_layout(mdh_renderer *r, int32_t is_light, int32_t kind_ix, int32_t *count_off, int32_t *array_off, int32_t *stride, int32_t *elem_size)
{
   if (!r || kind_ix < 0 || kind_ix >= (is_light ? r->nlk : r->npk)) return seterr(MDH_E_INVALID, "bad kind index");
   const Kind &k = is_light ? r->lk[kind_ix] : r->pk[kind_ix];
   if (count_off) *count_off = k.count_off;
   if (array_off) *array_off = k.array_off;
   if (stride) *stride = k.stride;
   if (elem_size) *elem_size = k.elem_size;
   return MDH_OK;
}
extern "C" int32_t mdh_scene_buffer_size(mdh_renderer *r, int32_t *size, int32_t *total_light_off)
{
   if (!r) return seterr(MDH_E_INVALID, "null renderer");
   if (size) *size = (int32_t)r->scene_ubo.size();
   if (total_light_off) *total_light_off = r->total_light_off;
   return MDH_OK;
}
extern "C" int32_t mdh_read_scene_buffer(mdh_renderer *r, void *out, int32_t nbytes)
{
   if (!r || !out || nbytes < 0 || (size_t)nbytes > r->scene_ubo.size()) return seterr(MDH_E_INVALID, "bad argument");
   memcpy(out, r->scene_ubo.data(), (size_t)nbytes);
   return MDH_OK;
}
extern "C" int32_t mdh_read_partitioning(mdh_renderer *r, int32_t *out, int32_t n_ints)
{
   if (!r || !out) return seterr(MDH_E_INVALID, "bad argument");
   if (!r->part.enable) return seterr(MDH_E_STATE, "partitioning disabled");
   size_t total = (size_t)r->part_cells * (r->npk + r->part.index_count);
   if ((size_t)n_ints != total) return seterr(MDH_E_INVALID, "size mismatch");
   HIP_TRY(hipSetDevice(r->device));
   if (r->part_fence.version) HIP_TRY(hipEventSynchronize(r->part_fence.ev.ev)); // the last build
   HIP_TRY(hipMemcpy(out, r->d_part_ring[r->part_slot].ptr, total * 4, hipMemcpyDeviceToHost));
   return MDH_OK;
}
// the warnings of the last Update_Partitioning (scenes.adb:861-867 prints them): waits for that build only
extern "C" int32_t mdh_partition_warnings(mdh_renderer *r)
{
   if (!r) return 0;
   if (r->warn_pending) {
      (void)hipSetDevice(r->device);
      if (hipEventSynchronize(r->ev_warn.ev) != hipSuccess) return -1;
      r->part_warnings = *r->h_warn.ptr;
      r->warn_pending = false;
   }
   return r->part_warnings;
}

#ifdef MDH_DIAG
// rays started, SDF evaluations inside march loops, SDF evaluations in all, arg-min evaluations at hit points (lanes) of the
// last run of `pass`: what the oracle reports as orc_work_counters
extern "C" int32_t mdh_diag_work(mdh_renderer *r, int32_t pass, unsigned long long *out4)
{
   if (!r || !out4 || pass < 0 || pass >= MDH_PASS_COUNT) return MDH_E_INVALID;
   memcpy(out4, r->work[pass], sizeof r->work[pass]);
   return MDH_OK;
}
// the kernel variant pick_kernel chose at the last run of `pass`: out[0] = pfk (MDH_PF_*: ROOM, PART | PSMALL, or the general
// variant's PART / CUSTOM / FALLBACK bits), out[1] = 1 when the atlas addressing took the power-of-two variant
extern "C" int32_t mdh_diag_variant(mdh_renderer *r, int32_t pass, int32_t *out2)
{
   if (!r || !out2 || pass < 0 || pass >= MDH_PASS_COUNT) return MDH_E_INVALID;
   memcpy(out2, r->variant[pass], sizeof r->variant[pass]);
   return MDH_OK;
}
// segment_clear_bound against the unmodified march (raycast_visibility) on the committed scene, one segment A + vd [0, vmax]
// per lane.  A march is taken only where it must end (vmax <= 2^12: every step adds at least MDH_EPS, which exceeds half an ulp
// of total there); other lanes report vis = -1.
struct DiagSegArgs {
   int n;
   const float *A, *vd, *vmax;
   int *clear;
   float *vis;
};
template <int PART> __global__ __launch_bounds__(64) void k_diag_segments(KScene sc, DiagSegArgs a)
{
   stage_table(sc);
   const int q = blockIdx.x * 64 + threadIdx.x;
   if (q >= a.n) return;
   const f3 A = F3(a.A[3 * q], a.A[3 * q + 1], a.A[3 * q + 2]), vd = F3(a.vd[3 * q], a.vd[3 * q + 1], a.vd[3 * q + 2]);
   const float vmax = a.vmax[q];
   a.clear[q] = segment_clear_bound<PART>(sc, A, vd, vmax) ? 1 : 0;
   a.vis[q] = vmax <= 4096.0f ? raycast_visibility<PART>(sc, A, vd, vmax) : -1.0f;
}
// variant 0: the scan pick_kernel picks for the committed scene (MDH_PF_ROOM or the general scan 0); 1: the general scan forced.
// thr_lim_out: H_VCLEAR and H_VCLEAR_LIM as commit_scene wrote them.  Scenes with a partition or user-defined kinds: MDH_E_STATE.
extern "C" int32_t mdh_diag_segments(mdh_renderer *r, int32_t variant, int32_t n, const float *A, const float *vd, const float *vmax,
                                     int32_t *clear_out, float *vis_out, float *thr_lim_out)
{
   if (!r || n < 0 || (n > 0 && (!A || !vd || !vmax || !clear_out || !vis_out)) || (variant != 0 && variant != 1)) return seterr(MDH_E_INVALID, "bad argument");
   if (r->part.enable != 0 || has_custom_kinds(r)) return seterr(MDH_E_STATE, "mdh_diag_segments: the scan variants only (no partition, no user-defined kinds)");
   HIP_TRY(hipSetDevice(r->device));
   if (!r->query_stream) HIP_TRY(hipStreamCreateWithFlags(&r->query_stream, hipStreamNonBlocking));
   hipStream_t qs = r->query_stream;
   int rc = ensure_committed(r, qs);
   if (rc != MDH_OK) return rc;
   if (r->residency) return seterr(MDH_E_STATE, "mdh_diag_segments: the bound reads the scene table in LDS (MDH_OPT_TABLE_RESIDENCY 0 only)");
   if (thr_lim_out) {
      const int32_t *H = (const int32_t *)r->table_host.data();
      thr_lim_out[0] = i_as_f(H[H_VCLEAR]);
      thr_lim_out[1] = i_as_f(H[H_VCLEAR_LIM]);
   }
   if (n == 0) return MDH_OK;
   const bool room = variant == 0 && room_census(r);
   float *d = nullptr;
   HIP_TRY(hipMalloc(&d, (size_t)n * 9 * sizeof(float)));
   DiagSegArgs a;
   a.n = n;
   a.A = d; a.vd = d + 3 * (size_t)n; a.vmax = d + 6 * (size_t)n;
   a.clear = (int *)(d + 7 * (size_t)n); a.vis = d + 8 * (size_t)n;
   hipError_t e = hipMemcpyAsync(d, A, (size_t)n * 12, hipMemcpyHostToDevice, qs);
   if (e == hipSuccess) e = hipMemcpyAsync(d + 3 * (size_t)n, vd, (size_t)n * 12, hipMemcpyHostToDevice, qs);
   if (e == hipSuccess) e = hipMemcpyAsync(d + 6 * (size_t)n, vmax, (size_t)n * 4, hipMemcpyHostToDevice, qs);
   if (e == hipSuccess && (rc = table_acquire(r, qs)) == MDH_OK) {
      PassKernel k;
      k.family = GK_k_diag_segments;
      k.pf = room ? MDH_PF_ROOM : 0;
      rc = launch_kernel_ptr(kernel_ptr(k), dim3((n + 63) / 64), dim3(64), lds_bytes(r), qs, r->ks, a);
      e = hipGetLastError();
      if (e == hipSuccess && rc == MDH_OK) rc = table_release(r, qs);
   }
   if (e == hipSuccess && rc == MDH_OK) e = hipMemcpyAsync(clear_out, a.clear, (size_t)n * 4, hipMemcpyDeviceToHost, qs);
   if (e == hipSuccess && rc == MDH_OK) e = hipMemcpyAsync(vis_out, a.vis, (size_t)n * 4, hipMemcpyDeviceToHost, qs);
   const hipError_t es = hipStreamSynchronize(qs);
   if (e == hipSuccess) e = es;
   const hipError_t ef = hipFree(d);
   if (e == hipSuccess) e = ef;
   HIP_TRY(e);
   return rc;
}
// debug: read and reset the lane-utilisation counters of mdh_march.h
extern "C" int32_t mdh_diag_read(unsigned long long *out16)
{
   if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_diag), sizeof(unsigned long long) * 16) != hipSuccess) return MDH_E_DEVICE;
   unsigned long long z[16] = {0};
   if (hipMemcpyToSymbol(HIP_SYMBOL(g_diag), z, sizeof z) != hipSuccess) return MDH_E_DEVICE;
   return MDH_OK;
}
// read and reset the count of wavefront-points that fetched their eight irradiance taps once (MDH_SHARE_TAPS, mdh_march.h),
// over every launch since the last call; waits for the device
extern "C" int32_t mdh_diag_shared_taps(unsigned long long *out1)
{
   if (!out1) return MDH_E_INVALID;
   if (hipDeviceSynchronize() != hipSuccess) return MDH_E_DEVICE;
   if (hipMemcpyFromSymbol(out1, HIP_SYMBOL(g_shared_taps), sizeof(unsigned long long)) != hipSuccess) return MDH_E_DEVICE;
   const unsigned long long z = 0;
   if (hipMemcpyToSymbol(HIP_SYMBOL(g_shared_taps), &z, sizeof z) != hipSuccess) return MDH_E_DEVICE;
   return MDH_OK;
}
#endif
#ifdef MDH_PHASES
extern "C" int32_t mdh_diag_phases(unsigned long long *out16)
{
   if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 16) != hipSuccess) return MDH_E_DEVICE;
   unsigned long long z[16] = {0};
   if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof z) != hipSuccess) return MDH_E_DEVICE;
   return MDH_OK;
}
#endif
#ifdef MDH_TIMELINE
// debug: the wave timeline of the last k_radiance launch (3 words per wave)
extern "C" int32_t mdh_diag_waves(unsigned long long *out, int32_t n_waves)
{
   if (n_waves > MDH_DIAG_WAVES) n_waves = MDH_DIAG_WAVES;
   if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_t), sizeof(unsigned long long) * 3 * n_waves) != hipSuccess) return MDH_E_DEVICE;
   return MDH_OK;
}
#endif

// ------------------------------------------------------------------ the kernels of this library
// (the last function of the file: see the declaration of kernel_ptr).  Exactly the instantiations that are built, in the
// order the code object holds them; a description that names none of them is an error of the caller, never another kernel.
// (k_screen<16, 2>, <6, 0> and <7, 0> are built and never picked: the census of the rooms has no mode-2 variant of its own and
//  scenes with user-defined kinds get the power-of-two addressing from hiprtc only -- pick_kernel)
static const void *kernel_ptr_path(const PassKernel &k);
static const void *kernel_ptr_inscatter(const PassKernel &k);
static const void *kernel_ptr_sweep(const PassKernel &k);
static const void *kernel_ptr_surface(const PassKernel &k);
static const void *kernel_ptr_path_frame(const PassKernel &k);
static const void *kernel_ptr_path_adaptive(const PassKernel &k);
static const void *kernel_ptr(const PassKernel &k)
{
   if (k.family >= GK_k_path_frame_adaptive && k.family <= GK_k_path_frame_resolve_adaptive) return kernel_ptr_path_adaptive(k);
   if (k.family >= GK_k_path_frame && k.family <= GK_k_path_frame_resolve) return kernel_ptr_path_frame(k);
   if (k.family >= GK_k_surface_field && k.family <= GK_k_surface_vertices_listed) return kernel_ptr_surface(k);
   if (k.family == GK_k_listed || ((k.family == GK_k_ray_query || k.family == GK_k_ray_stream) && k.what >= MDH_RQ_SPHERECAST)) return kernel_ptr_sweep(k);
   if (k.family == GK_k_path_trace) return kernel_ptr_path(k); // (the newer families, named behind this function)
   if (k.family == GK_k_point_inscatter || k.family == GK_k_ray_inscatter) return kernel_ptr_inscatter(k);
#define MDH_K(FAMILY, PF, ...) if (k.family == GK_##FAMILY && k.pf == (PF)) return (const void *)(__VA_ARGS__);
#define MDH_RAD(PF) if (k.family == GK_k_radiance && k.pf == (PF) && k.rec == 0) return (const void *)(k.small ? k_radiance<PF, true> : k_radiance<PF, false>);
// (MDH_OPT_RADIANCE_REPLAY: the recording and the replaying kernel of a variant, behind everything older)
#define MDH_RAD_REC(PF) if (k.family == GK_k_radiance && k.pf == (PF) && k.rec == 1) return (const void *)(k.small ? k_radiance<PF, true, 1> : k_radiance<PF, false, 1>); \
                        if (k.family == GK_k_radiance && k.pf == (PF) && k.rec == 2) return (const void *)(k.small ? k_radiance<PF, true, 2> : k_radiance<PF, false, 2>);
// (MDH_OPT_SCREEN_REPLAY: the recording and the replaying kernel of a fixed-mode variant, behind everything older)
#define MDH_SCR_REC(PF) if (k.family == GK_k_screen && k.pf == (PF) && k.mode == 0 && !k.alt && k.rec == 1) return k.gbuf ? (const void *)k_screen<PF, 0, true, false, 1> : (const void *)k_screen<PF, 0, false, false, 1>; \
                        if (k.family == GK_k_screen && k.pf == (PF) && k.mode == 0 && !k.alt && k.rec == 2) return k.gbuf ? (const void *)k_screen<PF, 0, true, false, 2> : (const void *)k_screen<PF, 0, false, false, 2>;
#define MDH_VIS(PF) MDH_K(k_visibility, PF, k_visibility<PF>)
#if MDH_SCAT_SPLIT
#define MDH_SCAT(PF) MDH_K(k_scat_march, PF, k_scat_march<PF>)
#else
#define MDH_SCAT(PF) MDH_K(k_scattering, PF, k_scattering<PF>)
#endif
#define MDH_SCR(PF, MODE, ALT) if (k.family == GK_k_screen && k.pf == (PF) && k.mode == MODE && k.alt == ALT && k.rec == 0) return k.gbuf ? (const void *)k_screen<PF, MODE, true, ALT> : (const void *)k_screen<PF, MODE, false, ALT>;
#define MDH_RQ(PF) if (k.family == GK_k_ray_query && k.pf == (PF)) return k.what == MDH_RQ_RAYCAST ? (const void *)k_ray_query<PF, MDH_RQ_RAYCAST> : k.what == MDH_RQ_VISIBILITY ? (const void *)k_ray_query<PF, MDH_RQ_VISIBILITY> : (const void *)k_ray_query<PF, MDH_RQ_SOFTSHADOW>;
#define MDH_RS(PF) if (k.family == GK_k_ray_stream && k.pf == (PF)) return k.what == MDH_RQ_RAYCAST ? (const void *)k_ray_stream<PF, MDH_RQ_RAYCAST> : k.what == MDH_RQ_VISIBILITY ? (const void *)k_ray_stream<PF, MDH_RQ_VISIBILITY> : (const void *)k_ray_stream<PF, MDH_RQ_SOFTSHADOW>;
#define MDH_SH(PF) if (k.family == GK_k_ray_shade && k.pf == (PF) && (k.mode == 0 || k.mode == 2)) return k.mode == 0 ? (const void *)k_ray_shade<PF, 0> : (const void *)k_ray_shade<PF, 2>;
#define MDH_PT(PF) if (k.family == GK_k_point_shade && k.pf == (PF) && (k.mode == 0 || k.mode == 2 || k.mode == 3)) return k.mode == 0 ? (const void *)k_point_shade<PF, 0> : k.mode == 2 ? (const void *)k_point_shade<PF, 2> : (const void *)k_point_shade<PF, 3>;
#define MDH_GTAB(PF) MDH_VIS(PF) MDH_SCAT(PF) MDH_RAD(PF) MDH_SCR(PF, 0, true) MDH_SCR(PF, 0, false) MDH_SCR(PF, 1, false) MDH_SCR(PF, 2, false)
   MDH_RAD(13) MDH_RAD(37) MDH_RAD(5) MDH_RAD(20) MDH_RAD(4) MDH_RAD(16) MDH_RAD(33) MDH_RAD(0) MDH_RAD(1) MDH_RAD(2) MDH_RAD(9) MDH_RAD(3)
   MDH_VIS(0) MDH_VIS(16) MDH_VIS(33) MDH_VIS(1) MDH_VIS(2) MDH_VIS(9) MDH_VIS(3)
   MDH_SCAT(0) MDH_SCAT(16) MDH_SCAT(33) MDH_SCAT(1) MDH_SCAT(2) MDH_SCAT(9) MDH_SCAT(3)
   MDH_SCR(20, 0, false) MDH_SCR(16, 0, false) MDH_SCR(16, 2, false) MDH_SCR(0, 0, true) MDH_SCR(4, 0, false) MDH_SCR(0, 0, false) MDH_SCR(0, 1, false) MDH_SCR(0, 2, false)
   MDH_SCR(37, 0, false) MDH_SCR(33, 0, false) MDH_SCR(33, 2, false) MDH_SCR(1, 0, true) MDH_SCR(5, 0, false) MDH_SCR(1, 0, false) MDH_SCR(1, 1, false) MDH_SCR(1, 2, false)
   MDH_SCR(6, 0, false) MDH_SCR(2, 0, false) MDH_SCR(2, 2, false) MDH_SCR(2, 0, true) MDH_SCR(2, 1, false)
   MDH_SCR(13, 0, false) MDH_SCR(9, 0, false) MDH_SCR(9, 2, false) MDH_SCR(9, 0, true) MDH_SCR(9, 1, false)
   MDH_SCR(7, 0, false) MDH_SCR(3, 0, false) MDH_SCR(3, 2, false) MDH_SCR(3, 0, true) MDH_SCR(3, 1, false)
   MDH_K(k_partition_build, 0, k_partition_build)
   MDH_K(k_eval_distance, 0, k.ada_div ? k_eval_distance<true> : k_eval_distance<false>)
#ifdef MDH_DIAG
   MDH_K(k_diag_segments, MDH_PF_ROOM, k_diag_segments<MDH_PF_ROOM>) MDH_K(k_diag_segments, 0, k_diag_segments<0>)
#endif
   MDH_GTAB(65)
   MDH_K(k_partition_build, MDH_PF_GTAB, k_partition_build_gtab<>)
   MDH_K(k_eval_distance, MDH_PF_GTAB, k.ada_div ? k_eval_distance_gtab<true> : k_eval_distance_gtab<false>)
   MDH_GTAB(73) MDH_GTAB(64)
   MDH_GTAB(192) // MDH_PF_GTAB | MDH_PF_BVH: the newest last, so that nothing older moves
   MDH_K(k_eval_distance, MDH_PF_GTAB | MDH_PF_BVH, k_eval_distance_bvh<>)
#if MDH_RAD_REPLAY_BUILT
   MDH_RAD_REC(20) MDH_RAD_REC(16) MDH_RAD_REC(4) MDH_RAD_REC(0)
#endif
#if MDH_SCR_REPLAY_BUILT
   MDH_SCR_REC(20) MDH_SCR_REC(16) MDH_SCR_REC(4) MDH_SCR_REC(0)
#endif
   // the ray queries (mdh_raycast, ..): the newest last, behind everything older.  The scan, the partition with either border,
   // global residency alone, with the partition, with the triangle BVH
   MDH_RQ(0) MDH_RQ(1) MDH_RQ(9) MDH_RQ(64) MDH_RQ(65) MDH_RQ(73) MDH_RQ(192)
   // ... and the same queries for device arrays, whose lanes take the next ray when theirs has ended (mdh_raycast_device, ..): behind them
   MDH_RS(0) MDH_RS(1) MDH_RS(9) MDH_RS(64) MDH_RS(65) MDH_RS(73) MDH_RS(192)
   // ... and the pixel program for a host's rays (mdh_shade_rays, mdh_shade_rays_device; mode 0 or 2) with the kernel that hands
   // out the camera's rays (mdh_camera_rays): the newest last
   MDH_SH(0) MDH_SH(1) MDH_SH(9) MDH_SH(64) MDH_SH(65) MDH_SH(73) MDH_SH(192)
   MDH_K(k_camera_rays, 0, k_camera_rays<>)
   // ... and the light at a host's own points (mdh_shade_points, mdh_shade_points_device; mode 0, 2 or 3): behind everything older
   MDH_PT(0) MDH_PT(1) MDH_PT(9) MDH_PT(64) MDH_PT(65) MDH_PT(73) MDH_PT(192)
   return nullptr;
#undef MDH_K
#undef MDH_RAD
#undef MDH_RAD_REC
#undef MDH_SCR_REC
#undef MDH_VIS
#undef MDH_SCAT
#undef MDH_SCR
#undef MDH_GTAB
#undef MDH_RQ
#undef MDH_RS
#undef MDH_SH
#undef MDH_PT
}
// ... and the path tracer along a host's rays (mdh_path_trace, mdh_path_trace_device), the newest family: kernel_ptr hands its
// descriptions on to this function, which is defined behind it, so that k_path_trace is first named behind every other kernel
// and the code object keeps the order of everything older
static const void *kernel_ptr_path(const PassKernel &k)
{
#define MDH_PATH(PF) if (k.pf == (PF)) return (const void *)k_path_trace<PF>;
   MDH_PATH(0) MDH_PATH(1) MDH_PATH(9) MDH_PATH(64) MDH_PATH(65) MDH_PATH(73) MDH_PATH(192)
   return nullptr;
#undef MDH_PATH
}
// ... and behind it the lights' fog at a host's points and along its rays (mdh_inscatter_points, mdh_inscatter_rays and their
// _device forms), in the same way: the newest kernels last, nothing older moves
static const void *kernel_ptr_inscatter(const PassKernel &k)
{
#define MDH_INS(PF) if (k.pf == (PF)) return k.family == GK_k_point_inscatter ? (const void *)k_point_inscatter<PF> : (const void *)k_ray_inscatter<PF>;
   MDH_INS(0) MDH_INS(1) MDH_INS(9) MDH_INS(64) MDH_INS(65) MDH_INS(73) MDH_INS(192)
   return nullptr;
#undef MDH_INS
}
// ... and behind that the swept spheres and contacts (mdh_spherecast, mdh_contacts and their _device forms): the new WHAT
// values of k_ray_query and k_ray_stream and the scan of listed kinds, first named here, behind every older kernel
static const void *kernel_ptr_sweep(const PassKernel &k)
{
#define MDH_SW(PF) if (k.pf == (PF)) { \
      if (k.family == GK_k_ray_query) return k.what == MDH_RQ_SPHERECAST ? (const void *)k_ray_query<PF, MDH_RQ_SPHERECAST> : k.what == MDH_RQ_CONTACT ? (const void *)k_ray_query<PF, MDH_RQ_CONTACT> : nullptr; \
      if (k.family == GK_k_ray_stream) return k.what == MDH_RQ_SPHERECAST ? (const void *)k_ray_stream<PF, MDH_RQ_SPHERECAST> : nullptr; }
   MDH_SW(0) MDH_SW(1) MDH_SW(9) MDH_SW(64) MDH_SW(65) MDH_SW(73) MDH_SW(192)
#undef MDH_SW
   if (k.family == GK_k_listed && (k.what == MDH_RQ_SPHERECAST || k.what == MDH_RQ_CONTACT)) {
      if (k.pf == 0) return k.what == MDH_RQ_SPHERECAST ? (const void *)k_listed<false, MDH_RQ_SPHERECAST> : (const void *)k_listed<false, MDH_RQ_CONTACT>;
      if (k.pf == MDH_PF_GTAB) return k.what == MDH_RQ_SPHERECAST ? (const void *)k_listed<true, MDH_RQ_SPHERECAST> : (const void *)k_listed<true, MDH_RQ_CONTACT>;
   }
   return nullptr;
}
// ... and behind that the surface mesher (mdh_surface_mesh, mdh_surface_mesh_device; mdh_surface.h): the field and the vertices
// in the queries' variants and over listed kinds, first named here; its three kernels that read no scene have no variants
static const void *kernel_ptr_surface(const PassKernel &k)
{
#define MDH_SF(PF) if (k.pf == (PF)) { \
      if (k.family == GK_k_surface_field) return (const void *)k_surface_field<PF>; \
      if (k.family == GK_k_surface_vertices) return (const void *)k_surface_vertices<PF>; }
   MDH_SF(0) MDH_SF(1) MDH_SF(9) MDH_SF(64) MDH_SF(65) MDH_SF(73) MDH_SF(192)
#undef MDH_SF
   if (k.family == GK_k_surface_field_listed) return k.pf == 0 ? (const void *)k_surface_field_listed<false> : k.pf == MDH_PF_GTAB ? (const void *)k_surface_field_listed<true> : nullptr;
   if (k.family == GK_k_surface_vertices_listed) return k.pf == 0 ? (const void *)k_surface_vertices_listed<false> : k.pf == MDH_PF_GTAB ? (const void *)k_surface_vertices_listed<true> : nullptr;
   return nullptr;
}
// ... and behind that a path-traced frame (mdh_path_frame_accumulate, .._rays, .._read; mdh_path_frame.h): k_path_trace's estimator
// over a captured camera's pixels in the queries' variants, with and without the recorded primary segment, first named here;
// the kernels of the rays and of the resolve read no scene and have no variants
static const void *kernel_ptr_path_frame(const PassKernel &k)
{
#define MDH_PFR(PF) if (k.family == GK_k_path_frame && k.pf == (PF)) return k.what ? (const void *)k_path_frame<PF, true> : (const void *)k_path_frame<PF, false>;
   MDH_PFR(0) MDH_PFR(1) MDH_PFR(9) MDH_PFR(64) MDH_PFR(65) MDH_PFR(73) MDH_PFR(192)
#undef MDH_PFR
   if (k.family == GK_k_path_frame_rays) return (const void *)k_path_frame_rays<>;
   if (k.family == GK_k_path_frame_resolve) return (const void *)k_path_frame_resolve<>;
   return nullptr;
}
// ... and behind that an adaptive path-traced frame (mdh_path_frame_begin_adaptive; mdh_path_frame_adaptive.h): the estimator with a count
// and two moments a pixel in the queries' variants, first named here; the kernels of a round's list, of the statistics and of
// the resolve read no scene and have no variants
static const void *kernel_ptr_path_adaptive(const PassKernel &k)
{
#define MDH_PFA(PF) if (k.family == GK_k_path_frame_adaptive && k.pf == (PF)) return (const void *)k_path_frame_adaptive<PF>;
   MDH_PFA(0) MDH_PFA(1) MDH_PFA(9) MDH_PFA(64) MDH_PFA(65) MDH_PFA(73) MDH_PFA(192)
#undef MDH_PFA
   if (k.family == GK_k_path_adapt_count) return (const void *)k_path_adapt_count<>;
   if (k.family == GK_k_path_adapt_scan) return (const void *)k_path_adapt_scan<>;
   if (k.family == GK_k_path_adapt_compact) return k.what ? (const void *)k_path_adapt_compact<true> : (const void *)k_path_adapt_compact<false>;
   if (k.family == GK_k_path_adapt_stats) return (const void *)k_path_adapt_stats<>;
   if (k.family == GK_k_path_frame_resolve_adaptive) return (const void *)k_path_frame_resolve_adaptive<>;
   return nullptr;
}
