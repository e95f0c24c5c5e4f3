// mdh_path_frame.h -- a path-traced FRAME on the device (mdh_path_frame_begin, .._accumulate, .._read, .._rays; mdh_api.hip): the
// estimator of k_path_trace (mdh_kernels.h) over the pixels of a W x H frame of a captured camera, with the sums kept in the
// renderer's own memory from call to call, sub-pixel jitter, the primary segment evaluated once where it cannot change, and
// the resolve.  Included by mdh_kernels.h behind mdh_surface.h, outside the hiprtc build; the functions of a pixel's screen
// position are mdh_path.h's (path_pixel_uv), which the host calls too (mdh_path_pixel_uv).
//
// THE PIXEL'S RAY.  Pixel (i, j), row 0 at the top, has ray id j W + i: the numbering of mdh_camera_rays with id_first = 0.
// path_frame_ray is path_pixel_uv followed by camera_ray -- without jitter tile_pixel's centre, k_camera_rays' rays to the bit.
//
// k_path_frame<PART, REUSE>.  PART is the scene's general variant, as in k_path_trace.  A wavefront takes an 8 x 8 tile as
// k_screen does (lane = (y & 7) * 8 + (x & 7)), not a row of 64: neighbouring pixels' paths stay together for longer.  Tiles
// cut by the right and bottom edges run with their outside lanes gone behind stage_table's barrier, the kernel's only one.
// A lane runs the sequence of operations it would run alone -- march_plain, sdf_info / primitive_info, path_direct, the mask,
// from_off, path_scatter_at, acc = acc + rgb per sample in sample order, the flat loop over segments -- so no bit depends on
// the mapping, and the sums are k_path_trace's over the same rays.
//   REUSE = false: every sample forms its primary ray at its start from the camera in the kernel's arguments -- with jitter
//         its own, without (a launch of one sample, where there is nothing to reuse: mdh_path_frame_accumulate) the pixel's
//         centre; nothing of it stays live but the direction the path arrives along.
//   REUSE = true (no jitter, more than one sample): the primary ray is the same in every sample, and so are its march, its sdf_info /
//         primitive_info and path_direct at its hit -- deterministic functions of the ray and the scene.  The lane evaluates them
//         the first time a sample of the launch starts and records what the segment hands on: whether it hit, what it adds
//         (path_direct's light, or the sky), the normal, the shifted origin, the material.  Every later sample starts from the
//         record and applies the same operations to the same values: the bits of marching again.  Twelve values stay live;
//         a template flag, not a run-time branch, so that the jittered kernel does not carry them.
// A ray that fails path_ray_valid is not marched: its pixel's sums become the quiet NaN 0x7fc00000, whatever they held.
//
// k_path_frame_rays, k_path_frame_resolve: a pixel per lane, no scene, no variants.  The resolve: rgb = sum / (float) S, one
// binary32 division a channel; tone_map: draw_screen.glsl:29 with k_ray_shade's operations; rgba8: pack_rgba8 of (that colour,
// 1), as k_present converts a framebuffer pixel (a NaN shows as 0).
#pragma once

struct PathFrameArgs {
   int W, H;
   int tiles_x, n_tiles;     // 8 x 8 tiles of the whole frame
   int bounces;              // 0 .. MDH_PATH_MAX_BOUNCES
   unsigned seed;
   int jitter;               // 0 / 1 (REUSE: 0)
   int sample_first, sample_count;
   float *sums;              // 3 W H, in and out, row-major, rows top first
};
MDH_DEV void path_frame_ray(const KCamera &cam, int i, int j, int W, int H, unsigned seed, unsigned sample, bool jitter, f3 &origin, f3 &dir)
{
   float u, v;
   path_pixel_uv(i, j, W, H, seed, sample, jitter, u, v);
   camera_ray(cam, u, v, origin, dir);
}
template <int PART, bool REUSE> __global__ __launch_bounds__(MDH_BLOCK) void k_path_frame(KScene sc, KCamera cam, PathFrameArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "ray queries: the general variants of built-in kinds");
   stage_table(sc); // (the kernel's only barrier: wavefronts past the last tile and lanes outside the frame leave behind it)
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
   const int tile = blockIdx.x * (MDH_BLOCK / 64) + wave;
   if (tile >= a.n_tiles) return; // wave-uniform
   const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
   const int i = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
   if (i >= a.W || j >= a.H) return; // a cut tile's outside lanes
   const size_t q = (size_t)j * (size_t)a.W + (size_t)i;
   const unsigned id = (unsigned)q;
   const float bad = __uint_as_float(MDH_RS_BAD_BITS);
   f3 acc = F3(a.sums[3 * q], a.sums[3 * q + 1], a.sums[3 * q + 2]);
   // the lane's path: its sample, the bounce of its next segment, the ray of that segment, what it has gathered
   int sample = a.sample_first, bounce = 0;
   const int sample_end = a.sample_first + a.sample_count;
   f3 ro, rd, mask = F3(1.0f, 1.0f, 1.0f), rgb = F3(0.0f, 0.0f, 0.0f);
   bool fresh = true; // the next segment is a sample's first: its ray is formed first
   // REUSE: the primary segment's record
   bool p_known = false, p_hit = false;
   int p_pm = 0;
   f3 p_add = F3(0.0f, 0.0f, 0.0f), p_N = F3(0.0f, 0.0f, 0.0f), p_from = F3(0.0f, 0.0f, 0.0f), p_dir = F3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
   while (sample < sample_end) { // one segment per iteration
      if (fresh && !(REUSE && p_known)) {
         path_frame_ray(cam, i, j, a.W, a.H, a.seed, (unsigned)sample, !REUSE && a.jitter != 0, ro, rd);
         if (!path_ray_valid(ro.x, ro.y, ro.z, rd.x, rd.y, rd.z)) { // not traced
            acc = F3(bad, bad, bad);
            break;
         }
         if (REUSE) p_dir = rd;
      }
      bool h;
      f3 add, N, from_off;
      int pm;
      if (REUSE && fresh && p_known) { // the recorded primary segment
         h = p_hit; add = p_add; N = p_N; from_off = p_from; pm = p_pm;
         rd = p_dir;
      } else {
         float t;
         int steps;
         h = march_plain<PART>(sc, ro, rd, sc.max_dist, t, steps);
         N = F3(0.0f, 0.0f, 0.0f); from_off = N; pm = 0;
         if (!h) { // render_probes.glsl:287
            const float s = rd.y * 0.7f;
            add = F3(0.30f - s, 0.36f - s, 0.60f - s);
         } else {
            const f3 P = ro + rd * t;
            int index = -1;
            (void)sdf_info<PART>(sc, P, index);
            primitive_info<false, (PART & MDH_PF_GTAB) != 0>(sc, index, P, N, pm);
            from_off = P + (N * MDH_MIN_STEP) * 5.0f;
            add = path_direct<PART>(sc, P, N, from_off, rd, get_material(sc, pm));
         }
         if (REUSE && fresh) { p_known = true; p_hit = h; p_add = add; p_N = N; p_from = from_off; p_pm = pm; }
      }
      fresh = false;
      rgb = rgb + mask * add;
      bool ended = true;
      if (h) {
         const Material m = get_material(sc, pm);
         mask = mask * m.albedo;
         if (bounce < a.bounces) {
            const float dv[3] = {rd.x, rd.y, rd.z}, nv[3] = {N.x, N.y, N.z};
            float out[3];
            path_scatter_at(dv, nv, m.roughness, a.seed, id, (unsigned)sample, (unsigned)bounce, out);
            if (path_dir_finite(out[0], out[1], out[2])) {
               ro = from_off;
               rd = F3(out[0], out[1], out[2]);
               ++bounce;
               ended = false;
            }
         }
      }
      if (ended) { // the sample is complete: the next one starts at its primary ray
         acc = acc + rgb;
         ++sample;
         bounce = 0;
         fresh = true;
         mask = F3(1.0f, 1.0f, 1.0f); rgb = F3(0.0f, 0.0f, 0.0f);
      }
   }
   a.sums[3 * q] = acc.x; a.sums[3 * q + 1] = acc.y; a.sums[3 * q + 2] = acc.z;
}

// mdh_path_frame_rays, mdh_path_frame_rays_device: the rays the accumulator gives its pixels for one sample
struct PathFrameRayArgs {
   int W, H;
   unsigned seed;
   int sample, jitter;
   float *org, *dir; // 3 W H each
};
template <int = 0> __global__ __launch_bounds__(256) void k_path_frame_rays(KCamera cam, PathFrameRayArgs a) // (a template: built where it is first named, mdh_api.hip: kernel_ptr_path_frame)
{
   const long lin = (long)blockIdx.x * 256 + threadIdx.x;
   if (lin >= (long)a.W * a.H) return;
   const int j = (int)(lin / a.W), i = (int)(lin - (long)j * a.W);
   f3 origin, dir;
   path_frame_ray(cam, i, j, a.W, a.H, a.seed, (unsigned)a.sample, a.jitter != 0, origin, dir);
   const size_t q = (size_t)lin;
   a.org[3 * q] = origin.x; a.org[3 * q + 1] = origin.y; a.org[3 * q + 2] = origin.z;
   a.dir[3 * q] = dir.x; a.dir[3 * q + 1] = dir.y; a.dir[3 * q + 2] = dir.z;
}

// mdh_path_frame_read, mdh_path_frame_read_device: the resolve
struct PathFrameResolveArgs {
   int n;             // W H
   int samples;       // S >= 1
   int tone_map;
   const float *sums; // 3 n
   float *rgb;        // 3 n, or null
   unsigned *rgba8;   // n, or null
   float *sums_out;   // 3 n, or null: the raw sums
};
template <int = 0> __global__ __launch_bounds__(256) void k_path_frame_resolve(PathFrameResolveArgs a)
{
   const long lin = (long)blockIdx.x * 256 + threadIdx.x;
   if (lin >= (long)a.n) return;
   const size_t q = (size_t)lin;
   const f3 s = F3(a.sums[3 * q], a.sums[3 * q + 1], a.sums[3 * q + 2]);
   if (a.sums_out) { a.sums_out[3 * q] = s.x; a.sums_out[3 * q + 1] = s.y; a.sums_out[3 * q + 2] = s.z; }
   if (!a.rgb && !a.rgba8) return;
   const float count = (float)a.samples;
   f3 c = F3(s.x / count, s.y / count, s.z / count);
   if (a.tone_map) // draw_screen.glsl:29
      c = F3(spow(sdiv(c.x, c.x + 1.0f), 0.4545f), spow(sdiv(c.y, c.y + 1.0f), 0.4545f), spow(sdiv(c.z, c.z + 1.0f), 0.4545f));
   if (a.rgb) { a.rgb[3 * q] = c.x; a.rgb[3 * q + 1] = c.y; a.rgb[3 * q + 2] = c.z; }
   if (a.rgba8) a.rgba8[q] = pack_rgba8(make_float4(c.x, c.y, c.z, 1.0f));
}
