// mdh_path_frame_adaptive.h -- an ADAPTIVE path-traced frame on the device (mdh_path_frame_begin_adaptive, mdh_path_frame_accumulate on such
// a frame, mdh_path_frame_stats; mdh_api.hip): the accumulator of mdh_path_frame.h with a count n and two moments m1, m2 a pixel, the
// stopping rule of mdh_path.h (path_pixel_active, which the host calls too: mdh_path_pixel_active) evaluated where a round
// starts, and a deterministic compaction of the pixels still running.  Included by mdh_kernels.h behind mdh_path_frame.h,
// outside the hiprtc build.
//
// SLOTS.  A pixel's slot is tile * 64 + lane, the 8 x 8 tile numbering of k_path_frame (lane = (y & 7) * 8 + (x & 7)); the
// slots of a cut tile that lie outside the frame are never active.  A workgroup of the first three kernels handles 256
// consecutive slots: four tiles, a wavefront a tile.
//
// A ROUND (mdh_path_frame_accumulate) is four launches on the query stream, no atomics anywhere:
//   k_path_adapt_count     every slot evaluates path_pixel_active from the state; ballot, popcount, the workgroup's total through LDS
//   k_path_adapt_scan      one workgroup: the totals become their exclusive scan in place, the grand total goes to wg[nblocks]
//   k_path_adapt_compact   an active slot's place = its workgroup's base + the wavefronts before it + mbcnt of the ballot;
//                          list[place] = pixel id.  COMPACT = false (MDH_OPT_PATH_FRAME_COMPACT 0, the default): list[slot] = pixel id, or -1
//                          for a retired or outside slot -- a retired pixel keeps its lane and idles
//   k_path_frame_adaptive  lane g takes list[g], loads its pixel's state, runs min (sample_count, max_samples - n) samples with
//                          the body of k_path_frame<PART, false> operation for operation, the sample index being the pixel's
//                          OWN count (pixel id with count n holds samples 0 .. n - 1 of (seed, id)), and updates acc, m1, m2
//                          and n per completed sample (path_pixel_update), then stores
// A slot's place is a function of the state alone, so the list keeps slot order -- neighbours in space stay neighbours in a
// wavefront -- and no bit depends on the mapping: both values of the option give the same state.  The host does not know
// the active count and never waits for it: the estimator's grid is sized for all slots, and a workgroup whose first lane is at
// or beyond the count leaves BEFORE stage_table's barrier -- workgroup-uniform: the count is one word every thread reads --,
// so an empty workgroup stages nothing.  No recorded primary segment (no REUSE form): with the pixel's own sample index
// a launch's samples differ from pixel to pixel, and the record's twelve registers were measured not to pay.
// A pixel whose ray fails path_ray_valid is not marched: its sums, m1 and m2 become the quiet NaN 0x7fc00000, n stays, and the
// rule retires it.
//
// k_path_adapt_stats: one workgroup; the pixels active under the rule now and the sum of n, as two 64-bit words, summed in a
// fixed order.  A SERIAL PASS: a thread walks W H / 256 pixels (8 100 at 1080p) and thread 0 adds the 256 partial sums -- a
// diagnostic, not a step of a round; a host that asks every round pays it every round (the header says so).  k_path_frame_resolve_adaptive: k_path_frame_resolve with rgb = sum / (float) n of the pixel.
#pragma once

struct PathAdaptArgs {
   int W, H;
   int tiles_x, n_tiles;    // 8 x 8 tiles of the whole frame
   int n_slots, nblocks;    // 64 n_tiles, and the workgroups of 256 slots
   int bounces;
   unsigned seed;
   int jitter;
   int sample_count;        // of this round
   int min_samples, max_samples;
   float tolerance, floor;
   int compact;             // MDH_OPT_PATH_FRAME_COMPACT
   float *sums;             // 3 W H
   int *count;              // W H
   float *moments;          // 2 W H: (m1, m2) a pixel
   int *list;               // n_slots
   int *wg;                 // nblocks + 1: the workgroups' totals, then their scan; wg[nblocks]: the grand total
   long long *active_out, *total_out; // k_path_adapt_stats: either may be null
};
// the pixel of a slot, or -1 outside the frame
MDH_DEV int path_adapt_pixel(const PathAdaptArgs &a, int slot)
{
   if (slot >= a.n_slots) return -1;
   const int tile = slot >> 6, lane = slot & 63;
   const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
   const int i = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
   return i < a.W && j < a.H ? j * a.W + i : -1; // (below 2^26)
}
MDH_DEV bool path_adapt_active(const PathAdaptArgs &a, int id)
{
   return id >= 0 && path_pixel_active(a.count[id], a.moments[2 * (size_t)id], a.moments[2 * (size_t)id + 1], a.min_samples, a.max_samples, a.tolerance, a.floor);
}
template <int = 0> __global__ __launch_bounds__(MDH_BLOCK) void k_path_adapt_count(PathAdaptArgs a)
{
   __shared__ int s_wave[MDH_BLOCK / 64];
   const int slot = blockIdx.x * MDH_BLOCK + threadIdx.x; // (below 2^29 + 256: a frame one pixel wide has 2^23 tiles)
   const bool active = path_adapt_active(a, path_adapt_pixel(a, slot));
   const int mine = __popcll(__ballot(active));
   if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mine;
   __syncthreads();
   if (threadIdx.x == 0) {
      int total = 0;
      for (int w = 0; w < MDH_BLOCK / 64; ++w) total += s_wave[w];
      a.wg[blockIdx.x] = total;
   }
}
// one workgroup: a.wg[0 .. nblocks) becomes its exclusive scan, MDH_BLOCK entries a round with the carry of the rounds before
// (k_surface_scan's scheme, one row)
template <int = 0> __global__ __launch_bounds__(MDH_BLOCK) void k_path_adapt_scan(PathAdaptArgs a)
{
   __shared__ int s_wave[MDH_BLOCK / 64];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   int carry = 0;
   for (int base = 0; base < a.nblocks; base += MDH_BLOCK) { // (uniform: every thread runs every round)
      const int at = base + threadIdx.x;
      const int x = at < a.nblocks ? a.wg[at] : 0;
      int incl = x;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
         const int up = __shfl_up(incl, d, 64);
         if (lane >= d) incl += up;
      }
      if (lane == 63) s_wave[wave] = incl;
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < MDH_BLOCK / 64; ++w) { before += w < wave ? s_wave[w] : 0; total += s_wave[w]; }
      if (at < a.nblocks) a.wg[at] = carry + before + incl - x;
      carry += total;
      __syncthreads(); // (s_wave is rewritten by the next round)
   }
   if (threadIdx.x == 0) a.wg[a.nblocks] = carry;
}
template <bool COMPACT> __global__ __launch_bounds__(MDH_BLOCK) void k_path_adapt_compact(PathAdaptArgs a)
{
   __shared__ int s_wave[MDH_BLOCK / 64];
   const int slot = blockIdx.x * MDH_BLOCK + threadIdx.x;
   const int id = path_adapt_pixel(a, slot);
   const bool active = path_adapt_active(a, id);
   if (!COMPACT) {
      if (slot < a.n_slots) a.list[slot] = active ? id : -1;
      return;
   }
   const unsigned long long ballot = __ballot(active);
   const int before = surf_waves_before(s_wave, __popcll(ballot)); // (the kernel's only barrier; every thread comes through)
   if (active) a.list[a.wg[blockIdx.x] + before + surf_lanes_below(ballot)] = id; // (a place below the grand total <= n_slots)
}

template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_path_frame_adaptive(KScene sc, KCamera cam, PathAdaptArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "ray queries: the general variants of built-in kinds");
   // the listed pixels: all slots without compaction, the grand total with it -- one word, the same for every thread
   const int listed = a.compact ? __builtin_amdgcn_readfirstlane(a.wg[a.nblocks]) : a.n_slots;
   if ((int)(blockIdx.x * MDH_BLOCK) >= listed) return; // workgroup-uniform, before the barrier: an empty workgroup stages nothing
   stage_table(sc); // (the kernel's only barrier)
   const int g = blockIdx.x * MDH_BLOCK + threadIdx.x;
   if (g >= listed) return;
   const int pixel = a.list[g];
   if (pixel < 0) return; // (no compaction: a retired or outside slot idles)
   const int j = pixel / a.W, i = pixel - j * a.W;
   const size_t q = (size_t)pixel;
   const unsigned id = (unsigned)pixel;
   const float bad = __uint_as_float(MDH_RS_BAD_BITS);
   f3 acc = F3(a.sums[3 * q], a.sums[3 * q + 1], a.sums[3 * q + 2]);
   int n = a.count[q];
   float m1 = a.moments[2 * q], m2 = a.moments[2 * q + 1];
   // the lane's path, as in k_path_frame<PART, false>: the sample is the pixel's own count
   int bounce = 0;
   const int left = a.max_samples - n;
   const int sample_end = n + (a.sample_count < left ? a.sample_count : left);
   f3 ro, rd, mask = F3(1.0f, 1.0f, 1.0f), rgb = F3(0.0f, 0.0f, 0.0f);
   bool fresh = true;
#pragma unroll 1
   while (n < sample_end) { // one segment per iteration
      if (fresh) {
         path_frame_ray(cam, i, j, a.W, a.H, a.seed, (unsigned)n, a.jitter != 0, ro, rd);
         if (!path_ray_valid(ro.x, ro.y, ro.z, rd.x, rd.y, rd.z)) { // not traced: n stays, and the rule retires the pixel
            acc = F3(bad, bad, bad);
            m1 = bad; m2 = bad;
            break;
         }
      }
      float t;
      int steps;
      const bool h = march_plain<PART>(sc, ro, rd, sc.max_dist, t, steps);
      f3 add, N = F3(0.0f, 0.0f, 0.0f), from_off = N;
      int pm = 0;
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
      fresh = false;
      rgb = rgb + mask * add;
      bool ended = true;
      if (h) {
         const Material m = get_material(sc, pm);
         mask = mask * m.albedo;
         if (bounce < a.bounces) {
            const float dv[3] = {rd.x, rd.y, rd.z}, nv[3] = {N.x, N.y, N.z};
            float out[3];
            path_scatter_at(dv, nv, m.roughness, a.seed, id, (unsigned)n, (unsigned)bounce, out);
            if (path_dir_finite(out[0], out[1], out[2])) {
               ro = from_off;
               rd = F3(out[0], out[1], out[2]);
               ++bounce;
               ended = false;
            }
         }
      }
      if (ended) { // the sample is complete
         acc = acc + rgb;
         path_pixel_update(rgb.x, rgb.y, rgb.z, n, m1, m2);
         bounce = 0;
         fresh = true;
         mask = F3(1.0f, 1.0f, 1.0f); rgb = F3(0.0f, 0.0f, 0.0f);
      }
   }
   a.sums[3 * q] = acc.x; a.sums[3 * q + 1] = acc.y; a.sums[3 * q + 2] = acc.z;
   a.count[q] = n;
   a.moments[2 * q] = m1; a.moments[2 * q + 1] = m2;
}

// mdh_path_frame_stats: the pixels active now and the samples taken, in a fixed order (a thread's pixels, the lanes, the wavefronts)
template <int = 0> __global__ __launch_bounds__(MDH_BLOCK) void k_path_adapt_stats(PathAdaptArgs a)
{
   __shared__ long long s_active[MDH_BLOCK], s_total[MDH_BLOCK];
   long long active = 0, total = 0;
   const int np = a.W * a.H;
   for (int id = threadIdx.x; id < np; id += MDH_BLOCK) {
      active += path_adapt_active(a, id) ? 1 : 0;
      total += a.count[id];
   }
   s_active[threadIdx.x] = active; s_total[threadIdx.x] = total;
   __syncthreads();
   if (threadIdx.x == 0) {
      active = 0; total = 0;
      for (int t = 0; t < MDH_BLOCK; ++t) { active += s_active[t]; total += s_total[t]; }
      if (a.active_out) *a.active_out = active;
      if (a.total_out) *a.total_out = total;
   }
}

// the resolve of an adaptive frame: the pixel's own count
template <int = 0> __global__ __launch_bounds__(256) void k_path_frame_resolve_adaptive(PathFrameResolveArgs a, const int *count)
{
   const long lin = (long)blockIdx.x * 256 + threadIdx.x;
   if (lin >= (long)a.n) return;
   const size_t q = (size_t)lin;
   const f3 s = F3(a.sums[3 * q], a.sums[3 * q + 1], a.sums[3 * q + 2]);
   if (a.sums_out) { a.sums_out[3 * q] = s.x; a.sums_out[3 * q + 1] = s.y; a.sums_out[3 * q + 2] = s.z; }
   if (!a.rgb && !a.rgba8) return;
   const float c_n = (float)count[q];
   f3 c = F3(s.x / c_n, s.y / c_n, s.z / c_n);
   if (a.tone_map) // draw_screen.glsl:29
      c = F3(spow(sdiv(c.x, c.x + 1.0f), 0.4545f), spow(sdiv(c.y, c.y + 1.0f), 0.4545f), spow(sdiv(c.z, c.z + 1.0f), 0.4545f));
   if (a.rgb) { a.rgb[3 * q] = c.x; a.rgb[3 * q + 1] = c.y; a.rgb[3 * q + 2] = c.z; }
   if (a.rgba8) a.rgba8[q] = pack_rgba8(make_float4(c.x, c.y, c.z, 1.0f));
}
