// mdh_kernels.h -- the gfx950 kernels, one per pass of Renderers.Render
// (reference madarch/madarch-renderers.adb:302-321) plus the partition-table build
// and the batched distance query.  See mdh_device.h for the device functions and
// DESIGN.md for the launch shapes and the HBM layout.
#pragma once

#include "mdh_device.h"

#ifndef MDH_BLOCK
#define MDH_BLOCK 256 // 4 wavefronts; every wavefront owns one 8x8 tile
#endif

#include "mdh_march.h"
#define MDH_SHADE shade_structured
#ifdef MDH_PHASES
#define PH_KERNEL_BEGIN() float *pk = park_base(sc); if ((threadIdx.x & 63) < 32) ph_acc_(pk)[threadIdx.x & 63] = 0ull; PH_T0(pk_t)
#define PH_KERNEL_END() do { PH_ADD(pk_t, 11); if ((threadIdx.x & 63) < 16) atomicAdd(&g_phase[threadIdx.x & 63], ph_acc_(pk)[threadIdx.x & 63]); } while (0)
#else
#define PH_KERNEL_BEGIN() do { } while (0)
#define PH_KERNEL_END() do { } while (0)
#endif
#ifndef MDH_RAD_PROBES_PER_WAVE
#define MDH_RAD_PROBES_PER_WAVE 64 // 1, 4, 16 or 64 (measured on MI355X: see DESIGN.md)
#endif
// kernels of scenes with user-defined kinds carry the 64-register file of the MDH_X interpreter
// (not in a hiprtc build, where the programs are plain code)
// Mode 2 through the space partition (simple_scene: direct light + occlusion) waits for the partition's L2 round trips and
// has no probe code: more wavefronts per SIMD hide more of them (measured at 1080p with frames in flight: 5 -> 4 416,
// 6 -> 4 871, 7 -> 5 110 Mpixels/s; with the probe code of mode 0 the same scene LOSES at 6 and 7: ball_game 1 407 / 1 338 /
// 1 272).
#ifndef MDH_DIRECT_WAVES_PER_SIMD
#define MDH_DIRECT_WAVES_PER_SIMD 7
#endif
// Mode 0 through the space partition (the reference's simple_scene and ball_game as they run): its march steps wait for a
// cell's bits and three rounds of LDS gathers -- six wavefronts per SIMD measured +5 % / +3 % on those frames (four: -12 %).
#ifndef MDH_PART_WAVES_PER_SIMD
#define MDH_PART_WAVES_PER_SIMD 6
#endif
// The variants for the census of the reference's rooms (MDH_PF_ROOM) need 80 registers where the general scan needs 96: six
// wavefronts per SIMD without a further spill (measured at config 3: five 5 681 - 5 726, six 5 818 - 5 863 Mpixels/s in flight).
#ifndef MDH_ROOM_WAVES_PER_SIMD
#define MDH_ROOM_WAVES_PER_SIMD 6
#endif
// (mode 2 through the partition's census variant: 60 registers, eight wavefronts per SIMD without a further spill -- simple_scene
//  direct 8 743 -> 8 982 Mpixels/s in flight)
#ifndef MDH_PSMALL_DIRECT_WAVES_PER_SIMD
#define MDH_PSMALL_DIRECT_WAVES_PER_SIMD 8
#endif
#define MDH_OCC_BUILTIN(PART, MODE) (((PART) & MDH_PF_PART) ? ((MODE) == 2 ? (((PART) & MDH_PF_PSMALL) ? MDH_PSMALL_DIRECT_WAVES_PER_SIMD : MDH_DIRECT_WAVES_PER_SIMD) : MDH_PART_WAVES_PER_SIMD) : (((PART) & MDH_PF_ROOM) && (MODE) == 0 ? MDH_ROOM_WAVES_PER_SIMD : MDH_WAVES_PER_SIMD))
#ifdef MDH_JIT
#define MDH_OCC(PART, MODE) MDH_OCC_BUILTIN(PART, MODE)
#else
#define MDH_OCC(PART, MODE) (((PART) & MDH_PF_CUSTOM) ? 2 : MDH_OCC_BUILTIN(PART, MODE))
#endif
// The radiance kernel is built for more wavefronts per SIMD than the screen kernel: beside two screen passes it then
// takes less of the register file (measured with frames in flight: 5 -> 3775, 6 -> 3800, 7 -> 3830, 8 -> 3845 Mpix/s;
// at 8 a wavefront alone on its SIMD, as in an 8-way sharded frame, runs 5 % slower on its spills: 7).
#ifndef MDH_RAD_WAVES_PER_SIMD
#define MDH_RAD_WAVES_PER_SIMD 7
#endif
// A launch that leaves most wavefront slots empty anyway (the reference's default 36 probes; a rank's slice of a sharded
// frame) gains nothing from a small register budget: its kernel variant (SMALL) is built for five wavefronts per SIMD --
// 86 VGPRs, 16 instead of 96 bytes of scratch (the radiance pass of a rank's slice -2 %, light_shafts +0.6 to +1.3 %:
// profiles/r02_x_radiance_small_launch.log).
#ifndef MDH_RAD_SMALL_WAVES_PER_SIMD
#define MDH_RAD_SMALL_WAVES_PER_SIMD 5
#endif
#define MDH_OCC_RAD_BUILTIN(SMALL) ((SMALL) ? MDH_RAD_SMALL_WAVES_PER_SIMD : MDH_RAD_WAVES_PER_SIMD)
#ifdef MDH_JIT
#define MDH_OCC_RAD(PART, SMALL) MDH_OCC_RAD_BUILTIN(SMALL)
#else
#define MDH_OCC_RAD(PART, SMALL) (((PART) & MDH_PF_CUSTOM) ? 2 : MDH_OCC_RAD_BUILTIN(SMALL))
#endif
#ifndef MDH_RAD_QVIS
#define MDH_RAD_QVIS 1 // probe-visibility rays through the wave's ray queue (mdh_march.h: queued_visibility)
#endif
#ifndef MDH_SCAT_BATCH
#define MDH_SCAT_BATCH 8 // scattering steps whose froxel taps are in flight together
#endif
#ifndef MDH_WAVES_PER_SIMD
#define MDH_WAVES_PER_SIMD 5 // register budget of the march kernels (measured, pipelined frames: 5 > 6 > 4 waves/SIMD)
#endif

// ------------------------------------------------------------------------ screen pass
// a colour as the RGBA8 default framebuffer of the reference's window holds it (see k_present below;
// unorm8 is the atlas store's conversion, mdh_device.h)
__device__ __forceinline__ unsigned pack_rgba8(float4 c) { return (unsigned)unorm8(c.x) | ((unsigned)unorm8(c.y) << 8) | ((unsigned)unorm8(c.z) << 16) | ((unsigned)unorm8(c.w) << 24); }
struct ScreenArgs {
   int W, H;
   int tiles_x, n_tiles; // 8x8 tiles of the whole image
   int rank, world;      // this launch draws tiles rank, rank + world, ...
   int ao_steps;
   int spec_mode; // M_COMPUTE_INDIRECT_SPECULAR (MDH_OPT_INDIRECT_SPECULAR)
   float4 *fb; // W*H, row 0 = top
   int *gb_index;
   float *gb_t;
   int *gb_steps;
   unsigned *window; // MDH_OPT_WINDOW: the window's RGBA8 pixels (pinned host memory, written over PCIe), or null
   // MDH_OPT_SCREEN_ORDER: the launch's tiles in the order of an earlier pass's wavefront durations, slowest first.  A
   // pass ends with its slowest wavefront; in image order the long tiles (rays that graze surfaces for hundreds of
   // steps) start anywhere, and the pass of simple_scene spent 45 % of its time with a few of them on an empty chip.
   int n_own;             // tiles this launch draws: own index 0 .. n_own - 1, tile = rank + own * world
   const unsigned *order; // [n_own] the own index at every place of the launch, or null: image order
   unsigned char *cost;   // [n_own] written by the pass when not null: the tile's wavefront duration as a sort key
   // A launch too small to fill the chip (a rank's share of a sharded frame, a small window) is the latency of its slowest
   // wavefront, and a wavefront alone on its SIMD issues one instruction every four cycles whatever its lanes do: `split` = 1, 2
   // gives a tile to two wavefronts of 8x4 pixels or four of 4x4 (32 / 16 lanes each, the others idle from the start) -- every
   // wavefront marches only as long as ITS pixels need and the tile's work runs on several SIMDs.  A pixel's operations do not
   // depend on which lanes march beside it: the same bits (tests/test_gpu_parity.py::test_split_tiles_change_no_pixel).
   // (measured: splitting only the slowest tiles at the head of an ORDERED launch, four wavefronts of 4x4 pixels each, gained nothing)
   int split;
   // MDH_OPT_SCREEN_REPLAY (mdh_march.h: PixelRecord): [n_own * 64] the records of the launch's pixels, written by
   // k_screen<.., 1>, read by k_screen<.., 2>; nullptr for the kernel that only marches.  A pixel's record is at
   // own index * 64 + (y & 7) * 8 + (x & 7): whichever place, wavefront or lane draws the pixel (screen_record_index)
   PixelRecord *rec;
};
MDH_DEV size_t screen_record_index(int own, int i, int j) { return (size_t)own * 64 + (size_t)((j & 7) * 8 + (i & 7)); }
// place of a launch -> its index into the launch's tiles, the part of the tile, the split factor (ScreenArgs::split)
MDH_DEV void screen_place(const ScreenArgs &a, int place, int &idx, int &sub, int &split)
{
   idx = place >> a.split; sub = place & ((1 << a.split) - 1); split = a.split;
}
#ifndef MDH_SCREEN_SPLIT_DEFAULT
#define MDH_SCREEN_SPLIT_DEFAULT 2560 // MDH_OPT_SCREEN_SPLIT's initial value
#endif
// a wavefront's duration in ticks of s_memtime (which need not be the shader clock) as a key of the counting sort (k_rad_hist ...)
#ifndef MDH_TILE_COST_SHIFT
#define MDH_TILE_COST_SHIFT 12
#endif
MDH_DEV unsigned char tile_cost_key(unsigned cycles) { return (unsigned char)min(cycles >> MDH_TILE_COST_SHIFT, 255u); }

// draw_screen.glsl:20-30.  One wavefront per 8x8 pixel tile: lane = (y & 7) * 8 + (x & 7);
// the tile's 64 pixels walk the structured pixel program of mdh_march.h together.
//
// Nothing of the prologue stays live across the pixel program: the pixel's coordinates, its camera ray and the
// arguments only the epilogue needs (volumetrics, framebuffer, camera) are derived AGAIN after it, from the kernel
// argument segment read through a pointer the compiler cannot trace back and from a lane index taken from the hardware
// (tile_pixel).  Kept live they cost ~10 VGPRs and ~20 SGPRs which the compiler spilled to scratch (80 bytes per
// lane written and read back through HBM: 172 MB per launch at 1080p against a 33 MB framebuffer).
MDH_DEV void tile_pixel(const ScreenArgs &a, int tile, int sub, int split, int lane, int &i, int &j, float &u, float &v)
{
   if (split == 0) { // (wave-uniform)
      i = (tile % a.tiles_x) * 8 + (lane & 7);
      j = (tile / a.tiles_x) * 8 + (lane >> 3);
   } else if (split == 1) { // the tile's upper or lower 8x4 pixels
      i = (tile % a.tiles_x) * 8 + (lane & 7);
      j = (tile / a.tiles_x) * 8 + sub * 4 + ((lane >> 3) & 3);
      if (lane >= 32) i = a.W; // (no pixel: not valid)
   } else { // one of its four 4x4 quadrants
      i = (tile % a.tiles_x) * 8 + (sub & 1) * 4 + (lane & 3);
      j = (tile / a.tiles_x) * 8 + (sub >> 1) * 4 + ((lane >> 2) & 3);
      if (lane >= 16) i = a.W;
   }
   u = centre(i, a.W);
   v = -centre(j, a.H); // row 0 = top
}
// ALT: the variant whose second shaded point runs render_probes.glsl's other two indirect-specular bodies (modes 1 and 3)
// REC (MDH_OPT_SCREEN_REPLAY): 0 = the pass as it marches, 1 = the same and every pixel's PixelRecord stored, 2 = the pass from
// the records.  Lanes outside the image (partial tiles, the idle lanes of a split tile) read and write none; a launch
// draws its own rank's tiles only, so no other rank's record is touched.  The recording kernel takes
// MDH_SCR_RECORD_PARK_ROWS rows of LDS, the replaying one the marching kernel's.
template <int PART, int MODE, bool GBUF, bool ALT = false, int REC = 0>
__global__ __launch_bounds__(MDH_BLOCK, MDH_OCC(PART, MODE)) void k_screen(KScene sc, KProbes pr, KVolumetrics vol, KCamera cam, ScreenArgs a)
{
   static_assert(REC == 0 || (MDH_SCR_REPLAY && MODE == 0 && !ALT && (PART & ~(MDH_PF_ROOM | MDH_PF_POW2)) == 0),
                 "records are of the fixed mode's pixel program over the brute-force scan or the rooms' census");
   stage_table(sc);
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
   const int place = blockIdx.x * (MDH_BLOCK / 64) + wave;
   int pidx, psub, psplit;
   screen_place(a, place, pidx, psub, psplit);
   if (pidx >= a.n_own) return; // wave-uniform
   const unsigned t_begin = (unsigned)__builtin_amdgcn_s_memtime();
   const int own = a.order ? (int)a.order[pidx] : pidx;
   const int tile = a.rank + own * a.world;
   PH_KERNEL_BEGIN();
   MDH_DIAG_WAVE(own);
   f3 c;
   PrimaryHit ph;
   bool hit;
   f3 pos;
   {
      int i, j;
      float u, v;
      tile_pixel(a, tile, psub, psplit, lane, i, j, u, v);
      const bool valid = i < a.W && j < a.H;
      f3 origin, dir;
      camera_ray(cam, u, v, origin, dir);
      MachineCfg cfg; // renderers.adb:136-143
      cfg.direct_specular = true;
      cfg.spec_mode = a.spec_mode;
      cfg.ao_steps = a.ao_steps;
      constexpr bool NULLB = null_brdf_screen(PART, MODE, GBUF, ALT, REC); // (mdh_march.h: which instantiations shade every light)
      // (mdh_march.h: which instantiations fetch every lane's taps -- 0 -- and which of the others take a folded corner's weight from its twin -- 2)
      // ... and which search the second point's best probe best first -- 4 beside either)
      // ... and which bound the sphere's and the box's distance once per ray in front of their two marches -- 8)
      constexpr int SHARET = (!share_taps_screen(PART, GBUF, REC) ? 0 : folded_twins_screen(PART, GBUF, REC) ? 2 : 1) | (best_first_screen(PART, GBUF, REC) ? 4 : 0) |
                             (ray_bounds_screen(PART, GBUF, REC) ? 8 : 0);
      if (REC == 2) {
         RayRecord rec = {0u, 0u, -1, 0u}, rec2 = {0u, 0u, -1, 0u};
         if (valid) {
            const PixelRecord *q = a.rec + screen_record_index(own, i, j);
            rec = q->first; rec2 = q->second;
         }
         c = MDH_SHADE<PART, MODE, ALT ? 2 : 1, false, REC, SHARET, NULLB>(sc, pr, cfg, valid, origin, dir, ph, hit, pos, rec, rec2);
      } else
      c = MDH_SHADE<PART, MODE, ALT ? 2 : 1, false, REC, SHARET, NULLB>(sc, pr, cfg, valid, origin, dir, ph, hit, pos);
   }
   struct KArgs { KScene sc; KProbes pr; KVolumetrics vol; KCamera cam; ScreenArgs a; };
   // (the kernel argument segment lays the by-value arguments out like this struct: each at its natural alignment, all of
   //  them 8-byte aligned aggregates of 4- and 8-byte members -- checked here rather than assumed)
   static_assert(alignof(KScene) == 8 && alignof(KProbes) == 8 && alignof(KVolumetrics) == 8 && alignof(ScreenArgs) == 8 && alignof(KCamera) == 4, "kernel argument alignments");
   static_assert(__builtin_offsetof(KArgs, pr) == sizeof(KScene) && __builtin_offsetof(KArgs, vol) == sizeof(KScene) + sizeof(KProbes) &&
                 __builtin_offsetof(KArgs, cam) == sizeof(KScene) + sizeof(KProbes) + sizeof(KVolumetrics) && __builtin_offsetof(KArgs, a) % 8 == 0, "KArgs is the kernel argument segment of k_screen");
   typedef const KArgs __attribute__((address_space(4))) *KArgsPtr; // constant address space: scalar loads
   KArgsPtr ka = (KArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
   asm volatile("" : "+s"(ka));
   KVolumetrics vol2;
   ScreenArgs a2;
   KCamera cam2;
   {
      typedef const int __attribute__((address_space(4))) *IntPtr;
      IntPtr pv = (IntPtr)&ka->vol, pa = (IntPtr)&ka->a, pc = (IntPtr)&ka->cam;
      int *dv = (int *)&vol2, *da = (int *)&a2, *dc = (int *)&cam2;
#pragma unroll
      for (int q = 0; q < (int)(sizeof(KVolumetrics) / 4); ++q) dv[q] = pv[q];
#pragma unroll
      for (int q = 0; q < (int)(sizeof(ScreenArgs) / 4); ++q) da[q] = pa[q];
#pragma unroll
      for (int q = 0; q < (int)(sizeof(KCamera) / 4); ++q) dc[q] = pc[q];
   }
#define vol vol2
#define a a2
#define cam cam2
   // the pixel again (the same integer and fp32 operations on the same inputs: the same values)
   int i, j;
   float u, v;
   {
      int wave2 = wave;
      asm volatile("" : "+s"(wave2));
      const int place2 = (int)blockIdx.x * (MDH_BLOCK / 64) + wave2;
      int pidx2, psub2, psplit2;
      screen_place(a, place2, pidx2, psub2, psplit2);
      const int own2 = a.order ? (int)a.order[pidx2] : pidx2;
      const int tile2 = a.rank + own2 * a.world;
      tile_pixel(a, tile2, psub2, psplit2, lane_index_fresh(), i, j, u, v);
      // (everything but the tone map and the stores is behind the wavefront: what it took decides its place in later passes)
      if (a.cost && lane_index_fresh() == 0) a.cost[own2] = tile_cost_key((unsigned)__builtin_amdgcn_s_memtime() - t_begin);
   }
   const bool valid = i < a.W && j < a.H;
#ifdef MDH_PHASES
   if (!valid) { PH_KERNEL_END(); return; }
#endif
   if (!valid) return;
   if (REC == 1) { // the pixel's record from its parked parts (a miss parked its steps only; no reflection ray: flags 0)
      float *pk = (float *)(s_tab + ka->sc.table_f4 + ka->sc.part_bits_f4); // (park_base, from the argument segment)
      const int wb = park_wave_base(pk);
      PixelRecord q = {{0u, 0u, -1, 0u}, {0u, 0u, -1, 0u}};
      int vis = 0, flags = 0, vis2 = 0, index2 = -1;
      if (hit) {
         const f3 p1 = park_load3<MDH_PARK_REC>(pk, wb);
         q.first.t = (unsigned)__float_as_int(p1.x); q.first.index = __float_as_int(p1.y); q.first.sd0 = (unsigned)__float_as_int(p1.z);
         vis = __float_as_int(park_load1<MDH_PARK_REC + 3>(pk, wb));
         flags = __float_as_int(park_load1<MDH_PARK_REC2 + 4>(pk, wb));
         if (flags & 2) {
            const f3 p2 = park_load3<MDH_PARK_REC2>(pk, wb);
            q.second.t = (unsigned)__float_as_int(p2.x); index2 = __float_as_int(p2.y); q.second.sd0 = (unsigned)__float_as_int(p2.z);
            vis2 = __float_as_int(park_load1<MDH_PARK_REC2 + 3>(pk, wb));
         }
         q.second.index = a.ao_steps > 0 ? __float_as_int(park_load1<MDH_PARK_REC_AO>(pk, wb)) : 0;
      }
      q.first.word = ray_record_word(hit, __float_as_int(park_load1<MDH_PARK_REC + 4>(pk, wb)), vis);
      q.second.word = pixel_record_word2((flags & 2) != 0, (flags & 1) != 0, index2, vis2);
      int wave3 = wave;
      asm volatile("" : "+s"(wave3));
      int pidx3, psub3, psplit3;
      screen_place(a, (int)blockIdx.x * (MDH_BLOCK / 64) + wave3, pidx3, psub3, psplit3);
      const int own3 = a.order ? (int)a.order[pidx3] : pidx3;
      a.rec[screen_record_index(own3, i, j)] = q;
   }
   if (MODE == 0 && vol.enabled) {
      f3 origin, dir;
      camera_ray(cam, u, v, origin, dir);
      c = render_volumetrics(sc, vol, c, origin, pos, hit, F2(u, v));
   }
   if (MODE != 1) // draw_screen.glsl:29
      c = F3(spow(sdiv(c.x, c.x + 1.0f), 0.4545f), spow(sdiv(c.y, c.y + 1.0f), 0.4545f), spow(sdiv(c.z, c.z + 1.0f), 0.4545f));
   const size_t px = (size_t)j * a.W + i;
   a.fb[px] = make_float4(c.x, c.y, c.z, 1.0f);
   if (a.window) a.window[px] = pack_rgba8(make_float4(c.x, c.y, c.z, 1.0f));
   if (GBUF) {
      a.gb_index[px] = ph.index;
      a.gb_t[px] = ph.t;
      a.gb_steps[px] = ph.steps;
   }
#undef vol
#undef a
#undef cam
   PH_KERNEL_END();
}

// ---------------------------------------------------------------------- radiance pass
// compute_probe_radiance.glsl:16-27.  One lane per radiance texel (one probe ray); a wavefront = the same
// octahedral texel of MDH_RAD_PROBES_PER_WAVE = 64 consecutive probes (64 parallel rays from 64 origins).
#ifndef MDH_RAD_ORDER_DEFAULT
#define MDH_RAD_ORDER_DEFAULT 1 // MDH_OPT_RADIANCE_ORDER's initial value
#endif
// a step count on a scale of 16 levels: 0 .. 7 as they are, then 8-11, 12-15, 16-23, 24-31, 32-47, 48-63, 64-95, 96 and more
// (rays of one level differ by a third at most; the two levels of a ray are one byte, one pass of the counting sort)
MDH_DEV int rad_level(int steps)
{
   if (steps < 8) return steps;
   const int l = 31 - __builtin_clz((unsigned)steps); // 3 for 8-15, 4 for 16-31 ...
   return min(15, 8 + 2 * (l - 3) + ((steps >> (l - 1)) & 1));
}
struct RadOrder {
   const unsigned *order; // [n_rays] ray at every place, or nullptr: rays in probe order
   unsigned char *steps;  // [n_rays] every ray's sort key (rad_level of its primary-march and shadow steps), written by the pass; or nullptr
   int n_rays;
   // MDH_OPT_RADIANCE_REPLAY (mdh_march.h: RayRecord): [n_rays] the rays' records, written by k_radiance<.., 1>, read by
   // k_radiance<.., 2>, indexed by the ray; nullptr for the kernel that only marches
   RayRecord *rec;
   // Every wavefront is full, also in launches that leave most wavefront slots of the chip empty.  (measured, rank 0's radiance
   // slice of an 8-way sharded frame, 1 024 full wavefronts on 1 024 SIMDs: 0.094 ms full, 0.096 ms half filled, 0.125 ms quarter
   // filled, profiles/r03_x_radiance_partial_fill.log -- the rays are sorted by their march lengths already, so a wavefront's
   // lanes end together whatever their number, and four wavefronts of 16 issue four times the instructions)
};
// `first_round`: the workgroups the chip holds at once (0: not told).  The pass is ONE round of wavefronts and a
// remainder -- 8 192 wavefronts on 7 168 slots at the headline size -- and ends with its slowest wavefront.  A SIMD
// issues from its OLDEST wavefront first (measured: within the first round a wavefront's duration follows its launch
// position, 36 us for the first eighth to 88 us for the seventh, whichever probes it holds), so the remainder, which
// starts 35-65 us late in slots between six older wavefronts, would finish last by far: it raises its issue priority
// instead and runs at the speed of a wavefront alone (radiance pass 0.165 -> 0.147 ms).
// `ro`: the rays of the pass in the order of the PREVIOUS pass's primary-march lengths (RadOrder below), or no order.
// The texel (x, y) of probe probe_raw that lane `lin` of the launch computes (probe_raw = pr.probe_end: none)
MDH_DEV void radiance_texel(const KProbes &pr, const RadOrder &ro, long lin, int &x, int &y, int &probe_raw)
{
   const int per_probe = pr.rres * pr.rres;
   // a wavefront = a TxT texel tile (T*T = 64 / G) of the octahedral maps of G consecutive probes:
   // G = 1 is one 8x8 tile of one probe, G = 64 the same ray direction from 64 probes
   constexpr int G = MDH_RAD_PROBES_PER_WAVE, T = (G == 1) ? 8 : (G == 4) ? 4 : (G == 16) ? 2 : 1;
   const int lane = (int)(lin & 63);
   const long wave_global = lin >> 6;
   if (ro.order) { // lane = the ray at this place of the order (a ray: probe of the slice * texels + texel)
      const unsigned ray = lin < ro.n_rays ? ro.order[lin] : 0xffffffffu;
      if (pr.rshift >= 0) {
         probe_raw = ray == 0xffffffffu ? pr.probe_end : pr.probe_begin + (int)(ray >> (2 * pr.rshift));
         y = (int)(ray >> pr.rshift) & (pr.rres - 1);
         x = (int)ray & (pr.rres - 1);
      } else {
         probe_raw = ray == 0xffffffffu ? pr.probe_end : pr.probe_begin + (int)(ray / (unsigned)per_probe);
         const int rem = (int)(ray % (unsigned)per_probe);
         y = rem / pr.rres;
         x = rem - y * pr.rres;
      }
   } else
   if ((pr.rres % T) == 0) {
      const int tpr = pr.rres / T, tiles = tpr * tpr;      // texel tiles per probe
      const int group = (int)(wave_global / tiles), tile = (int)(wave_global % tiles);
      probe_raw = pr.probe_begin + group * G + lane / (T * T);
      const int l = lane % (T * T);
      x = (tile % tpr) * T + (l % T);
      y = (tile / tpr) * T + (l / T);
   } else { // resolutions that are no multiple of the tile edge: row-major, one probe per run
      probe_raw = pr.probe_begin + (int)(lin / per_probe);
      const int rem = (int)(lin % per_probe);
      y = rem / pr.rres;
      x = rem - y * pr.rres;
   }
}
// The pass is ONE kernel.  (measured: as two -- every ray's marches, hit point and direct light into per-ray records at eight
// wavefronts per SIMD, then the probe visibility queue, the irradiance taps and the store from the records -- 0.180 instead of
// 0.125 ms)
// REC: 0 = the pass as it marches, 1 = the same and every real ray's RayRecord stored, 2 = the pass from the records (lanes
// past the ray count, in a launch padded to whole wavefronts and probe groups, read and write none).  The replaying kernel
// is built for the register budget of the marching one (measured: DESIGN.md section 4, item 11) and takes
// MDH_REPLAY_PARK_ROWS rows of LDS instead of MDH_PARK_DWORDS.
template <int PART, bool SMALL = false, int REC = 0> __global__ __launch_bounds__(MDH_BLOCK, MDH_OCC_RAD(PART, SMALL)) void k_radiance(KScene sc, KProbes pr, int first_round, RadOrder ro)
{
   static_assert(REC == 0 || (MDH_RAD_REPLAY && MDH_RAD_QVIS && MDH_SHARE_FIRST_STEP), "the records hold the queue's bits and the shared first step");
   if (first_round > 0 && (int)blockIdx.x >= first_round) __builtin_amdgcn_s_setprio(3);
   stage_table(sc);
   f3 c;
   PrimaryHit ph;
   PH_KERNEL_BEGIN();
   {
      const long lin = (long)blockIdx.x * MDH_BLOCK + threadIdx.x;
      int x, y, probe_raw;
      radiance_texel(pr, ro, lin, x, y, probe_raw);
      const bool valid = probe_raw < pr.probe_end;
      MDH_DIAG_WAVE(lin >> 6);
      const int probe = valid ? probe_raw : pr.probe_begin;
      const int ty = probe / pr.pcx, tx = probe - ty * pr.pcx;
      const int i = tx * pr.rres + x, j = ty * pr.rres + y; // texel of the reference's 2-D atlas image
      const f2 nc = F2((centre(i, pr.pcx * pr.rres) + 1.0f) * 0.5f, (centre(j, pr.pcy * pr.rres) + 1.0f) * 0.5f);
      // coord_to_probe_id / probe position (probe_utils.glsl:19-40)
      const int probe_id = (int)(nc.y * (float)pr.pcy) * pr.pcx + (int)(nc.x * (float)pr.pcx);
      const f3 world = grid_to_world(pr, probe_id_to_grid(pr, probe_id));
      const f3 ray_dir = ray_id_to_ray_dir(F2(fract_(nc.x * (float)pr.pcx), fract_(nc.y * (float)pr.pcy)));
      MachineCfg cfg; // renderers.adb:115-117: no specular; AO and volumetrics macros undefined
      cfg.direct_specular = false;
      cfg.spec_mode = 0;
      cfg.ao_steps = 0;
      bool hit;
      f3 pos;
      if (REC == 2) {
         RayRecord rec = {0u, 0u, -1, 0u};
         if (valid) rec = ro.rec[(size_t)(probe_raw - pr.probe_begin) * (pr.rres * pr.rres) + y * pr.rres + x];
         c = MDH_SHADE<PART, 0, 0, true, 2>(sc, pr, cfg, valid, world, ray_dir, ph, hit, pos, rec);
      } else
      c = MDH_SHADE<PART, 0, 0, MDH_RAD_QVIS != 0, REC, true, null_brdf_radiance(PART, SMALL, REC)>(sc, pr, cfg, valid, world, ray_dir, ph, hit, pos);
      if (REC == 1) ph.index = hit ? 1 : 0; // (the one bit of the record that must stay live: in the register of the arg-min, which the pass does not use)
   }
   // The texel again: nothing of the prologue stays live across the pixel program (its coordinates, the order's entry and
   // the arguments the store needs were eleven dwords that the seven-wavefront build kept in scratch memory).  The lane
   // index comes from the hardware, the arguments from the kernel argument segment through a pointer the compiler
   // cannot trace: the same integer operations on the same inputs.
   {
      struct KArgs { KScene sc; KProbes pr; int first_round; RadOrder ro; };
      static_assert(alignof(RadOrder) == 8 && sizeof(RadOrder) % 8 == 0 && __builtin_offsetof(KArgs, pr) == sizeof(KScene) && __builtin_offsetof(KArgs, first_round) == sizeof(KScene) + sizeof(KProbes) &&
                    __builtin_offsetof(KArgs, ro) == sizeof(KScene) + sizeof(KProbes) + 8, "KArgs is the kernel argument segment of k_radiance");
      typedef const KArgs __attribute__((address_space(4))) *KArgsPtr;
      KArgsPtr ka = (KArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(ka));
      typedef const int __attribute__((address_space(4))) *IntPtr;
      KProbes pr2;
      RadOrder ro2;
      {
         IntPtr pp = (IntPtr)&ka->pr, po = (IntPtr)&ka->ro;
         int *dp = (int *)&pr2, *dq = (int *)&ro2;
#pragma unroll
         for (int q = 0; q < (int)(sizeof(KProbes) / 4); ++q) dp[q] = pp[q];
#pragma unroll
         for (int q = 0; q < (int)(sizeof(RadOrder) / 4); ++q) dq[q] = po[q];
      }
      int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
      asm volatile("" : "+s"(wave));
      const long lin = (long)blockIdx.x * MDH_BLOCK + wave * 64 + lane_index_fresh();
      int x, y, probe_raw;
      radiance_texel(pr2, ro2, lin, x, y, probe_raw);
      if (probe_raw < pr2.probe_end) {
         const int ty = probe_raw / pr2.pcx, tx = probe_raw - ty * pr2.pcx;
         const int i = tx * pr2.rres + x, j = ty * pr2.rres + y;
         atlas_store(pr2.rad, pr2.fmt, atlas_index(pr2.pcx, pr2.rres, pr2.rshift, i, j), c);
         if (ro2.steps) // the ray's sort key: the levels of its primary-march and soft-shadow step counts
            ro2.steps[(size_t)(probe_raw - pr2.probe_begin) * (pr2.rres * pr2.rres) + y * pr2.rres + x] = (unsigned char)((rad_level(ph.steps & 0xffff) << 4) | rad_level(ph.steps >> 16));
         if (REC == 1) { // the ray's record: its parked parts (a miss parked its steps only)
            float *pk = (float *)(s_tab + ka->sc.table_f4 + ka->sc.part_bits_f4); // (park_base, from the argument segment)
            const int wb = park_wave_base(pk);
            RayRecord rec = {0u, 0u, -1, 0u};
            int vis = 0;
            if (ph.index) {
               const f3 v = park_load3<MDH_PARK_REC>(pk, wb);
               rec.t = (unsigned)__float_as_int(v.x); rec.index = __float_as_int(v.y); rec.sd0 = (unsigned)__float_as_int(v.z);
               vis = __float_as_int(park_load1<MDH_PARK_REC + 3>(pk, wb));
            }
            rec.word = ray_record_word(ph.index != 0, __float_as_int(park_load1<MDH_PARK_REC + 4>(pk, wb)), vis);
            ro2.rec[(size_t)(probe_raw - pr2.probe_begin) * (pr2.rres * pr2.rres) + y * pr2.rres + x] = rec;
         }
      }
   }
   PH_KERNEL_END();
}

// MDH_OPT_RADIANCE_MIPS: one level of the radiance atlas's mip chain from the level below -- the 2x2 box filter over the
// atlas image, ((a + b) + (c + d)) * 0.25 per channel in fp32 on the texels as stored, stored in the atlas's format.  Both
// levels are probe-major ([probe][y][x]); the resolution is a power of two, so no box crosses a probe's tile.
// thread = texel of the destination level (n = probes * res * res), res = its tile resolution
__global__ __launch_bounds__(256) void k_radiance_mips(const void *src, void *dst, int fmt, int res, int n)
{
   const int idx = blockIdx.x * 256 + threadIdx.x;
   if (idx >= n) return;
   const int per = res * res, p = idx / per, rem = idx - p * per, y = rem / res, x = rem - y * res;
   const int rs = 2 * res;
   const unsigned s0 = ((unsigned)(p * rs + 2 * y) * (unsigned)rs) + (unsigned)(2 * x), s1 = s0 + (unsigned)rs;
   const f3 a = atlas_texel<false>(src, fmt, s0, -1), b = atlas_texel<false>(src, fmt, s0 + 1, -1);
   const f3 c = atlas_texel<false>(src, fmt, s1, -1), d = atlas_texel<false>(src, fmt, s1 + 1, -1);
   atlas_store(dst, fmt, (unsigned)idx, ((a + b) + (c + d)) * 0.25f);
}

// ---- Rays in the order of their primary-march lengths.  In lock step a wavefront pays the LONGEST primary march
// among its 64 rays: 20 of 64 lanes are alive in an average step of that march, which is 60 % of the pass's SDF
// evaluations.  A probe ray's march hardly changes from frame to frame (the probes do not move): every pass leaves each
// ray's step count behind, three small kernels sort the rays by it -- a counting sort, longest first -- and the next pass
// takes its rays in that order, so that the rays of a wavefront end their marches together.  Which lane computes a
// texel changes, never what it holds.
//   k_rad_hist:    per chunk of rays (at most MDH_RO_MAX_CHUNKS chunks) a histogram of the 256 keys -> hist[chunk][key]
//   k_rad_scan:    exclusive prefix over keys (descending) and chunks -> the first place of every (key, chunk)
//   k_rad_scatter: the chunk's rays to their places
#define MDH_RO_MAX_CHUNKS 128 // (the scan keeps a key's counts of all chunks in registers)
// hist is [chunk][key]: every access below is 256 consecutive words
__global__ __launch_bounds__(256) void k_rad_hist(const unsigned char *steps, int n, int chunk, unsigned *hist)
{
   __shared__ unsigned h[256];
   h[threadIdx.x] = 0u;
   __syncthreads();
   const int base = blockIdx.x * chunk; // (chunk is a multiple of 1 024: four rays per thread and turn)
   for (int i = 4 * threadIdx.x; i < chunk; i += 1024) {
      if (base + i + 3 < n) {
         const unsigned w = *(const unsigned *)(steps + base + i);
         atomicAdd(&h[w & 255u], 1u); atomicAdd(&h[(w >> 8) & 255u], 1u); atomicAdd(&h[(w >> 16) & 255u], 1u); atomicAdd(&h[w >> 24], 1u);
      } else
         for (int q = 0; q < 4; ++q)
            if (base + i + q < n) atomicAdd(&h[steps[base + i + q]], 1u);
   }
   __syncthreads();
   hist[blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}
__global__ __launch_bounds__(256) void k_rad_scan(unsigned *hist, int chunks) // one workgroup; thread = key
{
   __shared__ unsigned after[256];
   unsigned v[MDH_RO_MAX_CHUNKS];
#pragma unroll
   for (int c = 0; c < MDH_RO_MAX_CHUNKS; ++c) v[c] = c < chunks ? hist[c * 256 + threadIdx.x] : 0u; // (all loads in flight together)
   unsigned sum = 0u;
#pragma unroll
   for (int c = 0; c < MDH_RO_MAX_CHUNKS; ++c) { const unsigned x = v[c]; v[c] = sum; sum += x; }
   // rays with a larger key come first: the sum of the totals of the keys above this one (a suffix scan in LDS)
   after[threadIdx.x] = sum;
   __syncthreads();
   for (int d = 1; d < 256; d <<= 1) {
      const unsigned add = (int)threadIdx.x + d < 256 ? after[threadIdx.x + d] : 0u;
      __syncthreads();
      after[threadIdx.x] += add;
      __syncthreads();
   }
   const unsigned before = after[threadIdx.x] - sum;
#pragma unroll
   for (int c = 0; c < MDH_RO_MAX_CHUNKS; ++c)
      if (c < chunks) hist[c * 256 + threadIdx.x] = v[c] + before;
}
__global__ __launch_bounds__(256) void k_rad_scatter(const unsigned char *steps, int n, int chunk, const unsigned *hist, unsigned *order)
{
   __shared__ unsigned place[256];
   place[threadIdx.x] = hist[blockIdx.x * 256 + threadIdx.x];
   __syncthreads();
   const int base = blockIdx.x * chunk;
   for (int i = 4 * threadIdx.x; i < chunk; i += 1024) {
      if (base + i + 3 < n) {
         const unsigned w = *(const unsigned *)(steps + base + i);
         order[atomicAdd(&place[w & 255u], 1u)] = (unsigned)(base + i);
         order[atomicAdd(&place[(w >> 8) & 255u], 1u)] = (unsigned)(base + i + 1);
         order[atomicAdd(&place[(w >> 16) & 255u], 1u)] = (unsigned)(base + i + 2);
         order[atomicAdd(&place[w >> 24], 1u)] = (unsigned)(base + i + 3);
      } else
         for (int q = 0; q < 4; ++q)
            if (base + i + q < n) order[atomicAdd(&place[steps[base + i + q]], 1u)] = (unsigned)(base + i + q);
   }
}

// The same scatter, STABLE: elements with equal keys keep their order.  The screen pass's tiles are sorted with it: tiles
// that took about as long stay in image order, where neighbours tap the same probes' texels (the unstable scatter above
// shuffles the tiles of a chunk: 3 % slower screen passes at equal keys).  Rounds of 256 elements; an element's place =
// the key's next place + the equal keys in front of it in its round.
__global__ __launch_bounds__(256) void k_order_scatter_stable(const unsigned char *keys, int n, int chunk, const unsigned *hist, unsigned *order)
{
   __shared__ unsigned place[256], cnt[256];
   __shared__ short kk[256];
   const int tid = threadIdx.x;
   place[tid] = hist[blockIdx.x * 256 + tid];
   const int base = blockIdx.x * chunk;
   for (int r0 = 0; r0 < chunk; r0 += 256) {
      const int i = base + r0 + tid;
      const bool in = r0 + tid < chunk && i < n;
      const int k = in ? (int)keys[i] : -1;
      kk[tid] = (short)k;
      cnt[tid] = 0u;
      __syncthreads();
      unsigned before = 0u;
      if (in) {
         for (int j = 0; j < tid; ++j) before += kk[j] == k ? 1u : 0u;
         atomicAdd(&cnt[k], 1u);
      }
      __syncthreads();
      if (in) order[place[k] + before] = (unsigned)i;
      __syncthreads();
      place[tid] += cnt[tid];
      __syncthreads();
   }
}

// Keys below `permille` thousandths of the MEDIAN key become 0 (behind k_rad_hist over the raw keys; the histogram is taken
// again afterwards): only the tiles that took clearly longer than most are moved to the front of the launch, all others
// stay in image order.  Every workgroup finds the median from the histogram by itself (256 keys x at most 128 chunks).
__global__ __launch_bounds__(256) void k_order_floor(unsigned char *keys, int n, int chunk, const unsigned *hist, int chunks, int permille)
{
   __shared__ unsigned total[256];
   __shared__ int floor_key;
   const int tid = threadIdx.x;
   unsigned sum = 0u;
   for (int c = 0; c < chunks; ++c) sum += hist[c * 256 + tid];
   total[tid] = sum;
   __syncthreads();
   if (tid == 0) {
      unsigned acc = 0u;
      int m = 0;
      for (; m < 255; ++m) { acc += total[m]; if (2u * acc >= (unsigned)n) break; }
      floor_key = (int)(((long)m * permille + 999) / 1000);
   }
   __syncthreads();
   const int f = floor_key, base = blockIdx.x * chunk;
   for (int i = tid; i < chunk; i += 256)
      if (base + i < n && (int)keys[base + i] < f) keys[base + i] = 0;
}

// -------------------------------------------------------------------- irradiance pass
// update_probe_irradiance.glsl:8-43: every irradiance texel sums its probe's rres x rres
// radiance taps (bilinear, at texel CORNERS, so the first row/column bleed in from the
// neighbouring tiles) in the reference's order.
//
// One workgroup per probe.  A tap's radiance and its ray direction depend on the probe and
// the tap only, not on the output texel: the workgroup evaluates each of the rres^2 taps
// once (bilinear fetch + octahedral decode, spread over all lanes) into LDS, then every
// lane owns one output texel and folds the taps in the reference's y, x order with LDS
// broadcast reads -- ~13 VALU per tap and lane instead of ~370.
#ifndef MDH_IRR_BLOCK
#define MDH_IRR_BLOCK 256 // all of them evaluate taps; the first ires^2 (one wavefront at 8x8) fold
#endif
// One wavefront folds a probe's taps, all four channels.  (measured: (x, y) on one wavefront and (z, weight) on another, the
// same bits with 7 instead of 13 instructions per tap and wavefront, is SLOWER, 0.040 against 0.038 ms for 512 probes,
// profiles/r03_x_irradiance_two_folders.log: the fold waits for its taps' LDS reads, and two wavefronts read every tap twice.
// The taps' weights computed by the wavefronts beside the folding one: bit-exact and not faster, 0.0368 - 0.0417 ms against
// 0.0370, profiles/r04_x_irradiance_weights_pipeline.log: a lone workgroup takes 30 us whatever its instruction count.)
#ifndef MDH_IRR_CHUNK
#define MDH_IRR_CHUNK 256 // taps per LDS buffer when one wavefront folds
#endif
// The form for probes of at most 64 texels: one channel of the fold per wavefront, the weights shared through LDS (k_irradiance)
#ifndef MDH_IRR_PRIO
#define MDH_IRR_PRIO 3 // s_setprio of that form's wavefronts
#endif
#ifndef MDH_IRR_CCHUNK
#define MDH_IRR_CCHUNK 32 // taps per weight buffer of that form (32: 18 KiB of LDS, 64: 34 KiB -- the same speed alone, 32 starts sooner beside the march kernels of frames in flight)
#endif
// LDS of that form: two weight buffers of 64 rows; its scratch in device memory: six planes of the taps (rounded up to whole chunks) per probe
#define MDH_IRR_CHANNELS_LDS ((size_t)2 * 64 * (MDH_IRR_CCHUNK + 4) * sizeof(float))
#define MDH_IRR_CHANNELS_PLANE(n) ((size_t)(((n) + 63) / 64 * 64))
typedef float pk2 __attribute__((ext_vector_type(2))); // two fp32 per VALU instruction (v_pk_mul_f32 / v_pk_add_f32: IEEE per component)
// MDH_OPT_PROBE_SETTLE (mdh_host.h: SettleTracker; DESIGN.md section 4, "Exact work elimination", item 13): a tracked pass
// (seq != 0) counts the texels it stores with other bits than `prev` -- the irradiance set the radiance pass read, this pass's
// own set when it runs in place -- holds at the same index, and the workgroup that finishes last hands the count to the host.
// Compiled out of the builds that count or time the work of passes.
#ifndef MDH_PROBE_SETTLE
#if defined(MDH_DIAG) || defined(MDH_PHASES)
#define MDH_PROBE_SETTLE 0
#else
#define MDH_PROBE_SETTLE 1
#endif
#endif
struct SettleArgs {
   unsigned long long *ctr;  // of the pass under way: workgroups done in the low word, texels changed in the high one; zero between passes
   unsigned long long *slot; // {changed, seq} in pinned host memory (SettleSlot), one 64-bit word
   unsigned seq;             // 0: an untracked pass, nothing of this runs
};
struct AtlasBits { unsigned x, y, z, w; }; // a texel as stored: the RGBA8 word in x (format 0), the four floats' bits (format 1)
MDH_DEV AtlasBits atlas_bits(const void *base, int fmt, unsigned idx)
{
   AtlasBits b = {0u, 0u, 0u, 0u};
   if (fmt == 0) b.x = atlas_rgba8(base, idx);
   else {
      const f4v t = ((GlobalF4)base)[idx];
      b.x = __float_as_uint(t.x); b.y = __float_as_uint(t.y); b.z = __float_as_uint(t.z); b.w = __float_as_uint(t.w);
   }
   return b;
}
// atlas_store, and whether the words stored differ from `old` (compared as integers: a NaN equals itself).  The words are
// atlas_word_*'s, stored here as atlas_store stores them: what is compared is what is stored.
MDH_DEV bool atlas_store_changed(void *base, int fmt, unsigned idx, f3 v, const AtlasBits &old)
{
   if (fmt == 0) {
      const uchar4 t = atlas_word_rgba8(v);
      ((uchar4 *)base)[idx] = t;
      return ((unsigned)t.x | (unsigned)t.y << 8 | (unsigned)t.z << 16 | (unsigned)t.w << 24) != old.x;
   }
   const float4 t = atlas_word_f32(v);
   ((float4 *)base)[idx] = t;
   return __float_as_uint(t.x) != old.x || __float_as_uint(t.y) != old.y || __float_as_uint(t.z) != old.z || __float_as_uint(t.w) != old.w;
}
// One lane per workgroup, behind the workgroup's stores.  ONE atomic carries both counters -- the workgroup's changed texels
// into the high word, one more workgroup done into the low one -- so the workgroup that finds itself last has the pass's total
// in the value the atomic returns, and nothing has to be ordered against anything: no fence.  (measured: the first form, two
// counters with __threadfence between them, made the pass 0.031 -> 0.039 ms alone and 0.072 -> 0.096 ms in flight at config
// 3, profiles/r11_probe_settle_ab.log -- a device-scope release on this chip writes the L2's dirty lines back, the
// workgroups' 12 MB of tap planes among them, once per workgroup.)  The last workgroup hands {changed, seq} to the host as
// one 64-bit store -- the host reads both or neither -- and puts the counter back to zero for the next pass (passes follow
// one another on their stream).
MDH_DEV void settle_report(const SettleArgs &sa, unsigned nchanged, unsigned nblocks)
{
   const unsigned long long before = atomicAdd(sa.ctr, ((unsigned long long)nchanged << 32) | 1ull);
   if ((unsigned)before + 1u != nblocks) return;
   const unsigned total = (unsigned)(before >> 32) + nchanged;
   __hip_atomic_store(sa.ctr, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
   __hip_atomic_store(sa.slot, (unsigned long long)total | (unsigned long long)sa.seq << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// `prev`, `hyst`: MDH_OPT_HYSTERESIS_PERMILLE (not in the reference; 0 = off): the texel is stored as
// mix (fresh, what the previous frame's atlas holds, hyst)
MDH_DEV f3 irradiance_blend(const KProbes &pr, const void *prev, float hyst, unsigned idx, f3 fresh)
{
   if (hyst == 0.0f) return fresh;
   const f3 old = atlas_texel(prev, pr.fmt, idx, -1);
   return F3(mix_(fresh.x, old.x, hyst), mix_(fresh.y, old.y, hyst), mix_(fresh.z, old.z, hyst));
}
// The pieces of k_irradiance's channel form (one channel of a probe's fold per wavefront, below): a wavefront's quarter of a
// chunk's weights (irr_produce) and a chunk folded into the wavefront's channel (irr_fold; RAD: the channel has a radiance
// plane, the weight's own chain adds w).
//   A tap's radiance and direction are the same for all 64 texels.  Read as LDS broadcasts they cost an LDS instruction and
//   four LDS cycles per four taps each, and with two probes on a CU the LDS array, not instruction issue, bounded the pass.
//   Here sixteen taps sit in ONE register, lane l holding tap l mod 16 (one 4-byte read per sixteen taps and plane), and
//   every multiplication takes its tap from that register through the DPP row broadcast (v_mul_f32_dpp row_newbcast:n -- lane
//   n of each row of sixteen to the whole row: the operand's route changes, the IEEE operation does not).
//   The LDS reads run ahead of their use -- a wavefront alone on its SIMD has nothing else to hide their latency behind:
//   everything the chunk reads is asked for before anything is computed (reads return in order: counted waits).
template <int N> MDH_DEV float irr_row_bcast(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + N, 0xf, 0xf, true)); }
template <int K> MDH_DEV float irr_comp(const float4 &v) { return K == 0 ? v.x : K == 1 ? v.y : K == 2 ? v.z : v.w; }
#define MDH_IRR_X16(X_) X_(0) X_(1) X_(2) X_(3) X_(4) X_(5) X_(6) X_(7) X_(8) X_(9) X_(10) X_(11) X_(12) X_(13) X_(14) X_(15)
// PT taps' weights for this lane's texel into the texel's row: the taps' directions in dxv, dyv, dzv (lane l holds tap l mod 16 of
// the register's sixteen), taps OFF .. OFF + PT - 1 of them
template <int OFF, int PT> MDH_DEV void irr_produce(float dxv, float dyv, float dzv, float *wrow, f3 irr_dir)
{
   float wn[16];
#define MDH_IRR_W1(n_) if ((n_) < PT) wn[n_] = max_((irr_dir.x * irr_row_bcast<(OFF + (n_)) & 15>(dxv) + irr_dir.y * irr_row_bcast<(OFF + (n_)) & 15>(dyv)) + irr_dir.z * irr_row_bcast<(OFF + (n_)) & 15>(dzv), 0.0f);
   MDH_IRR_X16(MDH_IRR_W1)
#undef MDH_IRR_W1
#pragma unroll
   for (int g = 0; g < PT / 4; ++g) *(float4 *)(wrow + 4 * g) = make_float4(wn[4 * g], wn[4 * g + 1], wn[4 * g + 2], wn[4 * g + 3]);
}
// 16 * NB taps folded into one channel: their weights w (this lane's texel), their radiance rv (lane l holds tap l mod 16 of each sixteen)
template <bool RAD, int NB> MDH_DEV float irr_fold(const float *rv, const float4 *w, float acc)
{
   // (four products, then their four additions: a DPP instruction that follows the one before it at a distance of two reuses
   //  its destination and waits a slot for it)
#define MDH_IRR_F4(q_)                                                                                                    \
   {                                                                                                                     \
      const float4 wq = w[4 * b + (q_)];                                                                                 \
      if (RAD) {                                                                                                         \
         const float p0 = irr_row_bcast<4 * (q_)>(rvb) * wq.x, p1 = irr_row_bcast<4 * (q_) + 1>(rvb) * wq.y, p2 = irr_row_bcast<4 * (q_) + 2>(rvb) * wq.z, p3 = irr_row_bcast<4 * (q_) + 3>(rvb) * wq.w; \
         acc = acc + p0; acc = acc + p1; acc = acc + p2; acc = acc + p3;                                                 \
      } else { acc = acc + wq.x; acc = acc + wq.y; acc = acc + wq.z; acc = acc + wq.w; }                                 \
   }
#pragma unroll
   for (int b = 0; b < NB; ++b) {
      const float rvb = rv[b];
      MDH_IRR_F4(0) MDH_IRR_F4(1) MDH_IRR_F4(2) MDH_IRR_F4(3)
   }
#undef MDH_IRR_F4
   return acc;
}
__global__ __launch_bounds__(MDH_IRR_BLOCK) void k_irradiance(KProbes pr, const void *prev, float hyst, float *tap_planes, SettleArgs sa)
{
   const bool settle = MDH_PROBE_SETTLE && sa.seq != 0u; // (uniform)
   extern __shared__ float4 s_taps[]; // [2 * rres * rres]: {rad.xyz, 1} {dir.xyz, -}
   const int probe = pr.probe_begin + blockIdx.x;
   if (probe >= pr.probe_end) return;
   const int ntaps = pr.rres * pr.rres;
   const int ty = probe / pr.pcx, tx = probe - ty * pr.pcx;
   const float pcx = (float)pr.pcx, pcy = (float)pr.pcy;
   const f2 step = F2(1.0f / pcx / (float)pr.rres, 1.0f / pcy / (float)pr.rres);
   // probe_id_to_coord of the probe the output texels belong to (probe_utils.glsl:52-56)
   const f2 rad_coord = F2((float)tx / pcx, (float)ty / pcy);
   // one tap: the bilinear fetch of the radiance atlas and the ray direction of its texel
#define MDH_IRR_STAGE(tap_, slot_)                                                                                      \
   do {                                                                                                                 \
      const int yy = (tap_) / pr.rres, xx = (tap_) - yy * pr.rres;                                                       \
      f2 c = F2(clamp_(rad_coord.x + (float)xx * step.x, step.x, 1.0f - step.x), clamp_(rad_coord.y + (float)yy * step.y, step.y, 1.0f - step.y)); \
      f3 rad = atlas_sample(pr.rad, pr.fmt, pr.pcx, pr.pcy, pr.rres, pr.rshift, pr.rad_w, pr.rad_h, c.x, c.y, -1);      \
      f3 rad_dir = ray_id_to_ray_dir(F2(fract_(c.x * pcx), fract_(c.y * pcy)));                                          \
      s_taps[2 * (slot_)] = make_float4(rad.x, rad.y, rad.z, 1.0f);                                                      \
      s_taps[2 * (slot_) + 1] = make_float4(rad_dir.x, rad_dir.y, rad_dir.z, 0.0f);                                      \
   } while (0)
#if MDH_FAST_NUMERICS
   if (pr.ires * pr.ires <= 64 && MDH_IRR_BLOCK == 256) {
      // The experiment's fold: every wavefront folds a QUARTER of the taps for all texels, the four partial sums are added
      // in a fixed order, (0 + 1) + (2 + 3) -- not the reference's order of additions (a tolerance-only result), but a
      // quarter of the pass's critical path.
      for (int t = threadIdx.x; t < ntaps; t += MDH_IRR_BLOCK) MDH_IRR_STAGE(t, t);
      __syncthreads();
      const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
      const int x = lane % pr.ires, y = lane / pr.ires;
      const int i = tx * pr.ires + x, j = ty * pr.ires + y;
      const f2 nc = F2((centre(i, pr.pcx * pr.ires) + 1.0f) * 0.5f, (centre(j, pr.pcy * pr.ires) + 1.0f) * 0.5f);
      const f3 irr_dir = ray_id_to_ray_dir(F2(fract_(nc.x * pcx), fract_(nc.y * pcy)));
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const int t0 = wv * (ntaps / 4), t1 = wv == 3 ? ntaps : t0 + ntaps / 4;
      for (int t = t0; t < t1; ++t) {
         const float4 r = s_taps[2 * t], d = s_taps[2 * t + 1];
         const float w = max_(dot(irr_dir, xyz(d)), 0.0f);
         acc.x += r.x * w; acc.y += r.y * w; acc.z += r.z * w; acc.w += w;
      }
      float4 *part = s_taps + 2 * ntaps;
      part[wv * 64 + lane] = acc;
      __syncthreads();
      if (wv == 0) {
         bool changed = false;
         if (lane < pr.ires * pr.ires) {
            const float4 a = part[lane], b = part[64 + lane], c = part[128 + lane], d = part[192 + lane];
            const f3 sum = F3((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z));
            const f3 irradiance = sum / ((a.w + b.w) + (c.w + d.w));
            const unsigned idx = atlas_index(pr.pcx, pr.ires, pr.ishift, i, j);
            const f3 v = irradiance_blend(pr, prev, hyst, idx, irradiance);
            if (settle) changed = atlas_store_changed(pr.irr, pr.fmt, idx, v, atlas_bits(prev, pr.fmt, idx));
            else atlas_store(pr.irr, pr.fmt, idx, v);
         }
         if (settle) { const unsigned n = (unsigned)__popcll(__ballot(changed)); if (lane == 0) settle_report(sa, n, gridDim.x); }
      }
      return;
   }
#endif
   if (pr.ires * pr.ires <= 64 && MDH_IRR_BLOCK == 256 && tap_planes) { // (the host's test: mdh_api.hip, MDH_PASS_IRRADIANCE)
      // Round 4 (second session): ONE CHANNEL PER WAVEFRONT.  A wavefront that is alone on its SIMD issues one instruction every
      // four cycles whatever the instruction (vector, LDS or scalar), so the lone folding wavefront of the forms below pays
      // ~17 issue slots per tap -- 74 cycles, 30 us for 1 024 taps -- while three wavefronts beside it idle.  The four sums of a
      // texel (x, y, z, weight) are four independent chains of additions: wavefront k carries channel k of all 64 texels, two
      // instructions per tap (one for the weight's chain), with a quarter of the taps' weights w = max (dot (irr_dir, rad_dir), 0)
      // computed by each wavefront one chunk ahead and shared through LDS ([texel][tap]: 16-byte reads and writes, rows 4 * odd
      // dwords apart).  The same multiplications and additions in the reference's order on every chain; the issue slots of a
      // probe's fold spread over four SIMDs instead of one.
      // all four wavefronts are the pass's critical path and meet at a barrier every chunk; beside the march kernels of the
      // neighbouring frames (five or seven wavefronts per SIMD, all of them older) the youngest wavefront of a SIMD gets the
      // issue slots the others leave: raised priority for the pass that heads the next frame's dependency chain
      __builtin_amdgcn_s_setprio(MDH_IRR_PRIO);
      constexpr int CH = MDH_IRR_CCHUNK, S = CH + 4, CHQ = CH / 4;
      static_assert((CH == 64 || CH == 32) && ((S / 4) & 1) == 1, "a wavefront's quarter of a chunk is a register of sixteen taps or half of one; weight rows 16-byte aligned, an odd number of quads apart");
      const int ntp = (ntaps + 63) / 64 * 64, nchunks = (ntaps + CH - 1) / CH;
      // The taps themselves (radiance and direction: the same for all 64 texels) go through a scratch buffer in device memory,
      // six planes of ntp floats per probe of the pass -- written by this workgroup, read back by it behind a barrier, sixteen
      // taps to a register, a turn ahead of their use: the LDS holds the weights only (18 KiB for chunks of 32 taps; with the taps
      // beside chunks of 64 the pass needed 59 KiB and, with frames in flight, waited for a CU that had them free: -8 % frame
      // rate, measured).
      float *g_dpl = tap_planes + (size_t)blockIdx.x * 6 * ntp; // [3][ntp] the taps' directions, a plane per component
      float *g_rch = g_dpl + 3 * ntp;                            // [3][ntp] their radiance, a plane per channel
      float *s_w = (float *)s_taps;                              // [2][64][S] weights of two chunks, a row per texel
      const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15;
      const int ntex = pr.ires * pr.ires;
      const int x = lane % pr.ires, y = lane / pr.ires;
      const int i = tx * pr.ires + x, j = ty * pr.ires + y;
      const f2 nc = F2((centre(i, pr.pcx * pr.ires) + 1.0f) * 0.5f, (centre(j, pr.pcy * pr.ires) + 1.0f) * 0.5f);
      const f3 irr_dir = ray_id_to_ray_dir(F2(fract_(nc.x * pcx), fract_(nc.y * pcy)));
      // MDH_OPT_PROBE_SETTLE: the RGBA8 word the texel held, asked for here, a whole fold ahead of its use (the lane owns the
      // texel: when the pass runs in place nothing else writes it before this lane's store).  One register; the four of a
      // float32 texel are read behind the fold instead (held through it they cost the kernel a workgroup per CU: 96 -> 98
      // vector registers, measured).
      const unsigned out_idx = atlas_index(pr.pcx, pr.ires, pr.ishift, i, j);
      unsigned out_old8 = 0u;
      if (settle && pr.fmt == 0 && wv == 0 && lane < ntex) out_old8 = atlas_rgba8(prev, out_idx);
#ifdef MDH_PHASES
      const unsigned long long ph_k0 = __builtin_amdgcn_s_memtime();
#endif
      // a thread's taps four at a time: the texels of all four asked for before the first direction is decoded (one round trip
      // to the atlas instead of four)
      for (int t0 = threadIdx.x; t0 < ntaps; t0 += 4 * MDH_IRR_BLOCK) {
         AtlasTap tap[4];
         f2 cc[4];
#pragma unroll
         for (int k = 0; k < 4; ++k) {
            const int t = min(t0 + k * MDH_IRR_BLOCK, ntaps - 1); // (a tap beyond the last: the last one again, not stored)
            const int yy = t / pr.rres, xx = t - yy * pr.rres;
            cc[k] = F2(clamp_(rad_coord.x + (float)xx * step.x, step.x, 1.0f - step.x), clamp_(rad_coord.y + (float)yy * step.y, step.y, 1.0f - step.y));
            tap[k] = atlas_tap_issue(pr.rad, pr.fmt, pr.pcx, pr.pcy, pr.rres, pr.rshift, pr.rad_w, pr.rad_h, cc[k].x, cc[k].y);
         }
#pragma unroll
         for (int k = 0; k < 4; ++k) {
            const int t = t0 + k * MDH_IRR_BLOCK;
            const f3 rad_dir = ray_id_to_ray_dir(F2(fract_(cc[k].x * pcx), fract_(cc[k].y * pcy)));
            const f3 rad = atlas_tap_resolve(pr.rad, pr.fmt, tap[k], -1);
            if (t < ntaps) {
               g_dpl[t] = rad_dir.x; g_dpl[ntp + t] = rad_dir.y; g_dpl[2 * ntp + t] = rad_dir.z;
               g_rch[t] = rad.x; g_rch[ntp + t] = rad.y; g_rch[2 * ntp + t] = rad.z;
            }
         }
      }
      __syncthreads(); // (the workgroup's stores are in L2 behind it; none of these lines was read before: nothing stale in this CU's L1)
#ifdef MDH_PHASES
      const unsigned long long ph_k1 = __builtin_amdgcn_s_memtime();
      unsigned long long ph_work = 0ull, ph_wait = 0ull;
      if (lane == 0) atomicAdd(&g_phase[8 + wv], ph_k1 - ph_k0); // (staging, its barrier included)
#endif
      float acc = 0.0f;
      const float *g_rc = g_rch + (wv < 3 ? wv : 0) * ntp; // this wavefront's channel
      if (ntaps % 64 == 0) {
         // Turns of 64 taps in 64 / CH chunks.  Chunk c: the weights' rows of the chunk asked for, this wavefront's quarter of
         // chunk c + 1's weights computed and stored, the chunk folded, barrier.  The registers of taps of the NEXT turn (radiance
         // of its 64 taps; directions of the sixteen taps whose weights this wavefront computes during it) are asked for at the
         // top of this one.  A direction register of turn s holds, for chunk 2 s + 1 + h (CH = 32; chunk s + 1 for CH = 64),
         // the wavefront's taps in lanes 8 h .. 8 h + 7.
         constexpr int HALVES = 64 / CH, PT = CH / 4, NB = CH / 16, NW = CH / 4;
         const int h16 = HALVES == 2 ? l16 >> 3 : 0, n16 = HALVES == 2 ? l16 & 7 : l16;
         auto dir_tap = [&](int turn) { return min(((turn * HALVES + 1 + h16) * CH + wv * PT + n16), ntp - 1); }; // (beyond the last chunk: never used)
         float dx, dy, dz, rv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
         { const int t = wv * PT + n16; dx = g_dpl[t]; dy = g_dpl[ntp + t]; dz = g_dpl[2 * ntp + t]; }
         irr_produce<0, PT>(dx, dy, dz, s_w + lane * S + wv * PT, irr_dir);
         { const int t = dir_tap(0); dx = g_dpl[t]; dy = g_dpl[ntp + t]; dz = g_dpl[2 * ntp + t]; }
         if (wv < 3) {
#pragma unroll
            for (int b = 0; b < 4; ++b) rv[b] = g_rc[16 * b + l16];
         }
         // (vmcnt (0): with loads pending on entry the compiler's wait-count pass makes every turn of the loop wait for the loads
         //  that turn has just issued)
         __builtin_amdgcn_s_waitcnt(0x0f70);
         asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
         const int nturns = ntaps / 64;
#pragma unroll 1
         for (int turn = 0; turn < nturns; ++turn) {
#ifdef MDH_PHASES
            const unsigned long long ph_t0 = __builtin_amdgcn_s_memtime();
            unsigned long long ph_b = 0ull;
#endif
            float dxn = 0.0f, dyn = 0.0f, dzn = 0.0f, rvn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (turn + 1 < nturns) {
               const int t = dir_tap(turn + 1);
               dxn = g_dpl[t]; dyn = g_dpl[ntp + t]; dzn = g_dpl[2 * ntp + t];
               if (wv < 3) {
#pragma unroll
                  for (int b = 0; b < 4; ++b) rvn[b] = g_rc[(turn + 1) * 64 + 16 * b + l16];
               }
            }
#pragma unroll
            for (int hf = 0; hf < HALVES; ++hf) {
               const int c = turn * HALVES + hf;
               const float *wr = s_w + (c & 1) * 64 * S + lane * S;
               float4 w[NW];
#pragma unroll
               for (int g = 0; g < NW; ++g) w[g] = *(const float4 *)(wr + 4 * g);
               if (c + 1 < nchunks) {
                  float *wn = s_w + ((c + 1) & 1) * 64 * S + lane * S + wv * PT;
                  if (hf == 0) irr_produce<0, PT>(dx, dy, dz, wn, irr_dir);
                  else irr_produce<8, PT>(dx, dy, dz, wn, irr_dir);
               }
               acc = wv < 3 ? irr_fold<true, NB>(rv + hf * NB, w, acc) : irr_fold<false, NB>(rv + hf * NB, w, acc);
#ifdef MDH_PHASES
               const unsigned long long ph_t1 = __builtin_amdgcn_s_memtime();
#endif
               asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#ifdef MDH_PHASES
               ph_b += __builtin_amdgcn_s_memtime() - ph_t1;
#endif
            }
#ifdef MDH_PHASES
            ph_wait += ph_b; ph_work += __builtin_amdgcn_s_memtime() - ph_t0 - ph_b;
#endif
            dx = dxn; dy = dyn; dz = dzn;
#pragma unroll
            for (int b = 0; b < 4; ++b) rv[b] = rvn[b];
         }
      } else {
         // radiance tiles whose texels are no multiple of 64 (not the reference's: 32 x 32): the same four chains tap by tap
         for (int c = 0; c <= nchunks; ++c) { // (turn c: the weights of chunk c, the fold of chunk c - 1)
            if (c < nchunks) {
               const int t0 = c * CH + wv * CHQ, t1 = min(t0 + CHQ, ntaps);
               float *wb = s_w + (c & 1) * 64 * S + lane * S - c * CH;
               for (int t = t0; t < t1; ++t) wb[t] = max_((irr_dir.x * g_dpl[t] + irr_dir.y * g_dpl[ntp + t]) + irr_dir.z * g_dpl[2 * ntp + t], 0.0f);
            }
            if (c > 0) {
               const int nh = min(CH, ntaps - (c - 1) * CH);
               const float *wr = s_w + ((c - 1) & 1) * 64 * S + lane * S, *rc = g_rc + (c - 1) * CH;
               for (int t = 0; t < nh; ++t) acc = wv < 3 ? acc + rc[t] * wr[t] : acc + wr[t];
            }
            __syncthreads();
         }
      }
#ifdef MDH_PHASES
      if (lane == 0) { atomicAdd(&g_phase[2 * wv], ph_work); atomicAdd(&g_phase[2 * wv + 1], ph_wait); }
#endif
      // the four sums of a texel back to one lane (through the weight rows: the loop's last barrier is behind every read of them)
      if (wv > 0) s_w[(wv - 1) * 64 + lane] = acc;
      __syncthreads();
      if (wv == 0) {
         bool changed = false;
         if (lane < ntex) {
            const f3 irradiance = F3(acc, s_w[lane], s_w[64 + lane]) / s_w[128 + lane];
            const f3 v = irradiance_blend(pr, prev, hyst, out_idx, irradiance);
            if (settle) {
               AtlasBits out_old = {out_old8, 0u, 0u, 0u};
               if (pr.fmt != 0) out_old = atlas_bits(prev, pr.fmt, out_idx);
               changed = atlas_store_changed(pr.irr, pr.fmt, out_idx, v, out_old);
            } else atlas_store(pr.irr, pr.fmt, out_idx, v);
         }
         // (behind the store: the fold's last wavefront has nothing left to do but this)
         if (settle) { const unsigned n = (unsigned)__popcll(__ballot(changed)); if (lane == 0) settle_report(sa, n, gridDim.x); }
      }
      return;
   }
   if (pr.ires * pr.ires <= 64) {
      // One wavefront folds (a lane per texel).  The taps go through LDS in chunks of MDH_IRR_CHUNK, two buffers: while the
      // folding wavefront works on chunk c, the others stage chunk c + 1.  The same taps in the same order; a quarter of
      // the LDS (room for the march kernels' workgroups beside it) and the staging hidden.
      constexpr int CH = MDH_IRR_CHUNK;
      const int nchunks = (ntaps + CH - 1) / CH;
      const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
      const int x = lane % pr.ires, y = lane / pr.ires; // (used by the folding lanes only)
      const int i = tx * pr.ires + x, j = ty * pr.ires + y;
      const f2 nc = F2((centre(i, pr.pcx * pr.ires) + 1.0f) * 0.5f, (centre(j, pr.pcy * pr.ires) + 1.0f) * 0.5f);
      const f3 irr_dir = ray_id_to_ray_dir(F2(fract_(nc.x * pcx), fract_(nc.y * pcy)));
      pk2 acc_xy = {0.0f, 0.0f}, acc_zw = {0.0f, 0.0f};
      const pk2 dir_xy = {irr_dir.x, irr_dir.y};
      for (int t = threadIdx.x; t < min(CH, ntaps); t += MDH_IRR_BLOCK) MDH_IRR_STAGE(t, t);
      __syncthreads();
      for (int c = 0; c < nchunks; ++c) {
         const int base = c * CH, n_here = min(CH, ntaps - base);
         const float4 *buf = s_taps + (size_t)(c & 1) * 2 * CH;
         if (wv == 0) {
            if (lane < pr.ires * pr.ires) {
#define MDH_IRR_FOLD(r_, d_)                                                                  \
               do {                                                                           \
                  const float4 r = (r_), d = (d_);                                            \
                  const pk2 d_xy = {d.x, d.y}, r_xy = {r.x, r.y}, r_z1 = {r.z, r.w};          \
                  const pk2 p = dir_xy * d_xy;                                                \
                  const float w = max_((p.x + p.y) + irr_dir.z * d.z, 0.0f);                  \
                  const pk2 ww = {w, w};                                                      \
                  acc_xy = acc_xy + r_xy * ww;                                                \
                  acc_zw = acc_zw + r_z1 * ww;                                                \
               } while (0)
               // six taps per turn in two groups of three, each group on its way from LDS while the other is folded (the
               // folding wavefront is the pass's critical path: 1 024 taps in the reference's order, each waiting for its two
               // LDS reads otherwise).  Three: two groups in flight are 12 LDS reads, and the counter a wavefront waits on holds 15.
#define MDH_IRR_FOLD_CHUNK()                                                                  \
               do {                                                                           \
                  constexpr int GR = 3;                                                       \
                  const int nt = n_here - n_here % (2 * GR);                                  \
                  int t = 0;                                                                  \
                  float4 ra[GR], da[GR], rb[GR], db[GR];                                      \
                  if (nt > 0) {                                                               \
                     _Pragma("unroll") for (int k = 0; k < GR; ++k) { ra[k] = buf[2 * k]; da[k] = buf[2 * k + 1]; } \
                  }                                                                           \
                  _Pragma("unroll 1") for (; t < nt; t += 2 * GR) {                           \
                     _Pragma("unroll") for (int k = 0; k < GR; ++k) { rb[k] = buf[2 * (t + GR + k)]; db[k] = buf[2 * (t + GR + k) + 1]; } \
                     _Pragma("unroll") for (int k = 0; k < GR; ++k) MDH_IRR_FOLD(ra[k], da[k]); \
                     const int tn = t + 2 * GR < nt ? t + 2 * GR : t; /* (the last turn reads its own taps again) */ \
                     _Pragma("unroll") for (int k = 0; k < GR; ++k) { ra[k] = buf[2 * (tn + k)]; da[k] = buf[2 * (tn + k) + 1]; } \
                     _Pragma("unroll") for (int k = 0; k < GR; ++k) MDH_IRR_FOLD(rb[k], db[k]); \
                  }                                                                           \
                  for (; t < n_here; ++t) MDH_IRR_FOLD(buf[2 * t], buf[2 * t + 1]);           \
               } while (0)
               MDH_IRR_FOLD_CHUNK();
#undef MDH_IRR_FOLD_CHUNK
#undef MDH_IRR_FOLD
            }
         } else if (c + 1 < nchunks) {
            const int nbase = base + CH, n_next = min(CH, ntaps - nbase), off = ((c + 1) & 1) * CH;
            for (int t = (int)threadIdx.x - 64; t < n_next; t += MDH_IRR_BLOCK - 64) MDH_IRR_STAGE(nbase + t, off + t);
         }
         __syncthreads();
      }
      if (wv == 0) {
         bool changed = false;
         if (lane < pr.ires * pr.ires) {
            const f3 irradiance = F3(acc_xy.x, acc_xy.y, acc_zw.x) / acc_zw.y;
            const unsigned idx = atlas_index(pr.pcx, pr.ires, pr.ishift, i, j);
            const f3 v = irradiance_blend(pr, prev, hyst, idx, irradiance);
            if (settle) changed = atlas_store_changed(pr.irr, pr.fmt, idx, v, atlas_bits(prev, pr.fmt, idx));
            else atlas_store(pr.irr, pr.fmt, idx, v);
         }
         if (settle) { const unsigned n = (unsigned)__popcll(__ballot(changed)); if (lane == 0) settle_report(sa, n, gridDim.x); }
      }
      return;
   }
   for (int tap = threadIdx.x; tap < ntaps; tap += MDH_IRR_BLOCK) MDH_IRR_STAGE(tap, tap);
#undef MDH_IRR_STAGE
   __syncthreads();
   unsigned n_changed = 0u; // (this lane's texels)
   for (int rem = threadIdx.x; rem < pr.ires * pr.ires; rem += MDH_IRR_BLOCK) {
      const int y = rem / pr.ires, x = rem - y * pr.ires;
      const int i = tx * pr.ires + x, j = ty * pr.ires + y;
      const f2 nc = F2((centre(i, pr.pcx * pr.ires) + 1.0f) * 0.5f, (centre(j, pr.pcy * pr.ires) + 1.0f) * 0.5f);
      const f3 irr_dir = ray_id_to_ray_dir(F2(fract_(nc.x * pcx), fract_(nc.y * pcy)));
      f3 irradiance = F3(0.0f, 0.0f, 0.0f);
      float total_weight = 0.0f;
      // the same operations, two per instruction: (x, y) and (z, weight) pairs.  1.0f * w = w exactly.
      pk2 acc_xy = {0.0f, 0.0f}, acc_zw = {0.0f, 0.0f};
      const pk2 dir_xy = {irr_dir.x, irr_dir.y};
      for (int tap = 0; tap < ntaps; ++tap) {
         const float4 r = s_taps[2 * tap], d = s_taps[2 * tap + 1];
         const pk2 d_xy = {d.x, d.y}, r_xy = {r.x, r.y}, r_z1 = {r.z, r.w};
         const pk2 p = dir_xy * d_xy;
         const float w = max_((p.x + p.y) + irr_dir.z * d.z, 0.0f);
         const pk2 ww = {w, w};
         acc_xy = acc_xy + r_xy * ww;
         acc_zw = acc_zw + r_z1 * ww;
      }
      irradiance = F3(acc_xy.x, acc_xy.y, acc_zw.x);
      total_weight = acc_zw.y;
      irradiance = irradiance / total_weight;
      const unsigned idx = atlas_index(pr.pcx, pr.ires, pr.ishift, i, j);
      const f3 v = irradiance_blend(pr, prev, hyst, idx, irradiance);
      if (settle) n_changed += atlas_store_changed(pr.irr, pr.fmt, idx, v, atlas_bits(prev, pr.fmt, idx)) ? 1u : 0u;
      else atlas_store(pr.irr, pr.fmt, idx, v);
   }
   if (settle) { // the wavefronts' counts through LDS (behind the last read of the taps), then one lane of the workgroup reports
      for (int off = 32; off > 0; off >>= 1) n_changed += (unsigned)__shfl_xor((int)n_changed, off);
      unsigned *s_cnt = (unsigned *)s_taps;
      __syncthreads();
      if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n_changed;
      __syncthreads();
      if (threadIdx.x == 0) {
         unsigned n = 0u;
         for (int w = 0; w < MDH_IRR_BLOCK / 64; ++w) n += s_cnt[w];
         settle_report(sa, n, gridDim.x);
      }
   }
}

// -------------------------------------------------------------------- visibility pass
// compute_frustrum_visibility.glsl:8-42: one visibility ray per froxel (x, y, depth slice) and light.
//
// One froxel per lane, in lock step: a wavefront marches until its longest ray ends, 34 of 64 lanes alive per step (r03_c4_*).
// (measured on MI355X, light_shafts 1080p: the rays of a wavefront's froxels as a queue with replacement, in two forms, took
//  the pass from 0.067 to 0.109 ms on its own and -1.5 % in flight -- serving a lane is ~250 instructions under a sparse mask,
//  as much as its march saves: DESIGN.md; two and four froxels per lane, one after the other: 0.074 -> 0.100 / 0.153 ms alone,
//  +-0 in flight -- it is the length of a wavefront's chain, not the staging of the table)
// the froxel texel (i, j) at place `lin` of the launch.  Which froxels share a wavefront decides how many of its lanes march
// together: the texture is vw x (vh * vz) texels, row j = slice * vh + y, and in launch order a wavefront of the reference's
// 100^3 froxels was a strip of 64 froxels along x (100 is no multiple of 8: no 8x8 tiles either).  Hence blocks of
// 4 x 4 froxels x 4 depth slices -- neighbours in space, whose rays to a light pass the same geometry.
MDH_DEV void froxel_texel(const KVolumetrics &vol, int W, int H, long lin, int &i, int &j)
{
   if (((vol.vw | vol.vh | vol.vz) & 3) == 0) {
      const long blk = lin >> 6;
      const int l = (int)(lin & 63), bxn = vol.vw >> 2, byn = vol.vh >> 2;
      const int bx = (int)(blk % bxn);
      const long rest = blk / bxn;
      const int by = (int)(rest % byn), bz = (int)(rest / byn);
      i = bx * 4 + (l & 3);
      j = (bz * 4 + (l >> 4)) * vol.vh + by * 4 + ((l >> 2) & 3);
   } else if ((W & 7) == 0 && (H & 7) == 0) {
      const long tile = lin >> 6;
      const int l = (int)(lin & 63), tpr = W >> 3;
      i = (int)(tile % tpr) * 8 + (l & 7);
      j = (int)(tile / tpr) * 8 + (l >> 3);
   } else {
      j = (int)(lin / W);
      i = (int)(lin - (long)j * W);
   }
}
// its sample point and the direction of its camera ray (compute_frustrum_visibility.glsl:22-37)
MDH_DEV void froxel_point(const KVolumetrics &vol, const KCamera &cam, int W, int H, int i, int j, f3 &pos, f3 &dir)
{
   const float px = centre(i, W), py = centre(j, H);
   const float norm_height = (py + 1.0f) * 0.5f;
   const float tex_height = norm_height * (float)vol.vz;
   const float depth = __builtin_floorf(tex_height);
   const float fract_height = tex_height - depth;
   const float frag_height = fract_height * 2.0f - 1.0f;
   f3 origin;
   camera_ray(cam, px, frag_height, origin, dir);
   pos = origin + (dir * depth) * vol.vstep;
}
// the texel's ray length: raycast (raymarching.glsl:25-37) without the arg-min -- only the collision point is used here
template <int PART> MDH_DEV float scattering_length(const KScene &sc, const KVolumetrics &vol, const KCamera &cam, int i, int j)
{
   const float px = centre(i, vol.sw), py = centre(j, vol.sh);
   f3 from, dir;
   camera_ray(cam, px, py, from, dir);
   const float max_depth = vol.vstep * (float)vol.vz; // volumetrics.glsl:3-4
   f3 to = from + dir * max_depth;
   int steps;
   float t;
   if (march_plain<PART>(sc, from, dir, sc.max_dist, t, steps)) to = from + dir * t;
   return min_(length(to - from), max_depth);
}
// `vis_blocks`: the workgroups of the launch that work on froxels; the ones behind them march the camera rays of the
// SCATTERING texels (k_scat_march's work: the texels' lengths, which depend on the camera and the scene only).  That march is
// a thousand wavefronts whose longest ray alone takes 40 us: inside this launch it hides under the froxels' rays (frames
// only: a single visibility pass leaves the scattering texture alone, pass_scattering).
template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_visibility(KScene sc, KVolumetrics vol, KCamera cam, int vis_blocks)
{
   stage_table(sc);
   if ((int)blockIdx.x >= vis_blocks) { // (workgroup-uniform)
      const long lin = (long)((int)blockIdx.x - vis_blocks) * MDH_BLOCK + threadIdx.x;
      if (lin >= (long)vol.sw * vol.sh) return;
      const int j = (int)(lin / vol.sw), i = (int)(lin - (long)j * vol.sw);
      vol.scat[(size_t)j * vol.sw + i].w = scattering_length<PART>(sc, vol, cam, i, j);
      return;
   }
   const int W = vol.vw, H = vol.vh * vol.vz;
   const long n = (long)W * H;
   // (a loop of ONE turn, left over from the measurement of two and four froxels per lane: without it the compiler allocates the
   //  kernel's registers differently -- removing it is a change of the kernel, to be measured as one)
#pragma unroll 1
   for (int turn = 0; turn < 1; ++turn) {
      const long lin = ((long)blockIdx.x + turn) * MDH_BLOCK + threadIdx.x;
      if (lin >= n) return;
      int i, j;
      froxel_texel(vol, W, H, lin, i, j);
      f3 pos, dir;
      froxel_point(vol, cam, W, H, i, j, pos, dir);
      f3 result = F3(0.0f, 0.0f, 0.0f);
      for (int l = 0; l < sc.total_lights; ++l) { // sample_lights :8-19
         f3 L;
         float L_dist;
         f3 radiance = sample_light<(PART & MDH_PF_CUSTOM) != 0>(sc, l, pos, F3(1.0f, 0.0f, 0.0f), L, L_dist); // compute_frustrum_visibility.glsl:12
         float visibility = raycast_visibility<PART>(sc, pos, L, L_dist);
         f3 L_in = radiance * (sexp(-L_dist * MDH_TAU) * visibility);
         result = result + (L_in * MDH_TAU) * henvey_greenstein_phase(L, dir);
      }
      float *o = vol.vis + ((size_t)j * W + i) * 3;
      o[0] = result.x; o[1] = result.y; o[2] = result.z;
   }
}

// -------------------------------------------------------------------- scattering pass
// accumulate_scattering.glsl:9-48.  Round 4: two kernels.
//   k_scat_march  one lane per scattering texel: the camera ray's collision point -> len (the texel's fourth component)
//   k_scat_fold   a texel's steps SPREAD OVER LANES.  Until round 3 one lane walked its texel's <= 100 froxel taps by itself
//                 (batches of 8 in flight): 980 wavefronts on 1 024 SIMDs, 142 VGPRs, 10.8 % of the VALU issue peak.  A step's
//                 tap and its exp (-f tau) factor depend on the texel and the step only, and f runs through the same values
//                 for every texel (f_0 = 0, f_k+1 = f_k + step in fp32): a workgroup takes MDH_SCAT_TEXELS texels, computes
//                 f_k, floor (f_k / froxel step) and exp (-f_k tau) once per step into LDS, then every (texel, step) pair's
//                 product tap * factor -- one lane each, all in flight together -- and finally one lane per texel and CHANNEL
//                 adds its products IN STEP ORDER (the same additions in the same order: the same bits).
#ifndef MDH_SCAT_SPLIT
#define MDH_SCAT_SPLIT 1
#endif
#ifndef MDH_SCAT_TEXELS
#define MDH_SCAT_TEXELS 16 // texels per workgroup of k_scat_fold (a power of two, at most 64)
#endif
#ifndef MDH_SCAT_CHUNK
#define MDH_SCAT_CHUNK 128 // steps whose products are in LDS together (16 texels x 128 steps x 12 B = 24 KB)
#endif
#ifndef MDH_SCAT_BLOCK
#define MDH_SCAT_BLOCK 256 // threads of k_scat_fold (measured 1 024: two workgroups per CU, the pass 0.045 -> 0.172 ms)
#endif
template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_scat_march(KScene sc, KVolumetrics vol, KCamera cam)
{
   stage_table(sc);
   const int W = vol.sw, H = vol.sh;
   const long lin = (long)blockIdx.x * MDH_BLOCK + threadIdx.x;
   if (lin >= (long)W * H) return;
   const int j = (int)(lin / W), i = (int)(lin - (long)j * W);
   vol.scat[(size_t)j * W + i].w = scattering_length<PART>(sc, vol, cam, i, j);
}
#ifndef MDH_JIT
__global__ __launch_bounds__(MDH_SCAT_BLOCK) void k_scat_fold(KVolumetrics vol)
{
   constexpr int T = MDH_SCAT_TEXELS, CH = MDH_SCAT_CHUNK;
   __shared__ float s_f[CH], s_rel[CH], s_e[CH]; // per step of the chunk: f, floor (f / froxel step), exp (-f tau)
   __shared__ float s_len[T];
   __shared__ int s_n[T];                        // steps of each texel: the k with f_k < len
   __shared__ float s_prod[CH][3][T];
   const int W = vol.sw, H = vol.sh, tid = threadIdx.x;
   const long first = (long)blockIdx.x * T, n_tex = (long)W * H;
   const float max_depth = vol.vstep * (float)vol.vz;
   if (tid < T) {
      const long lin = first + tid;
      s_len[tid] = lin < n_tex ? vol.scat[lin].w : 0.0f; // (k_scat_march)
      s_n[tid] = 0;
   }
   // lanes of the fold: channel c of texel t
   const int fc = tid / T, ft = tid % T;
   const bool folder = tid < 3 * T && first + ft < n_tex;
   float acc = 0.0f;
   for (int c0 = 0;; c0 += CH) {
      // the chunk's steps: f by the loop's own additions (every texel's loop runs through these values)
      if (tid < T) s_n[tid] = 0; // (steps of this chunk: set by the pair that holds the texel's last one)
      if (tid < CH) {
         float f = 0.0f;
         for (int q = 0; q < c0 + tid; ++q) f += vol.sstep;
         s_f[tid] = f;
         s_rel[tid] = __builtin_floorf(f / vol.vstep); // sample_visibility :9-15
         s_e[tid] = sexp(-f * MDH_TAU);
      }
      __syncthreads();
      if (!(s_f[0] < max_depth)) break; // (len <= max_depth: no texel has a step here; uniform)
      // (texel, step) pairs: the tap and its factor, one lane each -- four pairs per lane and turn, their 48 texel loads all in
      // flight together (pairs without a step -- f past the texel's length, a texel past the image -- load nothing: sampled
      // all the same, as the one-kernel form did, they double the pass's loads and it takes 0.066 instead of 0.045 ms)
      for (int p0 = tid; p0 < T * CH; p0 += 4 * MDH_SCAT_BLOCK) {
         float tx[4][3];
         bool live[4];
#pragma unroll
         for (int u = 0; u < 4; ++u) {
            const int p = p0 + u * MDH_SCAT_BLOCK;
            const int t = p % T, k = min(p / T, CH - 1);
            const long lin = min(first + t, n_tex - 1);
            live[u] = p < T * CH && first + t < n_tex && s_f[k] < s_len[t];
            tx[u][0] = tx[u][1] = tx[u][2] = 0.0f;
            if (live[u]) {
               const int j = (int)(lin / W), i = (int)(lin - (long)j * W);
               const f2 norm_pos = F2(0.5f * (centre(i, W) + 1.0f), 0.5f * (centre(j, H) + 1.0f));
               tex_sample<3>(vol.vis, vol.vw, vol.vh * vol.vz, norm_pos.x, (norm_pos.y + s_rel[k]) / (float)vol.vz, tx[u]);
               // (the last of the texel's steps in this chunk says how many there are: f grows, the steps are a prefix)
               if (k + 1 == CH || !(s_f[k + 1] < s_len[t])) s_n[t] = k + 1;
            }
         }
#pragma unroll
         for (int u = 0; u < 4; ++u) {
            const int p = p0 + u * MDH_SCAT_BLOCK;
            const int t = p % T, k = min(p / T, CH - 1);
            if (live[u]) {
               const f3 pr = F3(tx[u][0], tx[u][1], tx[u][2]) * s_e[k];
               s_prod[k][0][t] = pr.x; s_prod[k][1][t] = pr.y; s_prod[k][2][t] = pr.z;
            }
         }
      }
      __syncthreads();
      if (folder) { // L = L + tap * factor, step by step (eight products on their way from LDS at a time)
         const int m = s_n[ft];
         int k = 0;
         for (; k + 8 <= m; k += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = s_prod[k + q][fc][ft];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = acc + v[q];
         }
         for (; k < m; ++k) acc = acc + s_prod[k][fc][ft];
      }
      if (!__syncthreads_or(tid < T && s_n[tid] == CH)) break; // some texel filled the chunk: its loop goes on
   }
   if (folder) ((float *)&vol.scat[first + ft])[fc] = acc * vol.sstep;
}
#endif
// (the one-kernel form of rounds 1 to 3: MDH_SCAT_SPLIT = 0 and the literal build)
template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_scattering(KScene sc, KVolumetrics vol, KCamera cam)
{
   stage_table(sc);
   const int W = vol.sw, H = vol.sh;
   const long lin = (long)blockIdx.x * MDH_BLOCK + threadIdx.x;
   if (lin >= (long)W * H) return;
   const int j = (int)(lin / W), i = (int)(lin - (long)j * W);
   const float px = centre(i, W), py = centre(j, H);
   const f2 norm_pos = F2(0.5f * (px + 1.0f), 0.5f * (py + 1.0f));
   const float len = scattering_length<PART>(sc, vol, cam, i, j);
   f3 L = F3(0.0f, 0.0f, 0.0f);
   // The froxel taps of consecutive steps are independent, but each costs a trip to L2/HBM and the
   // pass has one wavefront per SIMD: steps go in batches of MDH_SCAT_BATCH whose loads are all in
   // flight together, then fold into L in step order (a step past `len` loads a valid texel and is
   // not added).  f runs through the same values as the reference's loop.
   for (float f = 0.0f; f < len;) {
      float fs[MDH_SCAT_BATCH], tx[MDH_SCAT_BATCH][3];
#pragma unroll
      for (int k = 0; k < MDH_SCAT_BATCH; ++k) {
         fs[k] = f;
         const float rel = __builtin_floorf(f / vol.vstep); // sample_visibility :9-15
         tex_sample<3>(vol.vis, vol.vw, vol.vh * vol.vz, norm_pos.x, (norm_pos.y + rel) / (float)vol.vz, tx[k]);
         f += vol.sstep;
      }
#pragma unroll
      for (int k = 0; k < MDH_SCAT_BATCH; ++k)
         if (fs[k] < len) L = L + F3(tx[k][0], tx[k][1], tx[k][2]) * exp_(-fs[k] * MDH_TAU);
   }
   L = L * vol.sstep;
   vol.scat[(size_t)j * W + i] = make_float4(L.x, L.y, L.z, len);
}

// ---------------------------------------------------------------- partition-table build
struct PartBuildArgs {
   int method;     // 0 CPU_Best, 1 CPU_Fast, 2 GPU_Fast (renderers.ads:93)
   int gx, gy, gz; // cells visited; GPU_Fast: 2 * (dims / 2), the compute dispatch of renderers.adb:539-549
   float sp[3], off[3];
   float gpu_diag; // Length(spacing) as the generated GLSL text carries it (scenes.adb:1140-1143)
   int *table;     // [cell][nk + index_count]
   int *warnings;
};
#define MDH_PART_MAX_PRE 256

// distance of primitive i of kind k through the table; ADA_DIV for the CPU builders, which
// go through Primitives.Eval_Dist (madarch-primitives.adb:90-108)
// GTAB: global residency of the scene table (mdh_device.h: Geo); UNI (with it): k and i are wave-uniform, and said to be
template <bool ADA_DIV, bool GTAB = false, bool UNI = false> MDH_DEV float part_dist(const KScene &sc, int k, int i, f3 x)
{
   const typename Geo<GTAB>::F4 s_tab = Geo<GTAB>::f4(sc); // (shadows the LDS table)
   // k may differ per lane here (candidate lists): plain per-lane header reads, not hdr()
   const int type = uni<UNI>(tab_int(H_KTYPE + k)), slot = uni<UNI>(tab_int(H_KSLOT + k) + prim_slots(type) * i);
   if (type == PK_CUSTOM) { // the program must be wave-uniform: one round per user-defined kind, its lanes active
      float r = 0.0f;
      const int nk = hdr(H_NK);
      for (int kk = 0; kk < nk; ++kk)
         if (hdr(H_KTYPE + kk) == PK_CUSTOM && k == kk) r = xdist<ADA_DIV>(kk, i, x);
      return r;
   }
   if (type == PK_TRIANGLE) return sd_triangle<ADA_DIV>(xyz(s_tab[slot]), xyz(s_tab[slot + 1]), xyz(s_tab[slot + 2]), x);
   return prim_dist(s_tab, type, slot, x);
}

// ONE WAVEFRONT PER GRID CELL (round 4; until round 3 one LANE per cell walked every loop below by itself, its candidate
// arrays in 784 bytes of scratch memory: 0.49 ms for simple_scene's 2 000 cells on 32 wavefronts, every frame of ball_game).
// Update_Partitioning_CPU (renderers.adb:551-755) for methods 0/1, partitioning_compute_grid_cell (scenes.adb:1120-1187)
// for method 2.  The reference's loops are kept as SETS and ORDERS, not as schedules:
//   * the closest primitive at the cell's centre: lanes = the instances of one kind at a time (a uniform type: no
//     divergence), a wave minimum -- min is order-free;
//   * the pre-candidates (closer than closest + the cell's diagonal) in scene order: ballot ranks, kind by kind;
//   * CPU_Best's 27 sample points (Find_Candidates, renderers.adb:669-723): lane s = sample point s in the reference's
//     loop order, the pre-candidates walked uniformly (LDS broadcasts) with the reference's strict `<` (the first of
//     equal distances wins); the points then accept their winners in order, which numbers them as the reference does;
//   * the lists, kind by kind in acceptance order, cut at Index_Count with one warning per overflowing kind
//     (Write_Partitioning_Info, renderers.adb:578-608).
MDH_DEV float wave_min(float v)
{
#pragma unroll
   for (int o = 32; o > 0; o >>= 1) v = min_(v, __shfl_xor(v, o));
   return v;
}
template <bool GTAB> MDH_DEV void partition_build(const KScene &sc, const PartBuildArgs &a)
{
   __shared__ unsigned short s_pre[MDH_PART_MAX_PRE]; // (kind << 12) | index, in scene order
   __shared__ unsigned char s_acc[MDH_PART_MAX_PRE];  // method 0: the candidate's acceptance number (0: not accepted)
   __shared__ unsigned short s_ord[32];               // method 0: the candidate accepted as number s + 1
   stage_table(sc);
   const int lin = blockIdx.x, lane = threadIdx.x;
   if (lin >= a.gx * a.gy * a.gz) return;
   const int X = lin / (a.gy * a.gz), Y = (lin / a.gz) % a.gy, Z = lin % a.gz;
   const int cell = X * a.gy * a.gz + Y * a.gz + Z;
   if (cell >= sc.part_cells) return;
   const f3 sp = F3(a.sp[0], a.sp[1], a.sp[2]), off = F3(a.off[0], a.off[1], a.off[2]);
   const int nk = hdr(H_NK);
   int npre = 0, nacc = 0;
   // every instance of every kind against `thr` at `center`, appended in scene order
#define MDH_PART_COLLECT(ADA_, center_, thr_)                                                                                \
   for (int k = 0; k < nk; ++k) {                                                                                           \
      const int n = hdr(H_KCOUNT + k);                                                                                      \
      for (int c = 0; c < n; c += 64) {                                                                                     \
         const int i = c + lane;                                                                                            \
         const bool in = i < n;                                                                                             \
         const float d = part_dist<ADA_, GTAB>(sc, k, in ? i : 0, center_);                                                 \
         const bool take = in && d < (thr_);                                                                                \
         const unsigned long long m = __ballot(take);                                                                       \
         const int at = npre + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); \
         if (take && at < MDH_PART_MAX_PRE) { s_pre[at] = (unsigned short)((k << 12) | i); s_acc[at] = 0; }                  \
         npre = min(MDH_PART_MAX_PRE, npre + (int)__popcll(m));                                                             \
      }                                                                                                                     \
   }
   if (a.method == 2) {
      const f3 center = (F3((float)X, (float)Y, (float)Z) + F3s(0.5f)) * sp + off;
      const float thr = closest_primitive<!GTAB, false, GTAB>(sc, center) + a.gpu_diag; // (global residency: no user-defined kinds, commit_scene)
      MDH_PART_COLLECT(false, center, thr)
   } else {
      const f3 grid_pos = F3((float)X, (float)Y, (float)Z) * sp + off;
      const float cell_diag = length(sp);
      const f3 center = grid_pos + sp * 0.5f;
      float closest = 1.0e10f;
      for (int k = 0; k < nk; ++k) {
         const int n = hdr(H_KCOUNT + k);
         for (int c = 0; c < n; c += 64)
            if (c + lane < n) closest = min_(closest, part_dist<true, GTAB>(sc, k, c + lane, center));
      }
      closest = wave_min(closest);
      MDH_PART_COLLECT(true, center, closest + cell_diag)
      if (a.method == 0) { // Find_Candidates, renderers.adb:669-723: 3x3x3 sample points, lane = point
         const int sx = lane / 9 + 1, sy = (lane / 3) % 3 + 1, sz = lane % 3 + 1;
         const f3 offv = (F3((float)sx, (float)sy, (float)sz) - F3s(1.0f)) / (F3s(3.0f) - F3s(1.0f));
         const f3 pt = offv * sp + grid_pos;
         float c = 1.0e10f;
         int ci = -1;
         for (int q = 0; q < npre; ++q) {
            const int e = __builtin_amdgcn_readfirstlane((int)s_pre[q]);
            const float d = part_dist<true, GTAB, GTAB>(sc, e >> 12, e & 0xfff, pt); // (one pre-candidate for all 27 points: a scalar load out of the image)
            if (d < c) { c = d; ci = q; }
         }
         // acceptance ORDER defines the order of a kind's indices: the points accept in the reference's loop order
         // (every lane keeps the same books: its own stores are what it reads back)
         for (int s = 0; s < 27; ++s) {
            const int q = __builtin_amdgcn_readlane(ci, s);
            if (q >= 0 && s_acc[q] == 0) { s_ord[nacc] = (unsigned short)q; s_acc[q] = (unsigned char)(++nacc); }
         }
      }
   }
#undef MDH_PART_COLLECT
   // write counts and indices kind by kind (Write_Partitioning_Info, renderers.adb:578-608);
   // the reference only warns when a cell overflows Index_Count, here the list is cut
   int *rec = a.table + (size_t)cell * (nk + sc.part_index_count);
   int written = 0;
   const int nlist = a.method == 0 ? nacc : npre; // the accepted candidates, in the order their kind's entries keep
   for (int k = 0; k < nk; ++k) {
      int n = 0;
      for (int c = 0; c < nlist; c += 64) {
         const int j = c + lane;
         const int e = j < nlist ? (int)s_pre[a.method == 0 ? (int)s_ord[j] : j] : -1;
         const bool mine = e >= 0 && (e >> 12) == k;
         const unsigned long long m = __ballot(mine);
         const int at = written + n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
         if (mine && at < sc.part_index_count) rec[nk + at] = e & 0xfff;
         n += (int)__popcll(m);
      }
      if (written + n > sc.part_index_count) {
         if (lane == 0) atomicAdd(a.warnings, 1);
         n = sc.part_index_count - written;
      }
      if (lane == 0) rec[k] = n;
      written += n;
   }
}
__global__ __launch_bounds__(64) void k_partition_build(KScene sc, PartBuildArgs a) { partition_build<false>(sc, a); }
template <int = 0> __global__ __launch_bounds__(64) void k_partition_build_gtab(KScene sc, PartBuildArgs a) { partition_build<true>(sc, a); } // global residency of the scene table (a template: built where it is first named, mdh_api.hip: kernel_ptr)

// The candidate lists of every cell once more as one bit per declared primitive (partitioning_closest_bits,
// mdh_device.h), derived from the lists exactly as the lookup walks them: kind by kind, a kind's entries up to its
// count, the whole walk cut at Index_Count.  One lane per cell; runs behind every build on the build's stream.
__global__ __launch_bounds__(64) void k_partition_bits(KScene sc, int *table)
{
   stage_table(sc);
   const int cell = blockIdx.x * 64 + threadIdx.x;
   if (cell >= sc.part_cells) return;
   const int nk = hdr(H_NK);
   const int *rec = table + (size_t)cell * (nk + sc.part_index_count);
   unsigned *words = (unsigned *)(table + sc.part_mask_off) + (size_t)cell * sc.part_mask_words;
   for (int q = 0; q < sc.part_mask_words; ++q) words[q] = 0u;
   int i = 0;
   for (int k = 0; k < nk; ++k) {
      const int size = i + rec[k], base = hdr(H_KBASE + k), kmax = hdr(H_KMAX + k);
      const int stop = min(size, sc.part_index_count);
      for (; i < stop; ++i) {
         const int pi = rec[nk + i];
         if (pi >= 0 && pi < kmax) words[(base + pi) >> 5] |= 1u << ((base + pi) & 31);
      }
      i = size;
   }
}

// ------------------------------------------------------------------- Eval_Distance_To
// renderers.adb:499-526, one query point per lane
struct EvalArgs {
   int n, n_kinds;
   int kinds[MDH_MAX_KINDS];
   int host_count[MDH_MAX_KINDS];
   const float *pts;
   float *normals;
   float *dist;
};
template <bool ADA_DIV, bool GTAB, bool BVH = false> MDH_DEV void eval_distance(const KScene &sc, const EvalArgs &a)
{
   const typename Geo<GTAB>::F4 s_tab = Geo<GTAB>::f4(sc); // (shadows the LDS table)
   stage_table(sc);
   const int q = blockIdx.x * 64 + threadIdx.x;
   if (q >= a.n) return;
   const f3 p = F3(a.pts[3 * q], a.pts[3 * q + 1], a.pts[3 * q + 2]);
   float closest = 1.0e10f;
   f3 normal = F3(0.0f, 0.0f, 0.0f);
   for (int kk = 0; kk < a.n_kinds; ++kk) {
      const int k = a.kinds[kk], type = hdr(H_KTYPE + k);
      // MDH_PF_BVH: the committed triangles through their hierarchy (bvh_triangles, mdh_device.h) -- the arg-min keeps the
      // lowest index of equal distances, as the loop below does, and the normal is computed once, for the winner
      if (BVH && !ADA_DIV && type == PK_TRIANGLE && hdr(H_KSLOT + k) == sc.tslot[PK_TRIANGLE] && a.host_count[k] == sc.tcount[PK_TRIANGLE]) {
         int best = -1;
         bvh_triangles<true>(sc, p, closest, best, 0);
         if (best >= 0) {
            const int slot = hdr(H_KSLOT + k) + 3 * best;
            normal = nrm_triangle<ADA_DIV>(xyz(s_tab[slot]), xyz(s_tab[slot + 1]), xyz(s_tab[slot + 2]), p);
         }
         continue;
      }
      for (int i = 0; i < a.host_count[k]; ++i) {
         float d = part_dist<ADA_DIV, GTAB, GTAB>(sc, k, i, p);
         if (d < closest) {
            closest = d;
            const int slot = hdr(H_KSLOT + k) + prim_slots(type) * i;
            float4 A = s_tab[uni<GTAB>(slot)];
            switch (type) {
            case PK_CUSTOM: normal = xnormal<ADA_DIV>(k, i, p); break;
            case PK_SPHERE: normal = normalize(p - xyz(A)); break;
            case PK_PLANE: normal = xyz(A); break;
            case PK_BOX: normal = nrm_box(A, s_tab[slot + 1], p); break;
            default: normal = nrm_triangle<ADA_DIV>(xyz(A), xyz(s_tab[slot + 1]), xyz(s_tab[slot + 2]), p); break;
            }
         }
      }
   }
   a.dist[q] = closest;
   if (a.normals) { a.normals[3 * q] = normal.x; a.normals[3 * q + 1] = normal.y; a.normals[3 * q + 2] = normal.z; }
}
template <bool ADA_DIV> __global__ __launch_bounds__(64) void k_eval_distance(KScene sc, EvalArgs a) { eval_distance<ADA_DIV, false>(sc, a); }
template <bool ADA_DIV> __global__ __launch_bounds__(64) void k_eval_distance_gtab(KScene sc, EvalArgs a) { eval_distance<ADA_DIV, true>(sc, a); } // global residency of the scene table
template <int = 0> __global__ __launch_bounds__(64) void k_eval_distance_bvh(KScene sc, EvalArgs a) { eval_distance<false, true, true>(sc, a); } // ... with the triangle BVH (the Ada division of MDH_OPT_ADA_EVAL_DIV is no distance: such queries scan)

// ------------------------------------------------------------------------ ray queries
// mdh_raycast, mdh_raycast_visibility, mdh_softshadows (mdh_api.hip): the shaders' raycast, raycast_visibility and softshadows
// (raymarching.glsl:4-56) for rays that come from the host.  One ray per lane, 64 consecutive rays per wavefront; PART is the
// scene's variant without its census (the census variants compute the general kernels' bits).  Built-in kinds only.  The
// marches carry the stall guard (mdh_device.h, above raycast): they end for every finite ray.
// Two more WHAT values serve mdh_spherecast and mdh_contacts over the whole scene (sweep_query below; DESIGN.md section 4,
// "Sweeping a host's spheres"); k_listed, behind the newest kernels of this file, serves them over the kinds a host lists.
#define MDH_RQ_RAYCAST 0
#define MDH_RQ_VISIBILITY 1
#define MDH_RQ_SOFTSHADOW 2
#define MDH_RQ_SPHERECAST 3 // mdh_spherecast: a sphere swept along the ray (spherecast, mdh_device.h)
#define MDH_RQ_CONTACT 4    // mdh_contacts: one evaluation at a sphere's centre
struct RayQueryArgs {
   int n;
   float tmin, k;      // soft shadow: the shader's min_dist and k
   const float *org;   // 3 n
   const float *dir;   // 3 n, used as given
   const float *tmax;  // n (visibility, soft shadow)
   int *hit, *index, *steps; // raycast: n each; all but hit may be null
   float *t, *pos, *normal;  // ... n, 3 n, 3 n
   float *out;               // visibility, soft shadow: n
   const float *radius;      // swept spheres and contacts: n, or null: 0 (there tmax may be null too: the scene's max_dist)
};
#ifndef MDH_JIT
#include "mdh_ray_stream.h"
// A swept sphere's or a contact's answers, and the answers of one that fails the lanes' test (sweep_valid, contact_valid:
// the host path's predicate, which the lanes apply whoever holds the arrays).  A contact's distance goes to a.t.
MDH_DEV bool sweep_valid(const KScene &sc, f3 from, f3 dir, float rho, float tmax)
{
   return rs_ray_valid(from.x, from.y, from.z, dir.x, dir.y, dir.z) && rs_sweep_radius_valid(rho, sc.max_dist) && rs_sweep_tmax_valid(tmax, sc.max_dist);
}
MDH_DEV bool contact_valid(const KScene &sc, f3 c, float rho) { return rs_centre_valid(c.x, c.y, c.z) && rs_sweep_radius_valid(rho, sc.max_dist); }
MDH_DEV void sweep_store(const RayQueryArgs &a, size_t q, int hit, int index, float t, int steps, f3 P, f3 N)
{
   a.hit[q] = hit;
   if (a.index) a.index[q] = index;
   if (a.t) a.t[q] = t;
   if (a.steps) a.steps[q] = steps;
   if (a.pos) { a.pos[3 * q] = P.x; a.pos[3 * q + 1] = P.y; a.pos[3 * q + 2] = P.z; }
   if (a.normal) { a.normal[3 * q] = N.x; a.normal[3 * q + 1] = N.y; a.normal[3 * q + 2] = N.z; }
}
MDH_DEV void contact_store(const RayQueryArgs &a, size_t q, float dist, int index, f3 N)
{
   a.t[q] = dist;
   if (a.index) a.index[q] = index;
   if (a.normal) { a.normal[3 * q] = N.x; a.normal[3 * q + 1] = N.y; a.normal[3 * q + 2] = N.z; }
}
// the whole scene as every pass sees it: the march without an arg-min, one sdf_info at the hit
template <int PART, int WHAT> MDH_DEV void sweep_query(const KScene &sc, const RayQueryArgs &a, size_t q)
{
   const f3 zero = F3(0.0f, 0.0f, 0.0f);
   const f3 from = F3(a.org[3 * q], a.org[3 * q + 1], a.org[3 * q + 2]);
   const float rho = a.radius ? a.radius[q] : 0.0f;
   if (WHAT == MDH_RQ_CONTACT) {
      if (!contact_valid(sc, from, rho)) { contact_store(a, q, __uint_as_float(MDH_RS_BAD_BITS), -1, zero); return; }
      int index = -1, material;
      const float dist = sdf_info<PART>(sc, from, index) - rho;
      f3 N = zero;
      if (a.normal && index >= 0) primitive_info<false, (PART & MDH_PF_GTAB) != 0>(sc, index, from, N, material);
      contact_store(a, q, dist, index, N);
      return;
   }
   const f3 dir = F3(a.dir[3 * q], a.dir[3 * q + 1], a.dir[3 * q + 2]);
   const float tmax = a.tmax ? a.tmax[q] : sc.max_dist;
   if (!sweep_valid(sc, from, dir, rho, tmax)) { sweep_store(a, q, -1, -1, 0.0f, 0, zero, zero); return; }
   int steps = 0;
   float t = 0.0f;
   f3 P = zero, N = zero;
   if (spherecast<PART>(sc, from, dir, rho, tmax, P, t, steps)) {
      const int index = sweep_index<PART>(sc, P, a.normal != nullptr, N);
      sweep_store(a, q, 1, index, t, steps, P, N);
   } else
      sweep_store(a, q, 0, -1, 0.0f, steps, zero, zero);
}
#endif
template <int PART, int WHAT> __global__ __launch_bounds__(MDH_BLOCK) void k_ray_query(KScene sc, RayQueryArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "ray queries: the general variants of built-in kinds");
   stage_table(sc); // (the kernel's only barrier: lanes past n leave behind it)
   const long lin = (long)blockIdx.x * MDH_BLOCK + threadIdx.x;
   if (lin >= (long)a.n) return;
   const size_t q = (size_t)lin;
#ifndef MDH_JIT
   if (WHAT == MDH_RQ_SPHERECAST || WHAT == MDH_RQ_CONTACT) { sweep_query<PART, WHAT>(sc, a, q); return; }
#endif
   const f3 from = F3(a.org[3 * q], a.org[3 * q + 1], a.org[3 * q + 2]);
   const f3 dir = F3(a.dir[3 * q], a.dir[3 * q + 1], a.dir[3 * q + 2]);
   if (WHAT == MDH_RQ_VISIBILITY) { a.out[q] = raycast_visibility<PART, true>(sc, from, dir, a.tmax[q]); return; }
   if (WHAT == MDH_RQ_SOFTSHADOW) { a.out[q] = softshadows<PART, true>(sc, from, dir, a.tmin, a.tmax[q], a.k); return; }
   int index = -1, steps = 0;
   float t = 0.0f;
   f3 P = F3(0.0f, 0.0f, 0.0f), N = F3(0.0f, 0.0f, 0.0f);
   const bool h = raycast<PART, true>(sc, from, dir, index, P, t, steps);
   if (h) {
      int material;
      if (a.normal) primitive_info<false, (PART & MDH_PF_GTAB) != 0>(sc, index, P, N, material);
   } else {
      index = -1; // (the arg-min of the last step is no hit)
      t = 0.0f;
      P = F3(0.0f, 0.0f, 0.0f);
   }
   a.hit[q] = h ? 1 : 0;
   if (a.index) a.index[q] = index;
   if (a.t) a.t[q] = t;
   if (a.steps) a.steps[q] = steps;
   if (a.pos) { a.pos[3 * q] = P.x; a.pos[3 * q + 1] = P.y; a.pos[3 * q + 2] = P.z; }
   if (a.normal) { a.normal[3 * q] = N.x; a.normal[3 * q + 1] = N.y; a.normal[3 * q + 2] = N.z; }
}

// mdh_raycast_device, mdh_raycast_visibility_device, mdh_softshadows_device (mdh_api.hip): the same three queries for rays
// that live in device memory, with the marches in step form (mdh_device.h: RayMarch) so that A LANE TAKES THE NEXT RAY WHEN
// ITS OWN HAS ENDED.  The grid is at most what the device holds at once; its wavefronts share the launch's counter `next`
// (zeroed before the launch) and take rays from it as mdh_ray_stream.h says: a wavefront with at least `refill` idle lanes,
// or none busy, has lane 0 add the number of its idle lanes to the counter -- one vector atomic -- and its j-th idle lane
// takes ray base + j while that is below n.  A wavefront whose hand-out reached n asks no more and ends when its lanes have;
// nothing waits for another wavefront, so every grid size serves every ray exactly once.  refill = 64: rounds of 64
// consecutive rays, k_ray_query's schedule.  A lane stores its answers at its ray's index as soon as the ray ends.
// The host cannot look at these rays, so a lane tests its ray before marching it (rs_ray_valid, rs_tmax_valid: the host
// path's predicate) and answers one that fails without a march: raycast with a miss of 0 steps, the other two with NaN.
// stage_table's barrier is the only one: every thread of the workgroup reaches it, and none leaves the loop through a
// barrier.  Not part of the hiprtc build (built-in kinds only).
// MDH_RQ_SPHERECAST is the fourth march (spherecast_step, with the lane's radius beside its RayMarch): its lanes test radius and
// length too (sweep_valid) and ask for the hit's arg-min when they store (sweep_index), among the lanes that hit alone.
#ifndef MDH_JIT
#include "mdh_ray_stream.h"
struct RayStreamArgs {
   RayQueryArgs q;
   unsigned *next; // the launch's counter of rays handed out
   int refill;     // 1 .. 64
};
template <int PART, int WHAT> MDH_DEV void ray_stream_store(const KScene &sc, const RayQueryArgs &a, size_t q, const RayMarch &m, int status)
{
   if (WHAT == MDH_RQ_VISIBILITY) { a.out[q] = status == MDH_RS_HIT ? 0.0f : 1.0f; return; }
   if (WHAT == MDH_RQ_SOFTSHADOW) { a.out[q] = status == MDH_RS_HIT ? 0.0f : m.res; return; }
   if (WHAT == MDH_RQ_SPHERECAST) { // the arg-min the march did not carry, asked once at the centre of contact
      const f3 zero = F3(0.0f, 0.0f, 0.0f);
      if (status == MDH_RS_HIT) {
         const f3 C = m.from + m.dir * m.total;
         f3 Nc;
         const int index = sweep_index<PART>(sc, C, a.normal != nullptr, Nc);
         sweep_store(a, q, 1, index, m.total, m.n, C, Nc);
      } else
         sweep_store(a, q, 0, -1, 0.0f, m.n, zero, zero);
      return;
   }
   const bool h = status == MDH_RS_HIT;
   int index = -1; // (a miss: the arg-min of the last step is no hit)
   float t = 0.0f;
   f3 P = F3(0.0f, 0.0f, 0.0f), N = F3(0.0f, 0.0f, 0.0f);
   if (h) {
      index = m.index;
      P = m.from + m.dir * m.total;
      t = m.total;
      int material;
      if (a.normal) primitive_info<false, (PART & MDH_PF_GTAB) != 0>(sc, index, P, N, material);
   }
   a.hit[q] = h ? 1 : 0;
   if (a.index) a.index[q] = index;
   if (a.t) a.t[q] = t;
   if (a.steps) a.steps[q] = m.n;
   if (a.pos) { a.pos[3 * q] = P.x; a.pos[3 * q + 1] = P.y; a.pos[3 * q + 2] = P.z; }
   if (a.normal) { a.normal[3 * q] = N.x; a.normal[3 * q + 1] = N.y; a.normal[3 * q + 2] = N.z; }
}
// a ray that is not marched
template <int WHAT> MDH_DEV void ray_stream_refuse(const RayQueryArgs &a, size_t q)
{
   if (WHAT == MDH_RQ_VISIBILITY || WHAT == MDH_RQ_SOFTSHADOW) { a.out[q] = __uint_as_float(MDH_RS_BAD_BITS); return; }
   a.hit[q] = -1;
   if (a.index) a.index[q] = -1;
   if (a.t) a.t[q] = 0.0f;
   if (a.steps) a.steps[q] = 0;
   if (a.pos) { a.pos[3 * q] = 0.0f; a.pos[3 * q + 1] = 0.0f; a.pos[3 * q + 2] = 0.0f; }
   if (a.normal) { a.normal[3 * q] = 0.0f; a.normal[3 * q + 1] = 0.0f; a.normal[3 * q + 2] = 0.0f; }
}
template <int PART, int WHAT> __global__ __launch_bounds__(MDH_BLOCK) void k_ray_stream(KScene sc, RayStreamArgs sa)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "ray queries: the general variants of built-in kinds");
   static_assert(MDH_BLOCK % MDH_RS_WAVE == 0, "whole wavefronts");
   stage_table(sc); // (the kernel's only barrier; every thread is still here)
   const RayQueryArgs &a = sa.q;
   const int lane = threadIdx.x & 63;
   const unsigned n = (unsigned)a.n;
   const int refill = sa.refill;
   RayMarch m;
   float rho = 0.0f;   // a swept sphere's radius
   long long ray = -1; // the lane's ray; -1: idle
   int status = MDH_RS_OUT;
   bool drained = false; // (wave-uniform) the counter has passed n: this wavefront takes no more rays
   for (;;) {
      const unsigned long long idle = __ballot(ray < 0);
      const int n_idle = __popcll(idle);
      if (!drained && rs_refills(n_idle, refill)) { // (wave-uniform: every lane of the wavefront is in this loop)
         unsigned base = 0;
         if (lane == 0) base = atomicAdd(sa.next, (unsigned)n_idle);
         base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
         if (ray < 0) {
            ray = rs_ray_of(base, idle, lane, n);
            if (ray >= 0) {
               const size_t q = (size_t)ray;
               const float ox = a.org[3 * q], oy = a.org[3 * q + 1], oz = a.org[3 * q + 2];
               const float dx = a.dir[3 * q], dy = a.dir[3 * q + 1], dz = a.dir[3 * q + 2];
               const float tmax = WHAT == MDH_RQ_RAYCAST || (WHAT == MDH_RQ_SPHERECAST && !a.tmax) ? sc.max_dist : a.tmax[q];
               if (WHAT == MDH_RQ_SPHERECAST) rho = a.radius ? a.radius[q] : 0.0f;
               if (WHAT == MDH_RQ_SPHERECAST ? !sweep_valid(sc, F3(ox, oy, oz), F3(dx, dy, dz), rho, tmax)
                                             : !rs_ray_valid(ox, oy, oz, dx, dy, dz) || (WHAT != MDH_RQ_RAYCAST && !rs_tmax_valid(tmax, sc.max_dist))) {
                  ray_stream_refuse<WHAT>(a, q);
                  ray = -1; // (idle again: the next hand-out serves the lane)
               } else
                  status = march_begin(m, F3(ox, oy, oz), F3(dx, dy, dz), WHAT == MDH_RQ_SOFTSHADOW ? a.tmin : 0.0f, tmax);
            }
         }
         drained = rs_drained(base, n_idle, n);
      }
      if (__ballot(ray >= 0) == 0ull) {
         if (drained) break;
         continue; // (every ray of the hand-out was refused: the next one)
      }
      if (ray >= 0) {
         if (status == MDH_RS_GO)
            status = WHAT == MDH_RQ_SPHERECAST ? spherecast_step<PART>(sc, m, rho) : WHAT == MDH_RQ_RAYCAST ? raycast_step<PART>(sc, m) : WHAT == MDH_RQ_VISIBILITY ? visibility_step<PART>(sc, m) : softshadows_step<PART>(sc, m, a.k);
         if (status != MDH_RS_GO) {
            ray_stream_store<PART, WHAT>(sc, a, (size_t)ray, m, status);
            ray = -1;
         }
      }
   }
}

// mdh_shade_rays, mdh_shade_rays_device (mdh_api.hip): the frame's pixel program -- pixel_color_probes,
// render_probes.glsl:246-291 -- for rays that come from the host, where k_screen feeds it the camera's.  One ray per lane, 64
// consecutive rays per wavefront; PART is the scene's general variant, as in k_ray_query, MODE the screen mode (0 or 2).
// shade_structured works with wave-wide ballots and the park rows of its wavefront, so every lane of a wavefront that has a ray
// goes through it: lanes past n, and lanes whose ray is not shaded, as lane_valid = false.  The marches in there carry no stall
// guard: a lane tests its ray first (rs_shade_ray_valid, mdh_ray_stream.h: the host-array call's predicate) and the host has
// tested the scene, which together keep every march parameter below 2^14.  A ray that fails is answered with the quiet NaN in
// all three colours, hit = -1, index = -1, t = 0, steps = 0.  No volumetrics: a free ray has no screen position to look the
// fog up by.  stage_table's barrier is the only one.  As in k_screen nothing of the prologue stays live across the pixel
// program: the ray's index and the arguments the stores need are derived again behind it.
struct RayShadeArgs {
   int n;
   int tone_map;  // 0: the linear colour; 1: draw_screen.glsl:29 on it, as k_screen stores it
   int ao_steps;  // MDH_OPT_AO_STEPS
   int spec_mode; // MDH_OPT_INDIRECT_SPECULAR (0 or 2: the bodies of SPEC = 1)
   const float *org, *dir; // 3 n each
   float *rgb;             // 3 n
   int *hit, *index, *steps; // n each, or null
   float *t;                 // n, or null
};
MDH_DEV bool ray_shade_load(const RayShadeArgs &a, long lin, f3 &from, f3 &dir)
{
   from = F3(0.0f, 0.0f, 0.0f); dir = F3(0.0f, 0.0f, 0.0f);
   if (lin >= (long)a.n) return false;
   const size_t q = (size_t)lin;
   const float ox = a.org[3 * q], oy = a.org[3 * q + 1], oz = a.org[3 * q + 2];
   const float dx = a.dir[3 * q], dy = a.dir[3 * q + 1], dz = a.dir[3 * q + 2];
   if (!rs_shade_ray_valid(ox, oy, oz, dx, dy, dz)) return false;
   from = F3(ox, oy, oz); dir = F3(dx, dy, dz);
   return true;
}
template <int PART, int MODE> __global__ __launch_bounds__(MDH_BLOCK, MDH_OCC(PART, MODE)) void k_ray_shade(KScene sc, KProbes pr, RayShadeArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "ray queries: the general variants of built-in kinds");
   static_assert(MODE == 0 || MODE == 2, "the fixed mode, or direct light times occlusion");
   stage_table(sc); // (the kernel's only barrier)
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
   if (((long)blockIdx.x * (MDH_BLOCK / 64) + wave) * 64 >= (long)a.n) return; // wave-uniform: no ray in this wavefront
   PH_KERNEL_BEGIN();
   f3 c;
   PrimaryHit ph;
   bool hit;
   f3 pos;
   {
      f3 from, dir;
      const bool valid = ray_shade_load(a, ((long)blockIdx.x * (MDH_BLOCK / 64) + wave) * 64 + lane, from, dir);
      MachineCfg cfg; // renderers.adb:136-143
      cfg.direct_specular = true;
      cfg.spec_mode = a.spec_mode;
      cfg.ao_steps = a.ao_steps;
      c = MDH_SHADE<PART, MODE, 1, false>(sc, pr, cfg, valid, from, dir, ph, hit, pos);
   }
   struct KArgs { KScene sc; KProbes pr; RayShadeArgs a; };
   static_assert(alignof(KScene) == 8 && alignof(KProbes) == 8 && alignof(RayShadeArgs) == 8, "kernel argument alignments");
   static_assert(__builtin_offsetof(KArgs, pr) == sizeof(KScene) && __builtin_offsetof(KArgs, a) == sizeof(KScene) + sizeof(KProbes), "KArgs is the kernel argument segment of k_ray_shade");
   typedef const KArgs __attribute__((address_space(4))) *KArgsPtr; // constant address space: scalar loads
   KArgsPtr ka = (KArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
   asm volatile("" : "+s"(ka));
   RayShadeArgs a2;
   {
      typedef const int __attribute__((address_space(4))) *IntPtr;
      IntPtr pa = (IntPtr)&ka->a;
      int *da = (int *)&a2;
#pragma unroll
      for (int q = 0; q < (int)(sizeof(RayShadeArgs) / 4); ++q) da[q] = pa[q];
   }
   // the ray again (the same loads and the same predicate: the same answer)
   int wave2 = wave;
   asm volatile("" : "+s"(wave2));
   const long lin = ((long)blockIdx.x * (MDH_BLOCK / 64) + wave2) * 64 + lane_index_fresh();
   if (lin >= (long)a2.n) { PH_KERNEL_END(); return; }
   const size_t q = (size_t)lin;
   f3 from2, dir2;
   if (!ray_shade_load(a2, lin, from2, dir2)) { // not shaded
      const float bad = __uint_as_float(MDH_RS_BAD_BITS);
      a2.rgb[3 * q] = bad; a2.rgb[3 * q + 1] = bad; a2.rgb[3 * q + 2] = bad;
      if (a2.hit) a2.hit[q] = -1;
      if (a2.index) a2.index[q] = -1;
      if (a2.t) a2.t[q] = 0.0f;
      if (a2.steps) a2.steps[q] = 0;
      PH_KERNEL_END();
      return;
   }
   if (a2.tone_map) // draw_screen.glsl:29
      c = F3(spow(sdiv(c.x, c.x + 1.0f), 0.4545f), spow(sdiv(c.y, c.y + 1.0f), 0.4545f), spow(sdiv(c.z, c.z + 1.0f), 0.4545f));
   a2.rgb[3 * q] = c.x; a2.rgb[3 * q + 1] = c.y; a2.rgb[3 * q + 2] = c.z;
   if (a2.hit) a2.hit[q] = hit ? 1 : 0;
   if (a2.index) a2.index[q] = ph.index;
   if (a2.t) a2.t[q] = ph.t;
   if (a2.steps) a2.steps[q] = ph.steps;
   PH_KERNEL_END();
}

// mdh_camera_rays, mdh_camera_rays_device: the rays k_screen gives the pixels of a W x H frame (tile_pixel's centre, camera_ray:
// draw_screen.glsl:20-24), rows top first -- the same operations on the same values, so the frame's rays to the bit
struct CameraRayArgs {
   int W, H;
   float *org, *dir; // 3 W H each
};
template <int = 0> __global__ __launch_bounds__(256) void k_camera_rays(KCamera cam, CameraRayArgs a) // (a template: built where it is first named, mdh_api.hip: kernel_ptr)
{
   const long lin = (long)blockIdx.x * 256 + threadIdx.x;
   if (lin >= (long)a.W * a.H) return;
   const int j = (int)(lin / a.W), i = (int)(lin - (long)j * a.W);
   const float u = centre(i, a.W);
   const float v = -centre(j, a.H); // row 0 = top
   f3 origin, dir;
   camera_ray(cam, u, v, origin, dir);
   const size_t q = (size_t)lin;
   a.org[3 * q] = origin.x; a.org[3 * q + 1] = origin.y; a.org[3 * q + 2] = origin.z;
   a.dir[3 * q] = dir.x; a.dir[3 * q + 1] = dir.y; a.dir[3 * q + 2] = dir.z;
}

// mdh_shade_points, mdh_shade_points_device (mdh_api.hip): the light that arrives at points the host owns.  One point per lane,
// 64 consecutive points per wavefront, k_ray_shade's structure: stage_table's barrier is the only one, every lane of a
// wavefront that has a point goes through the program (lanes past n and lanes whose point is not shaded as lane_valid =
// false), nothing of the prologue stays live across the shading, and the stores take their arguments from the kernel argument
// segment again.  PART is the scene's general variant.  MODE:
//   0, 2  pixel_color_probes from the hit on (render_probes.glsl:253-285): shade_structured entered at the caller's point
//         (POINT, mdh_march.h) -- position, normal and material id as given, view_dir the shader's `dir` -- so a point that
//         mdh_raycast found gets the bits the frame gives its pixel;
//   3     sample_irradiance (render_probes.glsl:6-69) alone: point_irradiance below, no material, no light, no park rows.
// A lane tests its point first (rs_shade_point_valid, mdh_ray_stream.h: the host-array call's predicate); a point that fails
// is answered with the quiet NaN in all three colours and marches nothing.  Never any fog.
struct PointShadeArgs {
   int n;
   int tone_map;    // 0: the linear colour; 1: draw_screen.glsl:29 on it (modes 0 and 2)
   int ao_steps;    // MDH_OPT_AO_STEPS
   int spec_mode;   // MDH_OPT_INDIRECT_SPECULAR (0 or 2)
   int n_materials; // the material table's entries
   int pad_;
   const float *pos, *normal; // 3 n each
   const float *view;         // 3 n (modes 0 and 2)
   const int *material;       // n (modes 0 and 2)
   float *rgb;                // 3 n
};
// sample_irradiance (render_probes.glsl:6-69) in the oracle's operation order, one cage corner after the other: the weight
// from the angle, the visibility march from pos + normal * 0.05 * 5 over probe_distance - 0.25, the crush below 0.2, the
// trilinear factor, the bilinear tap of the irradiance atlas (either format), the square root of the texel; then the division
// by the total weight and the square, 0 when that weight is 0.  Nothing folded, shared or proved clear: the pixel program's
// eliminations are exact, so this literal form has their bits, and a host's points are few beside a frame's.
template <int PART> MDH_DEV f3 point_irradiance(const KScene &sc, const KProbes &pr, f3 pos, f3 normal)
{
   const int u8_tab = sc.u8_slot * 4;
   const i3 gp = world_to_grid(pr, pos);
   f3 irradiance = F3(0.0f, 0.0f, 0.0f);
   float total_weight = 0.0f;
   const f3 alpha = pos / F3(pr.sx, pr.sy, pr.sz) - F3((float)gp.x, (float)gp.y, (float)gp.z);
   const f3 from_off = pos + (normal * MDH_MIN_STEP) * 5.0f;
   f2 rid = ray_dir_to_ray_id(normal);
   rid = F2(clamp_(rid.x, pr.irr_lo, pr.irr_hi), clamp_(rid.y, pr.irr_lo, pr.irr_hi));
#pragma unroll 1
   for (int i = 0; i < 8; ++i) {
      const i3 q = cage_probe(pr, gp, i);
      const f3 hit_to_probe = grid_to_world(pr, q) - pos;
      const float probe_distance = length(hit_to_probe);
      const f3 dir_to_probe = sdiv3(hit_to_probe, probe_distance);
      const float angle = (dot(dir_to_probe, normal) + 1.0f) * 0.5f;
      float weight = angle * angle + 0.2f;
      // raycast_visibility, raymarching.glsl:39-56
      float vis = 1.0f;
      {
         const float vmax = probe_distance - MDH_MIN_STEP * 5.0f;
         float total = 0.0f;
         while (total < vmax) {
            const float sd = sdf<PART>(sc, from_off + dir_to_probe * total);
            if (sd < MDH_EPS) { vis = 0.0f; break; }
            total += sd;
         }
      }
      weight *= vis;
      const float crush = 0.2f;
      if (weight < crush) weight *= weight * weight * (1.0f / (crush * crush));
      const f3 tri = F3(mix_(1.0f - alpha.x, alpha.x, (float)(i & 1)), mix_(1.0f - alpha.y, alpha.y, (float)((i >> 1) & 1)),
                        mix_(1.0f - alpha.z, alpha.z, (float)((i >> 2) & 1)));
      weight *= tri.x * tri.y * tri.z;
      const f2 base = probe_id_to_coord(pr, grid_to_probe_id(pr, q));
      const f3 tx = atlas_sample(pr.irr, pr.fmt, pr.pcx, pr.pcy, pr.ires, pr.ishift, pr.irr_w, pr.irr_h, base.x + div_pcx(pr, rid.x), base.y + div_pcy(pr, rid.y), u8_tab, pr.m_ires);
      irradiance = irradiance + ssqrt3(tx) * weight;
      total_weight += weight;
   }
   if (total_weight == 0.0f) return F3(0.0f, 0.0f, 0.0f); // (render_probes.glsl:65: 0 / 0 fixed as 0)
   irradiance = sdiv3(irradiance, total_weight);
   return irradiance * irradiance;
}
template <int MODE> MDH_DEV bool point_shade_load(const PointShadeArgs &a, long lin, f3 &pos, f3 &normal, f3 &view, int &material)
{
   pos = F3(0.0f, 0.0f, 0.0f); normal = F3(0.0f, 0.0f, 0.0f); view = F3(0.0f, 0.0f, 0.0f);
   material = 0;
   if (lin >= (long)a.n) return false;
   const size_t q = (size_t)lin;
   const float px = a.pos[3 * q], py = a.pos[3 * q + 1], pz = a.pos[3 * q + 2];
   const float nx = a.normal[3 * q], ny = a.normal[3 * q + 1], nz = a.normal[3 * q + 2];
   float vx = 0.0f, vy = 0.0f, vz = 0.0f;
   int m = 0;
   if (MODE != 3) {
      vx = a.view[3 * q]; vy = a.view[3 * q + 1]; vz = a.view[3 * q + 2];
      m = a.material[q];
   }
   if (!rs_shade_point_valid(px, py, pz, nx, ny, nz, vx, vy, vz, m, MODE != 3 ? a.n_materials : 1)) return false;
   pos = F3(px, py, pz); normal = F3(nx, ny, nz); view = F3(vx, vy, vz);
   material = m;
   return true;
}
template <int PART, int MODE> __global__ __launch_bounds__(MDH_BLOCK, MDH_OCC(PART, MODE == 3 ? 2 : MODE)) void k_point_shade(KScene sc, KProbes pr, PointShadeArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "point queries: the general variants of built-in kinds");
   static_assert(MODE == 0 || MODE == 2 || MODE == 3, "the fixed mode, direct light times occlusion, or the irradiance alone");
   stage_table(sc); // (the kernel's only barrier)
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
   if (((long)blockIdx.x * (MDH_BLOCK / 64) + wave) * 64 >= (long)a.n) return; // wave-uniform: no point in this wavefront
   f3 c;
   if constexpr (MODE == 3) {
      f3 pos, normal, view;
      int material;
      c = F3(0.0f, 0.0f, 0.0f);
      if (point_shade_load<MODE>(a, ((long)blockIdx.x * (MDH_BLOCK / 64) + wave) * 64 + lane, pos, normal, view, material)) c = point_irradiance<PART>(sc, pr, pos, normal);
   } else {
      PH_KERNEL_BEGIN();
      PrimaryHit ph;
      bool hit;
      f3 pos_out;
      {
         f3 pos, normal, view;
         int material;
         const bool valid = point_shade_load<MODE>(a, ((long)blockIdx.x * (MDH_BLOCK / 64) + wave) * 64 + lane, pos, normal, view, material);
         MachineCfg cfg; // renderers.adb:136-143
         cfg.direct_specular = true;
         cfg.spec_mode = a.spec_mode;
         cfg.ao_steps = a.ao_steps;
         c = MDH_SHADE<PART, MODE, 1, false, 0, true, true, true>(sc, pr, cfg, valid, pos, view, ph, hit, pos_out, RayRecord{0u, 0u, -1, 0u}, RayRecord{0u, 0u, -1, 0u}, normal, material);
      }
      PH_KERNEL_END();
   }
   struct KArgs { KScene sc; KProbes pr; PointShadeArgs a; };
   static_assert(alignof(KScene) == 8 && alignof(KProbes) == 8 && alignof(PointShadeArgs) == 8, "kernel argument alignments");
   static_assert(__builtin_offsetof(KArgs, pr) == sizeof(KScene) && __builtin_offsetof(KArgs, a) == sizeof(KScene) + sizeof(KProbes), "KArgs is the kernel argument segment of k_point_shade");
   typedef const KArgs __attribute__((address_space(4))) *KArgsPtr; // constant address space: scalar loads
   KArgsPtr ka = (KArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
   asm volatile("" : "+s"(ka));
   PointShadeArgs a2;
   {
      typedef const int __attribute__((address_space(4))) *IntPtr;
      IntPtr pa = (IntPtr)&ka->a;
      int *da = (int *)&a2;
#pragma unroll
      for (int q = 0; q < (int)(sizeof(PointShadeArgs) / 4); ++q) da[q] = pa[q];
   }
   // the point again (the same loads and the same predicate: the same answer)
   int wave2 = wave;
   asm volatile("" : "+s"(wave2));
   const long lin = ((long)blockIdx.x * (MDH_BLOCK / 64) + wave2) * 64 + lane_index_fresh();
   if (lin >= (long)a2.n) return;
   const size_t q = (size_t)lin;
   {
      f3 pos2, normal2, view2;
      int material2;
      if (!point_shade_load<MODE>(a2, lin, pos2, normal2, view2, material2)) { // not shaded
         const float bad = __uint_as_float(MDH_RS_BAD_BITS);
         a2.rgb[3 * q] = bad; a2.rgb[3 * q + 1] = bad; a2.rgb[3 * q + 2] = bad;
         return;
      }
   }
   if (MODE != 3 && a2.tone_map) // draw_screen.glsl:29
      c = F3(spow(sdiv(c.x, c.x + 1.0f), 0.4545f), spow(sdiv(c.y, c.y + 1.0f), 0.4545f), spow(sdiv(c.z, c.z + 1.0f), 0.4545f));
   a2.rgb[3 * q] = c.x; a2.rgb[3 * q + 1] = c.y; a2.rgb[3 * q + 2] = c.z;
}

// mdh_path_trace, mdh_path_trace_device (mdh_api.hip): a path tracer along rays of the host's, the ground truth the probes are
// an approximation of.  One ray per lane, 64 consecutive rays per wavefront; PART is the scene's general variant, as in
// k_ray_query.  The estimator for one sample of one ray -- the reference's glsl/render_path.glsl, which it never includes:
//    mask = 1, rgb = 0;  up to bounces + 1 segments, each march_plain to max_dist;
//    a miss adds mask * sky (dir) (render_probes.glsl:287) and ends the path;
//    a hit runs sdf_info / primitive_info as the pixel program does, adds mask * compute_direct_lighting (lighting.glsl:1-40,
//    direct specular on: path_direct below), multiplies the mask by the albedo, and goes on from P + (N * MDH_MIN_STEP) * 5
//    -- where the shadow rays start -- along path_scatter's direction (mdh_path.h); a direction that is not finite ends the path.
// THREE DEVIATIONS from render_path.glsl, which cannot run as written: the sky is MASKED (the file adds it unmasked), it is
// added ONCE (the file adds it again for every bounce that is left), and the next ray's origin is OFFSET (the file starts it on
// the surface it just hit, where the first step is below epsilon).  The random numbers are path_u01's, not fract (sin ..).
// A lane adds its samples sample_first .. sample_first + sample_count - 1 to rgb[ray] in that order, starting from what the
// array holds: a run of samples split over two calls has the bits of one call.
// THE LOOP IS FLAT: it runs over segments, not over samples x bounces.  In one iteration every lane does the next segment of
// its own path, whichever sample and bounce that is; a lane whose path has ended begins its next sample while its neighbours
// take their next bounce, and the wavefront ends when all lanes have used up their samples.  No atomics, no shared counter, and
// a lane runs the sequence of operations it would run alone: no bit depends on its neighbours.  (MDH_PATH_LOCKSTEP, a
// switch of scripts/bench_path_trace.py's build only: the wavefront waits for its slowest path before the next sample.)
// No stall guard: a lane tests its ray first (path_ray_valid) and the host has tested the scene and the bounces; a ray that
// fails is answered with the quiet NaN in all three colours, hit = -1, index = -1, t = 0.  The optional outputs describe the
// primary segment.  No atlas is read, NO VOLUMETRICS, no occlusion term, no indirect specular.  stage_table's barrier is the only one.
#include "mdh_path.h"
#ifndef MDH_PATH_LOCKSTEP
#define MDH_PATH_LOCKSTEP 0
#endif
struct PathTraceArgs {
   int n;
   int bounces;              // 0 .. MDH_PATH_MAX_BOUNCES
   unsigned seed, id_first;  // ray i has id id_first + i
   int sample_first, sample_count;
   const float *org, *dir;   // 3 n each
   float *rgb;               // 3 n, in and out: the sums
   int *hit, *index;         // n each, or null
   float *t;                 // n, or null
};
// compute_direct_lighting (lighting.glsl:1-40) at P with normal N, seen along rd: the light loop of shade_structured
// (mdh_march.h) for its first point with direct specular on -- the shared first step, null_light in front of the BRDF, the
// shadow march with min_raw, sdiv3 -- as a lane's own function: no park rows, no wave-wide ballots
template <int PART> MDH_DEV f3 path_direct(const KScene &sc, f3 P, f3 N, f3 from_off, f3 rd, const Material &m)
{
   const float sd0 = MDH_SHARE_FIRST_STEP ? sdf<PART>(sc, from_off) : 0.0f;
   f3 Lo = F3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
   for (int li = 0; li < sc.total_lights; ++li) {
      f3 L;
      float L_dist;
      const f3 radiance = sample_light<false>(sc, li, P, N, L, L_dist);
      const float NdotL = max_(dot(N, L), 0.0f);
      f3 contrib = F3(0.0f, 0.0f, 0.0f); // (a light that is dark here or behind the surface: +0, null_light)
      if (!(MDH_NULL_BRDF && null_light(-rd, L, NdotL, radiance, m))) {
         f3 kD, kS;
         cook_torrance(N, -rd, L, NdotL, m.albedo, m.metallic, m.roughness, kD, kS);
         contrib = ((sdiv3(kD * m.albedo, MDH_PI) + kS) * radiance) * NdotL;
      }
      float shadows = 0.0f;
      const bool lit = MDH_SKIP_NULL_RAYS ? (contrib.x != 0.0f || contrib.y != 0.0f || contrib.z != 0.0f) : true;
      if (NdotL > MDH_EPS && lit) { // softshadows, raymarching.glsl:4-23
         float res = 1.0f, prev = 1e20f, total = 0.0f;
         bool blocked = false;
         bool first = MDH_SHARE_FIRST_STEP != 0;
         while (total < L_dist) {
            const float dist = first ? sd0 : sdf<PART>(sc, from_off + L * total);
            first = false;
            if (dist < MDH_EPS) { blocked = true; break; }
            const float y = dist * dist / (2.0f * prev);
            const float d = sqrt_(dist * dist - y * y);
            res = min_raw(res, 64.0f * d / max_(0.0f, total - y));
            prev = dist;
            total += dist;
         }
         shadows = blocked ? 0.0f : res;
      }
      Lo = Lo + contrib * shadows;
   }
   return Lo;
}
template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_path_trace(KScene sc, PathTraceArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "ray queries: the general variants of built-in kinds");
   stage_table(sc); // (the kernel's only barrier: lanes past n leave behind it)
   const long lin = (long)blockIdx.x * MDH_BLOCK + threadIdx.x;
   if (lin >= (long)a.n) return;
   const size_t q = (size_t)lin;
   const f3 org = F3(a.org[3 * q], a.org[3 * q + 1], a.org[3 * q + 2]);
   const f3 dir = F3(a.dir[3 * q], a.dir[3 * q + 1], a.dir[3 * q + 2]);
   if (!path_ray_valid(org.x, org.y, org.z, dir.x, dir.y, dir.z)) { // not traced
      const float bad = __uint_as_float(MDH_RS_BAD_BITS);
      a.rgb[3 * q] = bad; a.rgb[3 * q + 1] = bad; a.rgb[3 * q + 2] = bad;
      if (a.hit) a.hit[q] = -1;
      if (a.index) a.index[q] = -1;
      if (a.t) a.t[q] = 0.0f;
      return;
   }
   const unsigned id = a.id_first + (unsigned)q;
   f3 acc = F3(a.rgb[3 * q], a.rgb[3 * q + 1], a.rgb[3 * q + 2]);
   int p_hit = 0, p_index = -1; // the primary segment (the same in every sample)
   float p_t = 0.0f;
   // the lane's path: its sample, the bounce of its next segment, the ray of that segment, what it has gathered
   int sample = a.sample_first, bounce = 0;
   const int sample_end = a.sample_first + a.sample_count;
   f3 ro = org, rd = dir, mask = F3(1.0f, 1.0f, 1.0f), rgb = F3(0.0f, 0.0f, 0.0f);
#if MDH_PATH_LOCKSTEP
   bool waiting = false; // the lane's sample has ended and a neighbour's has not
#endif
#pragma unroll 1
   while (sample < sample_end) { // one segment per iteration
#if MDH_PATH_LOCKSTEP
      if (__ballot(!waiting) == 0ull) waiting = false; // (every lane has ended its sample: the next one, together)
      if (waiting) continue;
#endif
      float t;
      int steps;
      const bool h = march_plain<PART>(sc, ro, rd, sc.max_dist, t, steps);
      bool ended = true;
      if (!h) { // render_probes.glsl:287
         const float s = rd.y * 0.7f;
         rgb = rgb + mask * F3(0.30f - s, 0.36f - s, 0.60f - s);
      } else {
         const f3 P = ro + rd * t;
         int index = -1, pm;
         f3 N;
         (void)sdf_info<PART>(sc, P, index);
         primitive_info<false, (PART & MDH_PF_GTAB) != 0>(sc, index, P, N, pm);
         if (bounce == 0) { p_hit = 1; p_index = index; p_t = t; }
         const Material m = get_material(sc, pm);
         const f3 from_off = P + (N * MDH_MIN_STEP) * 5.0f;
         rgb = rgb + mask * path_direct<PART>(sc, P, N, from_off, rd, m);
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
      if (ended) { // the sample is complete: the next one starts at the primary ray
         acc = acc + rgb;
         ++sample;
         bounce = 0;
         ro = org; rd = dir;
         mask = F3(1.0f, 1.0f, 1.0f); rgb = F3(0.0f, 0.0f, 0.0f);
#if MDH_PATH_LOCKSTEP
         waiting = true;
#endif
      }
   }
   a.rgb[3 * q] = acc.x; a.rgb[3 * q + 1] = acc.y; a.rgb[3 * q + 2] = acc.z;
   if (a.hit) a.hit[q] = p_hit;
   if (a.index) a.index[q] = p_index;
   if (a.t) a.t[q] = p_t;
}

// mdh_inscatter_points, mdh_inscatter_rays and their _device forms (mdh_api.hip): the participating medium for points and rays
// of the host's -- the integrand of k_visibility evaluated anywhere, and the sum of accumulate_scattering.glsl:17-28 along any
// ray with the integrand EVALUATED at every step where k_scat_fold taps the froxels.  PART is the scene's general variant, as
// in k_ray_query; nothing of KVolumetrics enters: the answers do not depend on the froxel or scattering settings.
//    inscatter (pos, dir) = sample_lights of compute_frustrum_visibility.glsl:8-19, operation for operation the light loop of
//    k_visibility above (sample_light with the normal (1, 0, 0), MDH_TAU), which keeps its own copy: the visibility rays here
//    carry the stall guard (raycast_visibility<PART, true>: the same bits wherever the passes' march ends), because the points
//    come from outside;
//    a ray:  len = march ? min_ (length (to - org), tmax) : tmax, to = org + dir * tmax or, on a hit of the guarded march_plain
//            to max_dist, org + dir * t (scattering_length with max_depth := tmax);
//            L = 0; for (f = 0; f < len; f += step) L = L + inscatter ((dir * f) + org, dir) * sexp (-f * MDH_TAU);
//            rgb = L * step -- fp32, this order, f by repeated addition, THE SAMPLE POINT AS (dir * f) + org.
// A point or ray the host-array call refuses its batch for (rs_ray_valid, rs_inscatter_tmax_valid, rs_inscatter_f_valid:
// mdh_ray_stream.h) is not marched: the quiet NaN in rgb and len, -1 steps.  stage_table's barrier is the only one.
template <int PART> MDH_DEV f3 inscatter(const KScene &sc, f3 pos, f3 dir)
{
   f3 result = F3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
   for (int l = 0; l < sc.total_lights; ++l) { // sample_lights :8-19
      f3 L;
      float L_dist;
      f3 radiance = sample_light<false>(sc, l, pos, F3(1.0f, 0.0f, 0.0f), L, L_dist);
      float visibility = raycast_visibility<PART, true>(sc, pos, L, L_dist);
      f3 L_in = radiance * (sexp(-L_dist * MDH_TAU) * visibility);
      result = result + (L_in * MDH_TAU) * henvey_greenstein_phase(L, dir);
   }
   return result;
}
struct InscatterPointArgs {
   int n;
   const float *pos, *dir; // 3 n each
   const float *f;         // n, or null: no factor
   float *rgb;             // 3 n
};
// one point per lane, 64 consecutive points per wavefront
template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_point_inscatter(KScene sc, InscatterPointArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "ray queries: the general variants of built-in kinds");
   stage_table(sc); // (the kernel's only barrier: lanes past n leave behind it)
   const long lin = (long)blockIdx.x * MDH_BLOCK + threadIdx.x;
   if (lin >= (long)a.n) return;
   const size_t q = (size_t)lin;
   const f3 pos = F3(a.pos[3 * q], a.pos[3 * q + 1], a.pos[3 * q + 2]);
   const f3 dir = F3(a.dir[3 * q], a.dir[3 * q + 1], a.dir[3 * q + 2]);
   const float f = a.f ? a.f[q] : 0.0f;
   f3 rgb;
   if (!rs_ray_valid(pos.x, pos.y, pos.z, dir.x, dir.y, dir.z) || !rs_inscatter_f_valid(f)) {
      const float bad = __uint_as_float(MDH_RS_BAD_BITS);
      rgb = F3(bad, bad, bad);
   } else {
      rgb = inscatter<PART>(sc, pos, dir);
      if (a.f) rgb = rgb * sexp(-f * MDH_TAU); // (the product k_scat_fold forms)
   }
   a.rgb[3 * q] = rgb.x; a.rgb[3 * q + 1] = rgb.y; a.rgb[3 * q + 2] = rgb.z;
}
struct InscatterRayArgs {
   int n;
   int march;   // 1: the ray ends where it hits the scene
   float step;
   const float *org, *dir; // 3 n each
   const float *tmax;      // n
   float *rgb;             // 3 n
   float *len;             // n, or null
   int *steps;             // n, or null
};
// ONE WAVEFRONT PER RAY, four rays per workgroup, the ray's steps spread over the lanes in chunks of 64: lane k of chunk c
// evaluates step 64 c + k.  A chunk's sample points are neighbours along one line, so their visibility rays to a light pass
// the same geometry and end together -- the argument of the froxels' 4 x 4 x 4 blocks.  The wavefront keeps f at the chunk's
// base; a lane reaches its own f by its k additions of `step`, and the next base is the last lane's f + step: the serial
// loop's values to the bit.  Each lane forms its three products, and the wavefront adds them to its accumulator IN STEP
// ORDER, one lane's value broadcast at a time (v_readlane): 64 dependent additions per channel and chunk beside 64 x lights
// visibility marches, and exactly the serial sum.  The lanes with a step are a prefix of the chunk (f grows with the lane);
// the fold stops at their count, so that a lane past the ray's length adds nothing -- not even +0 into a -0.
// Everything per ray -- validity, the length's march -- is wave-uniform and done once.  No wavefront reads what another one
// wrote, no buffer in device memory beside the caller's arrays, one kernel.
template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_ray_inscatter(KScene sc, InscatterRayArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "ray queries: the general variants of built-in kinds");
   static_assert(MDH_BLOCK % MDH_RS_WAVE == 0, "whole wavefronts");
   stage_table(sc); // (the kernel's only barrier: wavefronts past n leave behind it)
   const int lane = threadIdx.x & 63;
   const long ray = (long)blockIdx.x * (MDH_BLOCK / MDH_RS_WAVE) + (threadIdx.x >> 6);
   if (ray >= (long)a.n) return; // (wave-uniform)
   const size_t q = (size_t)ray;
   const f3 org = F3(a.org[3 * q], a.org[3 * q + 1], a.org[3 * q + 2]);
   const f3 dir = F3(a.dir[3 * q], a.dir[3 * q + 1], a.dir[3 * q + 2]);
   const float tmax = a.tmax[q];
   if (!rs_ray_valid(org.x, org.y, org.z, dir.x, dir.y, dir.z) || !rs_inscatter_tmax_valid(tmax, sc.max_dist)) { // not marched
      if (lane == 0) {
         const float bad = __uint_as_float(MDH_RS_BAD_BITS);
         a.rgb[3 * q] = bad; a.rgb[3 * q + 1] = bad; a.rgb[3 * q + 2] = bad;
         if (a.len) a.len[q] = bad;
         if (a.steps) a.steps[q] = -1;
      }
      return;
   }
   float len = tmax;
   if (a.march) { // scattering_length with max_depth := tmax; march_plain (mdh_march.h) with the stall guard of the ray queries
      f3 to = org + dir * tmax;
      const SdfRegs regs = sdf_regs<(PART & MDH_PF_GTAB) != 0>(sc);
      float total = 0.0f;
      bool h = false;
      while (total < sc.max_dist) {
         const float dist = sdf<PART>(sc, org + dir * total, regs);
         if (dist < MDH_EPS) { h = true; break; }
         if (total + dist == total) break; // stalled: a miss
         total += dist;
      }
      if (h) to = org + dir * total;
      len = min_(length(to - org), tmax);
   }
   len = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(len))); // (every lane holds the same bits: said to the compiler)
   f3 acc = F3(0.0f, 0.0f, 0.0f);
   float base = 0.0f; // f of the chunk's first step
   int count = 0;
#pragma unroll 1
   while (base < len) { // (wave-uniform)
      float f = base;
      for (int k = 0; k < lane; ++k) f += a.step;
      const bool live = f < len;
      f3 pr = F3(0.0f, 0.0f, 0.0f);
      if (live) pr = inscatter<PART>(sc, dir * f + org, dir) * sexp(-f * MDH_TAU);
      const int m = __popcll(__ballot(live)); // the chunk's steps: lanes 0 .. m - 1
      for (int k = 0; k < m; ++k) { // L = L + product, step by step
         acc.x = acc.x + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pr.x), k));
         acc.y = acc.y + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pr.y), k));
         acc.z = acc.z + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pr.z), k));
      }
      count += m;
      if (m < MDH_RS_WAVE) break; // the ray's last step lay in this chunk
      base = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f), MDH_RS_WAVE - 1)) + a.step;
   }
   if (lane == 0) {
      acc = acc * a.step;
      a.rgb[3 * q] = acc.x; a.rgb[3 * q + 1] = acc.y; a.rgb[3 * q + 2] = acc.z;
      if (a.len) a.len[q] = len;
      if (a.steps) a.steps[q] = count;
   }
}

// ------------------------------------------------------------------------ swept spheres against listed kinds
// mdh_spherecast, mdh_contacts and their _device forms with a list of kinds (mdh_api.hip): the scene is the exact minimum
// over the listed kinds' committed instances in the order listed -- eval_distance's scan above (initial closest 1.0e10f, strict
// <: the lowest index wins a tie; no partition, no hierarchy) with the shaders' division always, since a march needs a
// distance.  The arg-min costs the scan one select, so the march carries it; `index` is the flat index every pass uses (the
// kind's base plus the instance), and the normal is primitive_info's of that index, computed once, for the winner -- what
// eval_distance computes at every improvement.  One ray or centre per lane, 64 consecutive ones per wavefront; the lanes apply
// the host path's predicate whoever holds the arrays.  WHAT: MDH_RQ_SPHERECAST or MDH_RQ_CONTACT.
struct ListedArgs {
   RayQueryArgs q;
   int n_kinds;
   int kinds[MDH_MAX_KINDS];
   int host_count[MDH_MAX_KINDS];
};
template <bool GTAB> MDH_DEV float listed_closest(const KScene &sc, const ListedArgs &la, f3 p, int &index)
{
   float closest = 1.0e10f;
   index = -1;
   for (int kk = 0; kk < la.n_kinds; ++kk) {
      const int k = la.kinds[kk], base = hdr(H_KBASE + k), count = la.host_count[k];
      for (int i = 0; i < count; ++i) {
         const float d = part_dist<false, GTAB, GTAB>(sc, k, i, p);
         if (d < closest) { closest = d; index = base + i; }
      }
   }
   return closest;
}
template <bool GTAB, int WHAT> __global__ __launch_bounds__(MDH_BLOCK) void k_listed(KScene sc, ListedArgs la)
{
   static_assert(WHAT == MDH_RQ_SPHERECAST || WHAT == MDH_RQ_CONTACT, "swept spheres and contacts");
   stage_table(sc); // (the kernel's only barrier: lanes past n leave behind it)
   const RayQueryArgs &a = la.q;
   const long lin = (long)blockIdx.x * MDH_BLOCK + threadIdx.x;
   if (lin >= (long)a.n) return;
   const size_t q = (size_t)lin;
   const f3 zero = F3(0.0f, 0.0f, 0.0f);
   const f3 from = F3(a.org[3 * q], a.org[3 * q + 1], a.org[3 * q + 2]);
   const float rho = a.radius ? a.radius[q] : 0.0f;
   int index = -1, material;
   f3 N = zero;
   if (WHAT == MDH_RQ_CONTACT) {
      if (!contact_valid(sc, from, rho)) { contact_store(a, q, __uint_as_float(MDH_RS_BAD_BITS), -1, zero); return; }
      const float dist = listed_closest<GTAB>(sc, la, from, index) - rho;
      if (a.normal && index >= 0) primitive_info<false, GTAB>(sc, index, from, N, material);
      contact_store(a, q, dist, index, N);
      return;
   }
   const f3 dir = F3(a.dir[3 * q], a.dir[3 * q + 1], a.dir[3 * q + 2]);
   const float tmax = a.tmax ? a.tmax[q] : sc.max_dist;
   if (!sweep_valid(sc, from, dir, rho, tmax)) { sweep_store(a, q, -1, -1, 0.0f, 0, zero, zero); return; }
   int steps = 0;
   bool h = false;
   float total = 0.0f;
   while (total < tmax) {
      const float dist = listed_closest<GTAB>(sc, la, from + dir * total, index) - rho;
      ++steps;
      if (dist < MDH_EPS) { h = true; break; }
      if (total + dist == total) break; // stalled: a miss
      total += dist;
   }
   if (!h) { sweep_store(a, q, 0, -1, 0.0f, steps, zero, zero); return; }
   const f3 P = from + dir * total;
   if (a.normal && index >= 0) primitive_info<false, GTAB>(sc, index, P, N, material);
   sweep_store(a, q, 1, index, total, steps, P, N);
}

// ------------------------------------------------------------------------ meshing the scene's surface
// mdh_surface_mesh, mdh_surface_mesh_device (mdh_api.hip): surface nets over a grid of the scene's distance -- the field,
// the counts, their scan, the vertices and the quads, every slot a function of the grid alone.  The definition and the
// kernels: mdh_surface.h.
#include "mdh_surface.h"
// ... and a path-traced frame: k_path_trace's estimator over the pixels of a captured camera, its rays and its resolve
#include "mdh_path_frame.h"
// ... and the adaptive one: a count and two moments a pixel, the stopping rule, the compaction of the pixels still running
#include "mdh_path_frame_adaptive.h"
#endif

// ---------------------------------------------------------------------- the window's pixels
// What Swap_Buffers (renderers.adb:320) puts on screen: the screen pass writes float colours and
// the default framebuffer of the reference's window is RGBA8 without sRGB encoding, so each
// channel is clamped to [0, 1] and converted to the nearest of the 256 levels (OpenGL 4.3 core
// section 2.3.5.1, round to nearest; ties to even; a NaN shows as 0).  16 bytes read and 4 written per pixel.
#ifndef MDH_JIT
__global__ __launch_bounds__(256) void k_present(const float4 *__restrict__ fb, unsigned *__restrict__ out, int n)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q < n) out[q] = pack_rgba8(fb[q]);
}
#endif
