// mdh_march.h -- pixel_color_probes (reference glsl/render_probes.glsl:246-291) for gfx950.
//
// Two formulations were built and measured on MI355X (BASELINE config 3, 1080p):
//  * a per-lane ray STATE MACHINE -- one shared march loop, lanes whose ray ended wait for a
//    ballot threshold and then run their transition together (the classic persistent-ray
//    design).  Bit-exact, but 3-4x SLOWER than the structured form at every threshold
//    (1.4-2.4 ms radiance, 3.4-4.4 ms screen vs 0.58 / 0.97 ms): the transitions (BRDF,
//    light sampling, atlas taps: ~40 % of the work) then run under sparse exec masks, and the
//    machine keeps every variable of every stage live across the loop.  Removed.
//  * the lock-step STRUCTURED form below, which is what the kernels run.
#pragma once

#include "mdh_device.h"

#ifndef MDH_REUSE_FOLDED
#define MDH_REUSE_FOLDED 1
#endif
#ifndef MDH_SHARE_FIRST_STEP
#define MDH_SHARE_FIRST_STEP 1
#endif
#define MDH_PARK_VD_ROW 19 // (rows 19-21: allocated by the host for scenes with a space partition, lds_bytes_screen; six wavefronts per SIMD need 22 rows or fewer)
#ifndef MDH_SKIP_NULL_RAYS
#define MDH_SKIP_NULL_RAYS 1
#endif
#ifndef MDH_TWIN_PREV
#define MDH_TWIN_PREV 1
#endif
#ifndef MDH_SHARE_TAPS
#define MDH_SHARE_TAPS 1 // a wavefront whose points share cage cell and normal fetches its eight irradiance taps once (shade_structured)
#endif
#ifndef MDH_TWIN_FOLDED
#define MDH_TWIN_FOLDED 1 // ... and a corner of it folded along y or z takes its twin's weight and visibility bit instead of computing them again
#endif

#ifndef MDH_BEST_FIRST
#ifdef MDH_DIAG
#define MDH_BEST_FIRST 0 // (the diagnostic builds count the in-order loop's rays: their work counters are pinned)
#else
#define MDH_BEST_FIRST 1 // the second point's cage probes visited by decreasing dot(probe_to_spec, -N): the first visible one is the loop's (shade_structured)
#endif
#endif
#ifdef MDH_BEST_STATS // the counter build (make beststats), summed over launches until mdh_diag_best_first takes them:
__device__ unsigned long long g_best_stats[4]; // wave-rounds of the fast path, lanes that won there, wavefronts in the fallback, lanes in it
#define MDH_BEST_STAT(slot, n) do { const unsigned long long n_ = (n); if ((threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) atomicAdd(&g_best_stats[slot], n_); } while (0)
#else
#define MDH_BEST_STAT(slot, n) do { } while (0)
#endif
#ifndef MDH_BEST_APPROX
#define MDH_BEST_APPROX 1 // the first round of that search ranks the corners by an approximate d and directs the winner only (best_approx below)
#endif
#ifdef MDH_BEST_STATS // (the same build; mdh_diag_best_approx takes them)
__device__ unsigned long long g_best_approx_stats[4]; // first-round lanes the rule gave a winner, lanes it gave no candidate, lanes it left undecided, wavefronts that ran the exact scan for them
#define MDH_BEST_APPROX_STAT(slot, n) do { const unsigned long long n_ = (n); if ((threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) atomicAdd(&g_best_approx_stats[slot], n_); } while (0)
#else
#define MDH_BEST_APPROX_STAT(slot, n) do { } while (0)
#endif

struct MachineCfg {
   bool direct_specular;   // M_COMPUTE_DIRECT_SPECULAR
   int spec_mode;          // M_COMPUTE_INDIRECT_SPECULAR: 0 none, 1 .. 3 the three bodies of render_probes.glsl:264-272
   int ao_steps;           // M_AMBIENT_OCCLUSION_STEPS
};

// cage probe i of the cell that holds p (render_probes.glsl:13-20)
MDH_DEV i3 cage_probe(const KProbes &pr, i3 gp, int i)
{
   i3 q;
   q.x = iclamp_(gp.x + (i & 1), 0, pr.gx - 1);
   q.y = iclamp_(gp.y + ((i >> 1) & 1), 0, pr.gy - 1);
   q.z = iclamp_(gp.z + ((i >> 2) & 1), 0, pr.gz - 1);
   return q;
}

// =============================================================================================
// shade_structured -- the same pixel program as lock-step structured code.
//
// All lanes of a wave walk the program together; the two shaded points of a pixel (the
// primary hit, and the hit of its reflection ray: `ctx` 0 and 1) go through ONE loop body,
// so every kind of ray has exactly one march loop in the code: hit rays (primary /
// reflection), soft shadow rays, probe visibility rays, AO taps.  Five SDF sites instead of
// the fifteen of a literal transcription -- the kernel stays inside the instruction cache
// and well under 128 VGPRs.
// =============================================================================================

// -DMDH_PHASES: wall cycles (s_memtime) per wave spent in each region of the pixel program, summed over waves
#ifdef MDH_PHASES
__device__ unsigned long long g_phase[16];
#define MDH_PH_SLOT 19 // one extra park slot: 32 u64 accumulators per wave
MDH_DEV unsigned long long *ph_acc_(float *pk) { return (unsigned long long *)(pk + MDH_PH_SLOT * MDH_BLOCK + (threadIdx.x & ~63)); }
MDH_DEV void ph_add_(float *pk, int id, unsigned long long dt)
{
   if ((int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) ph_acc_(pk)[id] += dt;
}
#define PH_T0(v) unsigned long long v = __builtin_amdgcn_s_memtime()
#define PH_ADD(v, id) do { unsigned long long n_ = __builtin_amdgcn_s_memtime(); ph_add_(pk, id, n_ - v); v = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PH_T0(v) do { } while (0)
#define PH_ADD(v, id) do { } while (0)
#endif
#ifdef MDH_TIMELINE
// wave timeline: [wave] = {start, end} in s_memrealtime ticks (100 MHz), {evals, hw id}
#define MDH_DIAG_WAVES 65536
__device__ unsigned long long g_wave_t[MDH_DIAG_WAVES * 3];
struct DiagWaveTimer {
   long wave;
   unsigned long long t0;
   __device__ DiagWaveTimer(long w) : wave(w), t0(__builtin_amdgcn_s_memrealtime()) {}
   __device__ ~DiagWaveTimer()
   {
      if ((threadIdx.x & 63) == 0 && wave < MDH_DIAG_WAVES) {
         g_wave_t[3 * wave] = t0;
         g_wave_t[3 * wave + 1] = __builtin_amdgcn_s_memrealtime();
         unsigned hw;
         asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
         g_wave_t[3 * wave + 2] = hw;
      }
   }
};
#define MDH_DIAG_WAVE(w) DiagWaveTimer diag_wave_timer_(w)
#else
#define MDH_DIAG_WAVE(w) do { } while (0)
#endif

// raymarching.glsl:25-51: plain sphere trace until a hit or tmax; `steps` counts SDF evaluations
// BOUNDS (MDH_RAY_BOUNDS, the screen pass's fixed mode over the rooms' census): the sphere's and the box's distance bounded from
// below along the whole ray, once, in front of the loop (mdh_device.h: ray_bounds) -- closest_primitive skips a solid's block
// where the bound exceeds the running minimum in every live lane.  The same positions, the same values, the same steps.
template <int PART, bool BOUNDS = false> MDH_DEV bool march_plain(const KScene &sc, f3 o, f3 d, float tmax, float &t_out, int &steps)
{
   int n = 0;
   bool h = false;
   float total = 0.0f;
   // the first sphere and box stay in registers for the whole march (measured: +0.7 %; the same in the shadow,
   // visibility-queue and occlusion marches ±0, in the per-corner visibility march -1 %: register pressure)
   const SdfRegs regs = sdf_regs<(PART & MDH_PF_GTAB) != 0>(sc);
   RayBounds rb;
   if (BOUNDS) rb = ray_bounds(regs, o, d, tmax);
   MDH_WORK(0);
   while (total < tmax) {
      MDH_DIAG_STEP(0);
      MDH_WORK(1);
      float dist;
      if constexpr (BOUNDS) dist = sdf<PART>(sc, o + d * total, regs, rb);
      else dist = sdf<PART>(sc, o + d * total, regs);
      ++n;
      if (dist < MDH_EPS) { h = true; break; }
      total += dist;
   }
   t_out = total;
   steps = n;
   return h;
}

// Per-lane parking space in LDS behind the scene table (MDH_PARK_DWORDS floats per thread,
// [slot][thread] so that a wave's access is one conflict-free row).  What the first shaded
// point leaves behind for the final combine -- position, normal, view direction, direct light,
// irradiance -- is cold while the reflection's point is shaded: parking it takes 15 VGPRs
// out of the live set of the inner loops, where hipcc would otherwise spill them to scratch
// (HBM round trips inside the probe loop; measured 47 % of the wave's cycles waiting).
// slots: 0-2 P, 3-5 N, 6-8 view direction, 9-11 direct light, 12-14 irradiance, 15-17 the reflection's colour,
// 18 material id; the visibility queue (radiance pass) uses 12-15 for its entries, 16 and 17 for first step and result
// before the irradiance is parked
#define MDH_PARK_SPEC 15
#define MDH_PARK_MAT 18
// the radiance pass's kernel that replays its rays' records (RayRecord below) runs no visibility queue: its material id waits in
// row 15, behind the irradiance, and the workgroup takes 16 rows
#define MDH_PARK_MAT_REPLAY 15
#define MDH_REPLAY_PARK_ROWS 16
// ... and the one that writes them parks what the record holds in five rows of its own (read back by the kernel's store)
#define MDH_PARK_REC 19 // t, arg-min index, first step, visibility bits, the primary march's steps
#define MDH_RECORD_PARK_ROWS 24
// mode 2 (direct light and occlusion only: no probes, no reflection) parks P, N, view direction, direct light and the
// material id: 13 rows, so that eight of its workgroups fit a CU's LDS
#define MDH_PARK_MAT_DIRECT 12
#ifdef MDH_PHASES
#define MDH_DIRECT_PARK_ROWS 20 // (room for the accumulators of the diagnostic, MDH_PH_SLOT)
#else
#define MDH_DIRECT_PARK_ROWS 13
#endif
#ifdef MDH_PHASES
#define MDH_PARK_DWORDS 20 // (row 19: the diagnostic's accumulators)
#else
#define MDH_PARK_DWORDS 19
#endif
// screen pass only, during the FIRST point's corner loop: the rows of its irradiance (12-14, parked behind the loop) and
// of the reflection's colour (15-17, cleared behind the loop) are free and hold what the loop needs at every corner but
// must not keep in registers across its marches -- the position inside the cage (alpha) and the clamped octahedral
// texel of N
#define MDH_PARK_ALPHA 12
#define MDH_PARK_RIDN 15
// ... and row 17, the one row of the reflection's colour that alpha and the texel leave free (12-14 and 15-16 are theirs), holds
// what a wavefront shares across its lanes there (MDH_SHARE_TAPS): sqrt(irradiance tap) of the eight cage probes, [corner][3]
// in the wavefront's first 24 columns.  Every lane reads every column: plain LDS accesses, ordered like queued_visibility's rows.
#define MDH_PARK_TAPS 17
typedef __attribute__((address_space(3))) float *ParkLds; // (row r, column c of a wavefront: park_wave_base + (r * MDH_BLOCK + c) * 4)
#define MDH_SCR_PARK_ROWS MDH_PARK_DWORDS
MDH_DEV float *park_base(const KScene &sc) { return (float *)(s_tab + sc.table_f4 + sc.part_bits_f4); }
// A thread's own column of the park rows is addressed WITHOUT an address register: ds_write_addtid_b32 /
// ds_read_addtid_b32 take M0[15:0] + offset + 4 * lane (scripts/addtid_probe.hip checks that on the box), so a park
// access costs one LDS instruction per dword and one scalar -- the LDS byte address of the wave's 64 columns in row 0
// -- stays live instead of a per-lane address that the compiler kept in scratch.  M0 is saved and restored (it is
// compiler-reserved); `s_nop 0`: one wait state between a write of M0 and an LDS add-TID instruction.  The reads wait
// for their data inside the statement (the compiler does not count the LDS operations of an asm statement).
MDH_DEV int park_wave_base(const float *pk)
{
   const unsigned lds = (unsigned)(size_t)(const __attribute__((address_space(3))) float *)pk;
   return __builtin_amdgcn_readfirstlane((int)(lds + (threadIdx.x & ~63u) * 4u));
}
template <int SLOT> MDH_DEV void park_store3(float *pk, int wb, f3 v)
{
   unsigned keep;
   asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tds_write_addtid_b32 %1 offset:%5\n\tds_write_addtid_b32 %2 offset:%6\n\t"
                "ds_write_addtid_b32 %3 offset:%7\n\ts_mov_b32 m0, %0"
                : "=&s"(keep) : "v"(v.x), "v"(v.y), "v"(v.z), "s"(wb), "i"(SLOT * MDH_BLOCK * 4), "i"((SLOT + 1) * MDH_BLOCK * 4), "i"((SLOT + 2) * MDH_BLOCK * 4) : "memory");
}
template <int SLOT> MDH_DEV f3 park_load3(const float *pk, int wb)
{
   unsigned keep;
   f3 v;
   asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tds_read_addtid_b32 %1 offset:%5\n\tds_read_addtid_b32 %2 offset:%6\n\t"
                "ds_read_addtid_b32 %3 offset:%7\n\ts_waitcnt lgkmcnt(0)\n\ts_mov_b32 m0, %0"
                : "=&s"(keep), "=&v"(v.x), "=&v"(v.y), "=&v"(v.z) : "s"(wb), "i"(SLOT * MDH_BLOCK * 4), "i"((SLOT + 1) * MDH_BLOCK * 4), "i"((SLOT + 2) * MDH_BLOCK * 4) : "memory");
   return v;
}
template <int SLOT> MDH_DEV f2 park_load2(const float *pk, int wb)
{
   unsigned keep;
   f2 v;
   asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tds_read_addtid_b32 %1 offset:%4\n\tds_read_addtid_b32 %2 offset:%5\n\t"
                "s_waitcnt lgkmcnt(0)\n\ts_mov_b32 m0, %0"
                : "=&s"(keep), "=&v"(v.x), "=&v"(v.y) : "s"(wb), "i"(SLOT * MDH_BLOCK * 4), "i"((SLOT + 1) * MDH_BLOCK * 4) : "memory");
   return v;
}
template <int SLOT> MDH_DEV void park_store1(float *pk, int wb, float v)
{
   unsigned keep;
   asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tds_write_addtid_b32 %1 offset:%3\n\ts_mov_b32 m0, %0"
                : "=&s"(keep) : "v"(v), "s"(wb), "i"(SLOT * MDH_BLOCK * 4) : "memory");
}
template <int SLOT> MDH_DEV float park_load1(const float *pk, int wb)
{
   unsigned keep;
   float v;
   asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tds_read_addtid_b32 %1 offset:%3\n\ts_waitcnt lgkmcnt(0)\n\ts_mov_b32 m0, %0"
                : "=&s"(keep), "=&v"(v) : "s"(wb), "i"(SLOT * MDH_BLOCK * 4) : "memory");
   return v;
}


// ---------------------------------------------------------------------------------------------
// queued_visibility -- the probe-visibility rays of the wave's 64 shaded points as ONE queue.
//
// In lock step a wave pays, for each of the 8 cage corners, the longest visibility ray among
// its lanes, while folded corners and rays that end at once leave lanes empty: the radiance
// pass ran its visibility marches at 15 of 64 lanes.  Here every lane first lists the rays its
// point really needs (corner i of lane l = entry l | i << 6, appended with a ballot prefix sum),
// then the wave marches the list with ray REPLACEMENT: a lane whose ray has ended takes the
// next entry, re-deriving origin, direction and length from the owner lane's parked P, N and
// first-step distance (bit for bit the arithmetic of the lock-step loop), and ORs the
// result into the owner's visibility word.  Results per ray are unchanged; only the schedule is.
//
// LDS: entries are u16 in park slots 12..15 of the wave (free until the irradiance is parked),
// slot 16 = first-step distance, slot 17 = visibility word.
// ---------------------------------------------------------------------------------------------
#ifndef MDH_CORNER_UNROLL
#define MDH_CORNER_UNROLL 8 // the cage-corner loop of the pixel program, unrolled: constant corner bits, no loop branch (measured 1, 2, 4, 8)
#endif
#ifndef MDH_QVIS_REFILL
#define MDH_QVIS_REFILL 16 // idle lanes that trigger a refill
#endif
MDH_DEV unsigned short *qvis_entry(float *pk, int wbase, int j)
{
   return (unsigned short *)(pk + (12 + (j >> 7)) * MDH_BLOCK + wbase) + (j & 127);
}
template <int PART>
MDH_DEV int queued_visibility(const KScene &sc, const KProbes &pr, float *pk, f3 P, f3 N, i3 gp, int folded, float sd0)
{
   const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
   int *words = (int *)(pk + 17 * MDH_BLOCK);
   pk[16 * MDH_BLOCK + threadIdx.x] = sd0;
   words[threadIdx.x] = 0;
   int bits = 0, njobs = 0;
   // The queue is taken from its head: every lane lists its FARTHEST cage corner first (the far side of each axis: the
   // corner j ^ far for j = 0 .. 7 goes from the farthest to the nearest), so that the longest rays of the wave start first
   // and its last rays are short ones -- the queue drains with fewer idle lanes.  The order of the list decides nothing else.
   int far = 0;
   {
      const f3 lo = grid_to_world(pr, gp);
      far = ((P.x - lo.x) < (lo.x + pr.sx - P.x) ? 1 : 0) | ((P.y - lo.y) < (lo.y + pr.sy - P.y) ? 2 : 0) | ((P.z - lo.z) < (lo.z + pr.sz - P.z) ? 4 : 0);
   }
#pragma unroll 1
   for (int j = 0; j < 8; ++j) {
      const int i = j ^ far;
      bool need = false;
      if (!(i & folded)) {
         const f3 hvec = grid_to_world(pr, cage_probe(pr, gp, i)) - P;
         const float vmax = length(hvec) - MDH_MIN_STEP * 5.0f;
         // raycast_visibility (raymarching.glsl:39-56) whose first step is known: sd0 at t = 0
         if (!(0.0f < vmax)) bits |= 1 << i;     // the loop is never entered
         else if (sd0 < MDH_EPS) { }             // blocked at once
         else if (!(sd0 < vmax)) bits |= 1 << i; // the first step already passes the probe
         else if (segment_clear<PART>(sc, P + (N * MDH_MIN_STEP) * 5.0f, sdiv3(hvec, length(hvec)), vmax)) bits |= 1 << i; // proved unblocked (the march's o, d, vmax)
         else need = true;
      }
      const unsigned long long m = __ballot(need);
      if (need) *qvis_entry(pk, wbase, njobs + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))) = (unsigned short)(lane | (i << 6));
      njobs += __popcll(m);
   }
   __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
   __builtin_amdgcn_wave_barrier();
   __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
   int head = 0, job = -1;
   float total = 0.0f, vmax = 0.0f;
   f3 o = F3(0.0f, 0.0f, 0.0f), d = F3(0.0f, 0.0f, 0.0f);
   // only the lanes whose point was hit are here: a wave with fewer of them than the refill threshold (rays that
   // left an open scene) must still start its queue
   const int refill = min((int)MDH_QVIS_REFILL, (int)__popcll(__ballot(true)));
   for (;;) {
      const unsigned long long idle = __ballot(job < 0);
      const int n_idle = __popcll(idle);
      if (head < njobs && n_idle >= refill) {
         if (job < 0) {
            const int my = head + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0u));
            if (my < njobs) {
               const int e = *qvis_entry(pk, wbase, my);
               const int owner = wbase + (e & 63), corner = e >> 6;
               const f3 oP = F3(pk[0 * MDH_BLOCK + owner], pk[1 * MDH_BLOCK + owner], pk[2 * MDH_BLOCK + owner]);
               const f3 oN = F3(pk[3 * MDH_BLOCK + owner], pk[4 * MDH_BLOCK + owner], pk[5 * MDH_BLOCK + owner]);
               const f3 hvec = grid_to_world(pr, cage_probe(pr, world_to_grid(pr, oP), corner)) - oP;
               const float dist = length(hvec);
               d = sdiv3(hvec, dist);
               vmax = dist - MDH_MIN_STEP * 5.0f;
               o = oP + (oN * MDH_MIN_STEP) * 5.0f;
               total = pk[16 * MDH_BLOCK + owner];
               job = e;
            }
         }
         head += n_idle;
      }
      if (__ballot(job >= 0) == 0ull) break;
      if (job >= 0) {
         MDH_DIAG_STEP(3);
         MDH_WORK(1);
         const float sd = sdf<PART>(sc, o + d * total);
         if (sd < MDH_EPS) job = -1; // blocked: the bit stays 0
         else {
            total += sd;
            if (!(total < vmax)) {
               atomicOr(&words[wbase + (job & 63)], 1 << (job >> 6));
               job = -1;
            }
         }
      }
   }
   __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
   __builtin_amdgcn_wave_barrier();
   __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
   return bits | words[threadIdx.x];
}

// sample_radiance_with_specular (render_probes.glsl:71-136, M_COMPUTE_INDIRECT_SPECULAR == 1) from the reflection's hit
// position on: the eight cage probes of the FIRST point (parked: slots 0-2, its material id in MDH_PARK_MAT) light
// that position, each weighted by a soft shadow ray from it towards the probe (k = 0.5, raymarching.glsl:4-23 with
// its min_dist) and the trilinear factor of the first point.  textureLod is level 0 (one level): lod
// only narrows the clamp of the tap; a total weight of 0 gives 0.
template <int PART>
MDH_DEV f3 radiance_with_specular(const KScene &sc, const KProbes &pr, const float *pk, int wb, f3 spec_pos, int u8_tab)
{
   const f3 pos = park_load3<0>(pk, wb);
   const float roughness = tab_float((sc.mat_slot + 2 * __float_as_int(park_load1<MDH_PARK_MAT>(pk, wb)) + 1) * 4);
   const f3 pos_to_spec_pos = spec_pos - pos;
   const i3 gp = world_to_grid(pr, pos);
   const f3 alpha = pos / F3(pr.sx, pr.sy, pr.sz) - F3((float)gp.x, (float)gp.y, (float)gp.z);
   const float lod = mix_(0.0f, (float)pr.rad_lods, roughness * 2.0f);
   const int new_res = pr.rres / (int)(lod + 1.0f);
   const float rmin = 0.5f / (float)new_res, rmax = 1.0f - rmin;
   float total_weight = 0.0f;
   f3 radiance = F3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
   for (int i = 0; i < 8; ++i) {
      const i3 q = cage_probe(pr, gp, i);
      f3 pts = (pos - grid_to_world(pr, q)) + pos_to_spec_pos; // probe_to_spec
      const float distance = length(pts);
      pts = pts / distance;
      float res = 1.0f, prev = 1e20f;
      bool blocked = false;
      const float tmax = distance - MDH_MIN_STEP * 5.0f;
      MDH_WORK(0);
      for (float total = MDH_MIN_STEP * 5.0f; total < tmax;) { // softshadows (spec_pos, -probe_to_spec, .., 0.5)
         MDH_WORK(1);
         const float dist = sdf<PART>(sc, spec_pos + (-pts) * total);
         if (dist < MDH_EPS) { blocked = true; break; }
         const float y = dist * dist / (2.0f * prev);
         const float d = sqrt_(dist * dist - y * y);
         res = min_(res, 0.5f * d / max_(0.0f, total - y));
         prev = dist;
         total += dist;
      }
      float weight = max_(blocked ? 0.0f : res, 0.001f);
      const f3 tri = F3(mix_(1.0f - alpha.x, alpha.x, (float)(i & 1)), mix_(1.0f - alpha.y, alpha.y, (float)((i >> 1) & 1)),
                        mix_(1.0f - alpha.z, alpha.z, (float)((i >> 2) & 1)));
      weight *= tri.x * tri.y * tri.z;
      const f2 base = probe_id_to_coord(pr, grid_to_probe_id(pr, q));
      f2 rid = ray_dir_to_ray_id(pts);
      rid = F2(clamp_(rid.x, rmin, rmax), clamp_(rid.y, rmin, rmax));
      const f3 tx = pr.rad_mips ? radiance_lod_sample(pr, lod, base.x + div_pcx(pr, rid.x), base.y + div_pcy(pr, rid.y), u8_tab) // (MDH_OPT_RADIANCE_MIPS)
                                : atlas_sample(pr.rad, pr.fmt, pr.pcx, pr.pcy, pr.rres, pr.rshift, pr.rad_w, pr.rad_h, base.x + div_pcx(pr, rid.x), base.y + div_pcy(pr, rid.y), u8_tab, pr.m_rres);
      radiance = radiance + tx * weight;
      total_weight += weight;
   }
   if (total_weight == 0.0f) return F3(0.0f, 0.0f, 0.0f);
   return radiance / total_weight;
}

// The probe settings again, from the kernel argument segment, at the point of use.  Both march kernels take
// (KScene, KProbes, ...): held in scalar registers from the kernel's entry, the 48 dwords of KProbes stay live across
// every march loop of the pixel program, and what does not fit is copied to and from VGPR lanes with a vector
// instruction per use (the screen kernel had a thousand such copies, a third of them in inner loops).  Re-read where a
// block of probe code begins -- a few scalar loads through a pointer the compiler cannot trace, served by the scalar
// cache -- they are live for that block only.
MDH_DEV KProbes probes_fresh(const KProbes &pr)
{
   struct KHead { KScene sc; KProbes pr; };
   typedef const KHead __attribute__((address_space(4))) *KHeadPtr;
   KHeadPtr ka = (KHeadPtr)__builtin_amdgcn_kernarg_segment_ptr();
   asm volatile("" : "+s"(ka));
   typedef const int __attribute__((address_space(4))) *IntPtr;
   IntPtr src = (IntPtr)&ka->pr;
   KProbes r;
   int *dst = (int *)&r;
#pragma unroll
   for (int q = 0; q < (int)(sizeof(KProbes) / 4); ++q) dst[q] = src[q];
   return r;
}

// best_approx (MDH_BEST_APPROX) -- the first round of the second point's best-first search (shade_structured) without the exact
// directions of the losers.  The exact scan computes, per unfolded corner i with h = P - pw_i (pw_i = grid_to_world (cage_probe (i))),
//    d_i = -((v.x N.x + v.y N.y) + v.z N.z),  v = h / sqrt_ (dot2 (h))    (a correctly rounded root and three IEEE divisions)
// and keeps the largest d_i > 0, the lowest index among equals.  Here every lane ranks the corners by
//    a_i = -((h.x N.x + h.y N.y) + h.z N.z) * v_rsq_f32 (dot2 (h))
// with h's three differences, their squares and their products with N formed once for the offsets 0 and 1 of each axis: the
// same float operations on the same values as grid_to_world and the subtraction of the scan (an unfolded axis is not clamped by
// cage_probe, so its offset-1 probe is gp + 1; a folded one takes its clamped offset-0 probe only), hence h is the scan's h bit
// for bit and only what follows it differs.
//
// The bound eps on |a_i - d_i|.  u = 2^-24 (one rounding to nearest, relative), L = |h|, t = -dot (h, N) / L the real value,
// |N| <= sqrt 3 (every component at most 1 in magnitude, tested below), terms of order u^2 left to the margin at the end.
//   d_i:  dot2 (h) has relative error 3 u (a product and two sums of positive terms), its root 3 u / 2 + u, each quotient
//         h.c / dist one more: 3.5 u per component of v.  The dot product with N adds a rounding per product and per sum, at
//         most 3 u on the sum of |v.c N.c| <= |v| |N|:  |d_i - t| <= 6.5 u |v| |N| <= 6.5 sqrt 3 u < 11.3 u.
//   a_i:  the products and sums of dot (h, N): 3 u L |N| absolute.  v_rsq_f32 is good to one ulp (2 u relative) of the inverse
//         root of a dot2 that is 3 u off (1.5 u on the root): 3.5 u on 1 / L.  The last product one more:
//         |a_i - t| <= (3 + 3.5 + 1) u |N| = 7.5 sqrt 3 u < 13 u.
// Range: |P.c| <= lim, the grid's far corner within lim (so every probe considered is) and |N.c| <= 1 are tested below, a NaN fails
// each of them, and lim <= 2^18: every h.c is finite, L <= 2 sqrt 3 lim and dot2 (h) <= 12 lim^2 < 2^40.  dot2 (h) >= 2^-40 is tested
// for the smallest one: L >= 2^-20, dot2 and its inverse root are normal, and a product h.c N.c or v.c N.c or a square that underflows
// is off by 2^-149 at most -- times 1 / L <= 2^20 still below 2^-129.  So no a_i is infinite or a NaN.  Together
// |a_i - d_i| < 24.3 u (1 + 2^-20), and eps = 2^-19 = 32 u holds it.  lim does not enter eps: every error above is relative to L |N|.
//
// The rule, per lane, with a_1 the largest a_i (lowest index among equals) and a_2 the runner-up (-4 where there is none: every
// a_i >= -sqrt 3 - eps):
//   1  a_1 - a_2 > 2 eps and a_1 > eps: d of that corner exceeds every other d_i (d_1 > a_1 - eps > a_2 + eps >= a_i + eps > d_i)
//      and is positive: the exact scan names it, whatever the order among the others.  `bi` is its index.
//   2  a_1 < -eps: every d_i < 0: the exact scan finds no candidate.
//   0  anything else -- a near tie, a_1 within eps of 0, a failed range test: undecided, the exact scan decides.
// A corner folded in this lane but not in every lane of the wavefront takes its twin's dot2 and 32 lim in the place of its N product:
// the other two products are at most 2 lim each, so dot (h, N) >= 28 lim and a <= -28 lim / (2 sqrt 3 lim) < -8: below the -4 that
// a_1 and a_2 start from, it enters neither.  A corner folded in every lane is not computed.
// (Inline constants, scalars and powers of two through v_ldexp_f32 only: a literal that a compare or a select cannot encode becomes a
//  register, which the compiler holds across the pixel program's loop over its two points -- item 19's lesson.  The x and y terms are
//  kept, the z terms formed per offset: eight registers of terms instead of twelve.)
#define MDH_BEST_APPROX_EPS_LOG2 (-19)
MDH_DEV int best_approx(const KProbes &pr, i3 gp, int folded, f3 P, f3 N, int &bi)
{
   const KProbes pq = probes_fresh(pr);
   const float lim = __int_as_float(hdr(H_VCLEAR_LIM));
   const int wf = (__ballot(!(folded & 1)) ? 0 : 1) | (__ballot(!(folded & 2)) ? 0 : 2) | (__ballot(!(folded & 4)) ? 0 : 4); // folded in every lane
   bool ok = (unsigned)__float_as_int(lim) <= 0x48800000u; // 0 <= lim <= 2^18, no NaN
   ok = ok && __builtin_fabsf(P.x) <= lim && __builtin_fabsf(P.y) <= lim && __builtin_fabsf(P.z) <= lim;
   ok = ok && __builtin_fabsf(N.x) <= 1.0f && __builtin_fabsf(N.y) <= 1.0f && __builtin_fabsf(N.z) <= 1.0f;
   ok = ok && __builtin_fabsf((float)(pq.gx - 1) * pq.sx) <= lim && __builtin_fabsf((float)(pq.gy - 1) * pq.sy) <= lim && __builtin_fabsf((float)(pq.gz - 1) * pq.sz) <= lim;
   const float out = __builtin_ldexpf(lim, 5); // a folded corner's place holder
   float sq[2][2], pn[2][2];
   {
      const float h0 = P.x - (float)iclamp_(gp.x, 0, pq.gx - 1) * pq.sx, h1 = P.x - (float)(gp.x + 1) * pq.sx;
      sq[0][0] = h0 * h0; pn[0][0] = h0 * N.x;
      sq[0][1] = (folded & 1) ? sq[0][0] : h1 * h1; pn[0][1] = (folded & 1) ? out : h1 * N.x;
   }
   {
      const float h0 = P.y - (float)iclamp_(gp.y, 0, pq.gy - 1) * pq.sy, h1 = P.y - (float)(gp.y + 1) * pq.sy;
      sq[1][0] = h0 * h0; pn[1][0] = h0 * N.y;
      sq[1][1] = (folded & 2) ? sq[1][0] : h1 * h1; pn[1][1] = (folded & 2) ? out : h1 * N.y;
   }
   float a1 = -4.0f, a2 = -4.0f, dmin = 4.0f; // (dmin: the smallest dot2, or 4)
   bi = -1;
#pragma unroll
   for (int bz = 0; bz < 2; ++bz) {
      if ((bz << 2) & wf) continue;
      const bool fz = bz && (folded & 4);
      const float hz = P.z - (float)((bz && !fz) ? gp.z + 1 : iclamp_(gp.z, 0, pq.gz - 1)) * pq.sz;
      const float sz = hz * hz, nz = fz ? out : hz * N.z;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
         if (j & wf) continue;
         const float d2 = (sq[0][j & 1] + sq[1][j >> 1]) + sz;
         const float dn = (pn[0][j & 1] + pn[1][j >> 1]) + nz;
         const float a = -dn * __builtin_amdgcn_rsqf(d2);
         dmin = min_(dmin, d2);
         if (a > a1) bi = j | (bz << 2);
         a2 = __builtin_amdgcn_fmed3f(a, a1, a2);
         a1 = max_(a1, a);
      }
   }
   ok = ok && __builtin_ldexpf(dmin, 40) >= 1.0f;
   const float lead = __builtin_ldexpf(a1 - a2, -MDH_BEST_APPROX_EPS_LOG2), top = __builtin_ldexpf(a1, -MDH_BEST_APPROX_EPS_LOG2); // in units of eps
   if (ok && lead > 2.0f && top > 1.0f) return 1;
   if (ok && top < -1.0f) return 2;
   return 0;
}

// ---------------------------------------------------------------------------------------------
// RayRecord -- what a probe ray's marches find, which follows from the scene's geometry alone (MDH_OPT_RADIANCE_REPLAY,
// DESIGN.md section 4, "Exact work elimination", item 11).  A probe ray starts at a fixed probe in a fixed octahedral
// direction: whether it hits, where (t), which primitive is nearest there (sdf_info's arg-min), how many steps it took,
// the first-step distance sd0 at the hit point's offset and the visibility of the hit point's eight cage probes do not
// change with lights, materials or atlases.  The pass that follows a pass over the same geometry writes one record per ray
// (REC = 1), the passes behind it read it back (REC = 2) and feed the same values into the same operations: P = ro + rd * t,
// primitive_info, the light loop with its shadow rays, the eight taps.  16 bytes, indexed by the RAY (probe of the slice *
// texels + texel), never by the lane: RadOrder moves rays between lanes.
// ---------------------------------------------------------------------------------------------
#ifndef MDH_RAD_REPLAY
#if defined(MDH_DIAG) || defined(MDH_PHASES)
#define MDH_RAD_REPLAY 0 // (the diagnostic builds count or time the work of the marches: they keep marching)
#else
#define MDH_RAD_REPLAY 1
#endif
#endif
#if MDH_RAD_REPLAY && defined(MDH_PHASES)
#error "MDH_PHASES keeps its accumulators in park row 19 (MDH_PH_SLOT): the recording kernel's rows start there and the replaying kernel allocates 16 rows -- build the phase timers with MDH_RAD_REPLAY=0"
#endif
struct RayRecord {
   unsigned t;     // the primary march's t, bit for bit
   unsigned sd0;   // sdf at P + 5 MIN_STEP N, bit for bit
   int index;      // sdf_info's arg-min at P
   unsigned word;  // bits 0-22 the primary march's steps, 23-30 queued_visibility's bits, 31 hit
};
static_assert(sizeof(RayRecord) == 16, "one 16-byte store per ray");
#define MDH_REC_STEPS_MASK 0x7fffffu
MDH_DEV unsigned ray_record_word(bool hit, int steps, int vis_bits)
{
   return min((unsigned)steps, MDH_REC_STEPS_MASK) | ((unsigned)(vis_bits & 255) << 23) | (hit ? 0x80000000u : 0u);
}

// ---------------------------------------------------------------------------------------------
// MDH_OPT_SCREEN_REPLAY ("Exact work elimination", item 12): the same for the screen pass's two shaded
// points.  A pixel of a standing camera over standing geometry finds the same primary hit, the same reflection hit, the same
// first steps and the same cage visibility in every frame; its occlusion term reads the geometry only.  One PixelRecord per
// pixel, indexed by the PIXEL (the tile's place among the rank's tiles * 64 + the pixel's place in its tile), never by the
// lane: MDH_OPT_SCREEN_ORDER moves tiles between launch places, MDH_OPT_SCREEN_SPLIT hands a tile to several wavefronts.
//   first:   RayRecord of the primary ray and its hit point, as above (word bits 23-30: the corner loop's eight bits)
//   second:  the reflection ray and its hit point: t and sd0 as above; `word` bits 0-21 the arg-min index + 1, bit 22 a
//            reflection ray was traced, 23-30 the corner loop's bits, 31 hit; `index` holds the 32 bits of the occlusion
//            term of the FIRST point (0 when no occlusion step is set)
// ---------------------------------------------------------------------------------------------
#ifndef MDH_SCR_REPLAY
#if defined(MDH_DIAG) || defined(MDH_PHASES)
#define MDH_SCR_REPLAY 0 // (the diagnostic builds count or time the work of the marches: they keep marching)
#else
#define MDH_SCR_REPLAY 1
#endif
#endif
#if MDH_SCR_REPLAY && defined(MDH_PHASES)
#error "MDH_PHASES keeps its accumulators in park row 19 (MDH_PH_SLOT), where the recording screen kernel's rows start -- build the phase timers with MDH_SCR_REPLAY=0"
#endif
struct PixelRecord { RayRecord first, second; };
static_assert(sizeof(PixelRecord) == 32, "two 16-byte loads or stores per pixel");
#define MDH_PIXEL_RECORD_BYTES 32
#define MDH_REC2_INDEX_MASK 0x3fffffu // the second point's arg-min index + 1 (a flat index into a table that fits LDS: below 4 096)
#define MDH_REC2_TRACED 0x400000u
// the recording screen kernel's park rows: MDH_PARK_REC + 0 .. 4 the first point's t, arg-min index, first step, visibility
// bits and the primary march's steps; + 5 .. 8 the same of the second point, + 9 its flags (bit 0 traced, bit 1 hit);
// + 10 the occlusion term
#define MDH_PARK_REC2 (MDH_PARK_REC + 5)
#define MDH_PARK_REC_AO (MDH_PARK_REC + 10)
#define MDH_SCR_RECORD_PARK_ROWS (MDH_PARK_REC + 11)
MDH_DEV unsigned pixel_record_word2(bool hit, bool traced, int index, int vis_bits)
{
   return min((unsigned)(index + 1), MDH_REC2_INDEX_MASK) | (traced ? MDH_REC2_TRACED : 0u) | ((unsigned)(vis_bits & 255) << 23) | (hit ? 0x80000000u : 0u);
}

// SPEC: 0 = no second point (the radiance pass), 1 = the reflection as the reference's renderer fixes it
// (M_COMPUTE_INDIRECT_SPECULAR = 2, or none), 2 = the kernel variant that holds the two other bodies of
// render_probes.glsl:264-272 (cfg.spec_mode 1 or 3; MDH_OPT_INDIRECT_SPECULAR)
// REC (the radiance pass with the queue only): 0 = march, 1 = march and park what a RayRecord holds (rows MDH_PARK_REC ..)
// for the kernel's store, 2 = take the record `rec` instead of the primary march, the arg-min scan, the first step and the queue
// REC with SPEC = 1 (the screen pass of the reference's fixed mode, brute-force scan or room census): the same for both
// shaded points -- 1 parks what a PixelRecord holds, 2 takes `rec` and `rec2` instead of both marches, both arg-min scans,
// both first steps, every visibility march of both corner loops and the occlusion steps
// NULLB: null_light in front of the BRDF (MDH_SKIP_NULL_BRDF); false where the caller's kernel has no register to spare for it.
// The predicate's lane masks live in SGPRs beside the light loop.  Which instantiations leave it out, and shade every light with
// the code they had before (resource_usage.sh and bench.py, before against after):
//   every space-partition variant (PART & MDH_PF_PART, decided in shade_structured): they run at 104 - 106 SGPRs; two of them
//       gained 16 bytes of scratch per lane, and simple_scene, whose point light leaves few wavefronts wholly null, lost 0.5 %;
//   k_screen <POW2, 0, GBUF>                 brute-force scan, power-of-two atlases, geometry buffer: scratch 32 -> 48 bytes per lane;
//   k_radiance <0 | POW2, SMALL, REC = 1>    the brute-force scan's recording kernel, small form: 101 SGPRs, 8 -> 7 wavefronts per SIMD.
constexpr bool null_brdf_screen(int PART, int MODE, bool GBUF, bool ALT, int REC) { return !(GBUF && PART == MDH_PF_POW2 && MODE == 0 && !ALT && REC == 0); }
constexpr bool null_brdf_radiance(int PART, bool SMALL, int REC) { return !((PART & ~MDH_PF_POW2) == 0 && SMALL && REC == 1); }
// SHARET (0, 1; 2 below): a wavefront's eight irradiance taps fetched once where its lanes share them (MDH_SHARE_TAPS, at the first point's corner
// loop); false where the caller's kernel would pay for it with scratch memory.  Every screen kernel that takes it keeps its
// wavefronts per SIMD; the eight below gained 16 bytes of scratch per lane and keep the code they had (resource_usage.sh, before
// against after):
//   k_screen <0, 0, no GBUF, REC 0>              brute-force scan, marching:                      16 -> 32
//   k_screen <ROOM, 0, GBUF and no GBUF, REC 2>  the rooms' census, replaying:                    64 -> 80, 48 -> 80
//   k_screen <ROOM | POW2, 0, no GBUF, REC 1>    ... with power-of-two atlases, recording:        32 -> 48
//   k_screen <ROOM | POW2, 0, GBUF, REC 0 and 1> ... with the geometry buffer:                    48 -> 64, 64 -> 80
//   k_screen <POW2, 0, GBUF, REC 0 and 1>        brute-force scan, power-of-two atlases, GBUF:    32 -> 48
constexpr bool share_taps_screen(int PART, bool GBUF, int REC)
{
   return !((PART == 0 && !GBUF && REC == 0) || (PART == MDH_PF_ROOM && REC == 2) || (PART == (MDH_PF_ROOM | MDH_PF_POW2) && !GBUF && REC == 1) ||
            (PART == (MDH_PF_ROOM | MDH_PF_POW2) && GBUF && REC != 2) || (PART == MDH_PF_POW2 && GBUF && REC != 2));
}
// SHARET = 2: a sharing wavefront's corner folded along y or z takes its twin's weight and visibility bit (MDH_TWIN_FOLDED; DESIGN.md
// section 4 item 16).  The screen kernels that share taps take it and keep their scratch memory and their wavefronts per SIMD to
// the digit -- the benchmark's k_screen <ROOM | POW2, 0, no GBUF, REC 0> 32 bytes and six; two gain one VGPR below their limit --
// but for seven, which keep the code they had.  Four paid with scratch memory (resource_usage.sh, before against after):
//   k_screen <0, 0, GBUF, REC 2>                 brute-force scan with the geometry buffer, replaying:  16 -> 32
//   k_screen <POW2, 0, no GBUF, REC 0>           ... with power-of-two atlases, marching:               16 -> 32
//   k_screen <POW2, 0, GBUF, REC 2>              ... with the geometry buffer, replaying:               16 -> 32
//   k_screen <ROOM | POW2, 0, no GBUF, REC 2>    the rooms' census, power-of-two atlases, replaying:    64 -> 96
// and three paid in a build that held this beside two parts since removed, and were not built with it alone:
//   k_screen <0, 0, GBUF, REC 0>, k_screen <ROOM, 0, no GBUF, REC 1>, k_screen <ROOM | POW2, 0, GBUF, REC 2>
// k_ray_shade <0, 0> and k_point_shade <0, 0> share taps too and are left as they are (shade_structured's default): their
// wavefronts are a caller's rays and points, not tiles of a surface.
constexpr bool folded_twins_screen(int PART, bool GBUF, int REC)
{
   return share_taps_screen(PART, GBUF, REC) &&
          !((PART == 0 && GBUF && REC != 1) || (PART == MDH_PF_POW2 && !GBUF && REC == 0) || (PART == MDH_PF_POW2 && GBUF && REC == 2) ||
            (PART == (MDH_PF_ROOM | MDH_PF_POW2) && REC == 2) || (PART == MDH_PF_ROOM && !GBUF && REC == 1));
}
// SHARET | 4: the second point's best cage probe searched best first (MDH_BEST_FIRST, in front of the corner loop; DESIGN.md section 4
// item 17) -- a bit of its own beside the two of the sharing level, which is SHARET & 3.  The screen kernels of the fixed mode over the built-in scans, marching and recording, take it and keep their registers,
// their scratch memory and their wavefronts per SIMD to the digit (the scan over the corners is a rolled loop: unrolled it cost
// every one of them 16 bytes of scratch per lane) -- but for three, which paid 16 bytes and keep the code they had
// (resource_usage.sh, before against after):
//   k_screen <0, 0, GBUF, REC 0>            brute-force scan with the geometry buffer, marching:      32 -> 48
//   k_screen <POW2, 0, GBUF, REC 1>         ... with power-of-two atlases, recording:                 32 -> 48
//   k_screen <ROOM, 0, GBUF, REC 1>         the rooms' census with the geometry buffer, recording:    64 -> 80
// k_ray_shade and k_point_shade are left as they are (shade_structured's default).
constexpr bool best_first_screen(int PART, bool GBUF, int REC)
{
   return REC != 2 && !(GBUF && ((PART == 0 && REC == 0) || (PART == MDH_PF_POW2 && REC == 1) || (PART == MDH_PF_ROOM && REC == 1)));
}
// MDH_RAY_BOUNDS (item 19 of "Exact work elimination", at march_plain above): the primary and the reflection march of the screen
// family's fixed mode over the rooms' census, marching and recording, with and without the geometry buffer.  No variant paid for the
// two registers in scratch memory or wavefronts (resource_usage.sh).  k_ray_shade and k_point_shade are left as they are.
constexpr bool ray_bounds_screen(int PART, bool GBUF, int REC)
{
   return REC != 2 && (PART & ~MDH_PF_POW2) == MDH_PF_ROOM;
}
// POINT (k_point_shade, mdh_kernels.h: mdh_shade_points): the first shaded point is the caller's -- `from` is the point itself,
// `dir_in` the direction it is seen along, `pt_normal` and `pt_material` what primitive_info would have said -- and context 0
// runs no primary march, no arg-min scan and no primitive_info: every valid lane "hits" at its point with index -1, t 0 and
// no steps, and everything from the offset origin on is the code of a marched hit.  false (every other kernel): nothing changes.
template <int PART, int MODE, int SPEC, bool QVIS, int REC = 0, int SHARET = 1, bool NULLB = true, bool POINT = false>
MDH_DEV f3 shade_structured(const KScene &sc, const KProbes &pr, const MachineCfg cfg, bool lane_valid, f3 from, f3 dir_in,
                            PrimaryHit &ph, bool &hit, f3 &pos_out, const RayRecord rec = RayRecord{0u, 0u, -1, 0u},
                            const RayRecord rec2 = RayRecord{0u, 0u, -1, 0u}, const f3 pt_normal = F3(0.0f, 0.0f, 0.0f), const int pt_material = 0)
{
   static_assert(!POINT || (REC == 0 && SPEC == 1 && !QVIS && MODE != 1), "a caller's point goes through the screen pass's program, mode 0 or 2, without records");
   static_assert(REC == 0 || (SPEC == 0 && QVIS && MODE == 0) || (SPEC == 1 && !QVIS && MODE == 0 && !(PART & MDH_PF_PART) && MDH_SHARE_FIRST_STEP),
                 "records are of the radiance pass's rays or of the screen pass's fixed mode without a space partition");
   constexpr bool SREC = REC != 0 && SPEC == 1; // the screen pass's records
   constexpr bool P2 = (PART & MDH_PF_POW2) != 0;
   constexpr bool NULL_BRDF = MDH_NULL_BRDF != 0 && NULLB && !(PART & MDH_PF_PART); // item 14 of "Exact work elimination": null_light in front of the BRDF
   constexpr bool REFLECT = SPEC != 0 && MODE == 0; // (modes 1 and 2 never shade a second point: no loop, and nothing kept for one)
   // The cage-corner loop unrolled where the registers allow it (the brute-force screen kernel of the reference's fixed mode:
   // 96 VGPRs with and without; the partition variants and the one for the optional specular modes would spill 80 - 200 bytes
   // per lane, the radiance kernel gains nothing): constant corner bits, no loop branch, the x-twin's terms at hand.
   constexpr int CORNER_UNROLL = ((PART & MDH_PF_PART) || SPEC != 1 || QVIS) ? 1 : MDH_CORNER_UNROLL;
   constexpr int PARK_MAT = MODE == 2 ? MDH_PARK_MAT_DIRECT : (REC == 2 && SPEC == 0) ? MDH_PARK_MAT_REPLAY : MDH_PARK_MAT; // (no probe rows in mode 2: MDH_DIRECT_PARK_ROWS)
   // the irradiance tap of a cage corner issued before its visibility march (its loads land during the march) -- not in the
   // space-partition variants, whose march needs the registers
   constexpr bool TAP_EARLY = !(PART & MDH_PF_PART);
   // the x-twin's probe term kept for the corner behind it (item 6 of "Exact work elimination") -- not in the space-partition
   // variants, where its four registers across the visibility march are scratch memory
   constexpr bool TWIN_PREV = MDH_TWIN_PREV != 0 && !(PART & MDH_PF_PART);
   // the first point's eight irradiance taps fetched once per wavefront where its lanes share them (item 15 of "Exact work
   // elimination", at the corner loop below): the screen family's fixed mode over the built-in scans only -- every other
   // instantiation is the code it was
   constexpr bool SHARE_TAPS = MDH_SHARE_TAPS != 0 && (SHARET & 3) && SPEC == 1 && !QVIS && MODE == 0 && TAP_EARLY && (PART & ~(MDH_PF_ROOM | MDH_PF_POW2)) == 0;
   // ... and in such a wavefront (item 16) a corner folded along y or z takes the weight and the visibility bit of the corner it
   // folds onto, kept in four registers
   constexpr bool TWIN_FOLDED = MDH_TWIN_FOLDED != 0 && (SHARET & 3) == 2 && SHARE_TAPS && CORNER_UNROLL == 8;
   // the second point's best cage probe searched by decreasing d = dot(probe_to_spec, -N) instead of corner by corner (item 17 of
   // "Exact work elimination", in front of the corner loop below): the screen family's fixed mode over the built-in scans,
   // marching and recording -- every other instantiation is the code it was
   constexpr bool BEST_FIRST = MDH_BEST_FIRST != 0 && (SHARET & 4) != 0 && MDH_SHARE_FIRST_STEP != 0 && MDH_REUSE_FOLDED != 0 && SPEC == 1 && !QVIS && MODE == 0 &&
                               (PART & ~(MDH_PF_ROOM | MDH_PF_POW2)) == 0 && REC != 2;
   // ... its first round ranked by approximate values, the exact direction formed for the winner alone (item 20, best_approx above)
   constexpr bool BEST_APPROX = MDH_BEST_APPROX != 0 && BEST_FIRST;
   // the sphere's and the box's distance bounded once per ray in front of the primary and the reflection march (item 19 of "Exact
   // work elimination", at march_plain): the screen family's fixed mode over the rooms' census, marching and recording
   constexpr bool RAY_BOUNDS = MDH_RAY_BOUNDS != 0 && (SHARET & 8) != 0 && SPEC == 1 && !QVIS && MODE == 0 && !POINT && REC != 2 && (PART & ~MDH_PF_POW2) == MDH_PF_ROOM;
   // the space-partition variants of the screen pass: the shaded point and its normal come back from park rows behind every
   // corner's visibility march (the second point's wait in the rows of its colour and in three rows of their own) and the probe's grid position is derived again there:
   // the lookups of that march need the registers -- kept live across it, these values went to scratch memory eight times per
   // shaded point (300 MB of spill stores per 1080p launch at six wavefronts per SIMD)
   constexpr bool PARK_VD = (PART & MDH_PF_PART) != 0 && SPEC == 1 && MODE == 0 && CORNER_UNROLL == 1;
   // the second point goes through the whole of pixel_color_probes' lighting (compute_indirect_specular) ...
   const bool full2 = SPEC == 2 && cfg.spec_mode == 3;
   // ... or is only a position that the cage probes of the FIRST point light (sample_radiance_with_specular)
   const bool cage1 = SPEC == 2 && cfg.spec_mode == 1;
   const int u8_tab = sc.u8_slot * 4;
   float *pk = park_base(sc);
   const int wb = park_wave_base(pk);
   hit = false;
   ph.index = -1; ph.t = 0.0f; ph.steps = 0;
   // (the reflection's colour and the primary hit's material id wait in LDS for the combine, like P, N and the light;
   //  the colour's rows are cleared behind the first point's corner loop, which uses them meanwhile)
   bool shaded = false; // the primary ray hit and the full shading ran
   // the ray that finds the next point to shade
   f3 ro = from, rd = dir_in;
   bool active = lane_valid;
   park_store3<6>(pk, wb, dir_in);
   if (SREC && REC == 1) park_store1<MDH_PARK_REC2 + 4>(pk, wb, __int_as_float(0)); // (no reflection ray so far)
#pragma unroll 1
   for (int ctx = 0; ctx < (REFLECT ? 2 : 1); ++ctx) {
      if (active) {
         float t;
         int steps;
         PH_T0(pt);
         bool h;
         if (REC == 2) { // the march's three results as recorded
            const RayRecord &q = (SREC && ctx) ? rec2 : rec;
            h = (q.word >> 31) != 0u;
            t = __int_as_float((int)q.t);
            steps = (int)(q.word & MDH_REC_STEPS_MASK); // (the second point's are read by nobody)
         } else if (POINT && ctx == 0) { // the caller's point: nothing to march
            h = true;
            t = 0.0f;
            steps = 0;
         } else
         h = march_plain<PART, RAY_BOUNDS>(sc, ro, rd, sc.max_dist, t, steps);
         if (REC == 1 && !(SREC && ctx)) park_store1<MDH_PARK_REC + 4>(pk, wb, __int_as_float(steps)); // (hit or miss: the sort key needs them)
         if (REC == 1 && SREC && ctx) park_store1<MDH_PARK_REC2 + 4>(pk, wb, __int_as_float(h ? 3 : 1)); // traced, and hit
         PH_ADD(pt, 0);
         if (ctx == 0) { hit = h; ph.steps = steps; }
         active = false; // a miss ends the chain (ctx 1: specular_col stays 0, render_probes.glsl:142-144)
         if (SPEC == 2 && ctx == 1 && full2 && !h) { // ... or is the sky seen along the reflection, render_probes.glsl:216-218
            const float s = rd.y * 0.7f;
            park_store3<MDH_PARK_SPEC>(pk, wb, F3(0.30f - s, 0.36f - s, 0.60f - s));
         }
         if (SPEC == 2 && ctx == 1 && cage1) {
            if (h) park_store3<MDH_PARK_SPEC>(pk, wb, radiance_with_specular<PART>(sc, pr, pk, wb, ro + rd * t, u8_tab));
         } else
         if (h) {
            f3 P = (POINT && ctx == 0) ? ro : ro + rd * t; // (the caller's point as given: its bits, a negative zero included)
            int index = -1;
            f3 N;
            int pm;
            MDH_WORK(3);
            if (POINT && ctx == 0) { N = pt_normal; pm = pt_material; } // (as given too; ph.index stays -1)
            else {
            if (REC == 2) index = (SREC && ctx) ? (int)(rec2.word & MDH_REC2_INDEX_MASK) - 1 : rec.index;
            else
            (void)sdf_info<PART>(sc, P, index);
            primitive_info<(PART & MDH_PF_CUSTOM) != 0, (PART & MDH_PF_GTAB) != 0>(sc, index, P, N, pm);
            }
            if (ctx == 0) {
               park_store1<PARK_MAT>(pk, wb, __int_as_float(pm));
               ph.index = index; ph.t = t;
               park_store3<0>(pk, wb, P);
               park_store3<3>(pk, wb, N);
            } else if (PARK_VD) { // (the second point's P in the rows of its colour -- written behind its corner loop -- and its N in rows of their own)
               park_store3<MDH_PARK_SPEC>(pk, wb, P);
               park_store3<MDH_PARK_VD_ROW>(pk, wb, N);
            }
            PH_ADD(pt, 1);
            if (MODE != 1) {
               const f3 from_off = P + (N * MDH_MIN_STEP) * 5.0f;
               // Every shadow and probe-visibility ray of this point starts AT from_off with t = 0, so
               // their first SDF evaluation is at the same position (from_off + dir * 0): it is done
               // once here and each ray replays its first iteration with this value.
               const float sd0 = REC == 2 ? __int_as_float((int)((SREC && ctx) ? rec2.sd0 : rec.sd0)) : MDH_SHARE_FIRST_STEP ? sdf<PART>(sc, from_off) : 0.0f;
               if (REC == 1) { // (t and the arg-min are dead from here on, the first step behind the queue: nothing more stays live for the record)
                  if (SREC && ctx) park_store3<MDH_PARK_REC2>(pk, wb, F3(t, __int_as_float(index), sd0));
                  else
                  park_store3<MDH_PARK_REC>(pk, wb, F3(t, __int_as_float(index), sd0));
               }
               // ---- compute_direct_lighting (lighting.glsl:1-40) at P, seen along rd
               f3 Lo = F3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
               for (int li = 0; li < sc.total_lights; ++li) {
                  // (the material is read again for every light, through an id the compiler cannot look through: read
                  //  once in front of the loop, what the BRDF derives from it -- F0, 1 - F0, k -- is hoisted and then
                  //  lives across the shadow march: eight dwords of scratch memory per ray in the seven-wavefront builds)
                  int pm_l = pm;
                  asm volatile("" : "+v"(pm_l));
                  Material m = get_material(sc, pm_l);
                  if (ctx && !full2) m.albedo = F3(0.0f, 0.0f, 0.0f); // render_probes.glsl:202-205
                  f3 L;
                  float L_dist;
                  f3 radiance = sample_light<(PART & MDH_PF_CUSTOM) != 0>(sc, li, P, N, L, L_dist);
                  float NdotL = max_(dot(N, L), 0.0f);
                  // a light that is dark here (outside a spot's cone) or behind the surface adds exactly nothing whatever the BRDF
                  // says, as long as the BRDF is finite (null_light, mdh_device.h): no BRDF, no shadow ray, and +0 in contrib's
                  // place -- Lo + (+0) * 0 has Lo's bits
                  f3 contrib = F3(0.0f, 0.0f, 0.0f);
                  if (!(NULL_BRDF && null_light(-rd, L, NdotL, radiance, m))) {
                     f3 kD, kS;
                     cook_torrance(N, -rd, L, NdotL, m.albedo, m.metallic, m.roughness, kD, kS);
                     if (ctx == 0 && !cfg.direct_specular) kS = F3(0.0f, 0.0f, 0.0f);
                     contrib = ((sdiv3(kD * m.albedo, MDH_PI) + kS) * radiance) * NdotL;
                  }
                  float shadows = 0.0f;
                  PH_ADD(pt, 2);
                  // a light that contributes exactly nothing here (outside a spot's cone, black BRDF)
                  // needs no shadow ray: Lo + (+-0) * shadows = Lo for every shadows in [0, 1]
                  const bool lit = MDH_SKIP_NULL_RAYS ? (contrib.x != 0.0f || contrib.y != 0.0f || contrib.z != 0.0f) : true;
                  if (NdotL > MDH_EPS && lit) { // softshadows, raymarching.glsl:4-23
                     float res = 1.0f, prev = 1e20f, total = 0.0f;
                     bool blocked = false;
                     bool first = MDH_SHARE_FIRST_STEP != 0;
                     MDH_WORK(0);
                     while (total < L_dist) {
                        MDH_DIAG_STEP(1 + ctx);
                        MDH_WORK(1);
                        if (SPEC == 0) ph.steps += 1 << 16; // (the radiance pass's sort key: shadow steps above the primary ones)
                        float dist = first ? sd0 : sdf<PART>(sc, from_off + L * total);
                        first = false;
                        if (dist < MDH_EPS) { blocked = true; break; }
                        float y = dist * dist / (2.0f * prev);
                        float d = sqrt_(dist * dist - y * y);
                        res = min_raw(res, 64.0f * d / max_(0.0f, total - y));
                        prev = dist;
                        total += dist;
                     }
                     shadows = blocked ? 0.0f : res;
                  }
                  Lo = Lo + contrib * shadows;
                  PH_ADD(pt, 3);
               }
               if (ctx == 0) park_store3<9>(pk, wb, Lo); // = direct
               f3 specular_col = Lo;                      // ctx 1: + the radiance tap below (render_probes.glsl:197-206)
               if (MODE == 2) {
                  shaded = true;
               } else {
                  // ---- the 8 cage probes of P (render_probes.glsl:13-63 and :156-184)
                  const KProbes pg = probes_fresh(pr);
                  i3 gp = world_to_grid(pg, P);
                  // sample_irradiance at this point (the first point; the second one in mode 3), or the best cage probe of the second
                  const bool irrp = ctx == 0 || full2;
                  // irrp: acc = sum sqrt(irradiance) * w, accw = sum w; else: acc = best probe_to_spec, accw = best weight
                  f3 acc = irrp ? F3(0.0f, 0.0f, 0.0f) : F3(0.0f, 0.0f, 1.0f);
                  float accw = irrp ? 0.0f : -2.0f;
                  int best_q = 0; // x | y << 10 | z << 20
                  // Cage corners that the clamp to the grid folds onto an earlier corner (P outside the
                  // probe grid along an axis: all six walls of the example rooms are) name the SAME probe,
                  // hence the same visibility ray: its result is reused instead of marched again.
                  // bit a of `folded`: corners differing only in axis a coincide.
                  int folded = ((gp.x < 0 || gp.x >= pg.gx - 1) ? 1 : 0) | ((gp.y < 0 || gp.y >= pg.gy - 1) ? 2 : 0) |
                               ((gp.z < 0 || gp.z >= pg.gz - 1) ? 4 : 0);
                  int vis_bits = 0; // bit i: visibility of corner i
                  PH_ADD(pt, 2);
                  if (REC == 2) vis_bits = (int)((((SREC && ctx) ? rec2.word : rec.word) >> 23) & 255u); // (P, N, the cage cell and its folds are still in registers)
                  else
                  if (QVIS && ctx == 0) {
                     vis_bits = queued_visibility<PART>(sc, pr, pk, P, N, gp, folded, sd0);
                     if (REC == 1) park_store1<MDH_PARK_REC + 3>(pk, wb, __int_as_float(vis_bits));
                     // Nothing of the point stays in registers across the queue (it is the pass's longest loop, and the
                     // kernel is built for seven wavefronts per SIMD: what stayed live -- P, N, the cage cell, twenty dwords
                     // -- went to scratch and back, 45 MB per launch at BASELINE config 3).  P and N wait in their park rows,
                     // where the queue itself reads them; the cage cell and its folds are derived again: the same operations
                     // on the same values.
                     P = park_load3<0>(pk, wb);
                     N = park_load3<3>(pk, wb);
                     const KProbes pg2 = probes_fresh(pr);
                     gp = world_to_grid(pg2, P);
                     folded = ((gp.x < 0 || gp.x >= pg2.gx - 1) ? 1 : 0) | ((gp.y < 0 || gp.y >= pg2.gy - 1) ? 2 : 0) | ((gp.z < 0 || gp.z >= pg2.gz - 1) ? 4 : 0);
                  }
                  PH_ADD(pt, 5);
                  // (Reusing the whole irradiance term of a folded corner's twin through a small register ring was
                  // measured: the 16 extra VGPRs cost what the taps saved -- DESIGN.md, dropped experiments.)
                  // what does not depend on the corner, once (the compiler can no longer hoist it by itself: inside the loop the
                  // probe parameters are read afresh per corner): the position inside the cage and the clamped octahedral
                  // texel of N
                  f3 alpha = F3(0.0f, 0.0f, 0.0f);
                  f2 rid_n = F2(0.0f, 0.0f);
                  const bool parked = REFLECT && ctx == 0; // (the rows are free then: see MDH_PARK_ALPHA)
                  if (irrp) {
                     alpha = P / F3(pg.sx, pg.sy, pg.sz) - F3((float)gp.x, (float)gp.y, (float)gp.z);
                     rid_n = ray_dir_to_ray_id(N);
                     rid_n = F2(clamp_(rid_n.x, pg.irr_lo, pg.irr_hi), clamp_(rid_n.y, pg.irr_lo, pg.irr_hi));
                     if (parked) { // five registers less through the visibility marches
                        park_store3<MDH_PARK_ALPHA>(pk, wb, alpha);
                        park_store1<MDH_PARK_RIDN>(pk, wb, rid_n.x);
                        park_store1<MDH_PARK_RIDN + 1>(pk, wb, rid_n.y);
                     }
                  }
                  // The irradiance tap of corner i reads the atlas at a place that the probe -- cage_probe (pq, gp, i) -- and the
                  // clamped texel of N decide, and nothing else of the point does.  An 8x8 tile on a wall, the floor or a box
                  // face has one N, bit for bit, and mostly one cage cell: its 64 lanes would compute the same eight taps.  Where
                  // every lane here holds the first one's gp and the first one's bits of N (-0 is not +0; a NaN is itself), the
                  // wavefront computes them in ONE pass, the lane of rank r among the active ones taking corner r & 7, and every
                  // corner reads its triple from the wavefront's row.  No bit changes: every input of corner i's tap is equal in
                  // all lanes by that test, rid_n included (a function of N and the probe parameters); the statements are the
                  // loop's own, in its order, nothing contracted; a value does not depend on the lane that computes it; and the
                  // sum acc + s_term * weight keeps its order i = 0 .. 7 and its per-lane weights.  A corner folded onto an
                  // earlier one names that one's probe (the clamp of cage_probe), so its slot holds that probe's value.
                  bool shared = false;
                  if (SHARE_TAPS && ctx == 0) {
                     const unsigned long long act = __ballot(true);
                     const int nx = __float_as_int(N.x), ny = __float_as_int(N.y), nz = __float_as_int(N.z);
                     const bool same = gp.x == __builtin_amdgcn_readfirstlane(gp.x) && gp.y == __builtin_amdgcn_readfirstlane(gp.y) &&
                                       gp.z == __builtin_amdgcn_readfirstlane(gp.z) && nx == __builtin_amdgcn_readfirstlane(nx) &&
                                       ny == __builtin_amdgcn_readfirstlane(ny) && nz == __builtin_amdgcn_readfirstlane(nz);
                     shared = __popcll(act) >= 8 && __ballot(same) == act;
                     if (shared) {
                        MDH_COUNT_SHARED_TAPS();
                        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(act >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)act, 0u));
                        const int c = rank & 7;
                        const KProbes pq = probes_fresh(pr);
                        const i3 q = cage_probe(pq, gp, c);
                        const f2 base = probe_id_to_coord<P2>(pq, grid_to_probe_id<P2>(pq, q));
                        const AtlasTap tap = atlas_tap_issue<P2>(pq.irr, pq.fmt, pq.pcx, pq.pcy, pq.ires, pq.ishift, pq.irr_w, pq.irr_h, base.x + div_pcx<P2>(pq, rid_n.x), base.y + div_pcy<P2>(pq, rid_n.y), pq.m_ires);
                        const f3 tx = atlas_tap_resolve(pq.irr, pq.fmt, tap, u8_tab);
                        f3 s;
                        if (pq.fmt == 0 && !MDH_HYBRID_NUMERICS) s = F3(sqrt_unscaled_(tx.x), sqrt_unscaled_(tx.y), sqrt_unscaled_(tx.z));
                        else
                        s = ssqrt3(tx);
                        if (rank < 8) {
                           const ParkLds slot = (ParkLds)(unsigned)(wb + (MDH_PARK_TAPS * MDH_BLOCK + 3 * c) * 4);
                           slot[0] = s.x; slot[1] = s.y; slot[2] = s.z;
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                     }
                  }
                  // A corner folded onto its twin along x follows it directly (i - 1): the twin's probe term -- direction,
                  // visibility, weight before the trilinear factor, irradiance tap -- is this corner's, value for value,
                  // and is still in registers.  (Twins along y and z are two and four corners back: below.)
                  f3 s_keep = F3(0.0f, 0.0f, 0.0f);
                  float w_keep = 0.0f;
                  // A corner folded onto its twin along y or z (two and four corners back) in a SHARING wavefront: the irradiance
                  // tap is in the wavefront's row whichever corner asks, so the twin's term is one float -- its weight before the
                  // trilinear factor -- and its visibility bit.  Corner i keeps its weight in w_fold[i & 3]; the twin b = i & ~folds
                  // of a later corner is found in w_fold[b & 3] (a corner between them with the same index modulo 4 is b | 4: a twin
                  // of b itself, with b's weight).  The cell is the wavefront's, so its folds are one scalar: no lane diverges.
                  // Folds along two or three axes take the same path: b clears every folded bit of y and z, and a corner that
                  // also folds along x holds what the x-twin in front of it left (twin_prev), which is b's value again.
                  float w_fold[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                  const int folds = (TWIN_FOLDED && shared) ? (__builtin_amdgcn_readfirstlane(folded) & 6) : 0;
                  // The second point's loop names ONE probe: the first corner in index order that attains the maximum of W_i, where
                  // W_i = d_i = dot(probe_to_spec_i, -N) if corner i is visible and d_i * 0 otherwise (MDH_SKIP_NULL_RAYS rests on
                  // the same reading).  In index order a wavefront runs a corner's clearance test while ANY of its lanes can still
                  // win there.  Here every lane takes its untried corner of largest d > 0 (the lowest index among equals) per round
                  // -- a scan with the loop's own statements in the loop's order, nothing contracted, no test and no march -- and
                  // sends that one ray through the immediate outcomes, segment_clear and the march.  A visible candidate c is the
                  // loop's probe: every corner of larger d was tried before it and is blocked, W = +0 < d_c; every corner of equal d
                  // and lower index likewise; every other W_j <= d_j <= d_c, and an equal one has a higher index, so it is not
                  // strictly larger; a NaN wins in neither form.  Only best_q and acc leave the loop, and they are c's: the same
                  // operations on the same values.  A lane that runs out of candidates of positive d without a visible one (all
                  // blocked, none in front, a NaN) takes the in-order loop below from corner 0 as it is; the lanes that hold a
                  // winner sit it out.  The record (REC 1) of a winner: 1 for the winner and for every untried corner (a skipped
                  // corner's value), 0 for a tried and blocked one.  The replaying kernel's in-order loop over these bits sees
                  // W'_c = d_c, +0 at the tried corners, and d_j at the untried ones, which are <= d_c and above index c where equal
                  // (or not positive, or NaN): it names c.  A fallback lane's record is the loop's own.
                  bool in_order = true;
                  // (the second point's direct light waits in the rows of its colour, where it goes anyway, from here to the radiance
                  //  tap below: three registers that the ranking's terms take)
                  if (BEST_APPROX && ctx == 1) park_store3<MDH_PARK_SPEC>(pk, wb, specular_col);
                  if (BEST_FIRST && ctx == 1) {
                     int tried = 0; // bit i: corner i was a candidate and is blocked
                     bool searching = true;
                     in_order = false;
                     // the candidate of the round; a winner's stays as it is (a lane that is not searching scans nothing)
                     float bvmax = 0.0f;
                     f3 bvd = F3(0.0f, 0.0f, 0.0f);
                     int bi = -1, bq = 0;
                     bool round0 = true;
#pragma unroll 1
                     for (;;) {
                        if (searching) {
                           float bd = 0.0f;
                           bi = -1;
                           // The first round ranks the corners by best_approx's a_i where that decides in every searching lane of
                           // the wavefront: a winner runs the scan's statements once, for its corner (the same operations on the
                           // same values: bvd, bvmax and bq are the scan's; d is read by nobody), a lane without a candidate goes
                           // to the in-order loop as the scan would send it.  One undecided lane, and the wavefront scans as it
                           // did (the scan costs a wavefront the same whether one lane or all run it).  Later rounds always scan.
                           bool scan = true;
                           if (BEST_APPROX && round0) {
                              int wi;
                              const int state = best_approx(pr, gp, folded, P, N, wi);
                              scan = __ballot(state == 0) != 0ull;
                              MDH_BEST_APPROX_STAT(0, __popcll(__ballot(state == 1)));
                              MDH_BEST_APPROX_STAT(1, __popcll(__ballot(state == 2)));
                              MDH_BEST_APPROX_STAT(2, __popcll(__ballot(state == 0)));
                              if (scan) MDH_BEST_APPROX_STAT(3, 1);
                              if (!scan && state == 1) {
                                 bi = wi;
                                 const KProbes pq = probes_fresh(pr);
                                 const i3 q = cage_probe(pq, gp, bi);
                                 const f3 pw = grid_to_world(pq, q);
                                 const f3 hvec = P - pw;
                                 const float dist = length(hvec);
                                 f3 vd = sdiv3(hvec, dist);
                                 vd = -vd;
                                 bvd = vd; bvmax = dist - MDH_MIN_STEP * 5.0f; bq = q.x | (q.y << 10) | (q.z << 20);
                              }
                           }
                           if (scan)
#pragma unroll 1
                           for (int i = 0; i < 8; ++i) {
                              if ((i & folded) || ((tried >> i) & 1)) continue;
                              const KProbes pq = probes_fresh(pr);
                              const i3 q = cage_probe(pq, gp, i);
                              const f3 pw = grid_to_world(pq, q);
                              const f3 hvec = P - pw;
                              const float dist = length(hvec);
                              f3 vd = sdiv3(hvec, dist);
                              vd = -vd;
                              const float d = dot(-vd, -N);
                              if (d > bd) { bd = d; bi = i; bvd = vd; bvmax = dist - MDH_MIN_STEP * 5.0f; bq = q.x | (q.y << 10) | (q.z << 20); }
                           }
                           if (bi < 0) { in_order = true; searching = false; }
                        }
                        round0 = false;
                        if (!__ballot(searching)) break;
                        MDH_BEST_STAT(0, 1);
                        // raycast_visibility of the candidate, as the loop runs it (a lane that is not searching has no ray: vmax 0)
                        float vis = 1.0f, total = 0.0f;
                        float vmax = searching ? bvmax : 0.0f;
                        if (0.0f < vmax && !(sd0 < MDH_EPS) && sd0 < vmax)
                           if (segment_clear<PART>(sc, from_off, bvd, vmax)) vmax = 0.0f;
                        bool first = true;
                        while (total < vmax) {
                           float sd = first ? sd0 : sdf<PART>(sc, from_off + bvd * total);
                           first = false;
                           if (sd < MDH_EPS) { vis = 0.0f; break; }
                           total += sd;
                        }
                        if (searching) {
                           if (vis != 0.0f) searching = false;
                           else tried |= 1 << bi;
                        }
                     }
                     MDH_BEST_STAT(1, __popcll(__ballot(!in_order)));
                     if (!in_order) { best_q = bq; acc = -bvd; } // (accw, the winner's d, is read by nobody behind the loop)
                     if (SREC && REC == 1 && !in_order) {
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                           if (!(i & folded) && !((tried >> i) & 1)) vis_bits |= 1 << i;
                     }
                     if (__ballot(in_order)) { MDH_BEST_STAT(2, 1); MDH_BEST_STAT(3, __popcll(__ballot(in_order))); }
                  }
                  if (in_order)
#pragma unroll CORNER_UNROLL
                  for (int i = 0; i < 8; ++i) {
                     // best probe: a folded corner has the weight of its twin, which is not strictly larger
                     if (MDH_REUSE_FOLDED && !irrp && (i & folded)) continue;
                     KProbes pq = probes_fresh(pr); // (live up to the visibility march, read again behind it)
                     f3 s_term = F3(0.0f, 0.0f, 0.0f); // sqrt(irradiance tap) of this corner's probe
                     float wpre = 0.0f;                // its weight before the trilinear factor
                     const i3 q = cage_probe(pq, gp, i);
                     const bool twin_prev = TWIN_PREV && irrp && (i & 1) && (folded & 1);
                     if (TWIN_FOLDED && (i & folds)) {
                        const ParkLds slot = (ParkLds)(unsigned)(wb + (MDH_PARK_TAPS * MDH_BLOCK + 3 * i) * 4); // (the twin's probe: the same triple)
                        s_term = F3(slot[0], slot[1], slot[2]);
                        wpre = (folds & 2) ? w_fold[i & 1] : w_fold[i & 3];
                        vis_bits |= ((vis_bits >> (i & ~folds)) & 1) << i;
                        if (!twin_prev) MDH_WORK(0); // (the folded corner's ray, which never took a step, counted as before; an x-twin's never was)
                     } else
                     if (twin_prev) {
                        s_term = s_keep;
                        wpre = w_keep;
                        vis_bits |= ((vis_bits >> (i - 1)) & 1) << i;
                     } else {
                     const f3 pw = grid_to_world(pq, q);
                     const f3 hvec = irrp ? (pw - P) : (P - pw);
                     const float dist = length(hvec);
                     f3 vd = sdiv3(hvec, dist); // irrp: dir_to_probe, else: probe_to_spec
                     if (!irrp) vd = -vd; // the visibility ray always runs from the point to the probe
                     // the irradiance tap of this corner (render_probes.glsl:44-58) depends on the probe and
                     // N only: its texel loads go out now and land while the visibility ray is marched
                     AtlasTap tap;
                     if (TAP_EARLY && irrp && !(SHARE_TAPS && shared)) { // (a sharing wavefront holds no tap across the march)
                        const f2 rid = parked ? park_load2<MDH_PARK_RIDN>(pk, wb) : rid_n;
                        const f2 base = probe_id_to_coord<P2>(pq, grid_to_probe_id<P2>(pq, q));
                        tap = atlas_tap_issue<P2>(pq.irr, pq.fmt, pq.pcx, pq.pcy, pq.ires, pq.ishift, pq.irr_w, pq.irr_h, base.x + div_pcx<P2>(pq, rid.x), base.y + div_pcy<P2>(pq, rid.y), pq.m_ires);
                     }
                     // raycast_visibility, raymarching.glsl:39-56
                     float vis = 1.0f, total = 0.0f;
                     float vmax = dist - MDH_MIN_STEP * 5.0f;
                     if (QVIS && ctx == 0) { // every distinct corner was traced by queued_visibility
                        vis = ((vis_bits >> (i & ~folded)) & 1) ? 1.0f : 0.0f;
                        vmax = 0.0f;
                     }
                     // the screen pass's record holds the loop's own bits: bit i is what `vis` was behind corner i's march (or
                     // behind the decision not to march it: folded, the twin's, no candidate, proved clear, an immediate outcome)
                     if (SREC && REC == 2) {
                        vis = ((vis_bits >> i) & 1) ? 1.0f : 0.0f;
                        vmax = 0.0f;
                     }
#if MDH_REUSE_FOLDED
                     if (i & folded) { // same probe as corner i & ~folded, already traced
                        vis = ((vis_bits >> (i & ~folded)) & 1) ? 1.0f : 0.0f;
                        vmax = 0.0f;
                     }
#endif
#if MDH_SKIP_NULL_RAYS
                     // ctx 1 keeps the probe with the largest dot(probe_to_spec, -N) * vis (strictly larger
                     // than the best so far).  With vis in {0, 1} the candidate is d or d * 0: once the best
                     // is >= 0, a probe with d <= best cannot win whatever its visibility.
                     if (!irrp && accw >= 0.0f && dot(-vd, -N) <= accw) vmax = 0.0f;
#endif
                     // a ray that segment_clear proves unblocked (behind the immediate outcomes: vmax <= 0, sd0 < EPS, sd0 >= vmax)
                     // is not marched: vis stays 1
                     if (!(SREC && REC == 2))
                     if (0.0f < vmax && (!MDH_SHARE_FIRST_STEP || (!(sd0 < MDH_EPS) && sd0 < vmax)))
                        if (segment_clear<PART>(sc, from_off, vd, vmax)) vmax = 0.0f;
                     bool first = MDH_SHARE_FIRST_STEP != 0;
                     PH_ADD(pt, 4);
                     if (!(QVIS && !REFLECT)) // (with the queue and no second point this loop is dead code)
                     MDH_WORK(0);
                     if (!(QVIS && !REFLECT) && !(SREC && REC == 2))
                     while (total < vmax) {
                        MDH_DIAG_STEP(3 + ctx);
                        MDH_WORK(1);
                        float sd = first ? sd0 : sdf<PART>(sc, from_off + vd * total);
                        first = false;
                        if (sd < MDH_EPS) { vis = 0.0f; break; }
                        total += sd;
                     }
                     vis_bits |= (vis != 0.0f ? 1 : 0) << i;
                     pq = probes_fresh(pr);
                     i3 q2 = q;
                     if (PARK_VD) { // the point again, from its park rows (nothing in the march reads P or N: they need not live through it)
                        if (ctx == 0) { P = park_load3<0>(pk, wb); N = park_load3<3>(pk, wb); }
                        else { P = park_load3<MDH_PARK_SPEC>(pk, wb); N = park_load3<MDH_PARK_VD_ROW>(pk, wb); }
                        q2 = cage_probe(pq, gp, i); // (the same clamps of the same cell: the same probe)
                     }
                     PH_ADD(pt, 5);
                     if (irrp) { // render_probes.glsl:26-62
                        float angle = (dot(vd, N) + 1.0f) * 0.5f;
                        float weight = angle * angle + 0.2f;
                        weight *= vis;
                        const float crush = 0.2f;
                        if (weight < crush) weight *= weight * weight * (1.0f / (crush * crush));
                        wpre = weight;
                        if (SHARE_TAPS && shared) { // the wavefront's value of corner i: one address for all lanes, a broadcast read
                           const ParkLds slot = (ParkLds)(unsigned)(wb + (MDH_PARK_TAPS * MDH_BLOCK + 3 * i) * 4); // (from the scalar that is live anyway)
                           s_term = F3(slot[0], slot[1], slot[2]);
                        } else {
                        f3 tx;
                        if (TAP_EARLY) tx = atlas_tap_resolve(pq.irr, pq.fmt, tap, u8_tab);
                        else { // (the space-partition variants: the tap's eight registers do not live across the visibility march)
                           const f2 rid = parked ? park_load2<MDH_PARK_RIDN>(pk, wb) : rid_n;
                           const f2 base = probe_id_to_coord<P2>(pq, grid_to_probe_id<P2>(pq, q2));
                           tx = atlas_sample<P2>(pq.irr, pq.fmt, pq.pcx, pq.pcy, pq.ires, pq.ishift, pq.irr_w, pq.irr_h, base.x + div_pcx<P2>(pq, rid.x), base.y + div_pcy<P2>(pq, rid.y), u8_tab, pq.m_ires);
                        }
                        // A bilinear tap of an RGBA8 atlas is 0 or at least 2^-56: its texels are k / 255, its weights products of
                        // two factors from {0} and [2^-24, 1] (fx = px - floor (px) with px = cx W - 0.5 a multiple of 2^-24 below 1 --
                        // the subtraction is exact there -- and of ulp (px) above; 1 - fx likewise), its terms are not negative.  No
                        // rescaling can apply: the square root's nine-instruction core, 7 instructions less x 3 channels x 8 corners.
                        if (pq.fmt == 0 && !MDH_HYBRID_NUMERICS) s_term = F3(sqrt_unscaled_(tx.x), sqrt_unscaled_(tx.y), sqrt_unscaled_(tx.z));
                        else
                        s_term = ssqrt3(tx);
                        }
                     } else { // render_probes.glsl:170-183; probe_to_spec = -vd
                        float weight = dot(-vd, -N);
                        weight *= vis;
                        if (weight > accw) { accw = weight; best_q = q2.x | (q2.y << 10) | (q2.z << 20); acc = -vd; }
                     }
                     }
                     if (irrp) { // render_probes.glsl:34-62: the trilinear factor and the sum
                        float weight = wpre;
                        if (parked) alpha = park_load3<MDH_PARK_ALPHA>(pk, wb);
                        f3 tri = F3(mix_(1.0f - alpha.x, alpha.x, (float)(i & 1)), mix_(1.0f - alpha.y, alpha.y, (float)((i >> 1) & 1)),
                                    mix_(1.0f - alpha.z, alpha.z, (float)((i >> 2) & 1)));
                        weight *= tri.x * tri.y * tri.z;
                        acc = acc + s_term * weight;
                        accw += weight;
                        if (TWIN_PREV) { s_keep = s_term; w_keep = wpre; }
                        if (TWIN_FOLDED) w_fold[i & 3] = wpre;
                     }
                     PH_ADD(pt, 6);
                  }
                  if (SREC && REC == 1) { // the loop's eight bits
                     if (ctx) park_store1<MDH_PARK_REC2 + 3>(pk, wb, __int_as_float(vis_bits));
                     else park_store1<MDH_PARK_REC + 3>(pk, wb, __int_as_float(vis_bits));
                  }
                  if (SPEC == 2 && ctx == 1 && full2) { // render_probes.glsl:233-243: indirect (no specular of its own) + direct
                     f3 irr = F3(0.0f, 0.0f, 0.0f);
                     if (accw != 0.0f) { irr = sdiv3(acc, accw); irr = irr * irr; }
                     const Material m = get_material(sc, pm);
                     specular_col = compute_indirect_lighting(irr, F3(0.0f, 0.0f, 0.0f), -rd, N, reflect(rd, N), m.albedo, m.metallic, m.roughness) + specular_col;
                     park_store3<MDH_PARK_SPEC>(pk, wb, specular_col);
                  } else
                  if (ctx == 0) {
                     // render_probes.glsl:65-66 (0/0 fixed as 0)
                     f3 irr = F3(0.0f, 0.0f, 0.0f);
                     if (accw != 0.0f) { irr = sdiv3(acc, accw); irr = irr * irr; }
                     park_store3<12>(pk, wb, irr);
                     if (REFLECT) park_store3<MDH_PARK_SPEC>(pk, wb, F3(0.0f, 0.0f, 0.0f));
                     shaded = true;
                     // the reflection ray of render_probes.glsl:262-275 finds the next point
                     // (the material id comes back from its park slot: kept in a register across the corner loop it is spilled)
                     active = cfg.spec_mode != 0 && tab_float((sc.mat_slot + 2 * __float_as_int(park_load1<PARK_MAT>(pk, wb)) + 1) * 4) < 0.75f;
                     if (SREC && REC == 2) active = active && (rec2.word & MDH_REC2_TRACED) != 0u; // (the same bit: ScrRecKey holds what decides it)
                     ro = from_off;
                     rd = reflect(rd, N);
                  } else { // render_probes.glsl:186-208
                     i3 bq;
                     bq.x = best_q & 1023; bq.y = (best_q >> 10) & 1023; bq.z = (best_q >> 20) & 1023;
                     const KProbes pq = probes_fresh(pr);
                     f2 base = probe_id_to_coord<P2>(pq, grid_to_probe_id<P2>(pq, bq));
                     f2 brid = ray_dir_to_ray_id(acc);
                     brid = F2(clamp_(brid.x, pq.rad_lo, pq.rad_hi), clamp_(brid.y, pq.rad_lo, pq.rad_hi));
                     f3 radiance = (SPEC == 2 && pq.rad_mips) // (MDH_OPT_RADIANCE_MIPS, in the kernel variant of the optional paths only: textureLod (.., 1.0))
                        ? radiance_lod_sample(pq, 1.0f, base.x + div_pcx<P2>(pq, brid.x), base.y + div_pcy<P2>(pq, brid.y), u8_tab)
                        : atlas_sample<P2>(pq.rad, pq.fmt, pq.pcx, pq.pcy, pq.rres, pq.rshift, pq.rad_w, pq.rad_h, base.x + div_pcx<P2>(pq, brid.x), base.y + div_pcy<P2>(pq, brid.y), u8_tab, pq.m_rres);
                     if (BEST_APPROX) specular_col = park_load3<MDH_PARK_SPEC>(pk, wb);
                     specular_col = radiance + specular_col;
                     park_store3<MDH_PARK_SPEC>(pk, wb, specular_col);
                  }
                  PH_ADD(pt, 7);
               }
            }
         }
      }
   }
   // ---- everything parked comes back for the combine
   PH_T0(pc);
   const f3 dir = park_load3<6>(pk, wb);
   f3 result;
   pos_out = F3(0.0f, 0.0f, 0.0f);
   if (!hit) { // render_probes.glsl:287
      float s = dir.y * 0.7f;
      result = F3(0.30f - s, 0.36f - s, 0.60f - s);
      if (!lane_valid) result = F3(0.0f, 0.0f, 0.0f);
   } else {
      const f3 pos = park_load3<0>(pk, wb), normal = park_load3<3>(pk, wb);
      pos_out = pos;
      if (MODE == 1) {
         result = normal * 0.5f + F3s(0.5f);
      } else { // render_probes.glsl:277-285 and lighting.glsl:51-69
         (void)shaded;
         f3 direct = park_load3<9>(pk, wb);
         if (MODE == 0) {
            const f3 irr = park_load3<12>(pk, wb);
            const f3 specular_col = REFLECT ? park_load3<MDH_PARK_SPEC>(pk, wb) : F3(0.0f, 0.0f, 0.0f);
            Material m = get_material(sc, __float_as_int(park_load1<PARK_MAT>(pk, wb)));
            const f3 specular_dir = reflect(dir, normal);
            direct = direct + compute_indirect_lighting(irr, specular_col, -dir, normal, specular_dir, m.albedo, m.metallic, m.roughness);
         }
         float ao = 1.0f;
         if (SREC && REC == 2) { // the term as recorded: its steps read the geometry, pos and normal only
            if (cfg.ao_steps > 0) ao = __int_as_float(rec2.index);
         } else
         if (cfg.ao_steps > 0) {
            float ao_sum = 0.0f, max_ao_sum = 0.0f, factor = 1.0f;
#pragma unroll 1
            for (int i = 0; i < cfg.ao_steps; ++i) {
               f3 p = pos + (normal * (float)(i + 1)) * 0.1f;
               ao_sum += factor * sdf<PART>(sc, p);
               max_ao_sum += factor * (float)(i + 1) * 0.1f;
               factor = factor * 0.5f;
            }
            ao = 0.6f + sdiv(0.4f * ao_sum, max_ao_sum);
            if (SREC && REC == 1) park_store1<MDH_PARK_REC_AO>(pk, wb, ao);
         }
         result = direct * ao;
      }
   }
   PH_ADD(pc, 8);
   return result;
}
