// mdh_host.h -- the owners of what the host side of mdh_api.hip holds on the device: buffers, events, and the two
// orderings it keeps between its streams; and of what it carries from one pass to the next: the settle tracker, the replay
// schedule and the re-sort clock, which make no runtime call at all.  Host only: no device code, nothing of the MDH_* error
// plumbing; every function returns the runtime's own hipError_t and the caller wraps it (HIP_TRY).
//
// An owner that holds nothing makes no runtime call, neither when it is released nor when it is destroyed: a renderer
// that never reached a device is deleted without one (mdh_create).  Owners are members, never copied.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstring>

constexpr int HOST_NSTREAMS = 5; // the streams of a renderer that launch kernels (stream_index, mdh_api.hip)

// Memory and its capacity in elements: on the device, or (Pinned) page-locked on the host.
template <class T = unsigned char, bool Pinned = false>
struct DevBuf {
   T *ptr = nullptr;
   size_t cap = 0;
   DevBuf() = default;
   DevBuf(const DevBuf &) = delete;
   DevBuf &operator=(const DevBuf &) = delete;
   ~DevBuf() { (void)release(); }
   hipError_t release()
   {
      T *q = ptr;
      ptr = nullptr; cap = 0; // (first: whatever the free says, nobody frees q again)
      if (!q) return hipSuccess;
      return Pinned ? hipHostFree(q) : hipFree(q);
   }
   // Room for n elements.  The contents do not survive a growth, and whoever may still use the old memory has to be
   // drained first: that is the caller's.  After a failed allocation the buffer is empty.
   hipError_t grow(size_t n)
   {
      if (n <= cap) return hipSuccess;
      hipError_t e = release();
      if (e != hipSuccess) return e;
      void *q = nullptr;
      e = Pinned ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, n * sizeof(T));
      if (e != hipSuccess) return e;
      ptr = (T *)q; cap = n;
      return hipSuccess;
   }
   // as a member of create_all: the buffer with n elements
   struct Sized {
      DevBuf &b;
      size_t n;
      hipError_t create() { return b.grow(n); }
      void release() { (void)b.release(); }
   };
   Sized sized(size_t n) { return {*this, n}; }
};
template <class T>
using PinnedBuf = DevBuf<T, true>;

// An event that orders streams (no timing).
struct Event {
   hipEvent_t ev = nullptr;
   Event() = default;
   Event(const Event &) = delete;
   Event &operator=(const Event &) = delete;
   ~Event() { release(); }
   hipError_t create()
   {
      if (ev) return hipSuccess;
      hipEvent_t e = nullptr;
      const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
      if (rc == hipSuccess) ev = e;
      return rc;
   }
   void release()
   {
      if (ev) (void)hipEventDestroy(ev);
      ev = nullptr;
   }
};

// Resources that are looked for as one ("is it there?" asks any of them): all created, in order, or, when one creation
// fails, all empty again and that error returned.  Members have create() and release(): Event, Fence, RingUse, QueryBridge,
// DevBuf::sized.
template <class... M>
hipError_t create_all(M &&...m)
{
   hipError_t e = hipSuccess;
   ((e = e == hipSuccess ? m.create() : e), ...);
   if (e != hipSuccess) (m.release(), ...);
   return e;
}

// "What does a query run between?"  A query's kernel runs on the query stream qs, for a caller whose arrays another stream
// may hold, and -- where it reads what the frames write -- at its place among the frames on the main stream.  enter orders qs
// behind the main stream (frame) and behind the caller's stream (in); leave orders both behind the kernel (out).  Without a
// main stream only the caller's half is enqueued, and a caller that is qs itself needs none: no runtime call at all.
// One set of events serves every query: an event is recorded again only after the wait on it was enqueued, and a wait that
// is enqueued keeps the record it saw -- what every repeated call of one family has always relied on.
struct QueryBridge {
   Event frame, in, out;
   hipError_t create() { return create_all(frame, in, out); }
   void release() { frame.release(); in.release(); out.release(); }
   hipError_t enter(hipStream_t qs, hipStream_t caller, const hipStream_t *main)
   {
      hipError_t e = main ? order(frame, *main, qs) : hipSuccess;
      if (e == hipSuccess && caller != qs) e = order(in, caller, qs);
      return e;
   }
   hipError_t leave(hipStream_t qs, hipStream_t caller, const hipStream_t *main)
   {
      if (!main && caller == qs) return hipSuccess;
      hipError_t e = hipEventRecord(out.ev, qs);
      if (e == hipSuccess && main) e = hipStreamWaitEvent(*main, out.ev, 0);
      if (e == hipSuccess && caller != qs) e = hipStreamWaitEvent(caller, out.ev, 0);
      return e;
   }
private:
   static hipError_t order(Event &ev, hipStream_t first, hipStream_t then)
   {
      const hipError_t e = hipEventRecord(ev.ev, first);
      return e == hipSuccess ? hipStreamWaitEvent(then, ev.ev, 0) : e;
   }
};

// "Has this stream seen the latest write?"  The writer signals behind its write; a reader waits before its read, which
// costs a runtime call only on a stream that has not been ordered behind the latest signal yet.
struct Fence {
   Event ev;
   hipStream_t by = nullptr; // the stream of the last signal
   unsigned long long version = 0, seen[HOST_NSTREAMS] = {0};
   hipError_t create() { return ev.create(); }
   void release() { ev.release(); }
   hipError_t signal(hipStream_t st, int si)
   {
      const hipError_t e = hipEventRecord(ev.ev, st);
      if (e != hipSuccess) return e;
      by = st;
      seen[si] = ++version;
      return hipSuccess;
   }
   hipError_t wait(hipStream_t st, int si)
   {
      if (version == 0 || seen[si] == version) return hipSuccess;
      if (st != by) {
         const hipError_t e = hipStreamWaitEvent(st, ev.ev, 0);
         if (e != hipSuccess) return e;
      }
      seen[si] = version;
      return hipSuccess;
   }
   void mark_all_seen() // (the caller has waited on the host for everything signalled so far)
   {
      for (unsigned long long &s : seen) s = version;
   }
};

// "Who still reads this slot?" of a ring of N buffers: every stream that uses a slot marks it behind the use; before the
// slot is rewritten its readers are retired, by a wait on the host or on the stream that rewrites it.
template <int N>
struct RingUse {
   Event done[N][HOST_NSTREAMS];
   bool used[N][HOST_NSTREAMS] = {{false}};
   hipError_t create()
   {
      for (auto &slot : done)
         for (Event &e : slot) {
            const hipError_t rc = e.create();
            if (rc != hipSuccess) { release(); return rc; }
         }
      return hipSuccess;
   }
   void release()
   {
      for (auto &slot : done)
         for (Event &e : slot) e.release();
      forget();
   }
   hipError_t mark(int slot, hipStream_t st, int si)
   {
      const hipError_t e = hipEventRecord(done[slot][si].ev, st);
      if (e == hipSuccess) used[slot][si] = true;
      return e;
   }
   template <class F>
   hipError_t retire(int slot, F wait_for) // wait_for (stream index, its event) for every stream that marked the slot
   {
      for (int si = 0; si < HOST_NSTREAMS; ++si)
         if (used[slot][si]) {
            const hipError_t e = wait_for(si, done[slot][si].ev);
            if (e != hipSuccess) return e;
            used[slot][si] = false;
         }
      return hipSuccess;
   }
   hipError_t retire_on_host(int slot)
   {
      return retire(slot, [](int, hipEvent_t e) { return hipEventSynchronize(e); });
   }
   hipError_t retire_on_stream(int slot, hipStream_t st, int si_st) // (st's own uses are ordered by the stream itself)
   {
      return retire(slot, [&](int si, hipEvent_t e) { return si == si_st ? hipSuccess : hipStreamWaitEvent(st, e, 0); });
   }
   void forget() // (every stream was drained: nothing reads any slot)
   {
      for (auto &slot : used)
         for (bool &u : slot) u = false;
   }
};

// "Have the probe atlases stopped changing?" (MDH_OPT_PROBE_SETTLE; DESIGN.md section 4, "Exact work elimination", item 13).
// Every tracked irradiance pass of a frame reports, through one slot of a small ring in memory the device can write, how many
// texels it stored with other bits than the set it read held.  The tracker numbers the passes, remembers under which version of
// the probe passes' inputs and under which schedule each was enqueued, reads the slots that have arrived -- it never waits --
// and keeps the length of the run of consecutive unchanged passes.  A frame's probe passes may be left out once that run is
// MDH_SETTLE_PASSES long, all of it enqueued under the version and the schedule that still hold.
// No runtime call in here: the slots' memory is the caller's (pinned host memory in the renderer, plain memory in
// tests/settle_check.cpp).
#ifndef MDH_SETTLE_PASSES
#define MDH_SETTLE_PASSES 16 // exactness needs MDH_ATLAS_SETS (every set then holds the same bits); the rest is margin that costs nothing in steady state
#endif
struct alignas(8) SettleSlot { unsigned changed, seq; }; // the device writes both as ONE 64-bit store: changed in the low word, seq in the high one
struct SettleTracker {
   static constexpr int RING = 64; // tracked passes in flight stay below it: a slot is never rewritten before it was read
   SettleSlot *slots = nullptr;    // [RING], zeroed by the caller
   struct Meta { unsigned long long pass, version; int schedule; };
   Meta meta[RING] = {};
   unsigned long long version = 1;                  // of everything a probe pass reads besides the irradiance atlas: bump ()
   unsigned long long issued = 0;                   // irradiance passes of frames enqueued so far, tracked or not: a pass's number
   unsigned long long seq_issued = 0, seq_seen = 0; // tracked passes enqueued / whose slot was read
   unsigned long long floor = 0;                    // passes up to this number count for no run (reset)
   unsigned long long last_pass = 0, run_version = 0;
   int run_schedule = -1;
   long long run = 0;
   unsigned last_changed = 0;                       // texels the newest observed pass changed
   bool enabled = true;
   // the open frame: what frame_begin decided, and the version it decided under
   bool frame_skip = false;
   unsigned long long frame_version = 0;

   static unsigned long long next_seq(unsigned long long s) { return (unsigned)(s + 1) == 0u ? s + 2 : s + 1; } // (a slot's 0 means "nothing yet")
   void bump() { ++version; }
   void reset() { run = 0; floor = issued; }
   void set_enabled(bool on) { if (!on) { reset(); frame_skip = false; } enabled = on; } // (off inside an open frame: its passes run)
   long long current_run() const { return run_version == version ? run : 0; }
   // read the slots that have arrived, oldest first
   void poll()
   {
      while (seq_seen != seq_issued) {
         const unsigned long long s = next_seq(seq_seen);
         const SettleSlot *sl = slots + s % RING;
         static_assert(sizeof(SettleSlot) == sizeof(unsigned long long), "a slot is one 64-bit word");
         const unsigned long long word = __atomic_load_n((const unsigned long long *)(const void *)sl, __ATOMIC_ACQUIRE); // (both halves of one store)
         if ((unsigned)(word >> 32) != (unsigned)s) break;
         const unsigned changed = (unsigned)word;
         const Meta m = meta[s % RING];
         seq_seen = s;
         if (changed || m.pass != last_pass + 1 || m.pass <= floor || m.version != run_version || m.schedule != run_schedule) run = 0;
         run_version = m.version; run_schedule = m.schedule; last_pass = m.pass; last_changed = changed;
         if (!changed && m.pass > floor && run < (1ll << 62)) ++run;
      }
   }
   // A frame opens: may its probe passes be left out?  `eligible`: screen mode 0 and a single rank (no communicator, no peer
   // exchange, world 1 -- collectives stay matched across ranks).
   bool frame_begin(bool eligible, int schedule)
   {
      if (slots) poll();
      frame_version = version;
      frame_skip = enabled && eligible && slots && run >= MDH_SETTLE_PASSES && run_version == version && run_schedule == schedule;
      return frame_skip;
   }
   // asked for every probe pass of the open frame (an edit between frame_begin and the pass makes it run)
   bool skip_pass() const { return frame_skip && version == frame_version; }
   // An irradiance pass of the open frame is about to be launched.  Returns the slot's word for the kernel and *slot, or 0:
   // the pass runs untracked (the feature is off, the frame is not eligible or irregular, the ring is full), which ends the run.
   unsigned enqueue(bool trackable, int schedule, SettleSlot **slot)
   {
      ++issued;
      if (!enabled || !trackable || !slots || seq_issued - seq_seen >= RING - 2) return 0u; // (- 2: next_seq may pass over a number)
      seq_issued = next_seq(seq_issued);
      meta[seq_issued % RING] = {issued, frame_version, schedule};
      *slot = slots + seq_issued % RING;
      return (unsigned)seq_issued;
   }
   void untracked_pass() { ++issued; } // a probe pass outside the frame's one-radiance-then-one-irradiance pattern: the chain breaks
};

// "March, record or replay?" (MDH_OPT_RADIANCE_REPLAY, MDH_OPT_SCREEN_REPLAY; DESIGN.md section 4, "Exact work elimination",
// items 11 and 12).  A pass whose kernel has a REC argument marches (0), marches and records (1) or replays the records (2).
// The key is everything the marches read: what changed since the previous pass is marched plainly; what stood still for one
// pass is marched once more, by the recording kernel; valid records of the key are replayed while it holds.
// Key: plain data with operator== (RadRecKey, ScrRecKey).  No runtime call in here and no device memory: the records' buffer,
// its fences and what makes a recording kernel admissible are the caller's (mdh_api.hip; tests/schedule_check.cpp has none).
template <class Key>
struct ReplaySchedule {
   Key rec{}, seen{};                               // what the records are of / what the previous pass marched through
   bool rec_valid = false, seen_valid = false;
   bool no_memory = false;                          // the records' allocation failed: no further attempt until the key or the option changes
   long long stats[3] = {0, 0, 0};                  // passes launched marching, recording, replaying
   // `enabled`: the option is on and this variant is built with the recording kernels; `have_buffer`: the records' buffer
   // exists; `admissible`: a recording kernel may run (LDS, sizes)
   int choose(const Key &now, bool enabled, bool have_buffer, bool admissible) const
   {
      if (!enabled) return 0;
      if (rec_valid && have_buffer && now == rec) return 2;
      const bool stood = seen_valid && now == seen;
      if (no_memory && stood) return 0; // (not tried again, and no stream drained, in every frame)
      return stood && admissible ? 1 : 0;
   }
   void records_gone() { rec_valid = false; }       // the buffer is about to be regrown
   void allocation_failed() { no_memory = true; }   // ... and was not: the pass runs as 0
   // Behind the launch of a pass that ran as REC.  `seen_counts`: may the next pass record when its key is this one?
   void ran(int REC, const Key &now, bool seen_counts)
   {
      if (REC == 1) { rec = now; rec_valid = true; }
      else if (REC == 0) rec_valid = false; // (something moved, the option is off or this variant only marches)
      if (!(seen_valid && now == seen)) no_memory = false; // (a new key: the allocation may be tried again)
      seen = now;
      seen_valid = seen_counts;
      ++stats[REC];
   }
   // The option was set: the allocation may be tried again; off drops the records and, with `forget_seen`, the previous pass
   // too -- the first pass after the option comes back on then marches plainly, whatever its key.
   void option_set(bool on, bool forget_seen)
   {
      no_memory = false;
      if (!on) { rec_valid = false; if (forget_seen) seen_valid = false; }
   }
};
// everything a probe ray's marches read (rad_rec_key, mdh_api.hip)
struct RadRecKey {
   unsigned long geometry, inputs;      // geometry_edits, march_inputs
   unsigned long long part_version;     // Update_Partitioning's builds
   long rays;
   int grid[3], res[2], pc[2], probe_begin, probe_end;
   float spacing[3], max_dist;
   int pf, small, jit, residency, bvh, table_f4, part_bits_f4;
   bool operator==(const RadRecKey &o) const
   {
      return geometry == o.geometry && inputs == o.inputs && part_version == o.part_version && rays == o.rays &&
             memcmp(grid, o.grid, sizeof grid) == 0 && memcmp(res, o.res, sizeof res) == 0 && memcmp(pc, o.pc, sizeof pc) == 0 &&
             probe_begin == o.probe_begin && probe_end == o.probe_end && memcmp(spacing, o.spacing, sizeof spacing) == 0 && // (bits: a NaN spacing still equals itself)
             memcmp(&max_dist, &o.max_dist, sizeof max_dist) == 0 && pf == o.pf && small == o.small && jit == o.jit && residency == o.residency &&
             bvh == o.bvh && table_f4 == o.table_f4 && part_bits_f4 == o.part_bits_f4;
   }
};
// everything a screen march reads, and what decides which pixel holds what (scr_rec_key, mdh_api.hip)
struct ScrRecKey {
   RadRecKey march;                     // geometry, probe grid, max_dist, table layout, residency, BVH, JIT, the kernel's variant word
   float cam[12];                       // position and orientation BY VALUE: setting the camera to where it is changes nothing
   int W, H, rank, world, mode, spec, ao, gbuffer, window, split;
   unsigned long reflect_edits;         // Set_Material calls that took a material in use below the reflection's roughness threshold
   bool operator==(const ScrRecKey &o) const
   {
      return march == o.march && memcmp(cam, o.cam, sizeof cam) == 0 && W == o.W && H == o.H && rank == o.rank && world == o.world && mode == o.mode &&
             spec == o.spec && ao == o.ao && gbuffer == o.gbuffer && window == o.window && split == o.split && reflect_edits == o.reflect_edits;
   }
};

// "Is the stored order due for another sort?" (MDH_OPT_RADIANCE_ORDER: the probe rays; MDH_OPT_SCREEN_ORDER: the screen's
// tiles).  An order is sorted again every MDH_RAD_RESORT passes, and after MDH_RAD_RESORT_MOVING passes when what it follows
// moved since -- a stale order costs speed only, and the sort's launches are out of almost every frame.
// Of: the pass's own notes of what the stored order is of and what it was sorted under -- plain data that the pass writes and
// compares; whether the order at hand is that one ("have") and whether anything moved are the pass's to say.
#ifndef MDH_RAD_RESORT
#define MDH_RAD_RESORT 64
#endif
#ifndef MDH_RAD_RESORT_MOVING
#define MDH_RAD_RESORT_MOVING 8
#endif
template <class Of>
struct ResortClock {
   Of of{};
   bool ordered = false; // there is a stored order (forget)
   int age = 0;          // passes since it was sorted
   // asked once by every pass that could use an order: does this one sort?
   bool due(bool have, bool moved)
   {
      ++age;
      return !have || age >= MDH_RAD_RESORT || (moved && age >= MDH_RAD_RESORT_MOVING);
   }
   void sorted() { ordered = true; age = 0; } // (the pass has written `of`)
   void force() { age = MDH_RAD_RESORT; }     // the next pass that asks sorts
   void forget() { ordered = false; }         // the stored order is of something else, or its buffers are gone
};
struct RadOrderOf { long rays; int begin; unsigned long scene; };                      // the slice's rays, its first probe; geometry_edits when they were sorted
struct ScrOrderOf { int buf, n, rank, world; unsigned long geom; float cam[12]; };     // the buffer that holds the order, its tiles and their owner; geometry_edits when they were sorted; the camera when the sort was decided
