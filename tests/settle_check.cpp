// settle_check.cpp -- SettleTracker of madarch_amd/csrc/mdh_host.h (MDH_OPT_PROBE_SETTLE) on the CPU.  The tracker makes no
// runtime call: its slots are plain memory here, and a scripted "device" writes them the way k_irradiance's last workgroup
// does (changed and seq as one 64-bit word), late and out of step with the enqueues.  Every script states exactly which frames leave their
// probe passes out.  tests/test_settle_host.py builds this with -fsanitize=address,undefined and runs it.
#include "mdh_host.h"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#define CHECK(cond)                                                                 \
   do {                                                                             \
      if (!(cond)) {                                                                \
         fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
         exit(1);                                                                   \
      }                                                                             \
   } while (0)

// a renderer's frames as mdh_api.hip drives the tracker, and a device that finishes passes `lag` frames late
struct Rig {
   SettleSlot slots[SettleTracker::RING] = {};
   SettleTracker t;
   struct InFlight { SettleSlot *slot; unsigned seq, changed; };
   std::deque<InFlight> queue; // tracked passes the device has not finished, in order
   long frames = 0, skipped = 0, tracked = 0, untracked = 0;
   Rig() { t.slots = slots; }
   void device_finishes(size_t n) // the oldest n passes in flight report
   {
      for (; n > 0 && !queue.empty(); --n) {
         const InFlight f = queue.front();
         queue.pop_front();
         __atomic_store_n((unsigned long long *)(void *)f.slot, (unsigned long long)f.changed | (unsigned long long)f.seq << 32, __ATOMIC_RELEASE);
      }
   }
   // one frame (radiance, irradiance); `changed`: the texels its irradiance pass changes if it runs.  Returns whether its
   // probe passes were left out.  `lag`: passes that stay in flight behind this frame.
   bool frame(unsigned changed, size_t lag, bool eligible = true, int schedule = 1, bool edit_inside = false)
   {
      ++frames;
      t.frame_begin(eligible, schedule);
      if (edit_inside) t.bump(); // (an edit between mdh_frame_begin and the passes of a three-call frame)
      const bool skip_rad = t.skip_pass();
      const bool skip_irr = t.skip_pass();
      CHECK(skip_rad == skip_irr);
      if (skip_irr) { ++skipped; return true; }
      SettleSlot *slot = nullptr;
      const unsigned seq = t.enqueue(eligible, schedule, &slot);
      if (seq) {
         CHECK(slot >= slots && slot < slots + SettleTracker::RING);
         for (const InFlight &f : queue) CHECK(f.slot != slot); // a slot is never handed out while its pass is in flight
         queue.push_back({slot, seq, changed});
         ++tracked;
      } else
         ++untracked;
      if (queue.size() > lag) device_finishes(queue.size() - lag);
      return false;
   }
};

static const int N = MDH_SETTLE_PASSES;

// passes change texels for `settle` frames, then nothing; the device reports `lag` passes late: frame f (from 0) is the
// first one left out exactly when the host has seen N unchanged passes at its begin
static void lagged_static_scene(size_t lag, int settle)
{
   Rig g;
   for (int f = 0; f < 200; ++f) {
      const bool skipped = g.frame(f < settle ? 7u : 0u, lag);
      // at the begin of frame f the host has seen passes 0 .. f - 1 - lag; unchanged ones are settle .. : N of them when
      // f - lag - settle >= N
      CHECK(skipped == (f >= settle + N + (int)lag));
   }
   CHECK(g.skipped == 200 - (settle + N + (long)lag));
   CHECK(g.t.current_run() == N); // (no pass was enqueued after the first frame left out; the `lag` in flight never report)
}

int main()
{
   for (size_t lag = 0; lag <= 4; ++lag)
      for (int settle : {0, 1, 6, 8}) lagged_static_scene(lag, settle);

   { // a changed pass inside a run starts the count again
      Rig g;
      for (int f = 0; f < N - 1; ++f) CHECK(!g.frame(0u, 0));
      CHECK(!g.frame(3u, 0));
      CHECK(g.t.current_run() == 0 || g.t.current_run() == N - 1); // (the changed pass is seen at the next begin or already)
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.t.last_changed == 0u);
      CHECK(g.frame(0u, 0));
      CHECK(g.skipped == 1);
   }
   { // an edit: the run is worth nothing, frames run again and N unchanged passes under the new version settle again
      Rig g;
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0) && g.frame(0u, 0));
      g.t.bump();
      CHECK(g.t.current_run() == 0);
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0));
   }
   { // an edit between enqueue and arrival: passes enqueued before it count for nothing after it, however late they report
      Rig g;
      for (int f = 0; f < N + 2; ++f) CHECK(!g.frame(0u, 4)); // (4 in flight: the host has seen N - 2)
      g.t.bump();
      g.device_finishes(4); // (N + 2 unchanged passes have reported, all of the old version)
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0));
      CHECK(g.skipped == 1);
   }
   { // an edit inside an open frame that had decided to leave its passes out: they run
      Rig g;
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0));
      CHECK(!g.frame(0u, 0, true, 1, true));
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0)); // (the pass of the edited frame is of the old version: N more)
      CHECK(g.frame(0u, 0));
   }
   { // the ring wraps many times; slots are reused only after they were read
      Rig g;
      for (int f = 0; f < 10 * SettleTracker::RING; ++f) CHECK(!g.frame(1u, (size_t)(f % 5)));
      CHECK(g.untracked == 0 && g.tracked == 10 * SettleTracker::RING);
      g.device_finishes(8);
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0));
   }
   { // the device falls behind by more than the ring: passes run untracked and no slot is overwritten.  Unchanged passes: the
     // tracked ones are a run of N and more under the version that holds, so whatever ran behind them stored the same bits
      Rig g;
      for (int f = 0; f < 3 * SettleTracker::RING; ++f) CHECK(!g.frame(0u, 100000));
      CHECK(g.tracked < SettleTracker::RING && g.tracked >= N && g.untracked > 0);
      g.device_finishes(100000);
      CHECK(g.frame(0u, 0));
   }
   { // ... changing passes: the untracked ones are a gap in the chain, and the run starts behind it
      Rig g;
      for (int f = 0; f < 3 * SettleTracker::RING; ++f) CHECK(!g.frame(2u, 100000));
      g.device_finishes(100000);
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.t.current_run() == N - 1);
      CHECK(g.frame(0u, 0));
   }
   { // a gap inside a run that is still short: N - 1 unchanged passes, one untracked pass, and the count starts again
      Rig g;
      for (int f = 0; f < N - 1; ++f) CHECK(!g.frame(0u, 0));
      g.t.frame_begin(true, 1);
      g.t.untracked_pass(); // (a frame with a second radiance pass, say)
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0));
   }
   { // a schedule switch: a run under one schedule settles no frame of the other
      Rig g;
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0, true, 1));
      CHECK(g.frame(0u, 0, true, 1));
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0, true, 0));
      CHECK(g.frame(0u, 0, true, 0));
      CHECK(!g.frame(0u, 0, true, 1));
   }
   { // the option: off runs every frame and forgets the run; on again counts from nothing
      Rig g;
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0));
      g.t.set_enabled(false);
      CHECK(g.t.current_run() == 0);
      for (int f = 0; f < 3 * N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.tracked == N);
      g.t.set_enabled(true);
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0));
   }
   { // the option goes off inside an open frame that had decided to leave its passes out: they run
      Rig g;
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.t.frame_begin(true, 1) && g.t.skip_pass());
      g.t.set_enabled(false);
      CHECK(!g.t.skip_pass());
   }
   { // more than one rank (or another screen mode): never tracked, never left out; the renderer's switch between the two is an
     // edit (rank, world, communicator and screen mode all bump), so no run survives it
      Rig g;
      for (int f = 0; f < 4 * N; ++f) CHECK(!g.frame(0u, 0, false));
      CHECK(g.tracked == 0 && g.skipped == 0);
      g.t.bump();
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0, true));
      CHECK(g.frame(0u, 0, true));
      g.t.bump();
      for (int f = 0; f < 4 * N; ++f) CHECK(!g.frame(0u, 0, false));
      g.t.bump();
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0, true));
      CHECK(g.frame(0u, 0, true));
      CHECK(!g.frame(0u, 0, false)); // (and a settled tracker alone still runs the frame of several ranks)
   }
   { // reset (a frame was abandoned): passes enqueued before it never count
      Rig g;
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 2));
      g.t.reset();
      g.device_finishes(2);
      for (int f = 0; f < N; ++f) CHECK(!g.frame(0u, 0));
      CHECK(g.frame(0u, 0));
   }
   { // without slots (their allocation failed, or the feature is compiled out) nothing is tracked or left out
      SettleTracker t;
      SettleSlot *slot = nullptr;
      for (int f = 0; f < 3 * N; ++f) {
         CHECK(!t.frame_begin(true, 1) && !t.skip_pass());
         CHECK(t.enqueue(true, 1, &slot) == 0u && slot == nullptr);
      }
   }
   printf("settle_check: ok\n");
   return 0;
}
