// schedule_check.cpp -- ReplaySchedule and ResortClock of madarch_amd/csrc/mdh_host.h (MDH_OPT_RADIANCE_REPLAY,
// MDH_OPT_SCREEN_REPLAY, MDH_OPT_RADIANCE_ORDER, MDH_OPT_SCREEN_ORDER) on the CPU.  Neither makes a runtime call or owns device
// memory: a rig drives them the way pass_radiance, pass_screen and mdh_set_option of mdh_api.hip do, with a records' buffer
// that is a capacity and nothing else.  Every script states the exact REC of every pass (0 marches, 1 marches and records,
// 2 replays).  tests/test_schedules_host.py builds this with -fsanitize=address,undefined and runs it.
#include "mdh_host.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>

#define CHECK(cond)                                                                 \
   do {                                                                             \
      if (!(cond)) {                                                                \
         fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
         exit(1);                                                                   \
      }                                                                             \
   } while (0)

struct Key { // (the schedule asks a key for operator== and nothing else)
   int v;
   bool operator==(const Key &o) const { return v == o.v; }
};

// The two flavours differ at their call sites alone: whether the pass behind which the option was off counts as seen, and
// whether a failed allocation of the records is survived (radiance returns the error).
struct Rig {
   const bool screen;
   ReplaySchedule<Key> s;
   bool option = true, admissible = true, alloc_fails = false;
   size_t cap = 0, need = 1; // the records' buffer: its capacity, and what a recording pass needs
   int attempts = 0;         // allocations tried
   long passes = 0;
   explicit Rig(bool screen_flavour) : screen(screen_flavour) {}
   int pass(int key)
   {
      const Key now = {key};
      int rec = s.choose(now, option, cap > 0, admissible);
      CHECK(rec >= 0 && rec <= 2);
      if (rec == 2) CHECK(cap >= need); // (a replay never reads records that are not there)
      if (rec == 1 && need > cap) {
         s.records_gone();
         ++attempts;
         cap = 0; // (DevBuf::grow releases first: after a failed allocation the buffer is empty)
         if (alloc_fails) {
            CHECK(screen);
            s.allocation_failed();
            rec = 0;
         } else
            cap = need;
      }
      s.ran(rec, now, screen ? option : true);
      ++passes;
      CHECK(s.stats[0] + s.stats[1] + s.stats[2] == passes);
      return rec;
   }
   void set_option(bool on)
   {
      option = on;
      s.option_set(on, screen);
      if (!on) cap = 0; // (the buffer is released)
   }
   // the RECs of passes with these keys, as a string of digits
   std::string run(std::initializer_list<int> keys)
   {
      std::string out;
      for (int k : keys) out += (char)('0' + pass(k));
      return out;
   }
};

static void replay_scripts(bool screen)
{
   { // a standing key: march, record, replay for as long as it holds
      Rig g(screen);
      const int n = 12;
      for (int i = 0; i < n; ++i) CHECK(g.pass(7) == (i == 0 ? 0 : i == 1 ? 1 : 2));
      CHECK(g.s.stats[0] == 1 && g.s.stats[1] == 1 && g.s.stats[2] == n - 2);
      CHECK(g.attempts == 1);
   }
   { // a key that changes every pass, and two keys alternating: nothing ever stands still for a pass
      Rig g(screen);
      for (int i = 0; i < 20; ++i) CHECK(g.pass(100 + i) == 0);
      CHECK(g.run({1, 2, 1, 2, 1, 2, 1, 2}) == "00000000");
      CHECK(g.s.stats[0] == 28 && g.s.stats[1] == 0 && g.s.stats[2] == 0 && g.attempts == 0);
   }
   { // a change during replay: the new key is marched, recorded and replayed in its turn; the old key's records are gone
      Rig g(screen);
      CHECK(g.run({1, 1, 1, 1, 2, 2, 2, 2, 1, 1, 1}) == "0122" "0122" "012");
      CHECK(g.attempts == 1); // (the buffer is large enough: no second allocation)
   }
   { // recording never admissible (LDS, sizes): the key keeps marching, and the schedule still follows what was seen
      Rig g(screen);
      g.admissible = false;
      CHECK(g.run({5, 5, 5, 5, 5, 5}) == "000000");
      CHECK(g.s.seen_valid && g.s.seen == Key{5} && !g.s.rec_valid && g.attempts == 0);
      g.admissible = true;
      CHECK(g.run({5, 5}) == "12"); // (seen followed: no further plain pass)
   }
   { // valid records but no buffer: not replayed -- the key stands, so it is recorded again
      Rig g(screen);
      CHECK(g.run({3, 3, 3}) == "012");
      g.cap = 0;
      CHECK(g.s.rec_valid && g.s.choose(Key{3}, true, false, true) != 2);
      CHECK(g.run({3, 3}) == "12");
   }
   { // regrowth by a recording pass: whatever becomes of that pass, the old records are not replayed from the new buffer
      Rig g(screen);
      CHECK(g.run({3, 3, 3}) == "012");
      CHECK(g.s.choose(Key{3}, true, true, true) == 2);
      g.s.records_gone(); // (a pass regrows the buffer, and its launch fails: nothing ran)
      g.cap = g.need = 2;
      CHECK(g.s.choose(Key{3}, true, true, true) == 1);
      CHECK(g.run({3, 3}) == "12" && g.attempts == 1);
      // ... and a recording pass that finds the buffer too small regrows it for its own key
      g.need = 3;
      CHECK(g.run({4, 4, 4, 3}) == "0120" && g.attempts == 2 && g.cap == 3);
   }
   { // the option off: passes march, whatever stands
      Rig g(screen);
      g.set_option(false);
      CHECK(g.run({1, 1, 1, 1}) == "0000");
      CHECK(g.attempts == 0);
   }
}

// Option off and on again over the same key.  Radiance keeps what its passes saw: the first pass after the option comes back
// on records.  Screen forgets it: one plain pass first.  (tests/test_gpu_radiance_replay.py and test_gpu_screen_replay.py,
// test_option_flip: "pcr" "pp" "crr" and "pcr" "pp" "pcr".)
static void option_scripts()
{
   for (const bool between : {false, true}) {
      Rig rad(false), scr(true);
      CHECK(rad.run({1, 1, 1}) == "012" && scr.run({1, 1, 1}) == "012");
      rad.set_option(false); scr.set_option(false);
      CHECK(!rad.s.rec_valid && !scr.s.rec_valid);
      if (between) CHECK(rad.run({1, 1}) == "00" && scr.run({1, 1}) == "00");
      rad.set_option(true); scr.set_option(true);
      CHECK(rad.run({1, 1, 1}) == "122");
      CHECK(scr.run({1, 1, 1}) == "012");
      CHECK(rad.attempts == 2 && scr.attempts == 2); // (the buffer went with the option)
   }
   { // on set again while it is on: nothing is dropped
      Rig rad(false), scr(true);
      CHECK(rad.run({1, 1, 1}) == "012" && scr.run({1, 1, 1}) == "012");
      rad.set_option(true); scr.set_option(true);
      CHECK(rad.run({1, 1}) == "22" && scr.run({1, 1}) == "22");
   }
   { // a key that changed while the option was off: a plain pass first in both flavours
      Rig rad(false), scr(true);
      CHECK(rad.run({1, 1, 1}) == "012" && scr.run({1, 1, 1}) == "012");
      rad.set_option(false); scr.set_option(false);
      CHECK(rad.run({1}) == "0" && scr.run({1}) == "0");
      rad.set_option(true); scr.set_option(true);
      CHECK(rad.run({2, 2, 2}) == "012" && scr.run({2, 2, 2}) == "012");
   }
}

// the records' allocation fails (the screen flavour survives it)
static void allocation_scripts()
{
   Rig g(true);
   g.alloc_fails = true;
   CHECK(g.run({1, 1}) == "00" && g.attempts == 1);   // the pass that would have recorded runs as 0
   CHECK(g.s.no_memory && !g.s.rec_valid);
   for (int i = 0; i < 50; ++i) CHECK(g.pass(1) == 0); // the same key is not tried again however many passes follow
   CHECK(g.attempts == 1);
   CHECK(g.run({2}) == "0" && !g.s.no_memory);         // a new key allows the next attempt ...
   CHECK(g.run({2}) == "0" && g.attempts == 2 && g.s.no_memory);
   CHECK(g.run({2, 2, 2}) == "000" && g.attempts == 2);
   g.set_option(true);                                 // ... and so does setting the option
   CHECK(!g.s.no_memory);
   CHECK(g.run({2}) == "0" && g.attempts == 3);
   g.set_option(true);
   g.alloc_fails = false;                              // (memory is back)
   CHECK(g.run({2, 2, 2}) == "122" && g.attempts == 4);
   CHECK(g.s.stats[0] == g.passes - 3 && g.s.stats[1] == 1 && g.s.stats[2] == 2);
   { // off and on clears it too
      Rig h(true);
      h.alloc_fails = true;
      CHECK(h.run({1, 1, 1}) == "000" && h.attempts == 1);
      h.set_option(false);
      h.set_option(true);
      h.alloc_fails = false;
      CHECK(h.run({1, 1, 1}) == "012" && h.attempts == 2);
   }
}

// the renderer's keys compare by value (bits for the floats)
static void key_checks()
{
   RadRecKey a = {}, b = {};
   CHECK(a == b);
   b.geometry = 1; CHECK(!(a == b)); b = a;
   b.part_bits_f4 = 1; CHECK(!(a == b)); b = a;
   b.grid[2] = 1; CHECK(!(a == b)); b = a;
   const unsigned nan_bits = 0x7fc00000u;
   memcpy(&a.spacing[1], &nan_bits, 4);
   CHECK(!(a == b));
   b = a;
   CHECK(a == b); // (a NaN spacing still equals itself)
   ScrRecKey s = {}, t = {};
   CHECK(s == t);
   t.march.inputs = 1; CHECK(!(s == t)); t = s;
   t.cam[11] = 1.0f; CHECK(!(s == t)); t = s;
   t.reflect_edits = 1; CHECK(!(s == t)); t = s;
   t.split = 2; CHECK(!(s == t));
}

// the re-sort clock as a pass drives it: `have` is its own test of the stored order, `moved` its own test of what changed
struct Sorter {
   ResortClock<int> c; // (Of: whatever the pass notes; here the number of the sort)
   long passes = 0, sorts = 0;
   bool pass(bool moved, int of = 0)
   {
      ++passes;
      const bool have = c.ordered && c.of == of;
      if (!c.due(have, moved)) return false;
      c.of = of;
      c.sorted();
      ++sorts;
      return true;
   }
};
static void clock_scripts()
{
   static_assert(MDH_RAD_RESORT_MOVING >= 2 && MDH_RAD_RESORT > MDH_RAD_RESORT_MOVING, "the scripts below tell the two periods apart");
   { // without an order: due at once; standing still: due again at pass MDH_RAD_RESORT behind the sort, and so on
      Sorter s;
      CHECK(s.pass(false));
      for (int round = 0; round < 3; ++round) {
         for (int i = 1; i < MDH_RAD_RESORT; ++i) CHECK(!s.pass(false));
         CHECK(s.pass(false));
      }
      CHECK(s.sorts == 4 && s.passes == 1 + 3 * (long)MDH_RAD_RESORT);
   }
   { // moved: due at pass MDH_RAD_RESORT_MOVING
      Sorter s;
      CHECK(s.pass(true));
      for (int round = 0; round < 3; ++round) {
         for (int i = 1; i < MDH_RAD_RESORT_MOVING; ++i) CHECK(!s.pass(true));
         CHECK(s.pass(true));
      }
   }
   { // something moves late: due at once when the order is MDH_RAD_RESORT_MOVING passes old and more
      Sorter s;
      CHECK(s.pass(false));
      for (int i = 1; i < MDH_RAD_RESORT_MOVING + 3; ++i) CHECK(!s.pass(false));
      CHECK(s.pass(true));
      CHECK(!s.pass(true)); // "sorted" restarted the clock
   }
   { // "force": the next pass is due, standing still or not; "sorted" restarts
      Sorter s;
      CHECK(s.pass(false) && !s.pass(false) && !s.pass(false));
      s.c.force();
      CHECK(s.pass(false));
      for (int i = 1; i < MDH_RAD_RESORT; ++i) CHECK(!s.pass(false));
      CHECK(s.pass(false));
   }
   { // "forget": no order, due at once; an order of something else is none either
      Sorter s;
      CHECK(s.pass(false) && !s.pass(false));
      s.c.forget();
      CHECK(!s.c.ordered && s.pass(false) && s.c.ordered && !s.pass(false));
      CHECK(s.pass(false, 1) && !s.pass(false, 1) && s.pass(false, 0));
   }
   { // a pass that is due and does not sort (its launch failed) stays due
      ResortClock<int> c;
      CHECK(c.due(false, false) && c.due(false, false));
      c.sorted();
      for (int i = 1; i < MDH_RAD_RESORT; ++i) CHECK(!c.due(true, false));
      CHECK(c.due(true, false) && c.due(true, false));
   }
}

int main()
{
   replay_scripts(false);
   replay_scripts(true);
   option_scripts();
   allocation_scripts();
   key_checks();
   clock_scripts();
   printf("schedule_check: ok\n");
   return 0;
}
