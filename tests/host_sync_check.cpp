// host_sync_check.cpp -- the owners of madarch_amd/csrc/mdh_host.h, run on the CPU against stand-ins of the few
// runtime functions they call (no libamdhip64 is linked).  Every stand-in appends to a call log, and what the checks
// below expect of that log is what the renderer's hand-written code did before the owners existed: one wait per
// stream and version, no wait on the signalling stream, a free before the malloc that replaces it, every handle
// destroyed exactly once.  tests/test_host_sync.py builds this with -fsanitize=address,undefined and runs it.
#include "mdh_host.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

static std::vector<std::string> g_log;
static std::set<void *> g_live_mem;
static std::set<hipEvent_t> g_live_ev;
static long g_next_event = 0, g_mallocs = 0, g_frees = 0, g_ev_created = 0, g_ev_destroyed = 0;
static int g_fail_in = 0; // > 0: the g_fail_in-th creation from now on fails (hipMalloc, hipHostMalloc, hipEventCreateWithFlags)
static bool g_fail_free = false; // the next hipFree / hipHostFree reports an error (the memory behind it is given back all the same)

#define CHECK(cond)                                                                 \
   do {                                                                             \
      if (!(cond)) {                                                                \
         fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
         for (const std::string &l : g_log) fprintf(stderr, "   log: %s\n", l.c_str()); \
         exit(1);                                                                   \
      }                                                                             \
   } while (0)

static std::string name(const char *what, const void *a, const void *b = nullptr)
{
   char buf[96];
   if (b) snprintf(buf, sizeof buf, "%s %ld %ld", what, (long)(size_t)a, (long)(size_t)b);
   else snprintf(buf, sizeof buf, "%s %ld", what, (long)(size_t)a);
   return buf;
}
static bool creation_fails() { return g_fail_in > 0 && --g_fail_in == 0; }
static hipError_t alloc(const char *what, void **p, size_t n)
{
   g_log.push_back(what);
   if (creation_fails()) return hipErrorOutOfMemory;
   *p = malloc(n ? n : 1);
   g_live_mem.insert(*p);
   ++g_mallocs;
   return hipSuccess;
}
static hipError_t dealloc(const char *what, void *p)
{
   g_log.push_back(what);
   CHECK(g_live_mem.erase(p) == 1); // (a pointer that was handed out and not freed yet)
   free(p);
   ++g_frees;
   if (g_fail_free) { g_fail_free = false; return hipErrorInvalidValue; }
   return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return alloc("malloc", p, n); }
hipError_t hipFree(void *p) { return dealloc("free", p); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return alloc("host_malloc", p, n); }
hipError_t hipHostFree(void *p) { return dealloc("host_free", p); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
   g_log.push_back("event_create");
   CHECK(flags == hipEventDisableTiming);
   if (creation_fails()) return hipErrorOutOfMemory;
   *e = (hipEvent_t)(size_t)(100 + ++g_next_event);
   g_live_ev.insert(*e);
   ++g_ev_created;
   return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
   g_log.push_back(name("event_destroy", e));
   CHECK(g_live_ev.erase(e) == 1);
   ++g_ev_destroyed;
   return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st)
{
   CHECK(g_live_ev.count(e) == 1);
   g_log.push_back(name("record", e, st));
   return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
   CHECK(g_live_ev.count(e) == 1);
   g_log.push_back(name("sync", e));
   return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned)
{
   CHECK(g_live_ev.count(e) == 1);
   g_log.push_back(name("wait", st, e));
   return hipSuccess;
}
}

static hipStream_t stream(int si) { return (hipStream_t)(size_t)(si + 1); } // (stream index si; none of them null)
static const hipStream_t S0 = stream(0), S1 = stream(1), S2 = stream(2), S3 = stream(3);
static size_t mark() { return g_log.size(); }
static std::vector<std::string> since(size_t m) { return std::vector<std::string>(g_log.begin() + m, g_log.end()); }
using Log = std::vector<std::string>;

static void check_fence()
{
   Fence f;
   size_t m = mark();
   for (int si = 0; si < HOST_NSTREAMS; ++si) CHECK(f.wait(stream(si), si) == hipSuccess); // fresh: nothing to wait for
   CHECK(since(m).empty());
   CHECK(f.create() == hipSuccess && f.create() == hipSuccess); // (idempotent)
   CHECK(since(m) == Log{"event_create"});
   const hipEvent_t ev = f.ev.ev;
   m = mark();
   CHECK(f.signal(S1, 1) == hipSuccess);
   CHECK(since(m) == Log{name("record", ev, S1)} && f.version == 1);
   m = mark();
   CHECK(f.wait(S1, 1) == hipSuccess); // the signalling stream
   CHECK(since(m).empty());
   CHECK(f.wait(S2, 2) == hipSuccess);
   CHECK(since(m) == Log{name("wait", S2, ev)});
   CHECK(f.wait(S2, 2) == hipSuccess); // once per version
   CHECK(since(m).size() == 1);
   m = mark();
   CHECK(f.signal(S2, 2) == hipSuccess && f.version == 2);
   CHECK(f.wait(S2, 2) == hipSuccess);
   CHECK(f.wait(S1, 1) == hipSuccess);
   CHECK(since(m) == (Log{name("record", ev, S2), name("wait", S1, ev)}));
   m = mark();
   CHECK(f.signal(S1, 1) == hipSuccess);
   f.mark_all_seen();
   CHECK(f.wait(S3, 3) == hipSuccess && f.wait(S0, 0) == hipSuccess);
   CHECK(since(m) == Log{name("record", ev, S1)});
   // a stream that signalled, then another stream's handle under the same index (mdh_set_stream): seen, but not the signaller
   m = mark();
   CHECK(f.signal(S0, 0) == hipSuccess);
   CHECK(f.wait(stream(7), 0) == hipSuccess);
   CHECK(since(m).size() == 1);
}

static void check_ring()
{
   RingUse<4> u;
   CHECK(u.create() == hipSuccess);
   CHECK(g_live_ev.size() == 4 * HOST_NSTREAMS);
   size_t m = mark();
   CHECK(u.mark(1, S1, 1) == hipSuccess && u.mark(1, S2, 2) == hipSuccess);
   const hipEvent_t e1 = u.done[1][1].ev, e2 = u.done[1][2].ev;
   CHECK(e1 != e2);
   CHECK(since(m) == (Log{name("record", e1, S1), name("record", e2, S2)}));
   m = mark();
   CHECK(u.retire_on_stream(2, S1, 1) == hipSuccess && u.retire_on_host(2) == hipSuccess); // slot 2 was never marked
   CHECK(since(m).empty());
   CHECK(u.retire_on_stream(1, S1, 1) == hipSuccess);
   CHECK(since(m) == Log{name("wait", S1, e2)}); // S2's event only: S1's own use is ordered by the stream
   CHECK(u.retire_on_stream(1, S1, 1) == hipSuccess);
   CHECK(since(m).size() == 1);
   m = mark();
   CHECK(u.mark(3, S0, 0) == hipSuccess && u.mark(3, S2, 2) == hipSuccess);
   CHECK(u.retire_on_host(3) == hipSuccess);
   CHECK(since(m) == (Log{name("record", u.done[3][0].ev, S0), name("record", u.done[3][2].ev, S2), name("sync", u.done[3][0].ev), name("sync", u.done[3][2].ev)}));
   CHECK(u.retire_on_host(3) == hipSuccess);
   CHECK(since(m).size() == 4);
   CHECK(u.mark(0, S1, 1) == hipSuccess && u.mark(2, S3, 3) == hipSuccess);
   u.forget();
   m = mark();
   for (int q = 0; q < 4; ++q) CHECK(u.retire_on_host(q) == hipSuccess && u.retire_on_stream(q, S0, 0) == hipSuccess);
   CHECK(since(m).empty());
}

template <bool Pinned>
static void check_buf(const char *malloc_name, const char *free_name)
{
   size_t m = mark();
   {
      DevBuf<float, Pinned> b;
      CHECK(b.grow(0) == hipSuccess && since(m).empty()); // nothing asked for, nothing held
      CHECK(b.grow(100) == hipSuccess && b.ptr && b.cap == 100);
      CHECK(since(m) == Log{malloc_name}); // (nothing was held: no free)
      float *first = b.ptr;
      CHECK(b.grow(100) == hipSuccess && b.grow(7) == hipSuccess && b.ptr == first && b.cap == 100);
      CHECK(since(m).size() == 1);
      b.ptr[99] = 1.0f; // (n elements, not n bytes: the sanitizer watches)
      CHECK(b.grow(101) == hipSuccess && b.cap == 101);
      CHECK(since(m) == (Log{malloc_name, free_name, malloc_name}));
      CHECK(b.release() == hipSuccess && b.release() == hipSuccess && !b.ptr && b.cap == 0);
      CHECK(since(m).size() == 4 && since(m)[3] == free_name);
      CHECK(b.grow(5) == hipSuccess);
      g_fail_in = 1;
      CHECK(b.grow(50) == hipErrorOutOfMemory && !b.ptr && b.cap == 0);
      CHECK(since(m) == (Log{malloc_name, free_name, malloc_name, free_name, malloc_name, free_name, malloc_name}));
   }
   CHECK(since(m).size() == 7); // the destructor of a buffer whose allocation failed
   m = mark();
   {
      DevBuf<float, Pinned> b;
      CHECK(b.grow(3) == hipSuccess);
   }
   CHECK(since(m) == (Log{malloc_name, free_name})); // the destructor of one that holds memory
   // a free that reports an error: the pointer is forgotten before the call, so nobody frees it a second time
   // (alloc_atlases kept the first atlas's pointer when the second free failed, and mdh_destroy freed it again)
   m = mark();
   {
      DevBuf<float, Pinned> b;
      CHECK(b.grow(3) == hipSuccess);
      g_fail_free = true;
      CHECK(b.release() == hipErrorInvalidValue && !b.ptr && b.cap == 0);
      CHECK(b.release() == hipSuccess);
      CHECK(b.grow(4) == hipSuccess);
      g_fail_free = true;
      CHECK(b.grow(9) == hipErrorInvalidValue && !b.ptr && b.cap == 0); // (and no allocation on top of the failure)
      CHECK(since(m) == (Log{malloc_name, free_name, malloc_name, free_name}));
   }
   CHECK(since(m).size() == 4); // the destructor after a failed free: nothing
}

// the two groups of the screen pass: whichever creation fails, no member is left
static void check_groups()
{
   for (int k = 1; k <= 6; ++k) { // the tile order: three kinds of buffers and two events
      DevBuf<unsigned char> cost;
      DevBuf<unsigned> order[2], hist;
      Fence sorted;
      Event other;
      auto create = [&] { return create_all(cost.sized(5000), order[0].sized(5000), order[1].sized(5000), hist.sized(256), sorted, other); };
      g_fail_in = k;
      CHECK(create() == hipErrorOutOfMemory && g_fail_in == 0);
      CHECK(!cost.ptr && !cost.cap && !order[0].ptr && !order[1].ptr && !hist.ptr && !hist.cap && !sorted.ev.ev && !other.ev);
      CHECK(g_live_mem.empty() && g_live_ev.empty() && g_mallocs == g_frees && g_ev_created == g_ev_destroyed);
      CHECK(create() == hipSuccess);
      CHECK(cost.cap == 5000 && order[0].ptr && order[1].ptr && order[0].ptr != order[1].ptr && hist.cap == 256 && sorted.ev.ev && other.ev && sorted.ev.ev != other.ev);
      const size_t m = mark();
      CHECK(create() == hipSuccess && since(m).empty()); // (there already)
   }
   CHECK(g_live_mem.empty() && g_live_ev.empty());
   for (int k = 1; k <= 1 + HOST_NSTREAMS; ++k) { // the pixel records' events: the write and every stream's read
      Fence written;
      RingUse<1> reads;
      g_fail_in = k;
      CHECK(create_all(written, reads) == hipErrorOutOfMemory && g_fail_in == 0);
      CHECK(!written.ev.ev);
      for (const Event &e : reads.done[0]) CHECK(!e.ev);
      CHECK(g_live_ev.empty() && g_ev_created == g_ev_destroyed);
      CHECK(create_all(written, reads) == hipSuccess);
      CHECK(g_live_ev.size() == 1 + HOST_NSTREAMS);
   }
}

// the queries' bridge: the logs are ray_stream_run's (no main stream) and shade_query_run's (with it) as they stood before
// the bridge, written out by hand with in / out / frame for ev_rq_in, ev_sq_caller / ev_rq_out, ev_sq_done / ev_sq_frame
static void check_query_bridge()
{
   const hipStream_t main = S0, qs = S3, caller = S1;
   for (int k = 1; k <= 3; ++k) { // whichever creation fails, all three events are empty again
      QueryBridge b;
      g_fail_in = k;
      CHECK(b.create() == hipErrorOutOfMemory && g_fail_in == 0);
      CHECK(!b.frame.ev && !b.in.ev && !b.out.ev && g_live_ev.empty() && g_ev_created == g_ev_destroyed);
   }
   const long created = g_ev_created, destroyed = g_ev_destroyed;
   size_t m = mark();
   {
      QueryBridge b;
      DevBuf<unsigned> next;
      CHECK(create_all(next.sized(1), b) == hipSuccess && b.create() == hipSuccess); // (as a member of a group, and idempotent)
      CHECK(since(m) == (Log{"malloc", "event_create", "event_create", "event_create"}));
      const hipEvent_t frame = b.frame.ev, in = b.in.ev, out = b.out.ev;
      CHECK(frame != in && in != out && frame != out);
      for (int round = 0; round < 2; ++round) { // a second call records the same three events again
         // host arrays, no place among the frames (mdh_raycast): nothing at all
         m = mark();
         CHECK(b.enter(qs, qs, nullptr) == hipSuccess && b.leave(qs, qs, nullptr) == hipSuccess);
         CHECK(since(m).empty());
         // device arrays, no place among the frames (ray_stream_run)
         m = mark();
         CHECK(b.enter(qs, caller, nullptr) == hipSuccess);
         CHECK(since(m) == (Log{name("record", in, caller), name("wait", qs, in)}));
         m = mark();
         CHECK(b.leave(qs, caller, nullptr) == hipSuccess);
         CHECK(since(m) == (Log{name("record", out, qs), name("wait", caller, out)}));
         // host arrays at a place among the frames (shade_query_run, caller == qs)
         m = mark();
         CHECK(b.enter(qs, qs, &main) == hipSuccess);
         CHECK(since(m) == (Log{name("record", frame, main), name("wait", qs, frame)}));
         m = mark();
         CHECK(b.leave(qs, qs, &main) == hipSuccess);
         CHECK(since(m) == (Log{name("record", out, qs), name("wait", main, out)}));
         // device arrays at a place among the frames (shade_query_run, caller != qs)
         m = mark();
         CHECK(b.enter(qs, caller, &main) == hipSuccess);
         CHECK(since(m) == (Log{name("record", frame, main), name("wait", qs, frame), name("record", in, caller), name("wait", qs, in)}));
         m = mark();
         CHECK(b.leave(qs, caller, &main) == hipSuccess);
         CHECK(since(m) == (Log{name("record", out, qs), name("wait", main, out), name("wait", caller, out)}));
         CHECK(b.frame.ev == frame && b.in.ev == in && b.out.ev == out);
      }
      // the default stream as the caller's is a stream like any other, not "none"
      m = mark();
      CHECK(b.enter(qs, nullptr, nullptr) == hipSuccess && b.leave(qs, nullptr, nullptr) == hipSuccess);
      CHECK(since(m) == (Log{name("record", in, nullptr), name("wait", qs, in), name("record", out, qs), name("wait", nullptr, out)}));
      m = mark();
      b.release(); b.release();
      CHECK(since(m) == (Log{name("event_destroy", frame), name("event_destroy", in), name("event_destroy", out)}));
      CHECK(b.create() == hipSuccess); // ... and the destructor's turn
   }
   CHECK(g_live_ev.empty() && g_ev_created - created == 6 && g_ev_destroyed - destroyed == 6); // every event destroyed once
}

static void check_empty_owners()
{
   const size_t m = mark();
   {
      DevBuf<double> b;
      PinnedBuf<int> h;
      Event e;
      Fence f;
      RingUse<4> u;
      QueryBridge q;
      CHECK(b.release() == hipSuccess && h.release() == hipSuccess);
      e.release(); f.release(); u.release(); u.forget(); f.mark_all_seen(); q.release();
   }
   CHECK(since(m).empty());
}

int main()
{
   check_empty_owners();
   check_fence();
   check_ring();
   check_buf<false>("malloc", "free");
   check_buf<true>("host_malloc", "host_free");
   check_groups();
   check_query_bridge();
   CHECK(g_live_mem.empty() && g_live_ev.empty());
   CHECK(g_mallocs > 0 && g_mallocs == g_frees && g_ev_created > 0 && g_ev_created == g_ev_destroyed);
   printf("host_sync_check: ok (%ld allocations, %ld events, %zu runtime calls)\n", g_mallocs, g_ev_created, g_log.size());
   return 0;
}
