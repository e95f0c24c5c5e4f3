// ray_stream_check.cpp -- mdh_ray_stream.h (madarch_amd/csrc) on the CPU: the hand-out of rays to idle lanes and the
// ray-validity predicate of the device-array ray queries (k_ray_stream).  W wavefronts of 64 lanes share one counter, as the
// kernel's do; a ray is a scripted number of steps.  The wavefronts take their turns in a seeded order -- they are
// independent on the device, so every interleaving has to serve every ray exactly once -- and each turn is one pass of
// k_ray_stream's loop, written with the header's functions and nothing else.  Built with the address and
// undefined-behaviour sanitizers by tests/test_ray_stream_host.py.
#include "mdh_ray_stream.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t g_rng = 0x4D414441u;
static uint32_t rnd()
{
   g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
   return (uint32_t)(g_rng >> 33);
}

struct Wave {
   long long ray[64];
   int left[64]; // steps the lane's ray still takes
   bool drained = false, ended = false;
   std::vector<std::vector<unsigned>> rounds; // the rays of each hand-out, in lane order
   Wave() { for (int l = 0; l < 64; ++l) { ray[l] = -1; left[l] = 0; } }
};

// one pass of k_ray_stream's loop for one wavefront
static void turn(Wave &w, unsigned &next, unsigned n, int refill, const std::vector<int> &len, std::vector<int> &served)
{
   unsigned long long idle = 0;
   for (int l = 0; l < 64; ++l) idle |= (unsigned long long)(w.ray[l] < 0) << l;
   const int n_idle = rs_popcount(idle);
   if (!w.drained && rs_refills(n_idle, refill)) {
      const unsigned base = next;
      next += (unsigned)n_idle; // lane 0's atomicAdd
      std::vector<unsigned> round;
      int rank = 0;
      for (int l = 0; l < 64; ++l) {
         if (w.ray[l] >= 0) continue;
         EXPECT(rs_idle_rank(idle, l) == rank, "lane %d: rank %d, not %d", l, rs_idle_rank(idle, l), rank);
         ++rank;
         const long long q = rs_ray_of(base, idle, l, n);
         EXPECT(q >= -1 && q < (long long)n, "lane %d was handed ray %lld of %u", l, q, n);
         if (q < 0 || q >= (long long)n) continue;
         w.ray[l] = q;
         w.left[l] = len[(size_t)q];
         round.push_back((unsigned)q);
      }
      w.drained = rs_drained(base, n_idle, n);
      EXPECT(w.drained == ((unsigned long long)next >= n), "drained %d with the counter at %u of %u", (int)w.drained, next, n);
      w.rounds.push_back(round);
   }
   bool busy = false;
   for (int l = 0; l < 64; ++l) busy = busy || w.ray[l] >= 0;
   if (!busy) { w.ended = w.drained; return; }
   for (int l = 0; l < 64; ++l)
      if (w.ray[l] >= 0 && --w.left[l] <= 0) { // the ray's last step: its answer is stored, the lane is idle
         ++served[(size_t)w.ray[l]];
         w.ray[l] = -1;
      }
}

static void run(int W, unsigned n, int refill, const std::vector<int> &len, const char *what)
{
   std::vector<Wave> waves((size_t)W);
   std::vector<int> served(n, 0);
   unsigned next = 0;
   long long longest = 1;
   for (int v : len) longest = v > longest ? v : longest;
   // every turn either ends a step of a busy lane or hands rays out: no more than this many before everything has ended
   const long long cap = ((long long)n + 64) * (longest + 2) + 64ll * W + 1024;
   long long turns = 0;
   for (;;) {
      int live = 0;
      for (const Wave &w : waves) live += !w.ended;
      if (!live) break;
      Wave &w = waves[rnd() % (unsigned)W];
      if (w.ended) continue;
      if (++turns > cap) break;
      turn(w, next, n, refill, len, served);
   }
   EXPECT(turns <= cap, "%s: W %d n %u refill %d did not end within %lld turns", what, W, n, refill, cap);
   for (unsigned q = 0; q < n; ++q) EXPECT(served[q] == 1, "%s: W %d n %u refill %d: ray %u served %d times", what, W, n, refill, q, served[q]);
   EXPECT((unsigned long long)next <= (unsigned long long)n + 64ull * (unsigned)W, "%s: the counter ran to %u for %u rays and %d wavefronts", what, next, n, W);
   if (refill == 64) // lock step: a round is 64 consecutive rays (fewer only where the batch ends)
      for (const Wave &w : waves)
         for (const auto &round : w.rounds) {
            for (size_t i = 1; i < round.size(); ++i) EXPECT(round[i] == round[0] + i, "%s: a lock-step round is not consecutive at %zu", what, i);
            if (!round.empty()) EXPECT(round.size() == 64 || round[0] + round.size() == n, "%s: a lock-step round of %zu rays from %u of %u", what, round.size(), round[0], n);
         }
}

static void check_hand_out()
{
   const int waves[] = {1, 4, 16}, refills[] = {1, 2, 16, 63, 64};
   const unsigned counts[] = {0, 1, 63, 64, 65, 257, 1000};
   for (int W : waves)
      for (int refill : refills)
         for (unsigned n : counts) {
            std::vector<int> ones(n, 1), one_long(n, 1), geometric(n, 1);
            if (n) one_long[n / 3] = 1000;
            for (unsigned q = 0; q < n; ++q) { // mean 11 steps, a tail of hundreds
               int k = 1;
               while (k < 2000 && rnd() % 11u != 0u) ++k;
               geometric[q] = k;
            }
            run(W, n, refill, ones, "all 1");
            run(W, n, refill, one_long, "one of 1000");
            run(W, n, refill, geometric, "geometric");
         }
   // the arithmetic at the counter's far end: bases near 2^31 do not wrap
   const unsigned big = 0x7fffffffu;
   EXPECT(rs_ray_of(big - 1u, ~0ull, 0, big) == (long long)big - 1, "the last ray of 2^31 - 1");
   EXPECT(rs_ray_of(big - 1u, ~0ull, 1, big) == -1, "one past the last ray of 2^31 - 1");
   EXPECT(rs_ray_of(0xffffffc0u, ~0ull, 63, big) == -1, "a base just below 2^32");
   EXPECT(rs_drained(big - 1u, 1, big) && !rs_drained(big - 2u, 1, big), "drained at 2^31 - 1");
   EXPECT(rs_refills(64, 1) && rs_refills(1, 1) && !rs_refills(0, 1) && rs_refills(64, 64) && !rs_refills(63, 64) && rs_refills(16, 16) && !rs_refills(15, 16), "refill thresholds");
   EXPECT(rs_idle_rank(~0ull, 63) == 63 && rs_idle_rank(1ull << 63, 63) == 0 && rs_idle_rank(0x5ull, 2) == 1, "ranks");
}

static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static void check_predicate()
{
   const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
   const float snan = bits(0x7f800001u), neg_nan = bits(0xffc00000u);
   const float denorm = bits(0x00000001u), neg_denorm = bits(0x80000001u), big = std::numeric_limits<float>::max();
   EXPECT(rs_ray_valid(0.0f, -0.0f, denorm, neg_denorm, big, -big), "zeros, denormals and the largest floats are finite");
   EXPECT(rs_ray_valid(1.0f, 2.0f, 3.0f, 0.0f, 0.0f, 0.0f), "a zero direction is a finite one");
   const float bad[] = {inf, -inf, nan, snan, neg_nan};
   for (float b : bad)
      for (int at = 0; at < 6; ++at) {
         float v[6] = {1.0f, 2.0f, 3.0f, 0.5f, 0.5f, 0.5f};
         v[at] = b;
         EXPECT(!rs_ray_valid(v[0], v[1], v[2], v[3], v[4], v[5]), "component %d = %08x is refused", at, (unsigned)(b != b ? 0x7fc00000u : 0x7f800000u));
      }
   const float max_dist = 20.0f;
   EXPECT(rs_tmax_valid(max_dist, max_dist), "tmax = max_dist");
   EXPECT(rs_tmax_valid(std::nextafter(max_dist, 0.0f), max_dist), "tmax just below max_dist");
   EXPECT(!rs_tmax_valid(std::nextafter(max_dist, inf), max_dist), "tmax just above max_dist");
   EXPECT(rs_tmax_valid(0.0f, max_dist) && rs_tmax_valid(-1.0f, max_dist) && rs_tmax_valid(denorm, max_dist) && rs_tmax_valid(-big, max_dist), "short, negative and denormal lengths");
   EXPECT(!rs_tmax_valid(nan, max_dist) && !rs_tmax_valid(snan, max_dist) && !rs_tmax_valid(inf, max_dist) && !rs_tmax_valid(-inf, max_dist), "NaN and infinite lengths");
   EXPECT(!rs_tmax_valid(1.0f, nan) && rs_tmax_valid(big, inf), "a NaN max_dist admits nothing, an infinite one every finite length");
   // the host path's predicate (ray_query_check before this header: std::isfinite, tmax <= max_dist), value for value
   const float probe[] = {0.0f, -0.0f, denorm, neg_denorm, 1.0f, -1.0f, 19.999998f, 20.0f, 20.000002f, big, -big, inf, -inf, nan, snan, neg_nan};
   for (float x : probe) {
      EXPECT(rs_finite(x) == (bool)std::isfinite(x), "rs_finite (%a)", (double)x);
      EXPECT(rs_tmax_valid(x, max_dist) == (std::isfinite(x) && x <= max_dist), "rs_tmax_valid (%a)", (double)x);
   }
   EXPECT(MDH_RS_BAD_BITS == 0x7fc00000u && bits(MDH_RS_BAD_BITS) != bits(MDH_RS_BAD_BITS), "the answer of a refused ray is the quiet NaN");
   EXPECT(MDH_RAY_STREAM_REFILL_DEFAULT >= MDH_RS_REFILL_MIN && MDH_RAY_STREAM_REFILL_DEFAULT <= MDH_RS_REFILL_MAX && MDH_RS_REFILL_MAX == MDH_RS_WAVE, "the default threshold is one the option takes");
}

int main()
{
   check_hand_out();
   check_predicate();
   if (g_fail) { printf("ray_stream_check: %d failures\n", g_fail); return 1; }
   printf("ray_stream_check: ok\n");
   return 0;
}
