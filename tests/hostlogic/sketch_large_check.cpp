// tests/hostlogic/sketch_large_check.cpp -- mm_sketch_large_plan.h (the cut, the tile geometry and the sort schedule of k_sketch_large) on
// the host.  Built with -fsanitize=address,undefined and run by tests/test_sketch_large_plan.py.
//
//   sketch_large_check   runs the schedule serially, the way the kernel walks it (pairs by mm_skl_pair_low, tiles through a buffer of their
//                        own), for every N2 = 2 .. 2^18 at MM_SKL_TILE and at a tile of 8 entries, on three inputs each, against std::sort;
//                        prints "tile <MM_SKL_TILE>", "rounds <N2> <tile> <rounds> <global sweeps> <tile rounds>", "ok <what>" per check
//                        that passed and "FAIL ..." (with a non-zero status) for one that did not
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../mashmap_amd/csrc/mm_sketch_large_plan.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Ent { uint64_t h; uint32_t m; };
static bool ent_less(const Ent& a, const Ent& b) { return a.h != b.h ? a.h < b.h : a.m < b.m; }

struct Tally { int rounds = 0, sweeps = 0, tileRounds = 0; long steps = 0; };

// the kernel's walk of the schedule, one "thread"
static Tally run_schedule(std::vector<Ent>& e, int64_t tile) {
  const int64_t N2 = (int64_t)e.size();
  const int64_t TL = N2 < tile ? N2 : tile;
  std::vector<Ent> lds((size_t)TL);
  Tally t;
  int64_t lastK2 = 0, lastJ = 0;                     // the steps must come in the network's order: k2 ascending, j descending inside
  auto inOrder = [&](int64_t k2, int64_t j) {
    const bool ok = lastK2 == 0 ? (k2 == 2 && j == 1) : (lastJ > 1 ? (k2 == lastK2 && j == lastJ / 2) : (k2 == lastK2 * 2 && j == k2 / 2));
    CHECK(ok, "N2 %lld tile %lld: step (%lld, %lld) behind (%lld, %lld)", (long long)N2, (long long)tile, (long long)k2, (long long)j, (long long)lastK2, (long long)lastJ);
    lastK2 = k2; lastJ = j; t.steps++;
  };
  t.rounds = mm_skl_schedule(N2, tile,
    [&](int64_t k2, int64_t j) {
      t.sweeps++;
      CHECK(j >= tile && j < N2, "global step (%lld, %lld) at tile %lld", (long long)k2, (long long)j, (long long)tile);
      inOrder(k2, j);
      for (int64_t p = 0; p < N2 / 2; p++) {
        const int64_t i = mm_skl_pair_low(p, j), q = mm_skl_partner(i, j);
        CHECK(q == i + j && q < N2, "pair %lld of step j %lld: %lld, %lld", (long long)p, (long long)j, (long long)i, (long long)q);
        const Ent a = e[(size_t)i], b = e[(size_t)q];
        if (mm_skl_swaps(ent_less(b, a), i, k2)) { e[(size_t)i] = b; e[(size_t)q] = a; }
      }
    },
    [&](int64_t k2lo, int64_t k2hi) {
      t.tileRounds++;
      for (int64_t t0 = 0; t0 < N2; t0 += TL) {
        for (int64_t i = 0; i < TL; i++) lds[(size_t)i] = e[(size_t)(t0 + i)];
        const bool first = t0 == 0;
        mm_skl_tile_steps(k2lo, k2hi, tile, [&](int64_t k2, int64_t j) {
          CHECK(j < tile && j < TL && j >= 1, "tile step (%lld, %lld) at tile %lld", (long long)k2, (long long)j, (long long)tile);
          if (first) inOrder(k2, j);
          for (int64_t p = 0; p < TL / 2; p++) {
            const int64_t i = mm_skl_pair_low(p, j), q = mm_skl_partner(i, j);
            CHECK(i >= 0 && q == i + j && q < TL, "tile pair %lld of step j %lld: %lld, %lld of %lld", (long long)p, (long long)j, (long long)i, (long long)q, (long long)TL);   // one tile only
            const Ent a = lds[(size_t)i], b = lds[(size_t)q];
            if (mm_skl_swaps(ent_less(b, a), t0 + i, k2)) { lds[(size_t)i] = b; lds[(size_t)q] = a; }
          }
        });
        for (int64_t i = 0; i < TL; i++) e[(size_t)(t0 + i)] = lds[(size_t)i];
      }
    });
  return t;
}

static void schedule() {
  std::mt19937_64 rng(20260917);
  int sorts = 0;
  for (const int64_t tile : {(int64_t)8, (int64_t)MM_SKL_TILE}) {
    for (int lg = 1; lg <= 18; lg++) {
      const int64_t N2 = (int64_t)1 << lg;
      for (int kind = 0; kind < 3; kind++) {
        std::vector<Ent> e((size_t)N2);
        // random hashes out of a small range (runs of equal hashes, ordered by m) with padding entries at the end, as the kernel pads;
        // one hash with distinct m in random order; already sorted
        for (int64_t i = 0; i < N2; i++) {
          if (kind == 0) e[(size_t)i] = (i >= N2 - N2 / 5) ? Ent{MM_SKL_HASH_MAX, 0xFFFFFFFFu} : Ent{rng() % (uint64_t)(N2 / 3 + 2), (uint32_t)i};
          else if (kind == 1) e[(size_t)i] = Ent{77, (uint32_t)i};
          else e[(size_t)i] = Ent{(uint64_t)i / 3, (uint32_t)i};
        }
        if (kind == 1) std::shuffle(e.begin(), e.end(), rng);
        std::vector<Ent> exp = e;
        std::sort(exp.begin(), exp.end(), ent_less);
        const Tally t = run_schedule(e, tile);
        bool same = true;
        for (int64_t i = 0; i < N2 && same; i++) same = e[(size_t)i].h == exp[(size_t)i].h && e[(size_t)i].m == exp[(size_t)i].m;
        CHECK(same, "N2 %lld tile %lld input %d: not std::sort's order", (long long)N2, (long long)tile, kind);
        CHECK(t.steps == (long)lg * (lg + 1) / 2, "N2 %lld tile %lld: %ld steps", (long long)N2, (long long)tile, t.steps);
        CHECK(t.rounds == t.sweeps + t.tileRounds && t.rounds == mm_skl_rounds(N2, tile), "N2 %lld tile %lld: %d rounds", (long long)N2, (long long)tile, t.rounds);
        CHECK(mm_skl_n2(N2) == N2 && (N2 == 2 || mm_skl_n2(N2 - 1) == N2) && mm_skl_n2(N2 / 2 + 1) == N2, "mm_skl_n2 around %lld", (long long)N2);
        if (kind == 0 && (tile == MM_SKL_TILE || lg <= 6)) printf("rounds %lld %lld %d %d %d\n", (long long)N2, (long long)tile, t.rounds, t.sweeps, t.tileRounds);
        sorts++;
      }
    }
  }
  CHECK(mm_skl_n2(0) == 2 && mm_skl_n2(1) == 2 && mm_skl_n2(2) == 2 && mm_skl_n2(3) == 4, "mm_skl_n2 at the bottom");
  printf("tile %d\n", MM_SKL_TILE);
  if (!failures) printf("ok schedule %d sorts\n", sorts);
}

static void cut() {
  const int before = failures;
  long cases = 0;
  const int ns[] = {1, 2, 63, 64, 65, 70, 100, 2985, 8710, 8716, 8717, 8718, 9985, 23985, 39985, 99985, 199985, 1 << 20, 0x7fffffff};
  for (const int n : ns) {
    uint64_t prev = 0;
    for (int s = 1; s <= 66000; s += (s < 300 ? 1 : 7)) {
      const double want = (double)s + 5.0 * sqrt((double)s) + 64.0;
      const uint64_t T = mm_sketch_cut(s, n);
      CHECK((T == MM_SKL_HASH_MAX) == (want >= (double)n), "s %d n %d: T %llx", s, n, (unsigned long long)T);
      CHECK(T == MM_SKL_HASH_MAX || T < (1ull << 63), "s %d n %d: T %llx is half the range or more", s, n, (unsigned long long)T);
      CHECK(T == MM_SKL_HASH_MAX || T == (uint64_t)(want / (2.0 * (double)n) * 18446744073709551616.0), "s %d n %d: not k_sketch_global's expression", s, n);
      CHECK(T >= prev, "s %d n %d: the cut falls", s, n);
      CHECK(mm_sketch_want(s) == want, "s %d", s);
      prev = T; cases++;
    }
  }
  if (failures == before) printf("ok cut %ld cases\n", cases);
}

int main() {
  schedule();
  cut();
  if (failures) { printf("FAIL %d checks\n", failures); return 1; }
  printf("ok all\n");
  return 0;
}
