// tests/hostlogic/sketch_plan_check.cpp -- mm_sketch_plan.h (the sketch kernels' LDS layouts, the fast kernel's geometry, the route of a
// batch) on the host.  Built with -fsanitize=address,undefined and run by tests/test_sketch_plan.py.
//
//   sketch_plan_check    prints one row per plan of the grid below,
//                          K sl20 s L tabBytes | ok useFast spill stream SL threads HT QC wantFast HTH ldsFast ldsHard
//                        (the rows tests/golden/sketch_plan_rows.txt recorded from the planner as it stood inside mm_sketch.hip), then checks
//                        the two layouts over the same grid and every fragment length K .. min(L, 70000): "ok <what>" per check that
//                        passed, "FAIL ..." (with a non-zero status) for one that did not
#include <cstdio>
#include <initializer_list>
#include "../../mashmap_amd/csrc/mm_sketch_plan.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const int Ks[] = {1, 16, 19, 21, 32, 33, 49, 64};
static const int Ss[] = {1, 40, 130, 310, 498, 1279, 1280, 1998, 4000, 8190};
template <class F> static void grid(F&& f) {
  for (const int K : Ks)
    for (int sl20 = 0; sl20 <= ((K == 16 || K == 19 || K == 21) ? 1 : 0); sl20++)   // mm_check_params plans without strips of 20, the launcher with them where they are built
      for (const int s : Ss)
        for (const int L : {K, 64, 500, 1000, 5000, 10000, 20000, 60000, 262143, 262144, 450000, 3000000}) f(K, sl20 != 0, s, L, sketch_table_bytes(K));
}

// regions in order, each [begin, end) with the alignment the kernel relies on -- 16 for the tables (copied as uint4), the staged words,
// the queues and the keys (8-byte entries behind 16-byte rounded regions), the natural one of its words for what lies behind the
// occupancy words, whose number need not be even; returns the end of the last
struct Region { const char* name; size_t at, bytes, align; };
static size_t in_order(const char* what, int K, int s, int len, std::initializer_list<Region> rs) {
  size_t end = 0;
  for (const Region& r : rs) {
    CHECK(r.at == end, "%s K %d s %d len %d: %s begins at %zu, the region before it ends at %zu", what, K, s, len, r.name, r.at, end);
    CHECK(r.at % r.align == 0, "%s K %d s %d len %d: %s at %zu is not a multiple of %zu", what, K, s, len, r.name, r.at, r.align);
    end = r.at + r.bytes;
  }
  return end;
}

static void fast_layout(int K, int s, int len, const SketchPlan& P, size_t tabBytes, size_t& prev) {
  const int waves = P.g.threads / 64;
  const SkFastLayout y = sketch_fast_layout(tabBytes, len, P.g.HT, MM_SK_PAD, P.g.QC, waves);
  const size_t up = (size_t)((len + 15) / 16 + 4) * 4, upM = (size_t)((len + 31) / 32 + 3) * 4;
  const size_t end = in_order("fast", K, s, len, {
    {"tabs", y.tabs, tabBytes, 16}, {"sW", y.sW, mm_sk_up16(up), 16}, {"sM", y.sM, mm_sk_up16(upM), 16},
    {"qH", y.qH, (size_t)P.g.QC * waves * 8, 16}, {"qM", y.qM, (size_t)y.QTOT * 4, 16},
    {"key", y.key, (size_t)(y.NS + 2 * MM_SK_GUARD) * 8, 16}, {"occW", y.occW, (size_t)y.nOcc * 8, 8}, {"meta", y.meta, (size_t)y.NS * 4, 4},
    {"occP", y.occP, mm_sk_up16((size_t)y.nOcc * 4), 4}, {"qCnt", y.qCnt, 64, 4}, {"dup", y.dup, (size_t)MM_SK_DUPCAP * 4, 4}, {"counters", y.counters, 16, 4}});
  CHECK(end == y.bytes, "fast K %d s %d len %d: bytes %zu, regions end at %zu", K, s, len, y.bytes, end);
  CHECK(y.NS == P.g.HT + MM_SK_PAD && y.NS % 64 == 0 && y.nOcc * 64 == y.NS, "fast K %d s %d: NS %d", K, s, y.NS);
  // the queue words double as the list of occupied slots: at most the load limit, HT * 5 / 8, of them -- and hold the waves' queues
  CHECK(y.QTOT >= P.g.HT * 5 / 8 + 1 && y.QTOT >= P.g.QC * waves && y.QTOT % 4 == 0, "fast K %d s %d: QTOT %d for HT %d, %d x %d", K, s, y.QTOT, P.g.HT, P.g.QC, waves);
  // the staged words reach the last strip's window: 4 words from the strip's first, for strips of 16 and of 20 positions
  const int n = len - K + 1, lastB0 = (n - 1) / P.g.SL * P.g.SL;
  CHECK(K > 32 || (lastB0 >> 4) + 3 < y.nW, "fast K %d s %d len %d: strip at base %d reads past %d staged words", K, s, len, lastB0, y.nW);
  CHECK(y.bytes >= prev, "fast K %d s %d len %d: %zu bytes, %zu at the length before", K, s, len, y.bytes, prev);
  prev = y.bytes;
  // what k_hash_only carves: the same front, whatever the table and the queues are
  const SkFastLayout h = sketch_fast_layout(tabBytes, len, 0, 0, 0, 0);
  CHECK(h.tabs == y.tabs && h.sW == y.sW && h.nW == y.nW && h.sM == y.sM, "fast K %d s %d len %d: the front moves with the table", K, s, len);
}

static void hard_layout(int K, int s, int len, const SketchPlan& P, size_t tabBytes, size_t& prev) {
  const SkHardLayout y = sketch_hard_layout(tabBytes, len, P.HTH, MM_SK_PADH, P.spill, P.stream);
  const size_t up = P.stream ? 0 : (size_t)((len + 15) / 16 + 3) * 4, upM = P.stream ? 0 : (size_t)((len + 31) / 32 + 2) * 4;
  const size_t arr = P.spill ? 0 : (size_t)y.NS * 4;
  const size_t end = in_order("hard", K, s, len, {
    {"tabs", y.tabs, tabBytes, 16}, {"sW", y.sW, mm_sk_up16(up), 16}, {"sM", y.sM, mm_sk_up16(upM), 16},
    {"key", y.key, (size_t)(y.NS + 2 * MM_SK_GUARD) * 8, 16}, {"occW", y.occW, (size_t)y.nOcc * 8, 8},
    {"first", y.first, arr, 4}, {"last", y.last, arr, 4}, {"sum", y.sum, arr, 4},
    {"occP", y.occP, mm_sk_up16((size_t)y.nOcc * 4), 4}, {"counters", y.counters, 16, 4}});
  CHECK(end == y.bytes, "hard K %d s %d len %d: bytes %zu, regions end at %zu", K, s, len, y.bytes, end);
  CHECK(y.NS == P.HTH + MM_SK_PADH && y.NS % 64 == 0 && y.nOcc * 64 == y.NS, "hard K %d s %d: NS %d", K, s, y.NS);
  CHECK(P.HTH * 5 / 8 >= 2 * s, "hard K %d s %d: load limit %d of HT %d", K, s, P.HTH * 5 / 8, P.HTH);
  const int n = len - K + 1, lastStrip = (n - 1) >> 4;
  CHECK(P.stream || K > 32 || lastStrip + 2 < y.nW, "hard K %d s %d len %d: strip %d reads past %d staged words", K, s, len, lastStrip, y.nW);
  CHECK(y.bytes >= prev, "hard K %d s %d len %d: %zu bytes, %zu at the length before", K, s, len, y.bytes, prev);
  prev = y.bytes;
}

int main() {
  grid([](int K, bool sl20, int s, int L, size_t tabBytes) {
    const SketchPlan P = sketch_plan(K, s, L, tabBytes, sl20);
    printf("%d %d %d %d %zu | %d %d %d %d %d %d %d %d %d %d %zu %zu\n", K, (int)sl20, s, L, tabBytes, (int)P.ok, (int)P.useFast, (int)P.spill, (int)P.stream,
           P.g.SL, P.g.threads, P.g.HT, P.g.QC, P.g.wantFast, P.HTH, P.ldsFast, P.ldsHard);
  });
  long layouts = 0;
  grid([&](int K, bool sl20, int s, int L, size_t tabBytes) {
    const SketchPlan P = sketch_plan(K, s, L, tabBytes, sl20);
    // what the launch claims, from the same struct at the longest fragment
    const size_t atMaxFast = sketch_fast_layout(tabBytes, L, P.g.HT, MM_SK_PAD, P.g.QC, P.g.threads / 64).bytes;
    CHECK(atMaxFast == P.ldsFast, "K %d s %d L %d: fast layout %zu, plan %zu", K, s, L, atMaxFast, P.ldsFast);
    // (a streaming launch is sized as the spilled layout of an empty fragment, staging words included; the kernel's carve stages none)
    const size_t atMaxHard = P.stream ? sketch_hard_layout(tabBytes, 0, P.HTH, MM_SK_PADH, true, false).bytes : sketch_hard_layout(tabBytes, L, P.HTH, MM_SK_PADH, P.spill, false).bytes;
    CHECK(atMaxHard == P.ldsHard, "K %d s %d L %d: hard layout %zu, plan %zu", K, s, L, atMaxHard, P.ldsHard);
    CHECK(P.ok == (P.ldsHard <= MM_SK_LDS_LIMIT) && (!P.useFast || P.ldsFast <= MM_SK_LDS_LIMIT), "K %d s %d L %d: a launch beyond the LDS", K, s, L);
    CHECK(!P.useFast || (P.g.HT + MM_SK_PAD <= MM_SK_SLOT_LIMIT && L < MM_SK_DUP_POS_LIMIT), "K %d s %d L %d: the duplicate list's fields", K, s, L);
    CHECK(!P.stream || P.spill, "K %d s %d L %d: streaming without the spilled table", K, s, L);
    const int top = L < 70000 ? L : 70000;
    size_t prevF = 0, prevH = 0;
    for (int len = K; len <= top; len++) {
      if (P.useFast) fast_layout(K, s, len, P, tabBytes, prevF);
      if (P.ok) hard_layout(K, s, len, P, tabBytes, prevH);
      layouts++;
    }
    // the carve at any length the batch holds stays inside the launch's claim
    if (P.useFast && top >= K) CHECK(prevF <= P.ldsFast, "K %d s %d L %d: fast carve %zu beyond the launch's %zu", K, s, L, prevF, P.ldsFast);
    if (P.ok) {
      const size_t atL = sketch_hard_layout(tabBytes, L, P.HTH, MM_SK_PADH, P.spill, P.stream).bytes;
      CHECK(prevH <= atL && atL <= P.ldsHard, "K %d s %d L %d: hard carve %zu / %zu beyond the launch's %zu", K, s, L, prevH, atL, P.ldsHard);
    }
  });
  if (!failures) printf("ok layouts %ld\n", layouts);

  // the parameter classes of mm_create
  {
    const int before = failures;
    CHECK(sketch_check_params(19, 130, 5000, 8190, 65535).cls == MM_SKP_FITS, "the default parameters");
    CHECK(sketch_check_params(19, 4000, 40000, 8190, 65535).cls == MM_SKP_FITS, "every fragment on the hard list");
    CHECK(sketch_check_params(19, 8190, 5000, 8190, 65535).cls == MM_SKP_REFUSED && sketch_check_params(19, 8190, 5000, 8190, 65535).ldsBytes == 226272, "the table of the exact path beyond a CU's LDS");
    CHECK(sketch_check_params(19, 8191, 100000, 8190, 65535).cls == MM_SKP_BEYOND_LDS && sketch_check_params(19, 65535, 100000, 8190, 65535).cls == MM_SKP_BEYOND_LDS, "beyond the LDS kernels");
    CHECK(sketch_check_params(19, 65536, 100000, 8190, 65535).cls == MM_SKP_BEYOND_MAX, "beyond every kernel");
    grid([](int K, bool sl20, int s, int L, size_t tabBytes) {
      if (sl20) return;
      const SketchPlan P = sketch_plan(K, s, L, tabBytes, false);
      const SketchParamCheck c = sketch_check_params(K, s, L, 8190, 65535);
      CHECK(c.cls == (P.ok ? MM_SKP_FITS : MM_SKP_REFUSED) && c.ldsBytes == P.ldsHard, "K %d s %d L %d: class %d, %zu bytes", K, s, L, (int)c.cls, c.ldsBytes);
    });
    if (failures == before) printf("ok params\n");
  }
  // the fast cut: no cut where every position is wanted, below half the range elsewhere, never falling with `want`
  {
    const int before = failures;
    for (const int n : {1, 2, 63, 64, 482, 982, 4982, 9982, 59982, 262125}) {
      uint64_t prev = 0;
      for (int want = 1; want <= 9000; want++) {
        const uint64_t T = mm_sketch_fast_cut(want, n);
        CHECK((T == MM_SK_HASH_MAX) == (want >= n), "want %d n %d", want, n);
        CHECK(T == MM_SK_HASH_MAX || T <= (1ull << 63), "want %d n %d: T %llx", want, n, (unsigned long long)T);
        CHECK(T >= prev, "want %d n %d: the cut falls", want, n);
        prev = T;
      }
    }
    if (failures == before) printf("ok fast cut\n");
  }
  if (failures) { printf("FAIL %d checks\n", failures); return 1; }
  printf("ok all\n");
  return 0;
}
