// tests/hostlogic/sketch_drain_check.cpp -- the two decisions k_sketch_fast takes on the high words of its hashes, on the host: the cut as a
// multiple of 2^32 (mm_sketch_cut_hiword, mm_sketch_cut_last_hi) and the drain's keep / drop of a queued position (mm_sk_drain_keep), both
// from the head of mm_sketch_dev.h.  Built with -fsanitize=address,undefined and run by tests/test_sketch_drain.py.
//
//   sketch_drain_check   "cut K s: <plans> plans, <moved> moved" per (K, s), "ok <what>" per check that passed, "FAIL ..." (with a non-zero
//                        status) for one that did not
#include <cstdio>
#include <vector>
#include "../../mashmap_amd/csrc/mm_sketch_dev.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the cut: for every fragment of n positions the fast kernel can be given, the high-word cut lets through what the old one did ----
static void cuts() {
  for (const int K : {16, 19, 21, 32})
    for (const int s : {1, 40, 130, 310, 498, 1998}) {
      long plans = 0, moved = 0;
      for (int n = 1; n <= 25000; n++) {
        const SketchPlan P = sketch_plan(K, s, n + K - 1, sketch_table_bytes(K), K == 16 || K == 19 || K == 21);
        if (!P.ok || !P.useFast) continue;
        plans++;
        const uint64_t T = mm_sketch_fast_cut(P.g.wantFast, n), C = mm_sketch_cut_hiword(T);
        CHECK(C >= T, "K %d s %d n %d: cut %llx below %llx", K, s, n, (unsigned long long)C, (unsigned long long)T);
        CHECK((T == MM_SK_HASH_MAX) == (C == MM_SK_HASH_MAX), "K %d s %d n %d: %llx -> %llx, one of them is `no cut`", K, s, n, (unsigned long long)T, (unsigned long long)C);
        if (C == MM_SK_HASH_MAX) { CHECK(mm_sketch_cut_last_hi(C) == 0xFFFFFFFFu, "K %d s %d n %d: no cut, yet a high word fails", K, s, n); continue; }
        CHECK((uint32_t)C == 0u && C - T < (1ull << 32), "K %d s %d n %d: %llx -> %llx is not the next multiple of 2^32", K, s, n, (unsigned long long)T, (unsigned long long)C);
        if ((uint32_t)T == 0u) CHECK(C == T, "K %d s %d n %d: low word zero, %llx -> %llx", K, s, n, (unsigned long long)T, (unsigned long long)C);
        else moved++;
        // h < C  <=>  h.hi <= last
        const uint32_t last = mm_sketch_cut_last_hi(C);
        CHECK((((uint64_t)last << 32) | 0xFFFFFFFFull) < C && ((uint64_t)last + 1ull) << 32 >= C, "K %d s %d n %d: last passing high word %x under %llx", K, s, n, last, (unsigned long long)C);
      }
      printf("cut %d %d: %ld plans, %ld moved\n", K, s, plans, moved);
    }
  // the corners the planner does not reach
  CHECK(mm_sketch_cut_hiword(0xFFFFFFFF00000001ull) == MM_SK_HASH_MAX && mm_sketch_cut_hiword(0xFFFFFFFF00000000ull) == 0xFFFFFFFF00000000ull, "rounding past 2^64 is `no cut`");
  CHECK(mm_sketch_cut_hiword(1ull) == (1ull << 32) && mm_sketch_cut_last_hi(1ull << 32) == 0u, "the smallest cut");
  if (!failures) printf("ok cuts\n");
}

// ---- the drain: keep <=> the position has a k-mer (pos < n) without an N, which the strip loop's `ok` bit said per position before ----
template <int K>
static void drain_case(int len, const std::vector<int>& nAt, long& kept, long& dropped) {
  const int n = len - K + 1;
  std::vector<uint8_t> isN((size_t)len + 200, 1);                 // the bases behind the fragment are somebody else's: all N here
  for (int i = 0; i < len; i++) isN[i] = 0;
  for (const int i : nAt) if (i >= 0 && i < len) isN[i] = 1;
  const int nM = (len + 31) / 32 + 3;                             // SkFastLayout::nM
  std::vector<uint32_t> words(nM, 0u);
  bool any = false;
  for (int i = 0; i < nM * 32; i++) if (isN[i]) { words[i >> 5] |= 1u << (i & 31); if (i < len) any = true; }
  for (int pos = 0; pos < len + 64; pos++) {
    bool want = pos < n;
    for (int i = 0; want && i < K; i++) if (isN[pos + i]) want = false;
    const bool got = mm_sk_drain_keep<K>((uint32_t)pos, (uint32_t)(n > 0 ? n : 0), words.data());
    CHECK(got == want, "K %d len %d pos %d (first N %d of %zu): keep %d, want %d", K, len, pos, nAt.empty() ? -1 : nAt[0], nAt.size(), (int)got, (int)want);
    if (!any) CHECK(mm_sk_drain_keep<K>((uint32_t)pos, (uint32_t)(n > 0 ? n : 0), nullptr) == want, "K %d len %d pos %d without a mask", K, len, pos);
    (want ? kept : dropped)++;
  }
}
template <int K>
static void drain() {
  long kept = 0, dropped = 0;
  for (const int len : {K - 1, K, K + 1, K + 19, K + 20, 63, 64, 65, 96, 97, 128, 131, 200}) {
    if (len < K - 1) continue;
    drain_case<K>(len, {}, kept, dropped);
    for (int i = 0; i < len; i++) {
      drain_case<K>(len, {i}, kept, dropped);                                          // one N at every base: first and last base of every window
      if (i % 7 == 0) {
        drain_case<K>(len, {i, i + K}, kept, dropped);                                 // a clean window between two
        drain_case<K>(len, {i, i + 31, i + 32, i + 33}, kept, dropped);                // across a mask word
        drain_case<K>(len, {i, i + 1, i + 2, i + 64, i + 65}, kept, dropped);          // a run, and two words on
      }
    }
  }
  CHECK(kept > 1000 && dropped > 1000, "K %d: %ld kept, %ld dropped", K, kept, dropped);
  if (!failures) printf("ok drain %d: %ld kept, %ld dropped\n", K, kept, dropped);
}

int main() {
  cuts();
  drain<16>(); drain<19>(); drain<20>(); drain<21>(); drain<32>(); drain<33>(); drain<34>(); drain<40>(); drain<49>(); drain<63>(); drain<64>();
  return failures ? 1 : 0;
}
