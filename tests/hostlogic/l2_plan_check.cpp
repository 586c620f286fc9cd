// tests/hostlogic/l2_plan_check.cpp -- mm_l2_plan.h (the LDS geometry of the split L2 route and its chunk planner) on the host.  Built with
// -fsanitize=address,undefined and run by tests/test_l2_plan.py.
//
//   l2_plan_check        prints "step <s> ..." for every sketch size at which a field of the geometry changes, "ok <what>" per check that
//                        passed and "FAIL ..." (with a non-zero status) for one that did not
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../mashmap_amd/csrc/mm_l2_plan.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const size_t LIM = 163840;      // a CU's LDS
static const int MAX_S = 8190;         // MM_LDS_MAX_SKETCH

// ---- geometry: the expected side restates what mm_launch_l2 worked out inline before the header existed ------------------------------
static void geometry() {
  L2Geom prev{};
  int steps = 0;
  for (int s = 1; s <= MAX_S; s++) {
    const L2Geom g = mm_l2_geom(s);
    const int JB = s > 2046 ? 13 : 11;
    const int lpwN = JB == 11 ? 64 : ((size_t)(s + 2) * 32 <= 160 * 1024 ? 32 : 16);
    const int lpwW = JB == 11 ? ((size_t)(s + 2) * 128 <= 160 * 1024 ? 64 : 32) : ((size_t)(s + 2) * 32 <= 160 * 1024 ? 16 : 8);
    CHECK(g.ldsLoc <= LIM && g.ldsNarrow <= LIM && g.ldsWide <= LIM, "s %d: LDS %zu / %zu / %zu", s, g.ldsLoc, g.ldsNarrow, g.ldsWide);
    CHECK(mm_l2_geom_fits(s), "s %d", s);
    CHECK(g.wpb == 1 || g.wpb == 2 || g.wpb == 4, "s %d: wpb %d", s, g.wpb);
    CHECK(g.NB >= 256 && g.NB >= s && (g.NB & (g.NB - 1)) == 0 && (g.NB == 256 || g.NB / 2 < s), "s %d: NB %d", s, g.NB);
    CHECK(g.JB == JB && g.JB == mm_l2_jb(s), "s %d: JB %d", s, g.JB);
    CHECK(g.lpwN == lpwN && g.lpwW == lpwW, "s %d: lpw %d / %d, expected %d / %d", s, g.lpwN, g.lpwW, lpwN, lpwW);
    CHECK(g.ldsWide == (size_t)(s + 2) * lpwW * 2 && g.ldsNarrow == ((((size_t)(s + 2) * lpwN) + 15) & ~(size_t)15), "s %d: sweep LDS %zu / %zu", s, g.ldsNarrow, g.ldsWide);
    CHECK(g.ldsLoc == mm_locate_lds_per_wave(s, g.NB) * g.wpb, "s %d: ldsLoc %zu", s, g.ldsLoc);
    CHECK(g.wpb == 4 || mm_locate_lds_per_wave(s, g.NB) * g.wpb * 2 > LIM, "s %d: wpb %d could be twice that", s, g.wpb);
    CHECK(g.initStride == ((s + 3) & ~1) && g.initStride >= s + 2 && g.initStride % 2 == 0, "s %d: initStride %d", s, g.initStride);
    if (s == 1 || g.JB != prev.JB || g.NB != prev.NB || g.wpb != prev.wpb || g.lpwN != prev.lpwN || g.lpwW != prev.lpwW) {
      printf("step %d JB %d NB %d wpb %d lpwN %d lpwW %d ldsLoc %zu ldsNarrow %zu ldsWide %zu\n", s, g.JB, g.NB, g.wpb, g.lpwN, g.lpwW, g.ldsLoc, g.ldsNarrow, g.ldsWide);
      if (s > 1) {                                                       // the size below a step is where the step's reason peaks
        const L2Geom b = mm_l2_geom(s - 1);
        printf("below %d ldsLoc %zu ldsNarrow %zu ldsWide %zu\n", s, b.ldsLoc, b.ldsNarrow, b.ldsWide);
      }
      steps++;
    }
    prev = g;
  }
  const L2Geom top = mm_l2_geom(MAX_S);
  printf("top %d ldsLoc %zu ldsNarrow %zu ldsWide %zu\n", MAX_S, top.ldsLoc, top.ldsNarrow, top.ldsWide);
  if (!failures) printf("ok geometry %d steps\n", steps);
}

// ---- chunk planner against a linear one ------------------------------------------------------------------------------------------------
static std::vector<L2Chunk> linear(const std::vector<int64_t>& off, int64_t budget, int64_t& maxOps) {
  const int nC = (int)off.size() - 1;
  std::vector<L2Chunk> out;
  maxOps = off[nC];
  if (off[nC] <= budget || nC <= 1) { out.push_back(L2Chunk{0, nC, 0}); return out; }
  maxOps = 0;
  int c0 = 0;
  while (c0 < nC) {
    int c1 = c0 + 1;
    while (c1 < nC && off[c1 + 1] - off[c0] <= budget) c1++;
    out.push_back(L2Chunk{c0, c1 - c0, off[c0]});
    maxOps = std::max(maxOps, off[c1] - off[c0]);
    c0 = c1;
  }
  return out;
}

static int ceil_log2(int n) { int b = 0; while ((1 << b) < n) b++; return b; }

// one vector of per-candidate counts and one budget: the planner's chunks against the linear planner's, and an offAt that fails
static void plan_case(const std::vector<int64_t>& cnt, int64_t budget, std::mt19937_64& rng, long& nChunked, long& nOversize) {
  const int nC = (int)cnt.size();
  std::vector<int64_t> off(nC + 1, 0);
  for (int i = 0; i < nC; i++) off[i + 1] = off[i] + cnt[i];
  int64_t wantMax = 0;
  const std::vector<L2Chunk> want = linear(off, budget, wantMax);
  std::vector<int> callsAt;                                              // offAt calls, by the number of chunks complete when they came
  std::vector<L2Chunk> got;
  long calls = 0;
  auto offAt = [&](int i, int64_t& v) -> int {
    CHECK(i > 0 && i <= nC, "offAt(%d) of %d candidates", i, nC);
    calls++; callsAt.push_back((int)got.size());
    v = off[i];
    return 0;
  };
  int64_t gotMax = -1;
  const int rc = mm_l2_plan_chunks(nC, off[nC], budget, offAt, got, gotMax);
  CHECK(rc == 0, "rc %d", rc);
  CHECK(got.size() == want.size() && gotMax == wantMax, "nC %d budget %lld: %zu chunks of at most %lld, expected %zu of %lld", nC, (long long)budget, got.size(), (long long)gotMax, want.size(), (long long)wantMax);
  int at = 0;
  for (size_t i = 0; i < got.size() && i < want.size(); i++) {
    const L2Chunk& g = got[i];
    CHECK(g.c0 == want[i].c0 && g.n == want[i].n && g.base == want[i].base, "chunk %zu: %d + %d at %lld", i, g.c0, g.n, (long long)g.base);
    CHECK(g.c0 == at && (g.n >= 1 || nC == 0) && g.base == off[g.c0], "chunk %zu does not follow its predecessor", i);
    at = g.c0 + g.n;
    if (at > nC) break;
    const int64_t ops = off[at] - g.base;
    CHECK(ops <= budget || g.n == 1, "chunk %zu: %lld entries in %d candidates, budget %lld", i, (long long)ops, g.n, (long long)budget);
    if (ops > budget) nOversize++;
  }
  CHECK(at == nC, "the chunks end at %d of %d", at, nC);
  if (got.size() > 1) {
    nChunked++;
    std::vector<int> per(got.size(), 0);
    for (int k : callsAt) if (k < (int)per.size()) per[k]++;
    for (size_t i = 0; i < per.size(); i++) CHECK(per[i] <= ceil_log2(nC) + 2, "chunk %zu took %d reads, nC %d", i, per[i], nC);
  } else CHECK(calls == 0, "one chunk after %ld reads", calls);
  if (calls > 0) {                                                       // the k-th read fails: its code comes back
    const long k = 1 + (long)(rng() % (uint64_t)calls);
    long seen = 0;
    std::vector<L2Chunk> part; int64_t m = 0;
    const int rcF = mm_l2_plan_chunks(nC, off[nC], budget, [&](int i, int64_t& v) -> int { if (++seen == k) return -7; v = off[i]; return 0; }, part, m);
    CHECK(rcF == -7 && seen == k, "a failing read: rc %d after %ld of %ld reads", rcF, seen, k);
    CHECK(part.size() <= got.size(), "%zu chunks before the failing read", part.size());
  }
}

static void planner() {
  std::mt19937_64 rng(20240611);
  long nCases = 0, nChunked = 0, nOversize = 0;
  for (int it = 0; it < 600; it++) {
    const int nC = it < 8 ? it + 1 : 1 + (int)(rng() % (it % 3 == 0 ? 5000 : 300));
    const int kind = it % 4;                                             // 0: small counts with zeros, 1: wide spread, 2: mostly zero, 3: a few giants
    std::vector<int64_t> cnt(nC);
    for (auto& x : cnt) {
      if (kind == 0) x = (int64_t)(rng() % 8);
      else if (kind == 1) x = (int64_t)(rng() % 100000);
      else if (kind == 2) x = rng() % 10 ? 0 : (int64_t)(rng() % 5000);
      else x = rng() % 50 ? (int64_t)(rng() % 200) : (int64_t)1000000 + (int64_t)(rng() % 1000);
    }
    int64_t total = 0, largest = 0;
    for (int64_t x : cnt) { total += x; largest = std::max(largest, x); }
    const int64_t budgets[] = {0, 1, largest > 1 ? largest - 1 : 1, largest, largest + 1, total / 7 + 1, total / 2, total - 1, total, total + 1, (int64_t)(rng() % (uint64_t)(total + 2))};
    for (int64_t b : budgets) { if (b < 0) continue; plan_case(cnt, b, rng, nChunked, nOversize); nCases++; }
  }
  plan_case({5}, 1, rng, nChunked, nOversize);                           // nC == 1 beyond the budget: one chunk, no read
  plan_case({0}, 0, rng, nChunked, nOversize);
  plan_case({3, 3, 3, 3}, 12, rng, nChunked, nOversize);                 // totalOps <= budget
  plan_case({3, 3, 3, 3}, 11, rng, nChunked, nOversize);
  CHECK(nChunked > 1000 && nOversize > 1000, "%ld chunked plans, %ld chunks of one candidate beyond the budget", nChunked, nOversize);
  if (!failures) printf("ok planner %ld cases %ld chunked %ld oversize\n", nCases + 4, nChunked, nOversize);
}

int main() {
  geometry();
  planner();
  return failures ? 1 : 0;
}
