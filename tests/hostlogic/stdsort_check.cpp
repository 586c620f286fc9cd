// tests/hostlogic/stdsort_check.cpp -- mashmap_amd/csrc/mm_stdsort.h (std::sort of libstdc++ restated over an array of ids) beside the
// toolchain's std::sort: both sort the ids 0 .. n-1 by key[id] through a comparator that logs every call (a, b); the two logs and the
// two final permutations must be identical.  Stand-alone, built by tests/test_stdsort.py under -fsanitize=address,undefined.
//
// Sizes: every n in 0 .. 600 and some up to 5000.  Keys: all equal; 2, 3 and 17 distinct values in random and in interleaved order;
// sorted, reversed, organ-pipe; random distinct.  One more input per size in ADVERSARY_SIZES is built with McIlroy's adversary ("A Killer
// Adversary for Quicksort", 1999) run against std::sort and frozen as values: it drives the partitions into the depth limit, so the heap
// fallback (__partial_sort) is compared too; the header counts the times it got there (MM_STDSORT_COUNT_FALLBACK).
//
// Prints "allequal n N first F" for N = 17, 20, 33 (the element an all-ties sort puts first: the representative of a chain of N),
// "fallback inputs I taken T", "inputs I comparisons C" and "differences D"; exit status 1 when anything differs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#define MM_STDSORT_COUNT_FALLBACK 1
#include "../../mashmap_amd/csrc/mm_stdsort.h"

typedef std::vector<std::pair<int, int>> Log;
static long g_bad = 0, g_inputs = 0, g_comparisons = 0;

// -> the id the sorts put first (-1 for n == 0)
static int one(const std::vector<int>& key, const char* what) {
  const int n = (int)key.size();
  std::vector<uint16_t> a(n), b(n);
  std::iota(a.begin(), a.end(), (uint16_t)0); std::iota(b.begin(), b.end(), (uint16_t)0);
  Log la, lb;
  std::sort(a.begin(), a.end(), [&](uint16_t x, uint16_t y) { la.emplace_back(x, y); return key[x] < key[y]; });
  mm_std_sort(b.data(), n, [&](uint16_t x, uint16_t y) { lb.emplace_back(x, y); return key[x] < key[y]; });
  g_inputs++; g_comparisons += (long)la.size();
  if (a != b || la != lb) {
    if (g_bad++ < 10) {
      size_t d = 0;
      while (d < la.size() && d < lb.size() && la[d] == lb[d]) d++;
      std::fprintf(stderr, "%s n %d: permutations %s, comparisons %zu / %zu, first difference at call %zu\n", what, n, a == b ? "equal" : "DIFFER", la.size(), lb.size(), d);
    }
  }
  for (int i = 1; i < n; i++) if (key[b[i]] < key[b[i - 1]]) { if (g_bad++ < 10) std::fprintf(stderr, "%s n %d: not sorted\n", what, n); break; }
  return n ? (int)b[0] : -1;
}

// McIlroy's adversary against std::sort on n elements, frozen: the keys it ends up with
static std::vector<int> adversary(int n) {
  std::vector<int> val(n, n);                  // n: "gas", not yet decided
  int nsolid = 0, candidate = 0;
  std::vector<int> ids(n);
  std::iota(ids.begin(), ids.end(), 0);
  std::sort(ids.begin(), ids.end(), [&](int x, int y) {
    if (val[x] == n && val[y] == n) { if (x == candidate) val[x] = nsolid++; else val[y] = nsolid++; }
    if (val[x] == n) candidate = x; else if (val[y] == n) candidate = y;
    return val[x] < val[y]; });
  for (int& v : val) if (v == n) v = nsolid++;
  return val;
}

static void all_inputs(int n, std::mt19937_64& rng) {
  std::vector<int> key(n, 7);
  one(key, "all_equal");
  for (int d : {2, 3, 17}) {
    for (int i = 0; i < n; i++) key[i] = (int)(rng() % (uint64_t)d);
    one(key, "few_random");
    for (int i = 0; i < n; i++) key[i] = i % d;
    one(key, "few_interleaved");
  }
  for (int i = 0; i < n; i++) key[i] = i;
  one(key, "sorted");
  for (int i = 0; i < n; i++) key[i] = n - i;
  one(key, "reversed");
  for (int i = 0; i < n; i++) key[i] = i < n / 2 ? i : n - 1 - i;
  one(key, "organ_pipe");
  for (int i = 0; i < n; i++) key[i] = i;
  std::shuffle(key.begin(), key.end(), rng);
  one(key, "random_distinct");
}

int main() {
  std::mt19937_64 rng(20241019);
  for (int n = 0; n <= 600; n++) all_inputs(n, rng);
  for (int n : {601, 777, 1000, 1023, 1024, 1025, 2048, 3001, 4096, 5000}) all_inputs(n, rng);
  for (int n : {17, 20, 33}) std::printf("allequal n %d first %d\n", n, one(std::vector<int>(n, 1), "all_equal"));
  long fbInputs = 0;
  const long before = mm_stdsort_fallbacks;
  for (int n : {100, 257, 512, 600, 1000, 5000}) { one(adversary(n), "adversary"); fbInputs++; }
  std::printf("fallback inputs %ld taken %ld\n", fbInputs, mm_stdsort_fallbacks - before);
  std::printf("inputs %ld comparisons %ld\n", g_inputs, g_comparisons);
  std::printf("differences %ld\n", g_bad);
  return g_bad ? 1 : 0;
}
