// mashmap_amd/csrc/mm_sketch_large_plan.h -- what k_sketch_large (mm_sketch_large.hip, MM_OPT_SKETCH_LARGE) decides in integers: the cut
// below which a fragment's hashes go into the sort, the tile of the sort that lives in LDS, the padded sort length, and the bitonic
// network as a schedule of rounds -- sweeps over the whole slice in HBM while the partner distance is a tile or more, and rounds in which
// every tile is loaded into LDS once and takes all the steps whose partners lie inside it.  Plain C++17 without HIP types: shared by the
// kernel and by the CPU test (tests/hostlogic/sketch_large_check.cpp), which runs the schedule serially against std::sort.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "mm_sketch_plan.h"

#ifdef __HIPCC__
#define MM_SKL_HD __host__ __device__
#else
#define MM_SKL_HD
#endif

#define MM_SKL_HASH_MAX MM_SK_HASH_MAX          // MM_HASH_MAX of mm_device.h: "no cut", and the hash of a padding entry

// ---- the cut ------------------------------------------------------------------------------------------------------------------------
// Only hashes below T go into the sort, T placed where s + 5 sqrt(s) + 64 of the ~2n uniform strand hashes of a fragment of n k-mer
// positions are expected; MM_SKL_HASH_MAX = no cut, when that many are all there are: mm_sketch_want / mm_sketch_cut of
// mm_sketch_plan.h, which k_sketch_global calls too.

// ---- tile and sort geometry -------------------------------------------------------------------------------------------------------------
#define MM_SKL_TILE 4096                        // entries of the sort one tile holds in LDS (a power of two)
#define MM_SKL_ENTRY_BYTES 16                   // (hash, position << 1 | strand bit, padding)
#define MM_SKL_TABLE_BYTES 9216                 // the larger of the strip hashers' tables (MMProdTables; mm_sketch_large.hip asserts it)
#define MM_SKL_STATIC_BYTES (1024 * 4 + 16)     // the emission's per-thread counts and the cursor (what the compiler reports: 4 112)
#define MM_SKL_LDS_LIMIT (160 * 1024)           // a CU's LDS (gfx950)
static_assert((MM_SKL_TILE & (MM_SKL_TILE - 1)) == 0 && MM_SKL_TILE >= 2, "the tile is a power of two");
// 9 216 + 65 536 + 4 112 = 78 864 B: two workgroups of k_sketch_large share a CU's 163 840 B
static_assert(MM_SKL_TABLE_BYTES + MM_SKL_TILE * MM_SKL_ENTRY_BYTES + MM_SKL_STATIC_BYTES == 78864, "k_sketch_large: tables + one tile + static LDS");
static_assert(2 * (MM_SKL_TABLE_BYTES + MM_SKL_TILE * MM_SKL_ENTRY_BYTES + MM_SKL_STATIC_BYTES) <= MM_SKL_LDS_LIMIT, "two workgroups of k_sketch_large per CU");

// the padded sort length: the smallest power of two >= nSurv, at least 2
MM_SKL_HD inline int64_t mm_skl_n2(int64_t nSurv) { int64_t N2 = 2; while (N2 < nSurv) N2 <<= 1; return N2; }

// ---- the compare-exchange rule, stated once ----------------------------------------------------------------------------------------------
// Step (k2, j) of the bitonic network pairs entry i with its partner i ^ j; the pair is taken once, from its lower index (bit j of i
// clear), and ends ascending where (i & k2) == 0, descending elsewhere.  Pair p of the step (p = 0 .. N/2 - 1) has the lower index
// mm_skl_pair_low(p, j): p with a zero inserted at bit j.
MM_SKL_HD inline int64_t mm_skl_pair_low(int64_t p, int64_t j) { return ((p & ~(j - 1)) << 1) | (p & (j - 1)); }
MM_SKL_HD inline int64_t mm_skl_partner(int64_t i, int64_t j) { return i ^ j; }
// bLessA: the partner's entry sorts before entry i's.  True: the two swap.
MM_SKL_HD inline bool mm_skl_swaps(bool bLessA, int64_t i, int64_t k2) { return bLessA == ((i & k2) == 0); }

// ---- the schedule ----------------------------------------------------------------------------------------------------------------------
// The network over N2 entries (k2 = 2, 4 .. N2; j = k2/2 .. 1 inside each) as rounds, in order:
//   tileRound(k2lo, k2hi): every tile of `tile` entries (the whole array when N2 is smaller) is loaded once and takes the steps
//     mm_skl_tile_steps lists -- for every k2 in [k2lo, k2hi] the steps j = min(k2, tile)/2 .. 1, whose partners stay inside the tile --
//     and is stored back.  The opening round covers every k2 <= tile; each later one closes a single k2;
//   globalStep(k2, j): one sweep over all N2 entries with j >= tile.
// Returns the number of rounds.  N2 and tile are powers of two >= 2.
template <class G, class T>
MM_SKL_HD inline int mm_skl_schedule(int64_t N2, int64_t tile, G&& globalStep, T&& tileRound) {
  int rounds = 0;
  tileRound((int64_t)2, N2 < tile ? N2 : tile); rounds++;
  for (int64_t k2 = 2 * tile; k2 <= N2; k2 <<= 1) {
    for (int64_t j = k2 >> 1; j >= tile; j >>= 1) { globalStep(k2, j); rounds++; }
    tileRound(k2, k2); rounds++;
  }
  return rounds;
}
template <class S>
MM_SKL_HD inline void mm_skl_tile_steps(int64_t k2lo, int64_t k2hi, int64_t tile, S&& step) {
  for (int64_t k2 = k2lo; k2 <= k2hi; k2 <<= 1)
    for (int64_t j = (k2 < tile ? k2 : tile) >> 1; j > 0; j >>= 1) step(k2, j);
}
// rounds of the schedule, counted without running it
MM_SKL_HD inline int mm_skl_rounds(int64_t N2, int64_t tile) {
  return mm_skl_schedule(N2, tile, [](int64_t, int64_t) {}, [](int64_t, int64_t) {});
}
