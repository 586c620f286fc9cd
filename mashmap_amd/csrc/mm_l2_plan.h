// mashmap_amd/csrc/mm_l2_plan.h -- what the split L2 route (mm_launch_l2, mm_l2.hip) decides before it launches anything: the LDS geometry
// of k_l2_locate and the k_l2_sweep instances for a sketch size, and the cut of a batch's candidates into chunks whose located streams fit
// a budget.  Plain C++17 without HIP types: shared by the launcher, by k_l2_locate (mm_locate_lds_per_wave) and by the CPU test
// (tests/hostlogic/l2_plan_check.cpp), which sweeps every sketch size and checks the planner against a linear one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#ifdef __HIPCC__
#define MM_L2_HD __host__ __device__
#else
#define MM_L2_HD
#endif

#define MM_L2_LDS_LIMIT (160 * 1024)     // a CU's LDS (gfx950)

// width of the stream entries' sketch-position field: 11 bits for sketches of up to 2046 entries, 13 beyond
constexpr int mm_l2_jb(int s) { return s > 2046 ? 13 : 11; }

// LDS of one wave of k_l2_locate: sketch + sentinel (8 B each), their high words (4 B), NB + 1 bucket starts (2 B), strands (1 B)
MM_L2_HD constexpr static inline size_t mm_locate_lds_per_wave(int s, int NB) {
  const size_t b = (size_t)(s + 1) * 8 + (size_t)(s + 2) / 2 * 8 + (size_t)(NB + 4) * 2 + (((size_t)s + 15) & ~(size_t)15) + (((size_t)(s + 4) / 2 * 4 + 15) & ~(size_t)15);
  return (b + 15) & ~(size_t)15;
}

struct L2Geom {
  int JB;                    // mm_l2_jb(s)
  int NB;                    // buckets of k_l2_locate's query-sketch search
  int wpb;                   // its waves per workgroup
  size_t ldsLoc;             // its dynamic LDS
  int initStride;            // cells per row of the pre-load states: s + 2, rounded up to whole dwords
  int lpwN, lpwW;            // candidates per wave of the narrow (8-bit cells) and the wide (16-bit cells) sweep
  size_t ldsNarrow, ldsWide; // their dynamic LDS
};

constexpr L2Geom mm_l2_geom(int s) {
  L2Geom g{};
  g.JB = mm_l2_jb(s);
  // buckets of the query-sketch search: at least one per sketch entry (more buckets cost more to fill per candidate than the shorter
  // walks save: profiles/r02z_locate_buckets.txt)
  g.NB = 256; while (g.NB < s) g.NB <<= 1;
  // waves per workgroup: 4, fewer when four sketches + bucket tables would not fit a CU's LDS
  g.wpb = 4; while (g.wpb > 1 && mm_locate_lds_per_wave(s, g.NB) * g.wpb > MM_L2_LDS_LIMIT) g.wpb >>= 1;
  g.ldsLoc = mm_locate_lds_per_wave(s, g.NB) * g.wpb;
  g.initStride = (s + 3) & ~1;
  // candidates per wave of the sweeps (LPW): 64, fewer when the LDS state of 64 does not fit a CU -- 8-bit cells first, 16-bit cells
  // for the rare candidate whose 5-bit counters overflow
  // (JB == 11: always 64 lanes.  At s = 498 the state of 64 candidates is 32 KB, five waves per CU; 32 lanes per wave double the waves and
  // were measured slower all the same -- sweep 40.1 -> 55.7 ms at configs[4], profiles/NOTES.md round 5: the kernel is issue-bound even there)
  g.lpwN = g.JB == 11 ? 64 : ((size_t)(s + 2) * 32 <= MM_L2_LDS_LIMIT ? 32 : 16);
  g.lpwW = g.JB == 11 ? ((size_t)(s + 2) * 128 <= MM_L2_LDS_LIMIT ? 64 : 32) : ((size_t)(s + 2) * 32 <= MM_L2_LDS_LIMIT ? 16 : 8);
  g.ldsWide = (size_t)(s + 2) * g.lpwW * 2;                         // cells 0..S + one of padding, 16 bit
  g.ldsNarrow = (((size_t)(s + 2) * g.lpwN) + 15) & ~(size_t)15;    // 8 bit
  return g;
}
constexpr bool mm_l2_geom_fits(int s) {
  const L2Geom g = mm_l2_geom(s);
  return g.ldsLoc <= MM_L2_LDS_LIMIT && g.ldsNarrow <= MM_L2_LDS_LIMIT && g.ldsWide <= MM_L2_LDS_LIMIT;
}
// Every sketch size the split route sees (1..8190 = MM_LDS_MAX_SKETCH) fits a CU's LDS: wpb falls to 1 and lpwW to 8 before anything
// else gives.  Asserted at both sides of every step of the geometry; tests/hostlogic/l2_plan_check.cpp sweeps all of them.
static_assert(mm_l2_geom_fits(1) && mm_l2_geom_fits(256) && mm_l2_geom_fits(257) && mm_l2_geom_fits(512) && mm_l2_geom_fits(513), "L2 geometry: NB 256 -> 512 -> 1024");
static_assert(mm_l2_geom_fits(1024) && mm_l2_geom_fits(1025), "L2 geometry: NB 1024 -> 2048");
static_assert(mm_l2_geom_fits(1278) && mm_l2_geom_fits(1279), "L2 geometry: lpwW 64 -> 32 (163 840 B of wide cells at 1278)");
static_assert(mm_l2_geom_fits(2046) && mm_l2_geom_fits(2047), "L2 geometry: JB 11 -> 13, lpwN 64 -> 32, lpwW 32 -> 16");
static_assert(mm_l2_geom_fits(2048) && mm_l2_geom_fits(2049), "L2 geometry: NB 2048 -> 4096");
static_assert(mm_l2_geom_fits(2181) && mm_l2_geom_fits(2182), "L2 geometry: wpb 4 -> 2");
static_assert(mm_l2_geom_fits(4096) && mm_l2_geom_fits(4097), "L2 geometry: NB 4096 -> 8192");
static_assert(mm_l2_geom_fits(4366) && mm_l2_geom_fits(4367), "L2 geometry: wpb 2 -> 1 (163 840 B of k_l2_locate's tables at 4366)");
static_assert(mm_l2_geom_fits(5118) && mm_l2_geom_fits(5119), "L2 geometry: lpwN 32 -> 16, lpwW 16 -> 8 (163 840 B of cells at 5118)");
static_assert(mm_l2_geom_fits(8190), "L2 geometry: the largest LDS-resident sketch");

// ---------------------------------------------------------------------------------------------
// The located streams live in HBM only between the locate and the sweep kernels; a batch whose streams exceed the budget goes through the
// two in chunks of consecutive candidates.
struct L2Chunk { int c0, n; int64_t base; };     // candidates [c0, c0 + n), whose streams start at entry `base`

// Greedy: every chunk ends at the largest c1 with opOff[c1] - base <= budget, and holds at least one candidate.  offAt(i, v) sets
// v = opOff[i] for 0 < i <= nC (opOff[nC] = totalOps) and returns 0 or an error code, which ends the plan; it is asked about
// ceil(log2 nC) + 1 times per chunk.  Returns 0 with the chunks appended to `out` and the longest chunk's entries in maxChunkOps.
template <class OffAt>
int mm_l2_plan_chunks(int nC, int64_t totalOps, int64_t budget, OffAt&& offAt, std::vector<L2Chunk>& out, int64_t& maxChunkOps) {
  maxChunkOps = totalOps;
  if (totalOps <= budget || nC <= 1) { out.push_back(L2Chunk{0, nC, 0}); return 0; }
  maxChunkOps = 0;
  int c0 = 0; int64_t base = 0;
  while (c0 < nC) {
    int lo = c0 + 1, hi = nC;
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      int64_t v = 0; const int rc = offAt(mid, v); if (rc != 0) return rc;
      if (v - base <= budget) lo = mid; else hi = mid - 1;
    }
    int64_t end = 0; { const int rc = offAt(lo, end); if (rc != 0) return rc; }
    out.push_back(L2Chunk{c0, lo - c0, base});
    if (end - base > maxChunkOps) maxChunkOps = end - base;
    c0 = lo; base = end;
  }
  return 0;
}
