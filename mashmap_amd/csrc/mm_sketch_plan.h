// mashmap_amd/csrc/mm_sketch_plan.h -- what the query-side sketch kernels (mm_sketch.hip, mm_sketch_global.hip, mm_sketch_large.hip) decide
// in plain numbers before and while they run: the constants of their tables, the two cuts, the LDS layout of k_sketch_fast and
// k_sketch_hard -- ONE carve each, which the kernel takes its pointers from at the fragment's length and the launcher sizes the workgroup
// with at the batch's longest fragment --, the fast kernel's geometry, the route a batch takes (fast / all-hard / spilled / non-power-of-two
// table / stream) and the class of a parameter set.  Plain C++17 without HIP types: shared by the launchers, the kernels and the CPU test
// (tests/hostlogic/sketch_plan_check.cpp), which checks the layouts' properties and the plans against recorded rows.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MM_SK_HD __host__ __device__ __forceinline__
#else
#define MM_SK_HD inline
#endif

#define MM_SK_HASH_MAX 0xFFFFFFFFFFFFFFFFULL   // MM_HASH_MAX of mm_device.h: "no cut"

#define MM_SK_PAD 64               // spill slots behind the ordered tables (no wrap-around): fast kernel
#define MM_SK_PADH 256             // hard kernel
#define MM_SK_DUPCAP 256           // repeat occurrences a fast-kernel fragment may defer (more: the hard kernel takes the fragment)
#define MM_SK_GUARD 4              // always-empty slots on either side of the table: the ranking reads windows of that many neighbours
#define MM_SK_SLOT_LIMIT 8192      // the fast kernel's duplicate list names a slot in 13 bits ...
#define MM_SK_DUP_POS_LIMIT (1 << 18)   // ... and a position in 18 (with the strand bit between them)
#define MM_SK_LDS_LIMIT ((size_t)160 * 1024)   // a CU's LDS (gfx950) ...
#define MM_SK_LDS_UNIT ((size_t)1280)          // ... handed out in units of this many bytes
#define MM_SK_TABLE_BYTES 3072     // sizeof(MMTables), the strip hashers' tables for k-mers of 1..15 and 33..64 bases ...
#define MM_SK_PROD_TABLE_BYTES 9216   // ... and sizeof(MMProdTables), for 16..32 (mm_sketch.hip asserts both)
MM_SK_HD size_t sketch_table_bytes(int K) { return (K >= 16 && K <= 32) ? MM_SK_PROD_TABLE_BYTES : MM_SK_TABLE_BYTES; }

// ---- the cuts ---------------------------------------------------------------------------------------------------------------------
// The canonical hash is the smaller of two uniform 64-bit values, so P[h < T] ~ 2T / 2^64.  Any T gives the exact sketch as long as s
// distinct hashes survive it, which every kernel counts; MM_SK_HASH_MAX = no cut.
// The LDS kernels: T where `want` (> s, FastGeom::wantFast) of a fragment's n k-mer positions are expected to survive.  In float, as it
// always was: the value decides which fragments go to the hard list.
MM_SK_HD uint64_t mm_sketch_fast_cut(int want, int n) {
  return ((uint32_t)want >= (uint32_t)n) ? MM_SK_HASH_MAX : (uint64_t)((float)want / (float)(2 * n) * 18446744073709551616.0f);
}
// The global-memory kernels (k_sketch_global, k_sketch_large): T where s + 5 sqrt(s) + 64 are expected, in double.
MM_SK_HD double mm_sketch_want(int s) { return (double)s + 5.0 * sqrt((double)s) + 64.0; }
MM_SK_HD uint64_t mm_sketch_cut(int s, int n) {
  const double want = mm_sketch_want(s);
  return want >= (double)n ? MM_SK_HASH_MAX : (uint64_t)(want / (2.0 * (double)n) * 18446744073709551616.0);
}

// ---- LDS layouts ------------------------------------------------------------------------------------------------------------------
// Byte offsets from the start of the workgroup's dynamic LDS, in the order of the regions; `bytes` = the end of the last one.  The
// offsets up to and including the keys are multiples of 16 (tabBytes is one: the tables are copied as uint4); behind the occupancy words
// (8 bytes each, an odd number of them for some tables) they are multiples of 8, which is all the 4-byte words there need.  A layout
// grows with `len` and with nothing else the kernel sees per fragment, so the carve at a fragment's length never exceeds the launch's,
// sized at the longest (sketch_plan_check.cpp sweeps it).
MM_SK_HD size_t mm_sk_up16(size_t b) { return (b + 15) / 16 * 16; }
// words of the fast kernel's position queue: the per-wave queues, but at least the table's load limit (the memory lists the occupied slots later)
MM_SK_HD int sketch_fast_queue_total(int QC, int nWaves, int HT) { const int a = QC * nWaves, b = HT * 5 / 8 + 1; return ((a > b ? a : b) + 3) & ~3; }

struct SkFastLayout {          // k_sketch_fast; k_hash_only claims [0, sM): tables and staged code words
  int nW, nM;                  // staged code words (incl. 4 words of run-off for the last strip's window) and N-mask words (incl. 3)
  int NS, nOcc, QTOT;          // table slots HT + PAD (a multiple of 64), occupancy words, words of qM
  size_t tabs, sW, sM;         // hasher tables (copied as uint4), staged words
  size_t qH, qM;               // per-wave queues: hashes (8 B), pos << 1 | strand (QTOT words: later the list of occupied slots)
  size_t key;                  // MM_SK_GUARD guard slots, NS keys, MM_SK_GUARD guard slots (8 B each)
  size_t occW, meta, occP, qCnt, dup, counters, bytes;
};
MM_SK_HD SkFastLayout sketch_fast_layout(size_t tabBytes, int len, int HT, int PAD, int QC, int nWaves) {
  SkFastLayout y;
  y.nW = (len + 15) / 16 + 4; y.nM = (len + 31) / 32 + 3;
  y.NS = HT + PAD; y.nOcc = y.NS >> 6; y.QTOT = sketch_fast_queue_total(QC, nWaves, HT);
  size_t off = 0;
  y.tabs = off; off += tabBytes;
  y.sW = off; off += mm_sk_up16((size_t)y.nW * 4);
  y.sM = off; off += mm_sk_up16((size_t)y.nM * 4);
  y.qH = off; off += (size_t)QC * nWaves * 8;
  y.qM = off; off += (size_t)y.QTOT * 4;
  y.key = off; off += (size_t)(y.NS + 2 * MM_SK_GUARD) * 8;
  y.occW = off; off += (size_t)y.nOcc * 8;
  y.meta = off; off += (size_t)y.NS * 4;
  y.occP = off; off += mm_sk_up16((size_t)y.nOcc * 4);
  y.qCnt = off; off += 64;
  y.dup = off; off += (size_t)MM_SK_DUPCAP * 4;
  y.counters = off; off += 16;
  y.bytes = off;
  return y;
}

struct SkHardLayout {          // k_sketch_hard
  int nW, nM;                  // staged code words (incl. 3 words of run-off for the last strip) and N-mask words (incl. 2); none when streaming
  int NS, nOcc;
  size_t tabs, sW, sM, key, occW;
  size_t first, last, sum;     // NS int32 each; empty under `spill` (the arrays live in HBM scratch)
  size_t occP, counters, bytes;
};
MM_SK_HD SkHardLayout sketch_hard_layout(size_t tabBytes, int len, int HT, int PAD, bool spill, bool stream) {
  SkHardLayout y;
  y.nW = stream ? 0 : (len + 15) / 16 + 3; y.nM = stream ? 0 : (len + 31) / 32 + 2;
  y.NS = HT + PAD; y.nOcc = y.NS >> 6;
  const size_t arr = spill ? 0 : (size_t)y.NS * 4;
  size_t off = 0;
  y.tabs = off; off += tabBytes;
  y.sW = off; off += mm_sk_up16((size_t)y.nW * 4);
  y.sM = off; off += mm_sk_up16((size_t)y.nM * 4);
  y.key = off; off += (size_t)(y.NS + 2 * MM_SK_GUARD) * 8;
  y.occW = off; off += (size_t)y.nOcc * 8;
  y.first = off; off += arr;
  y.last = off; off += arr;
  y.sum = off; off += arr;
  y.occP = off; off += mm_sk_up16((size_t)y.nOcc * 4);
  y.counters = off; off += 16;
  y.bytes = off;
  return y;
}

// ---- the fast kernel's geometry ---------------------------------------------------------------------------------------------------
// for fragments of up to maxLen bases: positions per thread, threads, table and queue sizes
struct FastGeom { int SL, threads, HT, QC, wantFast; size_t lds; };
inline FastGeom sketch_fast_geom(int K, int s, int maxLen, size_t tabBytes, bool sl20Built) {
  FastGeom g;
  // survivors the fast kernel aims for: s + 4.2 sqrt(s) (their count is ~Poisson, so s stays about 4 sigma away): fewer = less queue /
  // table work and less LDS, more fragments redone by k_sketch_hard (measured, profiles/r02v_sketch_geometry.txt: 0.007 % of random
  // fragments at s = 130, 0.008 % at 310, 0.02 % at 498, at 44 ns each).
  g.wantFast = (int)(s + 4.2 * sqrt((double)s) + 0.999);
  int n = maxLen - K + 1; if (n < 1) n = 1;
  // positions per thread: 16, or 20 where that fills whole waves better (the workgroup's critical path is ceil(waves / 4 SIMDs) strips)
  auto wavesFor = [&](int SL) { int st = (n + SL - 1) / SL; int w = (st + 63) / 64; return w < 1 ? 1 : (w > 16 ? 16 : w); };
  g.SL = 16;
  if (sl20Built && 20 + K - 1 <= 48) {
    const int w16 = wavesFor(16), w20 = wavesFor(20);
    const int c16 = ((w16 + 3) / 4) * 16, c20 = ((w20 + 3) / 4) * 20;
    if (c20 < c16 || (c20 == c16 && w20 < w16)) g.SL = 20;
  }
  g.threads = wavesFor(g.SL) * 64;
  const int nWaves = g.threads / 64;
  // a wave queues the survivors of its 64 threads' strips: their expectation + qsig standard deviations; the table has htf slots per
  // wanted survivor (load limit = 5/8 of them).  The kernel's table phases wait on LDS latency and are hidden by the other workgroups
  // of the CU, whose number the LDS footprint decides (MM_SK_LDS_UNIT, MM_SK_LDS_LIMIT): the roomy geometry is kept unless a
  // tighter one lets one more workgroup in (s = 130: 7 instead of 6, s = 310: 5 instead of 4, s = 498: 4 instead of 3 -- 49 -> 42 ms per
  // 1.6 M fragments there).
  int nStrips = (n + g.SL - 1) / g.SL; if (nStrips < 1) nStrips = 1;
  const int passes = (nStrips + g.threads - 1) / g.threads;
  double ex = 64.0 * passes * g.SL * (double)g.wantFast / (double)n; if (ex > g.wantFast) ex = g.wantFast;
  auto shape = [&](double htf, double qsig) {
    int HT = (int)(htf * g.wantFast + 63) / 64 * 64; if (HT < 256) HT = 256;
    g.HT = HT;
    g.QC = ((int)(ex + qsig * sqrt(ex) + 8.0) + 3) & ~3;
    g.lds = sketch_fast_layout(tabBytes, maxLen, g.HT, MM_SK_PAD, g.QC, nWaves).bytes;
    const size_t alloc = (g.lds + MM_SK_LDS_UNIT - 1) / MM_SK_LDS_UNIT * MM_SK_LDS_UNIT;
    return (int)(MM_SK_LDS_LIMIT / alloc);          // workgroups a CU holds
  };
  const double cand[3][2] = {{2.4, 6.0}, {2.2, 6.0}, {2.2, 5.0}};
  int best = 0, bestWg = shape(cand[0][0], cand[0][1]);
  for (int i = 1; i < 3; i++) { const int wg = shape(cand[i][0], cand[i][1]); if (wg > bestWg) { bestWg = wg; best = i; } }
  (void)shape(cand[best][0], cand[best][1]);
  return g;
}
// hard kernel's table: the load limit, 5/8 of it, stays >= 2 s (the window [s, limit] the cut must hit is an octave wide); no larger
// than that needs, because its LDS sets how many listed fragments a CU works on at once (s = 130: 4 workgroups)
inline int sketch_ht_hard(int s) { const int w = (s * 16 + 4) / 5; int p = 1; while (p < (w < 1024 ? 1024 : w)) p <<= 1; return p; }
// ... and the smallest table (not a power of two) that keeps that load limit
inline int sketch_ht_hard_tight(int s) { return (((s * 16 + 4) / 5) + 63) / 64 * 64; }

// ---- the route --------------------------------------------------------------------------------------------------------------------
// How the two sketch kernels are run for (k, s, fragment length): the fast kernel when its geometry fits (LDS, table slots that fit the
// slot field of its duplicate list, positions that fit the position field), otherwise every fragment goes down the hard list; the hard
// kernel with its whole table in LDS when that fits, otherwise with the first / last / strand-sum arrays spilled to HBM scratch and, if the
// power-of-two table still does not fit, the smallest table that keeps its load limit (5/8) at 2 s.  stream: the staged fragment is what
// does not fit (a whole contig as one fragment under --noSplit) -- the exact kernel reads its words from global memory instead, and the
// launch is sized as the spilled layout of an empty fragment (the kernel's own carve stages nothing then: 32 bytes less).
// ok == false: not even that fits (ldsHard says how much it would take).
struct SketchPlan { bool ok, useFast, spill, stream = false; FastGeom g; int HTH; size_t ldsFast, ldsHard; };
inline SketchPlan sketch_plan(int K, int s, int maxLen, size_t tabBytes, bool sl20Built) {
  const size_t lim = MM_SK_LDS_LIMIT;
  SketchPlan P;
  P.g = sketch_fast_geom(K, s, maxLen, tabBytes, sl20Built);
  P.ldsFast = P.g.lds;
  P.useFast = P.ldsFast <= lim && P.g.HT + MM_SK_PAD <= MM_SK_SLOT_LIMIT && maxLen < MM_SK_DUP_POS_LIMIT;
  auto hard = [&](int len, bool spill) { return sketch_hard_layout(tabBytes, len, P.HTH, MM_SK_PADH, spill, false).bytes; };
  P.HTH = sketch_ht_hard(s);
  P.ldsHard = hard(maxLen, false);
  P.spill = P.ldsHard > lim;
  if (P.spill) {
    P.ldsHard = hard(maxLen, true);
    if (P.ldsHard > lim) { P.HTH = sketch_ht_hard_tight(s); P.ldsHard = hard(maxLen, true); }
  }
  if (P.ldsHard > lim) {
    P.stream = true;
    P.HTH = sketch_ht_hard(s);
    P.ldsHard = hard(0, true);
    if (P.ldsHard > lim) { P.HTH = sketch_ht_hard_tight(s); P.ldsHard = hard(0, true); }
  }
  P.ok = P.ldsHard <= lim;
  return P;
}

// ---- parameter sets ---------------------------------------------------------------------------------------------------------------
// What mm_create makes of (kmerSize, sketchSize, segLength) before anything is built: the LDS kernels hold it; no LDS kernel holds the
// sketch (beyond ldsMaxSketch = MM_LDS_MAX_SKETCH: the global-memory sketch kernels and the literal L2 kernels take every fragment);
// beyond maxSketch = MM_MAX_SKETCH (seeds are numbered in 16 bits); or refused, with the LDS the exact kernel's smallest form would take.
enum SketchParamClass : int { MM_SKP_FITS = 0, MM_SKP_BEYOND_LDS = 1, MM_SKP_BEYOND_MAX = 2, MM_SKP_REFUSED = 3 };
struct SketchParamCheck { SketchParamClass cls; size_t ldsBytes; };
inline SketchParamCheck sketch_check_params(int K, int s, int segLength, int ldsMaxSketch, int maxSketch) {
  if (s > maxSketch) return {MM_SKP_BEYOND_MAX, 0};
  if (s > ldsMaxSketch) return {MM_SKP_BEYOND_LDS, 0};
  const SketchPlan P = sketch_plan(K, s, segLength, sketch_table_bytes(K), false);
  return {P.ok ? MM_SKP_FITS : MM_SKP_REFUSED, P.ldsHard};
}

// ---- the global-memory kernels' scratch ---------------------------------------------------------------------------------------------
// entries of a workgroup's slice of the sort scratch: a power of two >= the longest fragment's positions ...
inline int64_t sketch_scratch_slice(int maxFragLen) { int64_t slice = 2; while (slice < maxFragLen) slice <<= 1; return slice; }
// ... and as many workgroups as ~8 GiB of scratch allow
inline int64_t sketch_scratch_grid_cap(int64_t slice, size_t entryBytes) { const int64_t g = ((int64_t)8 << 30) / (slice * (int64_t)entryBytes); return g < 1 ? 1 : g; }
