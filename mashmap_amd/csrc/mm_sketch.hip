// mashmap_amd/csrc/mm_sketch.hip -- a1 (pack) and a4 (query-fragment sketch) kernels.
//
//   k_pack2bit          makeUpperCaseAndValidDNA            src/map/include/commonFunc.hpp:97
//   k_sketch_fast / k_sketch_hard  CommonFunc::sketchSequence          src/map/include/commonFunc.hpp:183-288
//
// One workgroup per query fragment.  Integer-ALU bound (2 x MurmurHash3_x64_128 per base); the
// packed input is only 0.25 B/bp (+0.125 B/bp N mask).  See DESIGN.md for the roofline terms.
#include "mm_internal.h"
#include "mm_device.h"
#include "mm_sketch_dev.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>

// ---------------------------------------------------------------------------------------------
// k_pack2bit: ASCII -> 2 bit/base + 1 bit/base N mask.  One thread per 32 output bases.
// Reads are laid out at 32-base aligned offsets so code words (16 bases) and mask words (32 bases)
// of different reads never share a word.
// ---------------------------------------------------------------------------------------------
__global__ void k_pack2bit(const uint8_t* __restrict__ ascii, const int64_t* __restrict__ srcOff,
                           const int64_t* __restrict__ packOff, const int32_t* __restrict__ readLen, int nReads,
                           int64_t nChunks, uint32_t* __restrict__ bases2, uint32_t* __restrict__ nmask,
                           uint32_t* __restrict__ readHasN) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < nChunks; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b0 = c * 32;
    int lo = 0, hi = nReads;                        // last read with packOff <= b0
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (packOff[mid] <= b0) lo = mid; else hi = mid; }
    const int r = lo;
    const int64_t local = b0 - packOff[r];
    const int len = readLen[r];
    uint32_t wlo = 0, whi = 0, nm = 0;
    if (local < len) {
      const uint8_t* src = ascii + srcOff[r] + local;
      const int cnt = (len - local) < 32 ? (int)(len - local) : 32;
      for (int i = 0; i < cnt; i++) {
        const uint32_t ch = src[i] & 0xDFu;         // a-z -> A-Z (only letters can land on A/C/G/T)
        const bool ok = (ch == 'A') | (ch == 'C') | (ch == 'G') | (ch == 'T');
        const uint32_t code = ok ? (((ch >> 1) ^ (ch >> 2)) & 3u) : 0u;   // A0 C1 G2 T3
        if (i < 16) wlo |= code << (2 * i); else whi |= code << (2 * (i - 16));
        nm |= (ok ? 0u : 1u) << i;
      }
    }
    bases2[2 * c] = wlo; bases2[2 * c + 1] = whi;
    nmask[c] = nm;
    if (nm) atomicOr(&readHasN[r], 1u);
  }
}

// ---------------------------------------------------------------------------------------------
// LDS table that de-duplicates the survivors of the threshold filter AND orders them.
//   The home slot is a monotone function of the hash (hashes below the cut T are spread over
//   [0, HT)), collisions probe linearly WITHOUT wrap-around into `pad` spare slots.  Then
//     * every key of a cluster (maximal run of occupied slots) has its home inside the cluster,
//     * keys of an earlier cluster have a strictly smaller home, hence a strictly smaller hash,
//   so rank(key) = occupied slots before its cluster + keys of its own cluster that are smaller:
//   the table scan replaces compaction + sort.
// ---------------------------------------------------------------------------------------------
// (MM_SK_PAD, MM_SK_PADH, MM_SK_DUPCAP, MM_SK_GUARD and the LDS layouts: mm_sketch_plan.h; the cut's M / sh / home, SkCut: mm_sketch_dev.h)
static_assert(sizeof(MMTables) == MM_SK_TABLE_BYTES && sizeof(MMProdTables) == MM_SK_PROD_TABLE_BYTES, "mm_sketch_plan.h sizes the LDS with these tables");
static_assert(MM_SK_HASH_MAX == MM_HASH_MAX, "one value for `no cut`");
// slots of `counters`, the four LDS words each sketch table keeps beside itself (not mm_ctx::dCounters)
enum : int { MM_TC_KEYS = 0 /* distinct keys */, MM_TC_OVERFLOW = 1 /* load limit passed, spill area or duplicate list full */, MM_TC_OCCUPIED = 2 /* occupied slots */, MM_TC_DUPS = 3 /* deferred duplicates (fast kernel) */ };
struct SkTable : SkCut {          // the hard kernel's table: every occurrence is folded in with atomics as it is hashed
  uint64_t* key; int32_t* first; int32_t* last; int32_t* sum;
  uint32_t* counters;            // MM_TC_KEYS, MM_TC_OVERFLOW, MM_TC_OCCUPIED
  uint64_t* occW; uint32_t* occP; // occupancy bit words and their exclusive prefix counts
  uint32_t nSlots, maxLoad;

  // the number of distinct keys is kept in counters[MM_TC_KEYS] and the load limit flagged as it is passed: the kernel inserts straight from
  // the hash loop and must notice a flooded table early
  __device__ __forceinline__ void insert(uint64_t h, int pos, int st) {
    uint32_t slot = home(h);
    for (uint32_t probes = 1;; probes++) {
      // a flooded table (cut still too high) is abandoned early; looked at every 16th probe only, the volatile generic load is slow
      if ((probes & 15u) == 0 && ((volatile uint32_t*)counters)[MM_TC_OVERFLOW]) return;
      const unsigned long long prev = atomicCAS((unsigned long long*)&key[slot], (unsigned long long)MM_HASH_MAX,
                                                (unsigned long long)h);
      if (prev == MM_HASH_MAX) {
        if (atomicAdd(&counters[MM_TC_KEYS], 1u) >= maxLoad) atomicOr(&counters[MM_TC_OVERFLOW], 1u);
      }
      if (prev == MM_HASH_MAX || prev == h) {
        atomicMin(&first[slot], pos); atomicMax(&last[slot], pos); atomicAdd(&sum[slot], st);
        return;
      }
      if (++slot >= nSlots) { atomicOr(&counters[MM_TC_OVERFLOW], 1u); return; }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// k_sketch_hard<K>: the fragments k_sketch_fast gave up on -- tandem repeats, low complexity, N-rich -- exact for any input.
//   Survivors go straight from the hash loop into a larger table (duplicates collapse there, however many), and the cut T is
//   moved until s <= distinct <= load limit: first in proportion to the distinct count the previous cut produced (the fast
//   kernel leaves its own count in skCount[f] as the first hint), then by bisection once a cut has flooded the table.
// ---------------------------------------------------------------------------------------------
#define MM_SK_HINT_OVERFLOW 0xFFFFFFFFu   // skCount[f] of a listed fragment: a queue / table / duplicate list of the fast kernel overflowed
// SPILL: the first / last / strand-sum arrays of the table live in HBM scratch (`spill`: 3 x NS int32 per workgroup) instead of LDS --
// sketches beyond ~1500 entries, whose key table alone fills most of a CU's 160 KB (the reference's --dense derives sketchSize =
// 0.02 (1 + (1 - pi) / 0.05) (segLength - k): 1998 for --pi 80 -s 20000, parseCmdArgs.hpp:626-630).  Same atomics, slower memory; exact all the same.
template <int K, bool SPILL>
__device__ __forceinline__ void
mm_sketch_hard(unsigned char* smem, const int f, const uint4* __restrict__ gTabs, const uint32_t* __restrict__ bases2, const uint32_t* __restrict__ nmask,
               const DFrag* __restrict__ frags, const uint32_t* __restrict__ readHasN, int s, int wantFast, int HT, int PAD, int32_t* __restrict__ spill,
               const bool stream /* the fragment does not fit the LDS: its words are read from global memory as they are needed */,
               uint64_t* __restrict__ skHash, int2* __restrict__ skPos, int8_t* __restrict__ skStrand, uint32_t* __restrict__ skCount) {
  const DFrag fr = frags[f];
  const int len = fr.len;
  const int n = len - K + 1;                        // k-mer positions
  const int tid = threadIdx.x, nthr = blockDim.x;
  if (n <= 0) { if (tid == 0) skCount[f] = 0; return; }
  const bool hasN = readHasN[fr.readId] != 0;
  const uint32_t hint = skCount[f];                 // distinct survivors under the fast kernel's cut, or MM_SK_HINT_OVERFLOW

  // ---- LDS carve: sketch_hard_layout (mm_sketch_plan.h), which sized the launch at the longest fragment ----
  using Tabs = typename MMTabsFor<K>::type;
  const SkHardLayout lay = sketch_hard_layout(sizeof(Tabs), len, HT, PAD, SPILL, stream);
  const int nW = lay.nW, nM = lay.nM, NS = lay.NS, nOcc = lay.nOcc;   // NS: table slots (multiple of 64)
  Tabs* tabs = (Tabs*)(smem + lay.tabs);
  static_assert(sizeof(Tabs) % 16 == 0, "tables are copied in 16-byte pieces");
  for (int i = tid; i < (int)(sizeof(Tabs) / 16); i += nthr) ((uint4*)tabs)[i] = gTabs[i];   // visible after the first __syncthreads() below
  uint32_t* sW = (uint32_t*)(smem + lay.sW);
  uint32_t* sM = (uint32_t*)(smem + lay.sM);
  SkTable tab;
  tab.key = (uint64_t*)(smem + lay.key) + MM_SK_GUARD;   // MM_SK_GUARD always-empty slots on either side: the ranking reads windows
  tab.occW = (uint64_t*)(smem + lay.occW);
  if constexpr (SPILL) {
    int32_t* g = spill + (size_t)blockIdx.x * 3 * (size_t)NS;
    tab.first = g; tab.last = g + NS; tab.sum = g + 2 * (size_t)NS;
  } else {
    tab.first = (int32_t*)(smem + lay.first); tab.last = (int32_t*)(smem + lay.last); tab.sum = (int32_t*)(smem + lay.sum);
  }
  tab.occP = (uint32_t*)(smem + lay.occP);
  tab.counters = (uint32_t*)(smem + lay.counters);
  tab.nSlots = (uint32_t)NS; tab.maxLoad = (uint32_t)HT * 5u / 8u;

  // ---- stage the fragment, re-aligned so that LDS word j holds bases 16j..16j+15 ----
  const int64_t gw0 = fr.base >> 4; const int gsh = (int)(fr.base & 15) * 2;
  const int64_t gm0 = fr.base >> 5; const int gmsh = (int)(fr.base & 31);
  mm_sk_stage(sW, nW, bases2, gw0, gsh, tid, nthr);
  if (hasN) mm_sk_stage(sM, nM, nmask, gm0, gmsh, tid, nthr);
  // word j of the re-aligned fragment / of its N mask: from the LDS copy, or -- a fragment longer than the LDS (a whole contig under
  // --noSplit) -- straight from the packed batch, realigned on the fly (neighbouring strips share their words in the caches)
  auto wordAt = [&](int j) -> uint32_t {
    if (!stream) return sW[j];
    return mm_sk_word_at(bases2, gw0, gsh, j);
  };
  auto maskAt = [&](int j) -> uint32_t {
    if (!stream) return sM[j];
    return mm_sk_word_at(nmask, gm0, gmsh, j);
  };

  // Any cut gives the exact sketch as long as >= s distinct hashes survive it (checked below), so float estimates are enough.
  // `scaled(T, D)`: the cut under which 1.6 s distinct hashes are expected when T produced D (distinct counts grow with the cut
  // in proportion for all but pathological inputs; the loop below corrects those), at least twice T.
  auto scaled = [&](uint64_t T, uint32_t D) -> uint64_t {
    float r = 1.6f * (float)s / (float)(D ? D : 1u);
    if (r < 2.0f) r = 2.0f;
    const float t = (float)T * r;
    return t >= 1.8e19f ? MM_HASH_MAX : (uint64_t)t;
  };
  uint64_t T = mm_sketch_fast_cut(wantFast, n);     // the fast kernel's cut
  if (hint != MM_SK_HINT_OVERFLOW && T != MM_HASH_MAX) T = scaled(T, hint);
  uint64_t lo = 0, hi = MM_HASH_MAX; bool hiInf = true;   // bisection state (uniform across the block)
  const int nStrips = (n + 15) >> 4;
  uint32_t D = 0;

  for (int attempt = 0;; attempt++) {
    tab.set_cut(T, (uint32_t)HT);
    for (int i = tid; i < NS; i += nthr) { tab.key[i] = MM_HASH_MAX; tab.first[i] = 0x7fffffff; tab.last[i] = -1; tab.sum[i] = 0; }
    if (tid < MM_SK_GUARD) { tab.key[-1 - tid] = MM_HASH_MAX; tab.key[NS + tid] = MM_HASH_MAX; }
    if (tid < 4) tab.counters[tid] = 0;
    if constexpr (SPILL) __threadfence();                 // the spilled arrays' initial values, before other threads' atomics reach them
    __syncthreads();

    // ---- hash both strands of every k-mer ----
    const bool allPass = (T == MM_HASH_MAX);
    for (int strip = tid; strip < nStrips; strip += nthr) {
      // bit j: position strip*16+j exists and its k-mer holds no N
      const int rem = n - strip * 16;
      uint32_t ok = rem >= 16 ? 0xFFFFu : ((1u << rem) - 1u);
      if (hasN) ok &= ~mm_sk_strip_has_n<K>(strip, maskAt);
      auto onPos = [&](int j, uint64_t hf, uint64_t hr) {
        const int pos = strip * 16 + j;
        const uint64_t h = hf < hr ? hf : hr;
        bool pass = false;                          // nested ifs: the compiler keeps the three tests as exec masks
        if ((ok & (1u << j)) != 0) { if (hf != hr) { if (allPass || h < T) pass = true; } }
        if (pass) tab.insert(h, pos, hf < hr ? 1 : -1);
      };
      if constexpr (MMWideK<K>::value) {
        uint32_t ww[MMWideK<K>::NW];
#pragma unroll
        for (int i = 0; i < MMWideK<K>::NW; i++) ww[i] = wordAt(strip + i);
        mm_strip_hashes_wide<K>(ww, *tabs, onPos);
      } else mm_strip_hashes<K>(wordAt(strip), wordAt(strip + 1), wordAt(strip + 2), *tabs, onPos);
    }
    if constexpr (SPILL) __threadfence();                 // the atomics on the spilled arrays, before the ranking threads read them
    __syncthreads();

    // ---- occupancy words, their prefix counts, number of distinct keys ----
    mm_sk_occupancy(tab.key, tab.occW, tab.occP, NS, nOcc, tid, nthr, [&](int total) { tab.counters[MM_TC_OCCUPIED] = (uint32_t)total; });
    __syncthreads();

    D = tab.counters[MM_TC_OCCUPIED];
    const bool overflow = tab.counters[MM_TC_OVERFLOW] != 0;
    if (overflow) { hi = T; hiInf = false; }
    else if (D < (uint32_t)s && T != MM_HASH_MAX) { lo = T; }
    else break;
    T = hiInf ? scaled(T, D) : lo + (hi - lo) / 2;
    __syncthreads();
    if (attempt > 200) break;                       // cannot happen (bisection on 64 bits); keeps the loop bounded
  }

  // ---- rank every key inside its cluster; emit the s smallest, ascending (commonFunc.hpp:278-286) ----
  for (int slot = tid; slot < NS; slot += nthr) {
    const uint64_t k = tab.key[slot];
    if (k == MM_HASH_MAX) continue;
    int q;                                          // -> first slot of the cluster
    const uint32_t smaller = mm_sk_cluster_smaller(tab.key, slot, k, NS, q);
    const uint64_t below = tab.occW[q >> 6] & ((1ull << (q & 63)) - 1ull);
    const uint32_t rank = tab.occP[q >> 6] + (uint32_t)__popcll(below) + smaller;
    if (rank < (uint32_t)s) {
      const size_t o = (size_t)f * s + rank;
      skHash[o] = k;
      int vf, vl, vs;
      if constexpr (SPILL) {                          // written by device-scope atomics: read at the same scope, past the CU's L1
        vf = __hip_atomic_load(&tab.first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        vl = __hip_atomic_load(&tab.last[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        vs = __hip_atomic_load(&tab.sum[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else { vf = tab.first[slot]; vl = tab.last[slot]; vs = tab.sum[slot]; }
      skPos[o] = make_int2(vf, vl);
      skStrand[o] = mm_sk_strand(vs);
    }
  }
  if (tid == 0) skCount[f] = D < (uint32_t)s ? D : (uint32_t)s;
}

template <int K, bool SPILL>
__global__ void __launch_bounds__(1024)
k_sketch_hard(const uint4* __restrict__ gTabs, const uint32_t* __restrict__ bases2, const uint32_t* __restrict__ nmask,
              const DFrag* __restrict__ frags, const uint32_t* __restrict__ readHasN,
              const int32_t* __restrict__ fragList, const uint32_t* __restrict__ fragListCount, int s, int wantFast, int HT, int PAD, int32_t* __restrict__ spill, int stream,
              uint64_t* __restrict__ skHash, int2* __restrict__ skPos, int8_t* __restrict__ skStrand, uint32_t* __restrict__ skCount) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // the hard list's length stays on the device (no host round trip between the two kernels): a fixed grid walks it
  const uint32_t nList = *fragListCount;
  for (uint32_t i = blockIdx.x; i < nList; i += gridDim.x) {
    mm_sketch_hard<K, SPILL>(smem, fragList[i], gTabs, bases2, nmask, frags, readHasN, s, wantFast, HT, PAD, spill, stream != 0, skHash, skPos, skStrand, skCount);
    __syncthreads();                                // the next fragment reuses the LDS
  }
}

// every fragment on the hard list (sketches the fast kernel's LDS geometry cannot hold): no hint for the first cut
__global__ void __launch_bounds__(256)
k_sketch_all_hard(int nF, int32_t* __restrict__ hardList, uint32_t* __restrict__ hardCount, uint32_t* __restrict__ skCount) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f < nF) { hardList[f] = f; skCount[f] = MM_SK_HINT_OVERFLOW; }
  if (f == 0) *hardCount = (uint32_t)nF;
}

// ---------------------------------------------------------------------------------------------
// Fast sketch kernel, per fragment (one workgroup).  What paces it besides the hash loop is how many workgroups share a CU -- the
// table phases are LDS-latency bound and leave the VALU to whoever else is resident -- so the LDS footprint is kept small:
//   * a table slot is the 64-bit key plus ONE 32-bit word, the (position, strand) of the occurrence that claimed the slot.  Repeat
//     occurrences of a resident hash are rare outside repeats: they go on a short list, the slot gets a flag after the barrier, and
//     only flagged slots fold their list entries into first / last / strand sum when the sketch is written;
//   * the per-wave survivor queues hold the expected share of a wave plus six standard deviations, not a whole table's worth;
//   * SL positions per thread are chosen so that the threads fill whole waves (4 982 k-mers: 250 threads x 20 positions = 4 waves,
//     one per SIMD, instead of 312 x 16 = 5 waves of which two share a SIMD).
// A fragment that overflows any of it (queue, table, duplicate list) or keeps fewer than s distinct survivors goes to the hard list.
//
// The kernel is bound by VALU issue, not by waiting: at configs[1] (2 M fragments of 5 kbp, s = 130, k = 19) it issues vector instructions
// at the rate of the hash-only yardstick (SQ_INSTS_VALU per launch / kernel time: profiles/r14_13_configs1_pmc_SQ_INSTS_VALU.csv,
// r14_14_configs1_kernel_stats.csv),
//     k_hash_only<19,20>     22.0 G wave-instructions   35.3 ms   0.62 G / ms
//     k_sketch_fast<19,20>   26.3 G                     41.4 ms   0.64 G / ms        (k_l2_sweep 0.65, k_l2_locate 0.47, k_lookup_l1 0.41)
// so only fewer or cheaper vector instructions shorten it; one instruction per position is 0.156 G per launch, about 0.25 ms.  Hence the
// strip loop (onPos below) does per position only what decides whether the position is queued -- one v_min_u32 and one 32-bit compare on
// the high words of the two hashes -- and leaves the rest to the 3.6 % that pass (behind a wave-uniform branch) or, once per queued
// position, to the drain: which of the two hashes is the smaller, whether they tie, whether the position exists and its k-mer holds no N.
// The loop issues 8.05 VALU instructions per position on top of the hash-only loop's 135.7, of which 2 are outside that branch
// (profiles/sketch_opcode_histogram_hiword.txt; 12.6, all but the push outside a branch, with every test on 64 bits and per position:
// profiles/r14_04_sketch_opcode_histogram.txt).
// ---------------------------------------------------------------------------------------------
#define MM_SKF_FLAG 0x80000000u
struct SkFast : SkCut {
  uint64_t* key; uint32_t* meta;      // meta: bit 31 = has entries on the duplicate list, low bits = pos << 1 | (strand > 0) of the owner
  uint32_t* dup; uint32_t* counters;  // counters: MM_TC_OVERFLOW, MM_TC_OCCUPIED, MM_TC_DUPS
  uint64_t* occW; uint32_t* occP;
  uint32_t nSlots, maxLoad;
  __device__ __forceinline__ void insert(uint64_t h, uint32_t m) {
    uint32_t slot = home(h);
    for (;;) {
      const unsigned long long prev = atomicCAS((unsigned long long*)&key[slot], (unsigned long long)MM_HASH_MAX, (unsigned long long)h);
      if (prev == MM_HASH_MAX) { meta[slot] = m; return; }                     // the owner: a plain store, nobody reads it before the barrier
      if (prev == h) {
        const uint32_t at = atomicAdd(&counters[MM_TC_DUPS], 1u);
        if (at < MM_SK_DUPCAP) dup[at] = slot | (m << 13); else atomicOr(&counters[MM_TC_OVERFLOW], 1u);
        return;
      }
      if (++slot >= nSlots) { atomicOr(&counters[MM_TC_OVERFLOW], 1u); return; }
    }
  }
};

template <int K, int SL>
__device__ __forceinline__ void
mm_sketch_fast(unsigned char* smem, const int f, const uint4* __restrict__ gTabs, const uint32_t* __restrict__ bases2, const uint32_t* __restrict__ nmask,
               const DFrag* __restrict__ frags, const uint32_t* __restrict__ readHasN, int s, int wantFast, int HT, int PAD, int QC,
               uint64_t* __restrict__ skHash, int2* __restrict__ skPos, int8_t* __restrict__ skStrand,
               uint32_t* __restrict__ skCount, int32_t* __restrict__ hardList, uint32_t* __restrict__ hardCount,
               unsigned long long* __restrict__ phaseStats) {
  // MM_SKETCH_STATS: shader-clock cycles thread 0 spends up to each phase boundary, summed over workgroups (diagnostics only)
  unsigned long long tPrev = phaseStats ? __builtin_amdgcn_s_memtime() : 0ull;
  auto mark = [&](int ph) {
    if (phaseStats && threadIdx.x == 0) { const unsigned long long t = __builtin_amdgcn_s_memtime(); atomicAdd(&phaseStats[ph], t - tPrev); tPrev = t; }
  };
  const DFrag fr = frags[f];
  const int len = fr.len;
  const int n = len - K + 1;                        // k-mer positions
  const int tid = threadIdx.x, nthr = blockDim.x;
  if (n <= 0) { if (tid == 0) skCount[f] = 0; return; }
  const bool hasN = readHasN[fr.readId] != 0;

  // ---- LDS carve: sketch_fast_layout (mm_sketch_plan.h), which sized the launch at the longest fragment ----
  using Tabs = typename MMTabsFor<K>::type;
  const int nWaves = nthr >> 6;
  const SkFastLayout lay = sketch_fast_layout(sizeof(Tabs), len, HT, PAD, QC, nWaves);
  const int nW = lay.nW, nM = lay.nM, NS = lay.NS, nOcc = lay.nOcc;   // NS: table slots (multiple of 64)
  Tabs* tabs = (Tabs*)(smem + lay.tabs);
  for (int i = tid; i < (int)(sizeof(Tabs) / 16); i += nthr) ((uint4*)tabs)[i] = gTabs[i];   // visible after the first __syncthreads() below
  uint32_t* sW = (uint32_t*)(smem + lay.sW);
  uint32_t* sM = (uint32_t*)(smem + lay.sM);
  uint64_t* qH = (uint64_t*)(smem + lay.qH);        // per-wave queues: hashes
  uint32_t* qM = (uint32_t*)(smem + lay.qM);        //                  pos<<1 | (strand > 0); >= the table's load limit: the memory serves as the list of occupied slots later
  SkFast tab;
  tab.key = (uint64_t*)(smem + lay.key) + MM_SK_GUARD;
  tab.occW = (uint64_t*)(smem + lay.occW);
  tab.meta = (uint32_t*)(smem + lay.meta);
  tab.occP = (uint32_t*)(smem + lay.occP);
  uint32_t* qCnt = (uint32_t*)(smem + lay.qCnt);
  tab.dup = (uint32_t*)(smem + lay.dup);
  tab.counters = (uint32_t*)(smem + lay.counters);
  tab.nSlots = (uint32_t)NS; tab.maxLoad = (uint32_t)HT * 5u / 8u;

  // ---- stage the fragment, re-aligned so that LDS word j holds bases 16j..16j+15 ----
  mm_sk_stage(sW, nW, bases2, fr.base >> 4, (int)(fr.base & 15) * 2, tid, nthr);
  if (hasN) mm_sk_stage(sM, nM, nmask, fr.base >> 5, (int)(fr.base & 31), tid, nthr);
  // threshold: the canonical hash is the smaller of two uniform 64-bit values, so P[h < T] ~ 2T / 2^64; the cut is placed where
  // `wantFast` (> s) survivors are expected.  Any T gives the exact sketch as long as >= s distinct hashes survive (checked below).
  // From k = 16 on the loop tests the high words alone (HIWORD, below), so the cut is rounded up to a multiple of 2^32 there -- the same
  // value wherever wantFast / 2n >= 2^-9, the float's 24 bits then end above the low word (mm_sketch_dev.h).
  constexpr bool HIWORD = K >= 16;
  const uint64_t T = HIWORD ? mm_sketch_cut_hiword(mm_sketch_fast_cut(wantFast, n)) : mm_sketch_fast_cut(wantFast, n);
  const int nStrips = (n + SL - 1) / SL;
  tab.set_cut(T, (uint32_t)HT);
  for (int i = tid; i < NS; i += nthr) tab.key[i] = MM_HASH_MAX;
  if (tid < MM_SK_GUARD) { tab.key[-1 - tid] = MM_HASH_MAX; tab.key[NS + tid] = MM_HASH_MAX; }
  if (tid < 4) tab.counters[tid] = 0;
  __syncthreads();
  mark(0);                                          // staging + table init

  // ---- phase 1: hash both strands of every k-mer ----
  const uint32_t qBase = (uint32_t)(tid >> 6) * (uint32_t)QC, qEnd = qBase + (uint32_t)QC;
  uint32_t qHead = qBase;                           // wave-uniform (only ballots feed it)
  const uint64_t allPassM = (T == MM_HASH_MAX) ? ~0ull : 0ull;     // wave-uniform
  const uint32_t cutLast = mm_sketch_cut_last_hi(T), qLast = qEnd - 1u;   // HIWORD: the largest high word under the cut; the wave's last queue entry
  uint64_t tie = 0;                                 // HIWORD: lanes that queued a position whose two high words are equal (wave-uniform)
  for (int strip = tid; strip < nStrips; strip += nthr) {
    const int b0 = strip * SL;                      // first base of the strip: the 48-base window is cut out of four LDS words
    const int wi = b0 >> 4, bsh = (b0 & 15) * 2;
    // bit j: position b0 + j exists and its k-mer holds no N.  (HIWORD: the drain asks that of the few positions that reach it; positions
    // past the end and k-mers with an N, which hash as if it were an A, are queued like any other and dropped there)
    const int rem = n - b0;
    uint32_t ok = rem >= SL ? (uint32_t)((1ull << SL) - 1ull) : ((1u << rem) - 1u);
    if (!HIWORD && hasN) {
      const int mi = b0 >> 5, msh = b0 & 31;
      const uint64_t lo64 = (uint64_t)sM[mi] | ((uint64_t)sM[mi + 1] << 32);
      if constexpr (MMWideK<K>::value) {            // 16 + K - 1 > 64 mask bits: a 128-bit window
        const uint64_t hi64 = (uint64_t)sM[mi + 2] | ((uint64_t)sM[mi + 3] << 32);
        const uint64_t lo = msh ? ((lo64 >> msh) | (hi64 << (64 - msh))) : lo64, hi = msh ? (hi64 >> msh) : hi64;
        ok &= ~mm_window_or_wide<K>(lo, hi);
      } else {
        const uint64_t m64 = msh ? ((lo64 >> msh) | ((uint64_t)sM[mi + 2] << (64 - msh))) : lo64;
        ok &= ~(uint32_t)mm_window_or<K>(m64);
      }
    }
    const uint32_t pos2 = (uint32_t)b0 << 1;
    auto onPos = [&](int j, uint64_t hf, uint64_t hr) {
      if constexpr (HIWORD) {
        // What every position pays: one v_min_u32 of the two high words and one 32-bit compare.  Only ~3.6 % of the positions pass, and
        // what only they need is done behind a wave-uniform branch (taken when any of the 64 lanes passes) or left to the drain:
        //   * the canonical hash is not selected: every passing lane stores hr, the lanes with hf.hi < hr.hi then store hf over it (a wave's
        //     LDS writes land in program order), each store with its own constant strand bit and both at one address computation;
        //   * equal high words (hf == hr -- a k-mer that is its own reverse complement, which the reference skips, commonFunc.hpp:237 --
        //     or a 2^-32 coincidence) are not resolved on the low words: the wave remembers it and the fragment goes to the hard list;
        //   * an entry beyond the wave's queue overwrites the queue's last one: the count behind the loop sends the fragment to the
        //     hard list, nothing outside the queue is written.
        const uint32_t fh = (uint32_t)(hf >> 32), rh = (uint32_t)(hr >> 32);
        const uint64_t m = mm_mask_le32(mm_min_u32(fh, rh), cutLast);
        if (m) {
          const uint64_t mF = mm_mask_lt32(fh, rh);
          tie |= mm_mask_eq32(fh, rh) & m;
          uint32_t idx = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, qHead));
          idx = idx < qLast ? idx : qLast;
          if (__builtin_amdgcn_inverse_ballot_w64(m)) {
            qH[idx] = hr; qM[idx] = pos2 + (uint32_t)(2 * j);
            if (__builtin_amdgcn_inverse_ballot_w64(mF)) { qH[idx] = hf; qM[idx] = pos2 + (uint32_t)(2 * j + 1); }
          }
          qHead += (uint32_t)__popcll(m);
        }
      } else {
        // k-mers of up to 15 bases (many of them their own reverse complement, few distinct ones): every test on the full hashes, per position.
        // The tests as lane masks in scalar registers (mm_device.h): nothing but the two selects of the minimum touches a vector register
        // (the compiler's own `hf < hr ? hf : hr` is as fast at s = 130 and 0.5 ms per 2 M fragments slower at s = 310: profiles/r06b, r06c)
        const int pos = b0 + j;
        const uint64_t mLt = mm_mask_lt64(hf, hr);
        const uint64_t h = mm_mask_select64(mLt, hf, hr);
        const uint64_t m = mm_mask_nz32(ok & (1u << j)) & mm_mask_ne64(hf, hr) & (mm_mask_lt64(h, T) | allPassM);
        const uint32_t idx = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, qHead));
        if (__builtin_amdgcn_inverse_ballot_w64(m) && idx < qEnd) { qH[idx] = h; qM[idx] = ((uint32_t)pos << 1) | (__builtin_amdgcn_inverse_ballot_w64(mLt) ? 1u : 0u); }
        qHead += (uint32_t)__popcll(m);
      }
    };
    if constexpr (MMWideK<K>::value) {              // k-mers of 33..64 bases: 4 or 5 words per strip (SL == 16: the strip starts on a word)
      uint32_t ww[MMWideK<K>::NW];
#pragma unroll
      for (int i = 0; i < MMWideK<K>::NW; i++) ww[i] = sW[wi + i];
      mm_strip_hashes_wide<K>(ww, *tabs, onPos);
    } else {
      uint32_t w0 = sW[wi], w1 = sW[wi + 1], w2 = sW[wi + 2];
      if (SL % 16 != 0) {
        const uint32_t w3 = sW[wi + 3];
        if (bsh) { w0 = __builtin_amdgcn_alignbit(w1, w0, bsh); w1 = __builtin_amdgcn_alignbit(w2, w1, bsh); w2 = __builtin_amdgcn_alignbit(w3, w2, bsh); }
      }
      mm_strip_hashes<K, SL>(w0, w1, w2, *tabs, onPos);
    }
  }
  mark(1);                                          // thread 0's hash loop
  {
    // lanes that left the strip loop early (or never entered it) hold a stale count; lane 0 owns the smallest strip
    const uint32_t qCount = (uint32_t)__builtin_amdgcn_readfirstlane((int)(qHead - qBase));
    const bool tied = mm_bcast64_readfirstlane(tie) != 0ull;   // equal high words on a queued position: the exact kernel looks at all 64 bits
    if (mm_lane() == 0) { qCnt[tid >> 6] = qCount; if (qCount > (uint32_t)QC || tied) atomicOr(&tab.counters[MM_TC_OVERFLOW], 1u); }
  }
  __syncthreads();
  mark(2);                                          // waiting for the other waves' hash loops
  if (tab.counters[MM_TC_OVERFLOW] == 0) {
    // all threads drain all queues: entry g of the concatenated queues goes to thread g mod nthr, so every round of inserts is full
    uint32_t pre[17]; pre[0] = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) pre[w + 1] = pre[w] + (w < nWaves ? qCnt[w] : 0u);
    const uint32_t total = pre[16];
    // HIWORD: the loop queued positions without asking whether they have a k-mer (mm_sk_drain_keep: inside the fragment, no N)
    const uint32_t* const drainMask = hasN ? sM : nullptr;
    auto drain = [&](uint32_t at) {
      const uint32_t m = qM[at];
      if (!HIWORD || mm_sk_drain_keep<K>(m >> 1, (uint32_t)n, drainMask)) tab.insert(qH[at], m);
    };
    if (nWaves <= 4) {
      // the usual geometry (4 982 k-mers = 250 threads = 4 waves): three compares place an entry instead of the fifteen of the general form
      // below, which were a sixth of the instructions a survivor costs behind the hash loop
      const uint32_t p1 = pre[1], p2 = pre[2], p3 = pre[3];
      for (uint32_t g = (uint32_t)tid; g < total; g += (uint32_t)nthr) {
        const uint32_t w = (g >= p1 ? 1u : 0u) + (g >= p2 ? 1u : 0u) + (g >= p3 ? 1u : 0u);
        const uint32_t start = g >= p3 ? p3 : (g >= p2 ? p2 : (g >= p1 ? p1 : 0u));
        const uint32_t at = w * (uint32_t)QC + (g - start);
        drain(at);
      }
    } else
    for (uint32_t g = (uint32_t)tid; g < total; g += (uint32_t)nthr) {
      uint32_t w = 0, start = 0;                    // the queue entry g falls into, and where that queue starts in the concatenation
#pragma unroll
      for (int x = 1; x < 16; x++) if (g >= pre[x]) { w = (uint32_t)x; start = pre[x]; }
      const uint32_t at = w * (uint32_t)QC + (g - start);
      drain(at);
    }
  }
  __syncthreads();
  mark(3);                                          // queues drained into the table
  {
    // owners' stores are visible now: flag the slots that have entries on the duplicate list
    const uint32_t nd = tab.counters[MM_TC_DUPS] < MM_SK_DUPCAP ? tab.counters[MM_TC_DUPS] : MM_SK_DUPCAP;
    for (uint32_t i = (uint32_t)tid; i < nd; i += (uint32_t)nthr) atomicOr(&tab.meta[tab.dup[i] & 0x1FFFu], MM_SKF_FLAG);
  }
  // ---- occupancy words, their prefix counts, number of distinct keys ----
  mm_sk_occupancy(tab.key, tab.occW, tab.occP, NS, nOcc, tid, nthr,
                  [&](int total) { tab.counters[MM_TC_OCCUPIED] = (uint32_t)total; if ((uint32_t)total > tab.maxLoad) tab.counters[MM_TC_OVERFLOW] = 1u; });
  __syncthreads();
  const uint32_t D = tab.counters[MM_TC_OCCUPIED];
  if (tab.counters[MM_TC_OVERFLOW] != 0 || (D < (uint32_t)s && T != MM_HASH_MAX)) {
    // skCount[f] carries the first hint for the hard kernel's cut: the distinct count under this one, unless something overflowed
    if (tid == 0) { const uint32_t at = atomicAdd(hardCount, 1u); hardList[at] = f; skCount[f] = tab.counters[MM_TC_OVERFLOW] != 0 ? MM_SK_HINT_OVERFLOW : D; }
    return;
  }
  // the occupied slots in slot order (the queue memory is free again): every thread then ranks D / nthr keys instead of visiting
  // NS / nthr slots of which two thirds are empty; a key's position in that list is the number of occupied slots before it
  uint32_t* occList = qM;
  for (int slot = tid; slot < NS; slot += nthr) {
    const uint64_t m = tab.occW[slot >> 6];
    if ((m >> (slot & 63)) & 1ull) occList[tab.occP[slot >> 6] + (uint32_t)__popcll(m & ((1ull << (slot & 63)) - 1ull))] = (uint32_t)slot;
  }
  __syncthreads();
  mark(4);                                          // duplicate flags, occupancy, prefix counts, list of occupied slots

  // ---- rank every key inside its cluster; emit the s smallest, ascending (commonFunc.hpp:278-286) ----
  const uint32_t nDup = tab.counters[MM_TC_DUPS];
  for (int it = tid; it < (int)D; it += nthr) {
    const int slot = (int)occList[it];
    const uint64_t k = tab.key[slot];
    int q;                                          // -> first slot of the cluster
    const uint32_t smaller = mm_sk_cluster_smaller(tab.key, slot, k, NS, q);
    const uint32_t rank = (uint32_t)(it - (slot - q)) + smaller;               // every slot of [q, slot) is occupied
    if (rank < (uint32_t)s) {
      const uint32_t m = tab.meta[slot];
      int first = (int)((m & ~MM_SKF_FLAG) >> 1), last = first, sum = (m & 1u) ? 1 : -1;
      if (m & MM_SKF_FLAG) {                                                   // repeat occurrences: first / last position, strand sum (commonFunc.hpp:242-270)
        for (uint32_t i = 0; i < nDup; i++) {
          const uint32_t d = tab.dup[i];
          if ((int)(d & 0x1FFFu) != slot) continue;
          const int pos = (int)(d >> 14);
          first = pos < first ? pos : first; last = pos > last ? pos : last; sum += ((d >> 13) & 1u) ? 1 : -1;
        }
      }
      const size_t o = (size_t)f * s + rank;
      skHash[o] = k;
      skPos[o] = make_int2(first, last);
      skStrand[o] = mm_sk_strand(sum);
    }
  }
  if (tid == 0) skCount[f] = D < (uint32_t)s ? D : (uint32_t)s;
  mark(5);                                          // ranking + output (thread 0's share)
}

template <int K, int SL>
__global__ void __launch_bounds__(1024)
k_sketch_fast(const uint4* __restrict__ gTabs, const uint32_t* __restrict__ bases2, const uint32_t* __restrict__ nmask,
              const DFrag* __restrict__ frags, const uint32_t* __restrict__ readHasN, int s, int wantFast, int HT, int PAD, int QC,
              uint64_t* __restrict__ skHash, int2* __restrict__ skPos, int8_t* __restrict__ skStrand,
              uint32_t* __restrict__ skCount, int32_t* __restrict__ hardList, uint32_t* __restrict__ hardCount,
              unsigned long long* __restrict__ phaseStats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  mm_sketch_fast<K, SL>(smem, (int)blockIdx.x, gTabs, bases2, nmask, frags, readHasN, s, wantFast, HT, PAD, QC, skHash, skPos, skStrand, skCount,
                        hardList, hardCount, phaseStats);
}

// ---------------------------------------------------------------------------------------------
// k_hash_only<K, SL>: the integer roofline's yardstick, at the fast sketch kernel's OWN geometry: workgroup per
// fragment, the same thread count, the same SL positions per thread (window cut out of four LDS words), the same LDS claim (so the same
// number of workgroups share a CU), packed words and hasher tables in LDS -- but nothing besides the 2 x MurmurHash3_x64_128 per
// position: no N mask, no cut, no queues, no table.  The canonical hashes are folded into one value per thread that is stored only if
// it equals an impossible constant, so the hashes stay live and nothing is written.
// ---------------------------------------------------------------------------------------------
template <int K, int SL>
__global__ void __launch_bounds__(1024)
k_hash_only(const uint4* __restrict__ gTabs, const uint32_t* __restrict__ bases2, const DFrag* __restrict__ frags, uint64_t* __restrict__ sink) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const DFrag fr = frags[blockIdx.x];
  const int len = fr.len, n = len - K + 1;
  const int tid = threadIdx.x, nthr = blockDim.x;
  if (n <= 0) return;
  using Tabs = typename MMTabsFor<K>::type;
  // the front of the fast kernel's carve, [0, sM): tables and staged code words, which the table's and the queues' sizes do not move
  const SkFastLayout lay = sketch_fast_layout(sizeof(Tabs), len, 0, 0, 0, 0);
  Tabs* tabs = (Tabs*)(smem + lay.tabs);
  for (int i = tid; i < (int)(sizeof(Tabs) / 16); i += nthr) ((uint4*)tabs)[i] = gTabs[i];
  uint32_t* sW = (uint32_t*)(smem + lay.sW);
  mm_sk_stage(sW, lay.nW, bases2, fr.base >> 4, (int)(fr.base & 15) * 2, tid, nthr);
  __syncthreads();
  const int nStrips = (n + SL - 1) / SL;
  uint64_t acc = 0;
  for (int strip = tid; strip < nStrips; strip += nthr) {
    const int b0 = strip * SL;
    const int wi = b0 >> 4, bsh = (b0 & 15) * 2;
    // (the fast kernel's lines, word for word: as a shared helper they cost this kernel an instruction per strip, so they are stated twice)
    uint32_t w0 = sW[wi], w1 = sW[wi + 1], w2 = sW[wi + 2];
    if (SL % 16 != 0) {
      const uint32_t w3 = sW[wi + 3];
      if (bsh) { w0 = __builtin_amdgcn_alignbit(w1, w0, bsh); w1 = __builtin_amdgcn_alignbit(w2, w1, bsh); w2 = __builtin_amdgcn_alignbit(w3, w2, bsh); }
    }
    mm_strip_hashes<K, SL>(w0, w1, w2, *tabs, [&](int j, uint64_t hf, uint64_t hr) { acc += hf < hr ? hf : hr; });
  }
  if (acc == 0x9E3779B97F4A7C15ull) sink[0] = acc;
}

// strip-hasher tables, built once per context and k-mer size
template <int K>
__global__ void k_sketch_tables(typename MMTabsFor<K>::type* out) { mm_tables_init<K>(*out, (int)threadIdx.x, (int)blockDim.x); }

// (sketch_fast_geom, sketch_ht_hard, sketch_plan -- how the two kernels are run for (k, s, fragment length) -- and the layouts that size
// their LDS: mm_sketch_plan.h)

// Parameter combinations the LDS-resident kernels cannot hold are refused when the context is created (not after the reference
// index has been built): the sketch tables + a staged fragment of segLength bases.  (The L2 kernels hold every sketch of up to
// MM_LDS_MAX_SKETCH entries in LDS, whatever the other parameters: mm_l2_plan.h asserts it.)
int mm_check_params(const mm_params* p, std::string& err) {
  const int s = p->sketchSize, L = p->segLength;
  const SketchParamCheck chk = sketch_check_params(p->kmerSize, s, L, MM_LDS_MAX_SKETCH, MM_MAX_SKETCH);
  switch (chk.cls) {
    case MM_SKP_FITS: return MM_OK;
    // no LDS kernel holds this sketch: the global-memory sketch kernel (mm_sketch_global.hip) and the literal L2 kernels take every
    // fragment -- exact, slow; the stock binary runs these sizes (--dense at segments of 100 kbp), so they run here too
    // ... and so does the index build: k_winnow_tiles (mm_winnow.hip) keeps the sketch of a reference window in LDS up to
    // MM_WINNOW_LDS_SKETCH entries and in HBM beyond
    case MM_SKP_BEYOND_LDS: return MM_OK;
    case MM_SKP_BEYOND_MAX:
      err = "mm_create: sketchSize " + std::to_string(s) + " is beyond " + std::to_string(MM_MAX_SKETCH) + " (seeds are numbered in 16 bits by the literal mapping kernels)";
      return MM_ERR_ARG;
    case MM_SKP_REFUSED: break;
  }
  char b[400];
  snprintf(b, sizeof b, "mm_create: segLength %d with sketchSize %d needs %zu bytes of LDS in the sketch kernel (table of the exact path, spilled form); a CU has %zu",
           L, s, chk.ldsBytes, (size_t)MM_SK_LDS_LIMIT);
  err = b; return MM_ERR_ARG;
}

template <int K> struct MMHasSL20 { static constexpr bool value = (K >= 16 && K <= 21); };   // strips of 20 positions are built for these k-mer sizes

// the strip-hasher tables for kmerSize K in c->dSketchTabs (kept until another k-mer size asks)
template <int K>
static int ensure_sketch_tables(mm_ctx* c) {
  using Tabs = typename MMTabsFor<K>::type;
  if (c->sketchTabsK == K) return MM_OK;
  MM_HIP(c, c->dSketchTabs.ensure(sizeof(Tabs)));
  hipLaunchKernelGGL((k_sketch_tables<K>), dim3(1), dim3(256), 0, c->stream, c->dSketchTabs.as<Tabs>());
  MM_HIP(c, hipGetLastError());
  c->sketchTabsK = K;
  return MM_OK;
}

template <int K>
static int launch_sketch_k(mm_ctx* c) {
  const int s = c->P.sketchSize;
  const int nF = (int)c->nFrags;
  using Tabs = typename MMTabsFor<K>::type;
  const int maxLen = c->maxFragLen;
  const SketchPlan plan = sketch_plan(K, s, maxLen, sizeof(Tabs), MMHasSL20<K>::value);
  const FastGeom g = plan.g;
  const int HTH = plan.HTH;
  const int PAD = MM_SK_PAD, PADH = MM_SK_PADH;     // spill slots behind the ordered tables (no wrap-around)
  const size_t ldsFast = plan.ldsFast, ldsHard = plan.ldsHard;
  if (!plan.ok) { c->err = "fragment too long / sketch too large for the LDS-resident sketch kernel"; return MM_ERR_ARG; }
  int nStrips = (maxLen - K + 1 + 15) / 16; if (nStrips < 1) nStrips = 1;
  int threadsHard = ((nStrips + 63) / 64) * 64; if (threadsHard > 1024) threadsHard = 1024;
  if (const int rc = ensure_sketch_tables<K>(c)) return rc;
  MM_HIP(c, hipMemsetAsync(c->dCounters.as<unsigned long long>() + MM_CW_SKETCH, 0, (size_t)(MM_CW_SKETCH_END - MM_CW_SKETCH) * 8, c->stream));
  unsigned long long* phaseStats = nullptr;
  if (c->env.sketchStats) { phaseStats = c->dCounters.as<unsigned long long>() + MM_CW_SKETCH_PHASES; MM_HIP(c, hipMemsetAsync(phaseStats, 0, (size_t)(MM_CW_SKETCH_PHASES_END - MM_CW_SKETCH_PHASES) * 8, c->stream)); }
  if (plan.useFast) {
    KernelTimer t(c, MM_K_SKETCH);
    auto launch = [&](auto kern) {
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsFast);
      hipLaunchKernelGGL(kern, dim3(nF), dim3(g.threads), ldsFast, c->stream,
                         c->dSketchTabs.as<uint4>(), c->dBases2.as<uint32_t>(), c->dNmask.as<uint32_t>(), c->dFrags.as<DFrag>(), c->dReadHasN.as<uint32_t>(),
                         s, g.wantFast, g.HT, PAD, g.QC, c->dSkHash.as<uint64_t>(), c->dSkPos.as<int2>(), c->dSkStrand.as<int8_t>(),
                         c->dSkCount.as<uint32_t>(), c->dHardList.as<int32_t>(), c->dCounters.as<uint32_t>(), phaseStats);
    };
    if constexpr (MMHasSL20<K>::value) { if (g.SL == 20) launch(k_sketch_fast<K, 20>); else launch(k_sketch_fast<K, 16>); }
    else launch(k_sketch_fast<K, 16>);
    MM_HIP(c, hipGetLastError());
  } else {
    // the fast kernel's LDS geometry cannot hold this sketch: every fragment takes the exact path
    KernelTimer t(c, MM_K_SKETCH);
    hipLaunchKernelGGL(k_sketch_all_hard, dim3((nF + 255) / 256), dim3(256), 0, c->stream, nF, c->dHardList.as<int32_t>(), c->dCounters.as<uint32_t>(), c->dSkCount.as<uint32_t>());
    MM_HIP(c, hipGetLastError());
  }
  if (phaseStats && plan.useFast) {
    unsigned long long h[MM_CW_SKETCH_PHASES_END - MM_CW_SKETCH_PHASES];
    MM_HIP(c, hipMemcpyAsync(h, phaseStats, sizeof h, hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipStreamSynchronize(c->stream));
    fprintf(stderr, "[mm] sketch phases, shader-clock cycles per workgroup (thread 0), %d fragments, %d threads x %d positions, HT %d, queue %d/wave, lds %zu: stage+init %.0f | hash %.0f | wait %.0f | drain %.0f | occupancy+list %.0f | rank+emit %.0f\n",
            nF, g.threads, g.SL, g.HT, g.QC, ldsFast, (double)h[0] / nF, (double)h[1] / nF, (double)h[2] / nF, (double)h[3] / nF, (double)h[4] / nF, (double)h[5] / nF);
  }
  if (c->env.debug) {
    uint32_t nHard = 0;
    MM_HIP(c, hipMemcpyAsync(&nHard, c->dCounters.p, 4, hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipStreamSynchronize(c->stream));
    fprintf(stderr, "[mm] sketch: %d fragments, %u to the hard path%s, threads %d x %d positions, HT %d, lds %zu/%zu%s\n", nF, nHard, plan.useFast ? "" : " (fast kernel not usable at this size)",
            g.threads, g.SL, g.HT, ldsFast, ldsHard, plan.stream ? " (hard table: position / strand arrays in HBM; fragments read from global memory)" : plan.spill ? " (hard table: position / strand arrays in HBM)" : "");
  }
  {
    // fixed grid over the device-resident hard list (its workgroups leave at once when the list is empty or short)
    KernelTimer t(c, MM_K_SKETCH_HARD);
    const int grid = nF < 1024 ? nF : 1024;
    auto launchHard = [&](auto kern, int32_t* spill) {
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsHard);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(threadsHard), ldsHard, c->stream,
                         c->dSketchTabs.as<uint4>(), c->dBases2.as<uint32_t>(), c->dNmask.as<uint32_t>(), c->dFrags.as<DFrag>(), c->dReadHasN.as<uint32_t>(),
                         c->dHardList.as<int32_t>(), c->dCounters.as<uint32_t>(), s, g.wantFast, HTH, PADH, spill, plan.stream ? 1 : 0, c->dSkHash.as<uint64_t>(), c->dSkPos.as<int2>(), c->dSkStrand.as<int8_t>(),
                         c->dSkCount.as<uint32_t>());
    };
    if (plan.spill) {
      MM_HIP(c, c->dSketchSpill.ensure((size_t)grid * 3 * (size_t)(HTH + PADH) * 4 + 64));
      launchHard(k_sketch_hard<K, true>, c->dSketchSpill.as<int32_t>());
    } else launchHard(k_sketch_hard<K, false>, (int32_t*)nullptr);
    MM_HIP(c, hipGetLastError());
  }
  return MM_OK;
}

template <int K>
static int launch_hash_only_k(mm_ctx* c, int reps, double* msAvg) {
  using Tabs = typename MMTabsFor<K>::type;
  const int nF = (int)c->nFrags;
  const int maxLen = c->maxFragLen;
  // the sketch kernel's geometry for these fragments: positions per thread, threads per workgroup, LDS per workgroup
  const FastGeom g = sketch_fast_geom(K, c->P.sketchSize, maxLen, sizeof(Tabs), MMHasSL20<K>::value);
  // ... and where that claim cannot be made, what the kernel itself uses: the front of the carve, up to the end of the staged words
  const size_t need = sketch_fast_layout(sizeof(Tabs), maxLen, g.HT, MM_SK_PAD, g.QC, g.threads / 64).sM;
  const size_t lds = (g.lds > need && g.lds <= MM_SK_LDS_LIMIT) ? g.lds : need;
  if (const int rc = ensure_sketch_tables<K>(c)) return rc;
  MM_HIP(c, c->dCounters.ensure(MM_COUNTER_BYTES));
  float total = 0;
  for (int r = 0; r <= reps; r++) {                 // launch 0 is a warm-up
    MM_HIP(c, hipEventRecord(c->evA, c->stream));
    auto launch = [&](auto kern) {
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL(kern, dim3(nF), dim3(g.threads), lds, c->stream, c->dSketchTabs.as<uint4>(), c->dBases2.as<uint32_t>(), c->dFrags.as<DFrag>(),
                         c->dCounters.as<uint64_t>() + MM_CW_SKETCH_PHASES);   // the sink (never stored to)
    };
    if constexpr (MMHasSL20<K>::value) { if (g.SL == 20) launch(k_hash_only<K, 20>); else launch(k_hash_only<K, 16>); }
    else launch(k_hash_only<K, 16>);
    MM_HIP(c, hipGetLastError());
    MM_HIP(c, hipEventRecord(c->evB, c->stream));
    MM_HIP(c, hipEventSynchronize(c->evB));
    float ms = 0; MM_HIP(c, hipEventElapsedTime(&ms, c->evA, c->evB));
    if (r) total += ms;
  }
  *msAvg = total / reps;
  return MM_OK;
}

extern "C" int mm_bench_hash_only(mm_ctx* c, int reps, double* msAvg) {
  if (!c->nFrags || reps < 1 || !msAvg) { c->err = "mm_bench_hash_only: needs resident reads and reps >= 1"; return MM_ERR_ARG; }
  MM_HIP(c, hipSetDevice(c->device));
  switch (c->P.kmerSize) {
#define MM_CASE(KK) case KK: return launch_hash_only_k<KK>(c, reps, msAvg);
    MM_CASE(16) MM_CASE(19) MM_CASE(21)
#undef MM_CASE
    default: c->err = "mm_bench_hash_only: built for k = 16, 19, 21"; return MM_ERR_ARG;
  }
}

// the sketch's output arrays, the hard list and the counter block, for nF fragments of s entries
static int ensure_sketch_buffers(mm_ctx* c, size_t nF, size_t s) {
  MM_HIP(c, c->dSkHash.ensure(nF * s * 8 + 64));
  MM_HIP(c, c->dSkPos.ensure(nF * s * 8 + 64));
  MM_HIP(c, c->dSkStrand.ensure(nF * s + 64));
  MM_HIP(c, c->dSkCount.ensure(nF * 4 + 64));
  MM_HIP(c, c->dHardList.ensure(nF * 4 + 64));
  MM_HIP(c, c->dCounters.ensure(MM_COUNTER_BYTES));
  return MM_OK;
}

int mm_launch_sketch(mm_ctx* c) {
  const size_t nF = c->nFrags, s = (size_t)c->P.sketchSize;
  c->skLargeState = MM_SKL_STATE_KNOWN; c->skLargeFrags = c->skLargeUncut = 0;   // mm_sketch_large_counts: 0 / 0 unless k_sketch_large runs below
  if (s > MM_LDS_MAX_SKETCH) {
    if (const int rc = ensure_sketch_buffers(c, nF, s)) return rc;
    // no hard list here, and its length is read all the same (mm_pass_stats): the words every other sketch launch resets
    MM_HIP(c, hipMemsetAsync(c->dCounters.as<unsigned long long>() + MM_CW_SKETCH, 0, (size_t)(MM_CW_SKETCH_END - MM_CW_SKETCH) * 8, c->stream));
    return c->opt.sketchLarge ? mm_launch_sketch_large(c) : mm_launch_sketch_global(c);
  }
  // (for the largest batch the caller has announced: no reallocation when it comes)
  if (const int rc = ensure_sketch_buffers(c, mm_frag_cap(c, nF), s)) return rc;
  if (nF == 0) return MM_OK;
  switch (c->P.kmerSize) {
#define MM_CASE(KK) case KK: return launch_sketch_k<KK>(c);
    MM_FOR_EACH_K(MM_CASE)
#undef MM_CASE
    default: c->err = "kmerSize outside 1..64"; return MM_ERR_ARG;
  }
}

int mm_launch_pack_raw(mm_ctx* c, const uint8_t* dAscii, const int64_t* dSrcOff, const int64_t* dPackOff, const int32_t* dLen, int nReads,
                       int64_t nChunks, uint32_t* dB, uint32_t* dM, uint32_t* dHasN) {
  if (nChunks == 0) return MM_OK;
  int blocks = (int)((nChunks + 255) / 256); if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(k_pack2bit, dim3(blocks), dim3(256), 0, c->stream, dAscii, dSrcOff, dPackOff, dLen, nReads, nChunks, dB, dM, dHasN);
  MM_HIP(c, hipGetLastError());
  return MM_OK;
}

int mm_launch_pack(mm_ctx* c) {
  const int64_t nChunks = (int64_t)(c->nPackedBases / 32);
  if (nChunks == 0) return MM_OK;
  KernelTimer t(c, MM_K_PACK);
  int blocks = (int)((nChunks + 255) / 256); if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_pack2bit, dim3(blocks), dim3(256), 0, c->stream, c->dAscii.as<uint8_t>(), c->dReadSrcOff.as<int64_t>(),
                     c->dReadPackOff.as<int64_t>(), c->dReadLen.as<int32_t>(), (int)c->nReads, nChunks,
                     c->dBases2.as<uint32_t>(), c->dNmask.as<uint32_t>(), c->dReadHasN.as<uint32_t>());
  MM_HIP(c, hipGetLastError());
  return MM_OK;
}
