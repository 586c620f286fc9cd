// mashmap_amd/csrc/mm_sketch_large.hip -- k_sketch_large<K> (MM_OPT_SKETCH_LARGE): CommonFunc::sketchSequence (src/map/include/commonFunc.hpp:183-288)
// for sketches no LDS table holds (sketchSize beyond 8 190), the three phases of k_sketch_global (mm_sketch_global.hip) with
//   1. the hashes from the strip hashers of mm_device.h, their tables built in LDS once per workgroup, the fragment's 2-bit words and
//      N-mask words read from global memory as k_sketch_hard reads them in its stream mode;
//   2. the bitonic sort by the schedule of mm_sketch_large_plan.h: tiles of MM_SKL_TILE entries sorted in LDS, sweeps through HBM only
//      where the partner lies a tile or more away (s = 19 998: 6 sweeps and 4 tile rounds over 32 768 entries instead of 120 sweeps);
//   3. k_sketch_global's emission, as it stands there.
// The sort keys (hash, position << 1 | strand bit) are pairwise distinct, so the sorted slice -- and with it every output byte -- is the
// one k_sketch_global leaves.  One workgroup per fragment; a fragment with fewer than s distinct hashes below the cut is done again by the
// same workgroup without one.
#include "mm_internal.h"
#include "mm_device.h"
#include "mm_sketch_dev.h"
#include "mm_sketch_large_plan.h"
#include <algorithm>

namespace {

// (the entry of the sort, SkEnt, its order, the compaction and the emission: mm_sketch_dev.h, shared with k_sketch_global)
static_assert(sizeof(SkEnt) == MM_SKL_ENTRY_BYTES, "mm_sketch_large_plan.h sizes the tile by this entry");
static_assert(sizeof(MMProdTables) == MM_SKL_TABLE_BYTES && sizeof(MMTables) <= MM_SKL_TABLE_BYTES, "mm_sketch_large_plan.h sums the LDS with the larger table");
static_assert(MM_SKL_HASH_MAX == MM_HASH_MAX, "one value for `no cut`");

template <int K>
__global__ void __launch_bounds__(1024)
k_sketch_large(int nF, int s, int64_t slice /* entries per workgroup, a power of two >= the longest fragment's positions */,
               const uint32_t* __restrict__ bases2, const uint32_t* __restrict__ nmask, const DFrag* __restrict__ frags, const uint32_t* __restrict__ readHasN,
               SkEnt* scratch, uint64_t* __restrict__ skHash, int2* __restrict__ skPos, int8_t* __restrict__ skStrand, uint32_t* __restrict__ skCount,
               unsigned long long* __restrict__ sketchWords /* dCounters + MM_CW_SKETCH */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int sCount[1024];
  __shared__ int sTotal;
  static_assert(sizeof(sCount) + 16 == MM_SKL_STATIC_BYTES, "mm_sketch_large_plan.h sums the LDS with the counts and 16 bytes for the cursor");
  using Tabs = typename MMTabsFor<K>::type;
  Tabs* tabs = (Tabs*)smem;
  SkEnt* tileE = (SkEnt*)(smem + MM_SKL_TABLE_BYTES);                         // MM_SKL_TILE entries
  const int tid = threadIdx.x, nthr = blockDim.x;
  mm_tables_init<K>(*tabs, tid, nthr);                                      // once per workgroup: every fragment it takes hashes through them
  __syncthreads();
  SkEnt* e = scratch + (size_t)blockIdx.x * (size_t)slice;
  for (int f = blockIdx.x; f < nF; f += gridDim.x) {
    const DFrag fr = frags[f];
    const int n = fr.len - K + 1;
    if (n <= 0) { if (tid == 0) skCount[f] = 0; continue; }
    const bool hasN = readHasN[fr.readId] != 0;
    // word j of the fragment re-aligned to its first base / of its N mask, straight from the packed batch (mm_sketch_hard's stream mode:
    // neighbouring strips share their words in the caches; the run-off words behind the batch are there and zero)
    const int64_t gw0 = fr.base >> 4; const int gsh = (int)(fr.base & 15) * 2;
    const int64_t gm0 = fr.base >> 5; const int gmsh = (int)(fr.base & 31);
    auto wordAt = [&](int j) -> uint32_t { return mm_sk_word_at(bases2, gw0, gsh, j); };
    auto maskAt = [&](int j) -> uint32_t { return mm_sk_word_at(nmask, gm0, gmsh, j); };
    // any T gives the exact sketch as long as s distinct hashes survive it -- counted below; a fragment where they do not, a repeat, is
    // done again without a cut
    uint64_t T = mm_sketch_cut(s, n);
    const int nStrips = (n + 15) >> 4;
    for (int attempt = 0; attempt < 2; attempt++) {
    // ---- 1. hashes below the cut, compacted into the slice (wave-aggregated cursor).  At most n <= slice of them: no index leaves the slice ----
    if (tid == 0) sTotal = 0;
    __syncthreads();
    const bool allPass = (T == MM_HASH_MAX);
    for (int s0 = 0; s0 < nStrips; s0 += nthr) {
      // whole waves go through the ballots below: a lane behind the last strip hashes strip 0 again and keeps nothing of it
      const bool live = s0 + tid < nStrips;
      const int strip = live ? s0 + tid : 0;
      // bit j: position strip*16+j exists and its k-mer holds no N
      const int rem = n - strip * 16;
      uint32_t ok = !live ? 0u : rem >= 16 ? 0xFFFFu : ((1u << rem) - 1u);
      if (hasN) ok &= ~mm_sk_strip_has_n<K>(strip, maskAt);
      auto onPos = [&](int j, uint64_t hf, uint64_t hr) {
        const uint64_t h = hf < hr ? hf : hr;
        bool keep = false;                          // no N, the two strands differ (commonFunc.hpp:207-240), below the cut
        if ((ok & (1u << j)) != 0) { if (hf != hr) { if (allPass || h < T) keep = true; } }
        mm_sk_append(e, &sTotal, keep, h, ((uint32_t)(strip * 16 + j) << 1) | (hf < hr ? 1u : 0u));
      };
      if constexpr (MMWideK<K>::value) {
        uint32_t ww[MMWideK<K>::NW];
#pragma unroll
        for (int i = 0; i < MMWideK<K>::NW; i++) ww[i] = wordAt(strip + i);
        mm_strip_hashes_wide<K>(ww, *tabs, onPos);
      } else mm_strip_hashes<K>(wordAt(strip), wordAt(strip + 1), wordAt(strip + 2), *tabs, onPos);
    }
    __syncthreads();
    const int nSurv = sTotal;
    // ---- 2. padded to a power of two (N2 <= slice: the slice is one, and nSurv <= slice) and sorted ascending by (hash, position) ----
    const int64_t N2 = mm_skl_n2(nSurv);
    for (int64_t p = nSurv + tid; p < N2; p += nthr) e[p] = mm_sk_ent_padding();
    __threadfence_block();
    __syncthreads();
    const int TL = (int)(N2 < MM_SKL_TILE ? N2 : MM_SKL_TILE);               // entries of a tile: TL divides N2, so a tile never reaches past N2
    mm_skl_schedule(N2, MM_SKL_TILE,
      [&](int64_t k2, int64_t j) {                                            // one sweep through HBM; i < q = i + j < N2
        for (int64_t p = tid; p < (N2 >> 1); p += nthr) {
          const int64_t i = mm_skl_pair_low(p, j), q = mm_skl_partner(i, j);
          const SkEnt a = e[i], b = e[q];
          if (mm_skl_swaps(mm_sk_ent_less(b, a), i, k2)) { e[i] = b; e[q] = a; }
        }
        __threadfence_block();
        __syncthreads();
      },
      [&](int64_t k2lo, int64_t k2hi) {                                       // every tile through LDS once
        for (int64_t t0 = 0; t0 < N2; t0 += TL) {
          // (a thread loads the LDS entries it stored from at the end of the tile before: no barrier between the two)
          for (int i = tid; i < TL; i += nthr) tileE[i] = e[t0 + i];
          __syncthreads();
          mm_skl_tile_steps(k2lo, k2hi, MM_SKL_TILE, [&](int64_t k2, int64_t j) {
            for (int p = tid; p < (TL >> 1); p += nthr) {
              const int i = (int)mm_skl_pair_low(p, j), q = (int)mm_skl_partner(i, j);   // q = i + j < TL: j < TL
              const SkEnt a = tileE[i], b = tileE[q];
              if (mm_skl_swaps(mm_sk_ent_less(b, a), t0 + i, k2)) { tileE[i] = b; tileE[q] = a; }
            }
            __syncthreads();
          });
          for (int i = tid; i < TL; i += nthr) e[t0 + i] = tileE[i];
        }
        __threadfence_block();
        __syncthreads();
      });
    // ---- 3. one entry per distinct hash in order, the s smallest: mm_sk_emit_sorted ----
    if (mm_sk_emit_sorted(e, N2, s, T != MM_HASH_MAX, f, sCount, &sTotal, skHash, skPos, skStrand, skCount)) {
      T = MM_HASH_MAX; __syncthreads(); continue;     // fewer than s distinct hashes below the cut: once more without one
    }
    if (tid == 0) {
      atomicAdd(&sketchWords[MM_SKW_LARGE_FRAGS], 1ull);
      if (T == MM_HASH_MAX) atomicAdd(&sketchWords[MM_SKW_LARGE_UNCUT], 1ull);
    }
    __syncthreads();
    break;
    }  // attempt
  }
}

template <int K>
int launch_sketch_large_k(mm_ctx* c) {
  const int nF = (int)c->nFrags, s = c->P.sketchSize;
  const int64_t slice = sketch_scratch_slice(c->maxFragLen);
  const size_t lds = (size_t)MM_SKL_TABLE_BYTES + (size_t)MM_SKL_TILE * sizeof(SkEnt);
  auto kern = k_sketch_large<K>;
  MM_HIP(c, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // as many workgroups as the scratch cap allows, and no more than the device holds at once at this kernel's residency
  if (!c->chainCUs) { int cus = 0; MM_HIP(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device)); c->chainCUs = cus > 0 ? cus : 1; }
  int perCU = 0;
  MM_HIP(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, (const void*)kern, 1024, lds));
  if (perCU < 1) perCU = 1;
  const int grid = (int)std::min<int64_t>(std::min<int64_t>(nF, (int64_t)c->chainCUs * perCU), sketch_scratch_grid_cap(slice, sizeof(SkEnt)));
  MM_HIP(c, c->dSketchSpill.ensure((size_t)grid * (size_t)slice * sizeof(SkEnt) + 64));
  unsigned long long* words = c->dCounters.as<unsigned long long>() + MM_CW_SKETCH;     // reset by mm_launch_sketch
  {
    KernelTimer t(c, MM_K_SKETCH_HARD);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(1024), lds, c->stream, nF, s, slice, c->dBases2.as<uint32_t>(), c->dNmask.as<uint32_t>(), c->dFrags.as<DFrag>(),
                       c->dReadHasN.as<uint32_t>(), c->dSketchSpill.as<SkEnt>(), c->dSkHash.as<uint64_t>(), c->dSkPos.as<int2>(), c->dSkStrand.as<int8_t>(),
                       c->dSkCount.as<uint32_t>(), words);
    MM_HIP(c, hipGetLastError());
  }
  // the mapping pass resets the block: the two counts go to a page-locked spot right behind the kernel; mm_sketch_large_counts waits for
  // the copy, nothing else does
  static_assert(MM_SKW_LARGE_UNCUT == MM_SKW_LARGE_FRAGS + 1, "the two counts are copied as one range");
  MM_HIP(c, hipMemcpyAsync(c->hSkLarge.p, words + MM_SKW_LARGE_FRAGS, 16, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipEventRecord(c->skLargeDone, c->stream));
  c->skLargeState = MM_SKL_STATE_PENDING;
  return MM_OK;
}

}  // namespace

// every resident fragment through k_sketch_large (mm_launch_sketch routes here under MM_OPT_SKETCH_LARGE when the sketch does not fit the LDS kernels)
int mm_launch_sketch_large(mm_ctx* c) {
  if (c->nFrags == 0) return MM_OK;
  MM_HIP(c, c->hSkLarge.ensure(16));
  MM_HIP(c, c->skLargeDone.ensure(hipEventDisableTiming));
  switch (c->P.kmerSize) {
#define MM_CASE(KK) case KK: return launch_sketch_large_k<KK>(c);
    MM_FOR_EACH_K(MM_CASE)
#undef MM_CASE
    default: c->err = "kmerSize outside 1..64"; return MM_ERR_ARG;
  }
}

int mm_sketch_large_counts(mm_ctx* c, uint64_t* fragments, uint64_t* uncut) {
  if (c->skLargeState == MM_SKL_STATE_NONE) { c->err = "mm_sketch_large_counts: no sketch launch yet"; return MM_ERR_STATE; }
  if (c->skLargeState == MM_SKL_STATE_PENDING) {
    MM_HIP(c, hipSetDevice(c->device));
    MM_HIP(c, hipEventSynchronize(c->skLargeDone));
    const unsigned long long* h = c->hSkLarge.as<unsigned long long>();
    c->skLargeFrags = h[0]; c->skLargeUncut = h[1];
    c->skLargeState = MM_SKL_STATE_KNOWN;
  }
  if (fragments) *fragments = c->skLargeFrags;
  if (uncut) *uncut = c->skLargeUncut;
  return MM_OK;
}
