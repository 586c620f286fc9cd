// mashmap_amd/csrc/mm_map.hip -- device index + seed lookup + L1 mapping kernels (gfx950), and the launcher of a mapping pass.
//
//   mm_build_device_index   flattening of skch::Sketch for the device     winSketch.hpp:100-102
//   k_lookup_l1             getSeedHits (freq. seed removal) + getSeedIntervalPoints + computeL1CandidateRegions, fused:
//                           wave per fragment, up to 128 / 256 / 512 points sorted in registers   computeMap.hpp:818-843, 857-912, 916-1116
//   k_lookup_mid            the same for the fragments with more points than that (up to MM_MID_MAXPTS): wave per fragment, the
//                           points that can reach minimumHits picked by position bins in LDS
//   k_lookup_groups         under -Y reference groups (MM_OPT_L1_GROUP_FUSED): wave per queued fragment, the points of one group at a time
//                           sorted in registers and swept by the fused L1 -- no HBM point path for the fragments it finishes
//   k_l1_regions / k_l1_compact / k_l1_fix_offsets / k_l1_gate
//                           the fused kernels' candidates, written into 64 regions, made one dense array; the steady-state gate
//   the HBM point path, for what the fused kernels hand over (more points still, -Y groups, position groups spanning contigs), for
//   every fragment under MM_OPT_KEEP_POINTS / --skipPrefix, and for fragments longer than segLength (--noSplit):
//     k_gather_points, k_filter_points                    the interval points into dPts; those that cannot reach minimumHits dropped
//     k_sort_points_wave / _block / _global, k_classify_sort   sorters by list length (registers, LDS, HBM) and the split between them
//     k_l1_stream           L1 by a wave that streams the sorted points
//     k_l1_stream_groups    the same under -Y reference groups, one body per group extent (MM_OPT_L1_GROUP_STREAM)
//     k_l1_sweep            L1 by the literal one-thread-per-fragment sweep of mm_l1_core.h (what k_l1_stream leaves, or everything)
//     k_l1_window           the same sweep for fragments longer than segLength (windowLen != 0)
//   map_pass / mm_launch_map   one pass over the resident sketches, stage by stage; sized or steady-state
//   mm_results_download, mm_query_sketch_download, mm_points_download
//   (L2 lives in mm_l2.hip, the selection in mm_select.hip; the pass's device counters are described in mm_internal.h: MM_CW_*)
#include "mm_internal.h"
#include "mm_device.h"
#include "mm_l1_core.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#define MM_EMPTY MM_HT_EMPTY

// ---------------------------------------------------------------------------------------------
// host: flatten the reference index
// ---------------------------------------------------------------------------------------------
static inline uint64_t pack_point(int32_t seqId, int32_t pos, int side) {
  return ((uint64_t)(uint32_t)seqId << 33) | ((uint64_t)(uint32_t)pos << 1) | (side == 1 ? 1ull : 0ull);
}

// The index as the reference holds it (host mirrors: minmerIndex after dropFreqSeedSet, the lookup map flattened, the frequent seeds)
// -> device arrays -> mm_flatten_device_index (mm_index_dev.hip), which builds everything Map reads on the GPU.
int mm_build_device_index(mm_ctx* c, const int32_t* contigLen, const int32_t* refGroup, size_t nContigs) {
  DeviceIndex& I = c->idx;
  I.ready = false;
  const size_t n = c->hMinmers.size(), nk = c->hKeys.size(), np = c->hPoints.size();
  MM_HIP(c, c->dCounters.ensure(MM_COUNTER_BYTES));
  std::vector<uint64_t> pk(np);
  for (size_t i = 0; i < np; i++) pk[i] = pack_point(c->hPoints[i].seqId, c->hPoints[i].pos, c->hPoints[i].side);
  std::vector<uint8_t> fq(nk, 0);
  for (size_t i = 0; i < nk; i++) fq[i] = std::binary_search(c->hFreq.begin(), c->hFreq.end(), c->hKeys[i]) ? 1 : 0;
  DevBuf dRec;
  MM_HIP(c, dRec.ensure(n * sizeof(mm_minmer) + 64));
  MM_HIP(c, I.keys.ensure(nk * 8 + 64)); MM_HIP(c, I.keyOff.ensure((nk + 1) * 8 + 64)); MM_HIP(c, I.keyFreq.ensure(nk + 64)); MM_HIP(c, I.ptKeys.ensure(np * 8 + 64));
  if (n) MM_HIP(c, hipMemcpyAsync(dRec.p, c->hMinmers.data(), n * sizeof(mm_minmer), hipMemcpyHostToDevice, c->stream));
  if (nk) { MM_HIP(c, hipMemcpyAsync(I.keys.p, c->hKeys.data(), nk * 8, hipMemcpyHostToDevice, c->stream));
            MM_HIP(c, hipMemcpyAsync(I.keyFreq.p, fq.data(), nk, hipMemcpyHostToDevice, c->stream)); }
  MM_HIP(c, hipMemcpyAsync(I.keyOff.p, c->hOffsets.data(), (nk + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (np) MM_HIP(c, hipMemcpyAsync(I.ptKeys.p, pk.data(), np * 8, hipMemcpyHostToDevice, c->stream));
  MM_HIP(c, hipStreamSynchronize(c->stream));
  const int rc = mm_flatten_device_index(c, dRec.as<mm_minmer>(), n, nk, np, contigLen, refGroup, nContigs);
  c->mirrorMinmers = c->mirrorMap = true;
  return rc;
}

// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------
// value of lane (lane ^ M), M a power of two, without the LDS crossbar: DPP inside a row of 16, v_permlane{16,32}_swap
// (gfx950) across rows.  All 64 lanes must be active.
template <int M>
__device__ __forceinline__ uint32_t mm_lane_xor32(uint32_t v, int lane) {
  if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, MM_DPP_QUAD_1032, 0xf, 0xf, false);
  else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, MM_DPP_QUAD_2301, 0xf, 0xf, false);
  else if constexpr (M == 4) {                                   // banks 0,2 (lane bit 2 clear) read lane+4, banks 1,3 read lane-4
    const int t = __builtin_amdgcn_update_dpp((int)v, (int)v, 0x104 /* row_shl:4 */, 0xf, 0x5, false);
    return (uint32_t)__builtin_amdgcn_update_dpp(t, (int)v, 0x114 /* row_shr:4 */, 0xf, 0xa, false);
  } else if constexpr (M == 8) return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128 /* row_ror:8 */, 0xf, 0xf, false);
  else if constexpr (M == 16) {                                  // first' = (r0,r0,r2,r2), second' = (r1,r1,r3,r3)
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (lane & 16) ? r[0] : r[1];
  } else {
    static_assert(M == 32, "lane distance");
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);   // first' = (lo,lo), second' = (hi,hi)
    return (lane & 32) ? r[0] : r[1];
  }
}
template <int M>
__device__ __forceinline__ uint64_t mm_lane_xor64(uint64_t v, int lane) {
  return ((uint64_t)mm_lane_xor32<M>((uint32_t)(v >> 32), lane) << 32) | mm_lane_xor32<M>((uint32_t)v, lane);
}
__device__ __forceinline__ uint64_t mm_shfl_xor64(uint64_t v, int m, int lane) {   // m: a power of two known after unrolling
  switch (m) {
    case 1: return mm_lane_xor64<1>(v, lane);
    case 2: return mm_lane_xor64<2>(v, lane);
    case 4: return mm_lane_xor64<4>(v, lane);
    case 8: return mm_lane_xor64<8>(v, lane);
    case 16: return mm_lane_xor64<16>(v, lane);
    default: return mm_lane_xor64<32>(v, lane);
  }
}
// neighbour lanes (lane 0 / lane 63 keep their own value, as __shfl_up / __shfl_down do) through DPP wave shifts
__device__ __forceinline__ int mm_shfl_up1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ int mm_shfl_down1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ uint64_t mm_shfl_up64(uint64_t v, int d) {      // d == 1
  return ((uint64_t)(uint32_t)mm_shfl_up1((int)(v >> 32)) << 32) | (uint32_t)mm_shfl_up1((int)(uint32_t)v);
}
__device__ __forceinline__ uint64_t mm_shfl_down64(uint64_t v, int d) {    // d == 1
  return ((uint64_t)(uint32_t)mm_shfl_down1((int)(v >> 32)) << 32) | (uint32_t)mm_shfl_down1((int)(uint32_t)v);
}

struct MapFlags { int hg, skipSelf, skipPrefix, lowerTri; };

// ascending bitonic sort of 64*R keys held R per lane (R a power of two), element index = lane*R + r
template <int R>
__device__ __forceinline__ void mm_wave_bitonic(uint64_t (&k)[R], int lane) {
  constexpr int N = 64 * R;
#pragma unroll
  for (int k2 = 2; k2 <= N; k2 <<= 1) {
#pragma unroll
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      // one compare per exchange: the element keeps its key or takes the partner's (equal keys: either)
      if (j < R) {                                   // partner inside the lane
#pragma unroll
        for (int r = 0; r < R; r++) {
          if (r & j) continue;
          const bool up = (((lane * R + r) & k2) == 0);
          const uint64_t a = k[r], b = k[r | j];
          const bool swap = (a < b) != up;
          k[r] = swap ? b : a; k[r | j] = swap ? a : b;
        }
      } else {                                       // partner in lane ^ (j / R), same register
        const int lj = j / R;
#pragma unroll
        for (int r = 0; r < R; r++) {
          const int idx = lane * R + r;
          const uint64_t other = mm_shfl_xor64(k[r], lj, lane);
          const bool keepMin = ((idx & k2) == 0) == ((idx & j) == 0);
          const bool lt = k[r] < other;
          k[r] = (lt != keepMin) ? other : k[r];
        }
      }
    }
  }
}

// per-wave LDS scratch of the fused kernel
#define MM_FUSE_MAXRUNS 64
struct L1Run { int32_t seq, start, end, isize; };
template <int MAXPTS>
struct FuseScratchT {
  uint64_t a[MAXPTS];                // gathered points, later (seqId<<32 | pos) of every position group
  int32_t v[MAXPTS];                 // overlap count after every position group
  L1Run run[MM_FUSE_MAXRUNS];        // candidate runs before joining (a fragment with more goes to the literal sweep)
};

// Interval points of the fragment's surviving seeds -> dst[0..P) (skip_self / skip_prefix / lower_triangular applied,
// computeMap.hpp:891-896; dropped points become MM_EMPTY and sort to the end).  Returns the wave-wide count of kept points.
// ids (may be null): the seed every point came from, as a small number unique inside the fragment (its index in the raw sketch) -- what the
// windowLen != 0 sweep counts open windows per hash by (computeMap.hpp:950: hash_to_freq)
// done: points already at dst (updated); rdBase: number of the first round (a sketch probed in several batches calls this per batch)
template <class Dst, class ValAt>
__device__ __forceinline__ int mm_gather_points(Dst dst, int& done, int rdBase, int nRounds, ValAt&& valAt,
                                                const uint64_t* __restrict__ ptKeys, const int32_t* __restrict__ refGroup,
                                                int rg, int self, int seqCounter, MapFlags fl, int lane, uint16_t* __restrict__ ids = nullptr) {
  int nValid = 0;
  auto one = [&](uint64_t key, int at, int seed) {
    const int seqId = (int)(key >> 33);
    bool drop = false;
    if (fl.skipSelf && seqId == self) drop = true;
    if (fl.skipPrefix && refGroup[seqId] == rg) drop = true;
    if (fl.lowerTri && !(seqCounter > seqId)) drop = true;
    if (drop) key = MM_EMPTY; else nValid++;
    dst[at] = key;
    if (ids) ids[at] = (uint16_t)seed;
  };
  for (int rd = 0; rd < nRounds; rd++) {
    const uint64_t val = valAt(rd);                // table value of this lane's seed in round rd (0: none)
    const int c = (int)((val >> 1) & 0x7fffffull);
    const int my = done + mm_wave_excl_scan(c);
    const uint64_t src = val >> 24;
    // a short run is copied by the lane that owns the seed; a long one -- a seed of a repeat family brings hundreds of points, and the
    // other 63 lanes used to wait for the one that copied them point by point -- by the whole wave, 64 consecutive points at a time
    const bool longRun = c > 8;
    if (!longRun) for (int j = 0; j < c; j++) one(ptKeys[src + j], my + j, (rdBase + rd) * 64 + lane);
    uint64_t mLong = mm_ballot(longRun);
    while (mLong) {
      const int l = (int)__builtin_ctzll(mLong); mLong &= mLong - 1ull;
      const int cL = __shfl(c, l), myL = __shfl(my, l);
      const uint64_t srcL = mm_bcast64_shfl(src, l);
      for (int j = lane; j < cL; j += 64) one(ptKeys[srcL + j], myL + j, (rdBase + rd) * 64 + l);
    }
    done += mm_wave_sum(c);
  }
  return mm_wave_sum(nValid);
}

// computeL1CandidateRegions (computeMap.hpp:916-1116, windowLen == 0) on a wave-sorted point list, data-parallel form
// (SURVEY App. A.4): position groups = runs of equal pos; overlap after group g = inclusive prefix sum of (+1 OPEN, -1 CLOSE);
// pass 1 best = max; pass 2 runs of consecutive groups -- the last one excluded -- with overlap >= minimumHits, cut on seqId
// change; runs closer than segLength joined.  Returns -1 when the list needs the literal sweep instead (a position group that
// spans two contigs: there the reference's trailing pointer, which compares (seqId,pos), lags its leading pointer, which
// compares pos only); otherwise the number of candidates, which have been stored at sc.run[0..n).
template <int R, class FuseScratch>
__device__ __forceinline__ int mm_l1_fused(uint64_t (&k)[R], FuseScratch& sc, int sketchSizeQ, int minHits, int hg,
                                           const int32_t* __restrict__ cutoffs, int nCutoffs, int sParam, int segLength, int lane) {
  bool valid[R]; uint64_t prv[R], nxt[R];
#pragma unroll
  for (int e = 0; e < R; e++) valid[e] = k[e] != MM_EMPTY;
  {
    const uint64_t up = mm_shfl_up64(k[R - 1], 1), dn = mm_shfl_down64(k[0], 1);
    prv[0] = lane == 0 ? MM_EMPTY : up;
    nxt[R - 1] = lane == 63 ? MM_EMPTY : dn;
#pragma unroll
    for (int e = 1; e < R; e++) { prv[e] = k[e - 1]; nxt[e - 1] = k[e]; }
  }
  bool mixed = false; int delta[R]; bool gLast[R];
#pragma unroll
  for (int e = 0; e < R; e++) {
    const bool pv = prv[e] != MM_EMPTY, nv = nxt[e] != MM_EMPTY;
    if (valid[e] && pv && (uint32_t)(prv[e] >> 1) == (uint32_t)(k[e] >> 1) && (prv[e] >> 33) != (k[e] >> 33)) mixed = true;
    delta[e] = valid[e] ? ((k[e] & 1ull) ? 1 : -1) : 0;
    gLast[e] = valid[e] && (!nv || (uint32_t)(nxt[e] >> 1) != (uint32_t)(k[e] >> 1));
  }
  if (__ballot(mixed)) return -1;
  int laneSum = 0, laneGroups = 0;
#pragma unroll
  for (int e = 0; e < R; e++) { laneSum += delta[e]; laneGroups += gLast[e] ? 1 : 0; }
  int run = mm_wave_excl_scan(laneSum);
  int gidx = mm_wave_excl_scan(laneGroups);
  const int G = mm_wave_sum(laneGroups);
  int best = 0;
#pragma unroll
  for (int e = 0; e < R; e++) {
    run += delta[e];
    if (gLast[e]) { sc.a[gidx] = k[e] >> 1; sc.v[gidx] = run; gidx++; best = run > best ? run : best; }
  }
  best = mm_wave_max(best);
  if (G == 0) return 0;
  if (hg) {                                                       // computeMap.hpp:984-998
    if (best < minHits) return 0;
    const double div = (double)sParam / 1000.0 > 1.0 ? (double)sParam / 1000.0 : 1.0;
    int ci = (int)((double)(best < sketchSizeQ ? best : sketchSizeQ) / div);
    if (ci >= nCutoffs) ci = nCutoffs - 1;
    const int cut = cutoffs[ci];
    minHits = cut > minHits ? cut : minHits;
  }
  __threadfence_block();
  // pass 2 over the groups, again R per lane
  uint64_t gk[R]; bool flag[R];
#pragma unroll
  for (int e = 0; e < R; e++) {
    const int j = lane * R + e;
    gk[e] = j < G ? sc.a[j] : 0ull;
    flag[e] = j < G - 1 && sc.v[j] >= minHits;
  }
  bool pflag[R], nflag[R]; uint32_t pseq[R], nseq[R];
  {
    const int upf = mm_shfl_up1((int)flag[R - 1]), dnf = mm_shfl_down1((int)flag[0]);
    const int ups = mm_shfl_up1((int)(gk[R - 1] >> 32)), dns = mm_shfl_down1((int)(gk[0] >> 32));
    pflag[0] = lane != 0 && upf; pseq[0] = (uint32_t)ups;
    nflag[R - 1] = lane != 63 && dnf; nseq[R - 1] = (uint32_t)dns;
#pragma unroll
    for (int e = 1; e < R; e++) { pflag[e] = flag[e - 1]; pseq[e] = (uint32_t)(gk[e - 1] >> 32); nflag[e - 1] = flag[e]; nseq[e - 1] = (uint32_t)(gk[e] >> 32); }
  }
  bool rStart[R], rEnd[R]; int laneStarts = 0;
#pragma unroll
  for (int e = 0; e < R; e++) {
    const uint32_t sq = (uint32_t)(gk[e] >> 32);
    rStart[e] = flag[e] && (!pflag[e] || pseq[e] != sq);
    rEnd[e] = flag[e] && (!nflag[e] || nseq[e] != sq);
    laneStarts += rStart[e] ? 1 : 0;
  }
  int ridx = mm_wave_excl_scan(laneStarts);                       // runs that started before this lane
  const int nRuns = mm_wave_sum(laneStarts);
  if (nRuns == 0) return 0;
  if (nRuns > MM_FUSE_MAXRUNS) return -1;
  int myRun[R];
#pragma unroll
  for (int e = 0; e < R; e++) {
    if (rStart[e]) { sc.run[ridx].seq = (int32_t)(gk[e] >> 32); sc.run[ridx].start = (int32_t)(uint32_t)gk[e]; sc.run[ridx].isize = 0; ridx++; }
    myRun[e] = ridx - 1;
  }
  __threadfence_block();
#pragma unroll
  for (int e = 0; e < R; e++) {
    if (flag[e]) atomicMax(&sc.run[myRun[e]].isize, sc.v[lane * R + e]);
    if (rEnd[e]) sc.run[myRun[e]].end = (int32_t)(uint32_t)gk[e];
  }
  __threadfence_block();
  // join runs closer than segLength (computeMap.hpp:1102-1115); uniform across the wave, compacted in place
  int nOut = 0;
  L1Run pend = sc.run[0];
  for (int r = 1; r < nRuns; r++) {
    const L1Run x = sc.run[r];
    if (x.seq != pend.seq || x.start > pend.end + segLength) {
      __threadfence_block();
      if (lane == 0) sc.run[nOut] = pend;
      nOut++; pend = x;
    } else { pend.end = x.end; pend.isize = x.isize > pend.isize ? x.isize : pend.isize; }
  }
  __threadfence_block();
  if (lane == 0) sc.run[nOut] = pend;
  nOut++;
  __threadfence_block();
  return nOut;
}

// ---------------------------------------------------------------------------------------------
// k_lookup_l1: one wave per fragment (4 per workgroup, no workgroup barrier).
//   * probes the s sketch hashes in the open-addressing table (key -> offset,count,frequent)
//   * drops frequent seeds and compacts the sketch (Q.minmerTableQuery / Q.sketchSize, computeMap.hpp:834-839)
//   * FAST (<= 128 interval points, no skip_prefix grouping): gathers the points into LDS, sorts them in registers
//     (ascending packed key == (seqId, pos, CLOSE-before-OPEN), computeMap.hpp:885-907) and runs L1 on the spot --
//     the points never touch HBM
//   * otherwise (many points, -Y groups, a position group spanning contigs, or keepPoints for the parity API): reserves
//     slots in the global point buffer, gathers there and queues the fragment for k_sort_points_* + k_l1_sweep.
// ---------------------------------------------------------------------------------------------
// The table values of the sketch entries [base, base + 256) of a fragment, four per lane (entry base + u * 64 + lane): found[u] / val[u].
// Four sub-rounds are in flight together: their hash loads, filter tests / tag loads and first table slots are independent, so one
// memory round trip serves all of them instead of four.  Shared by k_lookup_l1 and k_gather_points.
template <bool TAGS>
__device__ __forceinline__ void mm_probe4(const SeedTable& T, const uint64_t* __restrict__ skHash, size_t fo, int cnt, int base, int lane,
                                          uint64_t (&h)[4], bool (&act)[4], bool (&found)[4], uint64_t (&val)[4]) {
  const HtSlot* __restrict__ ht = T.ht; const uint64_t htMask = T.mask;
  bool open[4];
#pragma unroll
  for (int u = 0; u < 4; u++) { const int r = base + u * 64 + lane; act[u] = r < cnt; h[u] = act[u] ? skHash[fo + r] : 0ull; }
  if constexpr (!TAGS) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      open[u] = act[u];
      if (T.filterMask && act[u]) { const uint64_t fb = mm_filter_bits(h[u]); open[u] = (T.filter[mm_filter_word(h[u], T.filterMask)] & fb) == fb; }
    }
    HtSlot sl[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { sl[u].key = MM_EMPTY; sl[u].val = 0; if (open[u]) sl[u] = ht[h[u] & htMask]; }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      found[u] = false; val[u] = 0;
      uint64_t slot = h[u] & htMask;
      while (open[u]) {                                            // first slot already loaded; further slots are rare (load <= 0.5)
        if (sl[u].key == h[u]) { found[u] = true; val[u] = sl[u].val; break; }
        if (sl[u].key == MM_EMPTY) break;
        slot = (slot + 1) & htMask;
        sl[u] = ht[slot];
      }
    }
  } else {
    // Tagged table (human-scale index).  One 16-byte load per seed fetches the tag bytes of its home bucket, out of an array 1/16 the
    // size of the table.  A slot is fetched only where a tag matches (a present seed, or one absent seed in ~40 by chance); an absent
    // seed ends at the first bucket with a free slot: its own, but for ~0.03 %.
    const uint8_t* __restrict__ tags = T.tags;
    uint4 tg[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { tg[u] = make_uint4(0u, 0u, 0u, 0u); if (act[u]) tg[u] = *(const uint4*)(tags + ((h[u] & htMask) & ~(uint64_t)(MM_TAG_BUCKET - 1))); }
    uint32_t cand[4]; bool emp[4]; HtSlot sl[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      mm_tag_scan(tg[u], mm_seed_tag(h[u]), cand[u], emp[u]);
      if (!act[u]) { cand[u] = 0; emp[u] = true; }
      sl[u].key = MM_EMPTY; sl[u].val = 0;
      if (cand[u]) sl[u] = ht[((h[u] & htMask) & ~(uint64_t)(MM_TAG_BUCKET - 1)) + (uint32_t)__builtin_ctz(cand[u])];   // the first candidates of all four sub-rounds travel together
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      found[u] = false; val[u] = 0;
      uint64_t b = (h[u] & htMask) & ~(uint64_t)(MM_TAG_BUCKET - 1);
      uint32_t cd = cand[u]; bool em = emp[u]; bool have = cd != 0;  // `have`: sl[u] holds the slot of cd's lowest bit
      while (cd || !em) {
        while (cd) {
          const uint32_t i = (uint32_t)__builtin_ctz(cd); cd &= cd - 1u;
          const HtSlot x = have ? sl[u] : ht[b + i];
          have = false;
          if (x.key == h[u]) { found[u] = true; val[u] = x.val; cd = 0; em = true; }
        }
        if (!em) {                                                   // a full bucket without the key: on to the next one
          b = (b + MM_TAG_BUCKET) & htMask;
          mm_tag_scan(*(const uint4*)(tags + b), mm_seed_tag(h[u]), cd, em);
        }
      }
    }
  }
}
// the long point runs of one probing sub-round of the fused kernel (lanes in mLong own a seed with more than 8 points), copied by the whole
// wave into the fragment's LDS list from their third point on; returns this lane's count of points that passed the seqId filters.  Not
// inlined: inside k_lookup_l1 the loop cost the uniform north_star workload 1.5 ms of registers and code layout (profiles/NOTES.md, round 5)
__device__ __noinline__ int mm_fused_long_runs(uint64_t mLong, int c, int my, uint64_t src, uint64_t* __restrict__ dst, const uint64_t* __restrict__ ptKeys,
                                               int self, int seqCounter, int skipSelf, int lowerTri, int lane) {
  int nValid = 0;
  while (mLong) {
    const int l = (int)__builtin_ctzll(mLong); mLong &= mLong - 1ull;
    const int cL = __shfl(c, l), myL = __shfl(my, l);
    const uint64_t srcL = mm_bcast64_shfl(src, l);
    for (int j = 2 + lane; j < cL; j += 64) {
      uint64_t key = ptKeys[srcL + j];
      const int seqId = (int)(key >> 33);
      bool drop = false;
      if (skipSelf && seqId == self) drop = true;
      if (lowerTri && !(seqCounter > seqId)) drop = true;
      if (drop) key = MM_EMPTY; else nValid++;
      dst[myL + j] = key;
    }
  }
  return nValid;
}
#define MM_LOOKUP_WPB 4             // waves (= fragments) per workgroup
#define MM_MID_MAXSKETCH 512        // k_lookup_mid (below): sketch sizes it serves,
#define MM_MID_MAXSEEDS 256         // surviving seeds WITH points whose runs its LDS lists (a fragment with more goes to the HBM path),
#define MM_MID_MAXKEEP 1024         // interval points that may survive its filter (sorted in registers, 16 per lane),
#define MM_MID_MAXPTS 16384         // and interval points of a fragment it takes (8 192 intervals: its 16-bit bin counters cannot overflow)
#define MM_L1_REGIONS 64            // L1 output cursors: a same-address atomic costs ~10 ns, so fragments spread over 64 of them
#define MM_L1_CURSOR_STRIDE 32      // u64 words between cursors (256 bytes)
// a joined run of fragment f as the L1 candidate the L2 stage reads
__device__ __forceinline__ void mm_store_candidate(mm_l1_candidate* __restrict__ l1, long long at, int f, const L1Run& x) {
  mm_l1_candidate o; o.frag = f; o.seqId = x.seq; o.rangeStartPos = x.start; o.rangeEndPos = x.end; o.intersectionSize = x.isize;
  l1[at] = o;
}
// The end of a fragment a lookup kernel finishes itself: its nOut candidates runs[0..nOut) go to region f mod 64 of the L1 buffer, filled
// from its own cursor (k_l1_compact closes the gaps afterwards).  Where they no longer fit, MM_PC_L1_OVERFLOW is raised and nOut becomes 0.
// Returns the position of the first one in the buffer (what l1Off[f] takes).
__device__ __forceinline__ unsigned long long mm_region_emit(int f, int& nOut, const L1Run* runs, mm_l1_candidate* __restrict__ l1, unsigned long long regionCap,
                                                             unsigned long long* __restrict__ l1Cursors, unsigned long long* __restrict__ counters, int lane) {
  const int region = f & (MM_L1_REGIONS - 1);
  unsigned long long at = 0;
  if (nOut > 0) {
    if (lane == 0) at = atomicAdd(&l1Cursors[(size_t)region * MM_L1_CURSOR_STRIDE], (unsigned long long)nOut);
    at = mm_bcast64_shfl(at, 0);
    if (at + (unsigned long long)nOut > regionCap) { if (lane == 0) atomicOr(&counters[MM_PC_L1_OVERFLOW], MM_OVERFLOWED); nOut = 0; }
  }
  const unsigned long long base = (unsigned long long)region * regionCap + at;
  for (int i = lane; i < nOut; i += 64) mm_store_candidate(l1, (long long)(base + i), f, runs[i]);
  return base;
}
template <int MAXPTS, bool TAGS>
__global__ void __launch_bounds__(MM_LOOKUP_WPB * 64, MAXPTS <= 128 ? 8 : MAXPTS <= 256 ? 6 : 5)
k_lookup_l1(int nFrags, int s, const DFrag* __restrict__ frags,
            const uint64_t* __restrict__ skHash, const int8_t* __restrict__ skStrand, const uint32_t* __restrict__ skCount,
            const SeedTable T, const uint64_t* __restrict__ ptKeys,
            const int32_t* __restrict__ readSelf, int seqCounterBase, MapFlags fl, int keepPoints,
            uint64_t* __restrict__ qHash, int8_t* __restrict__ qStrand,
            mm_frag_stats* __restrict__ stats, int64_t* __restrict__ ptOff, unsigned long long ptsCap,
            const int32_t* __restrict__ minHitsTab, const int32_t* __restrict__ cutoffs, int nCutoffs, int segLength,
            mm_l1_candidate* __restrict__ l1, unsigned long long regionCap, unsigned long long* __restrict__ l1Cursors,
            int64_t* __restrict__ l1Off, int32_t* __restrict__ bigList, int32_t* __restrict__ midList,
            unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS */) {
  typedef FuseScratchT<MAXPTS> FuseScratch;
  __shared__ FuseScratch scratch[MM_LOOKUP_WPB];
  const int wv = threadIdx.x >> 6;
  const int f = blockIdx.x * MM_LOOKUP_WPB + wv;
  const bool live = f < nFrags;
  FuseScratch& sc = scratch[wv];
  const int lane = (int)mm_lane();
  int nValid = 0, nOut = -1, outIdx = 0, P = 0, cnt = 0;
  uint64_t lastHash = 0;
  if (live) {
  cnt = (int)skCount[f];
  const size_t fo = (size_t)f * s;
  // per-read metadata early: nothing below depends on the probes to fetch it
  const int readId = frags[f].readId;
  const int self = readSelf[readId], seqCounter = seqCounterBase + readId;
  lastHash = cnt ? skHash[fo + cnt - 1] : 0ull;
  // The interval points are gathered into LDS batch by batch (256 sketch entries are probed at a time), as long as they fit (MAXPTS):
  // a sketch of more than 256 entries stays on the fused path too.  The order of the points is irrelevant: they are sorted next.
  bool fuseOk = !keepPoints && !fl.skipPrefix;                     // wave-uniform
  int done = 0;                                                    // points in sc.a so far
  auto put = [&](int at, uint64_t key) {
    const int seqId = (int)(key >> 33);
    bool drop = false;
    if (fl.skipSelf && seqId == self) drop = true;
    if (fl.lowerTri && !(seqCounter > seqId)) drop = true;
    if (drop) key = MM_EMPTY; else nValid++;
    sc.a[at] = key;
  };
  bool anyDrop = false;                                            // a frequent seed has been removed so far (wave-uniform)
  for (int base = 0; base < cnt; base += 256) {
    uint64_t h[4], val[4]; bool act[4], found[4];
    mm_probe4<TAGS>(T, skHash, fo, cnt, base, lane, h, act, found, val);
    // The sketch after frequent-seed removal goes to qHash/qStrand only if a seed was removed: otherwise it equals the raw sketch, and
    // readers (k_l2_locate, mm_query_sketch_download) take that instead (rawSketchSize == sketchSize in the fragment's stats).  In a
    // sketch of several batches the first removal back-fills the batches before it, which were the raw sketch unchanged.
    {
      bool drop = false;
#pragma unroll
      for (int u = 0; u < 4; u++) drop |= act[u] && found[u] && (val[u] & 1ull);
      if (__ballot(drop) != 0 && !anyDrop) {
        for (int i = lane; i < base; i += 64) { qHash[fo + i] = skHash[fo + i]; qStrand[fo + i] = skStrand[fo + i]; }
        anyDrop = true;
      }
    }
    int cU[4]; uint64_t src[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int r = base + u * 64 + lane;
      const bool keep = act[u] && !(found[u] && (val[u] & 1ull));
      const uint64_t m = __ballot(keep);
      if (keep && anyDrop) {
        const int idx = outIdx + (int)mm_popc_below(m);
        qHash[fo + idx] = h[u]; qStrand[fo + idx] = skStrand[fo + r];
      }
      const bool kf = keep && found[u];
      src[u] = val[u] >> 24;
      cU[u] = kf ? (int)((val[u] >> 1) & 0x7fffffull) : 0;
      outIdx += __popcll(m);
    }
    const int Pb = mm_wave_sum(cU[0] + cU[1] + cU[2] + cU[3]);
    P += Pb;
    if (fuseOk && Pb > 0) {
      if (done + Pb > MAXPTS) fuseOk = false;
      else {
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int c = cU[u];
          const int my = done + mm_wave_excl_scan(c);
          uint64_t k0 = MM_EMPTY, k1 = MM_EMPTY;
          if (c > 0) k0 = ptKeys[src[u]];
          if (c > 1) k1 = ptKeys[src[u] + 1];
          if (c > 0) put(my, k0);
          if (c > 1) put(my + 1, k1);
          // the rest of a short run by the lane that owns the seed, of a long one (a seed of a repeat family: up to hundreds of points
          // that still fit the fused list) by the whole wave, as in mm_gather_points
          const bool longRun = c > 8;
          if (!longRun) for (int j = 2; j < c; j++) put(my + j, ptKeys[src[u] + j]);
          const uint64_t mLong = mm_ballot(longRun);
          if (mLong) nValid += mm_fused_long_runs(mLong, c, my, src[u], sc.a, ptKeys, self, seqCounter, fl.skipSelf, fl.lowerTri, lane);   // (out of line: the hot path keeps its registers)
          done += mm_wave_sum(c);
        }
      }
    }
  }
  const int minHits0 = outIdx > 0 ? minHitsTab[outIdx] : 0;
  if (fuseOk && minHits0 > 0) {
    if (P == 0) nOut = 0;
    else {
      nValid = mm_wave_sum(nValid);
      const int padTo = P <= 64 ? 64 : P <= 128 ? 128 : P <= 256 ? 256 : 512;
      for (int j = P + lane; j < padTo; j += 64) sc.a[j] = MM_EMPTY;
      __threadfence_block();
      if (P <= 64) {
        uint64_t k[1] = {sc.a[lane]};
        mm_wave_bitonic<1>(k, lane);
        nOut = mm_l1_fused<1>(k, sc, outIdx, minHits0, fl.hg, cutoffs, nCutoffs, s, segLength, lane);
      } else if (P <= 128) {
        uint64_t k[2] = {sc.a[lane * 2], sc.a[lane * 2 + 1]};
        mm_wave_bitonic<2>(k, lane);
        nOut = mm_l1_fused<2>(k, sc, outIdx, minHits0, fl.hg, cutoffs, nCutoffs, s, segLength, lane);
      } else if constexpr (MAXPTS >= 256) {
        if (P <= 256) {
          uint64_t k[4] = {sc.a[lane * 4], sc.a[lane * 4 + 1], sc.a[lane * 4 + 2], sc.a[lane * 4 + 3]};
          mm_wave_bitonic<4>(k, lane);
          nOut = mm_l1_fused<4>(k, sc, outIdx, minHits0, fl.hg, cutoffs, nCutoffs, s, segLength, lane);
        } else if constexpr (MAXPTS >= 512) {
          uint64_t k[8];
#pragma unroll
          for (int e = 0; e < 8; e++) k[e] = sc.a[lane * 8 + e];
          mm_wave_bitonic<8>(k, lane);
          nOut = mm_l1_fused<8>(k, sc, outIdx, minHits0, fl.hg, cutoffs, nCutoffs, s, segLength, lane);
        }
      }
    }
  }
  // more points than the registers sort, nothing else in the way: k_lookup_mid filters them in LDS first (the fragment stays off the HBM
  // path unless more than 512 of its points can matter to L1)
  const bool toMid = nOut < 0 && midList && !fuseOk && !keepPoints && !fl.skipPrefix && minHits0 > 1 && cnt <= MM_MID_MAXSKETCH && P <= MM_MID_MAXPTS;
  if (toMid) {
    if (lane == 0) {
      mm_frag_stats st;
      st.rawSketchSize = cnt; st.sketchSize = outIdx; st.maxHash = lastHash; st.nPoints = 0; st.nL1 = 0; stats[f] = st;
      ptOff[2 * f] = 0; ptOff[2 * f + 1] = 0; l1Off[f] = 0;
      midList[atomicAdd(&counters[MM_PC_MID_LEN], 1ull)] = f;
    }
  } else if (nOut < 0) {
    // slow path: the fragment's points go to HBM -- gathered by k_gather_points (which looks the seeds up once more: this kernel keeps no
    // per-seed value beyond the batch it is probing), sorted and swept by the follow-up kernels.  Here: the slots (a power of two above
    // 64 for the sorters) and the queue entry.
    int slots = P;
    if (P > 64) { slots = 128; while (slots < P) slots <<= 1; }
    else if (keepPoints == 2 && P > 0) { slots = 2; while (slots < P) slots <<= 1; }      // windowed mode: every list goes through the LDS / HBM sorters
    if (lane == 0) {
      unsigned long long off = 0;
      if (slots > 0) off = atomicAdd(&counters[MM_PC_POINT_CURSOR], (unsigned long long)slots);
      bool ok = true;
      if (slots > 0 && off + (unsigned long long)slots > ptsCap) { ok = false; atomicOr(&counters[MM_PC_POINT_OVERFLOW], MM_OVERFLOWED); }
      mm_frag_stats st;
      st.rawSketchSize = cnt; st.sketchSize = outIdx; st.maxHash = lastHash; st.nPoints = 0; st.nL1 = 0; stats[f] = st;
      ptOff[2 * f] = (int64_t)off; ptOff[2 * f + 1] = ok ? (int64_t)slots : 0; l1Off[f] = 0;
      if (slots > 0 && ok) bigList[atomicAdd(&counters[MM_PC_BIG_LEN], 1ull)] = f;
    }
  }
  }  // live
  if (live && nOut >= 0) {                                         // fast path complete: emit the candidates
    const unsigned long long base = mm_region_emit(f, nOut, sc.run, l1, regionCap, l1Cursors, counters, lane);
    if (lane == 0) {
      mm_frag_stats st;
      st.rawSketchSize = cnt; st.sketchSize = outIdx; st.maxHash = lastHash; st.nPoints = nValid; st.nL1 = nOut; stats[f] = st;
      ptOff[2 * f] = 0; ptOff[2 * f + 1] = 0; l1Off[f] = (int64_t)base;
    }
  }
}

// k_gather_points: the interval points of the fragments k_lookup_l1 queued (more points than its registers hold, -Y reference groups,
// --noSplit, MM_OPT_KEEP_POINTS) -> the slots it reserved for them in HBM, one wave per queued fragment: the sketch is looked up again,
// batch by batch, and every surviving seed's point run is copied (getSeedIntervalPoints, computeMap.hpp:857-912, with the seqId
// filters of :891-896).  ids (windowed mode): the seed every point came from.
template <bool TAGS>
__global__ void __launch_bounds__(256)
k_gather_points(int nList, const int32_t* __restrict__ list, int s, const DFrag* __restrict__ frags, const uint64_t* __restrict__ skHash, const uint32_t* __restrict__ skCount,
                const SeedTable T, const uint64_t* __restrict__ ptKeys, const int32_t* __restrict__ refGroup, const int32_t* __restrict__ readGroup, const int32_t* __restrict__ readSelf,
                int seqCounterBase, MapFlags fl, mm_frag_stats* __restrict__ stats, const int64_t* __restrict__ ptOff, uint64_t* __restrict__ pts, uint16_t* __restrict__ ptIds,
                int32_t* __restrict__ ptKept, const unsigned long long* __restrict__ nDev) {
  if (nDev) nList = (int)*nDev;
  for (int li = blockIdx.x * 4 + (threadIdx.x >> 6); li < nList; li += gridDim.x * 4) {
  const int f = list[li];
  const int lane = (int)mm_lane();
  const int64_t off = ptOff[2 * f]; const int slots = (int)ptOff[2 * f + 1];
  if (slots <= 0) continue;
  const int cnt = (int)skCount[f];
  const size_t fo = (size_t)f * s;
  const int readId = frags[f].readId;
  const int rg = readGroup[readId], self = readSelf[readId], seqCounter = seqCounterBase + readId;
  int at = 0, nValid = 0;
  uint16_t* idDst = ptIds ? ptIds + off : nullptr;
  for (int base = 0; base < cnt; base += 256) {
    uint64_t h[4], val[4]; bool act[4], found[4];
    mm_probe4<TAGS>(T, skHash, fo, cnt, base, lane, h, act, found, val);
#pragma unroll
    for (int u = 0; u < 4; u++) val[u] = (act[u] && found[u] && !(val[u] & 1ull)) ? val[u] : 0ull;
    nValid += mm_gather_points(pts + off, at, base >> 6, 4, [&](int rd) { return rd == 0 ? val[0] : rd == 1 ? val[1] : rd == 2 ? val[2] : val[3]; },
                               ptKeys, refGroup, rg, self, seqCounter, fl, lane, idDst);
  }
  for (int j = at + lane; j < slots; j += 64) pts[off + j] = MM_EMPTY;
  if (lane == 0) { stats[f].nPoints = nValid; ptKept[f] = nValid; }      // ptKept: the points the L1 kernels will find at the head of the sorted list
  }
}

// k_filter_points: drops, BEFORE the sort, the interval points of a queued fragment that cannot matter to computeL1CandidateRegions
// (computeMap.hpp:916-1116, windowLen == 0).  Against a repeat-rich reference a fragment brings hundreds of scattered single hits with it
// (the lists that overflow the fused kernel are mostly those): the bitonic sorters paid for them with two thirds of a pass
// (profiles/r13a: 75 of 183 ms at the repeat-rich north_star workload).  Rule (tests/l1filter.py is its model, tests/test_l1_point_filter.py
// checks it against the oracle's literal L1 on fuzzed point sets): the gathered list is a sequence of (OPEN, CLOSE) pairs, one per
// interval [o, c) of a contig; the overlap count of a position is at most the number of intervals that intersect its 4 096-position bin, so
// an interval none of whose bins is intersected by minimumHits intervals covers no position that reaches minimumHits -- it neither starts,
// ends nor raises a candidate -- and goes, unless it holds the first or the last point of its contig: the reference's sweep groups points
// by `pos` alone (:967, :1047-1051), so the last point of one contig and the first of the next can share a group, and with both boundary
// groups kept whole that seam behaves as it did.  Bins are counted in a hashed LDS table (collisions only raise counts: more is kept, never
// less); a fragment with an interval over more than MM_FILT_MAXSPAN bins or with more contigs than the per-wave table holds is left as
// it is.  One wave per queued fragment, in place; the list's length (ptOff[2f+1], what the sorters go by) shrinks with it.
#define MM_FILT_SHIFT 12
#define MM_FILT_SLOTS 2048
#define MM_FILT_CONTIGS 128
#define MM_FILT_MAXSPAN 64
__device__ __forceinline__ uint32_t mm_bin_slot(uint32_t seq, uint32_t b) { return ((seq * 0x9E3779B1u + b * 0x85EBCA77u) >> 7) & (MM_FILT_SLOTS - 1); }
__global__ void __launch_bounds__(256)
k_filter_points(int nList, const int32_t* __restrict__ list, const mm_frag_stats* __restrict__ stats, const int32_t* __restrict__ minHitsTab,
                int64_t* __restrict__ ptOff, uint64_t* __restrict__ pts, int32_t* __restrict__ ptKept, const unsigned long long* __restrict__ nDev) {
  __shared__ uint32_t binCntAll[4][MM_FILT_SLOTS];
  __shared__ int32_t cKeyAll[4][MM_FILT_CONTIGS];
  __shared__ uint32_t cMinAll[4][MM_FILT_CONTIGS], cMaxAll[4][MM_FILT_CONTIGS];
  const int wv = threadIdx.x >> 6, lane = (int)mm_lane();
  uint32_t* binCnt = binCntAll[wv]; int32_t* cKey = cKeyAll[wv]; uint32_t* cMin = cMinAll[wv]; uint32_t* cMax = cMaxAll[wv];
  if (nDev) nList = (int)*nDev;
  for (int li = blockIdx.x * 4 + wv; li < nList; li += gridDim.x * 4) {
    const int f = list[li];
    const int64_t off = ptOff[2 * f]; const int slots = (int)ptOff[2 * f + 1];
    if (slots <= 2) continue;
    const mm_frag_stats st = stats[f];
    const int minHits = st.sketchSize > 0 ? minHitsTab[st.sketchSize] : 0;
    if (minHits <= 1) continue;                                    // every interval reaches a count of 1 (minimumHits 0: the literal sweep takes the list whole)
    const int pairs = slots >> 1;
    for (int i = lane; i < MM_FILT_SLOTS; i += 64) binCnt[i] = 0u;
    for (int i = lane; i < MM_FILT_CONTIGS; i += 64) { cKey[i] = -1; cMin[i] = 0xFFFFFFFFu; cMax[i] = 0u; }
    __threadfence_block();
    uint64_t* a = pts + off;
    bool giveUp = false;
    for (int i = lane; i < pairs; i += 64) {
      const uint64_t O = a[2 * i], C = a[2 * i + 1];
      if (O == MM_EMPTY) continue;
      const uint32_t seq = (uint32_t)(O >> 33), o = (uint32_t)(O >> 1), c = (uint32_t)(C >> 1);
      const uint32_t b0 = o >> MM_FILT_SHIFT, b1 = (c - 1u) >> MM_FILT_SHIFT;
      if (C == MM_EMPTY || c <= o || b1 - b0 >= (uint32_t)MM_FILT_MAXSPAN) { giveUp = true; continue; }
      for (uint32_t b = b0; b <= b1; b++) atomicAdd(&binCnt[mm_bin_slot(seq, b)], 1u);
      uint32_t sl = (seq * 0x9E3779B1u) >> 25;                       // 7 bits
      int tries = 0;
      for (; tries < MM_FILT_CONTIGS; tries++) {
        const int32_t prev = atomicCAS(&cKey[sl], -1, (int32_t)seq);
        if (prev == -1 || prev == (int32_t)seq) { atomicMin(&cMin[sl], o); atomicMax(&cMax[sl], c); break; }
        sl = (sl + 1u) & (MM_FILT_CONTIGS - 1);
      }
      if (tries == MM_FILT_CONTIGS) giveUp = true;
    }
    __threadfence_block();
    if (mm_ballot(giveUp)) continue;                               // left as it is (ptKept[f] is what k_gather_points wrote)
    int cursor = 0;                                                // pairs kept so far (wave-uniform)
    for (int base = 0; base < pairs; base += 64) {
      const int i = base + lane;
      uint64_t O = MM_EMPTY, C = MM_EMPTY;
      if (i < pairs) { O = a[2 * i]; C = a[2 * i + 1]; }
      bool keep = false;
      if (O != MM_EMPTY) {
        const uint32_t seq = (uint32_t)(O >> 33), o = (uint32_t)(O >> 1), c = (uint32_t)(C >> 1);
        const uint32_t b0 = o >> MM_FILT_SHIFT, b1 = (c - 1u) >> MM_FILT_SHIFT;
        for (uint32_t b = b0; b <= b1; b++) keep = keep || binCnt[mm_bin_slot(seq, b)] >= (uint32_t)minHits;
        uint32_t sl = (seq * 0x9E3779B1u) >> 25;
        while (cKey[sl] != (int32_t)seq) sl = (sl + 1u) & (MM_FILT_CONTIGS - 1);
        keep = keep || o == cMin[sl] || c == cMax[sl];               // the contig's first / last position group stays whole
      }
      const uint64_t m = mm_ballot(keep);
      // in place: every lane of this round has read its pair before anybody writes, and a pair only ever moves down
      if (keep) { const int at = cursor + (int)mm_popc_below(m); a[2 * at] = O; a[2 * at + 1] = C; }
      cursor += (int)__popcll(m);
    }
    const int kept = 2 * cursor;
    int newSlots = kept;
    if (kept > 64) { newSlots = 128; while (newSlots < kept) newSlots <<= 1; }
    for (int j = kept + lane; j < newSlots; j += 64) a[j] = MM_EMPTY;
    if (lane == 0) { ptOff[2 * f + 1] = (int64_t)newSlots; ptKept[f] = kept; }
    __threadfence_block();
  }
}

// k_lookup_mid: the fragments whose interval points outnumber what k_lookup_l1 sorts in registers (against a repeat-rich reference 31 % of
// the north_star fragments: hundreds of scattered single hits each) -- WITHOUT the trip through HBM (k_gather_points -> k_filter_points ->
// sorters -> k_l1_stream: 33 of that workload's 125 ms).  One wave per queued fragment: the seeds are probed once more and their table
// answers kept in LDS; a first sweep over the seeds' point runs counts, per 4 096-position bin, the intervals that intersect it (and per
// contig the first and last position), a second sweep keeps the intervals k_filter_points' rule keeps (same bins, same hashed table, same
// boundary rule: tests/l1filter.py is the model) and writes them into the LDS list; at most 512 survivors are sorted in registers and
// swept by mm_l1_fused exactly as in k_lookup_l1, and the candidates go to the same region cursors.  A fragment with more survivors, with
// an interval the filter gives up on, or whose sorted list needs the literal sweep is queued for the HBM path as k_lookup_l1 would have.
// 513 .. 1 024 surviving points: sixteen per lane.  Out of line: the common sizes keep their registers.
__device__ __noinline__ int mm_mid_sort16(FuseScratchT<MM_MID_MAXKEEP>& sc, int sketchSizeQ, int minHits, int hg, const int32_t* __restrict__ cutoffs, int nCutoffs,
                                          int sParam, int segLength, int lane) {
  uint64_t k[16];
#pragma unroll
  for (int e = 0; e < 16; e++) k[e] = sc.a[lane * 16 + e];
  mm_wave_bitonic<16>(k, lane);
  return mm_l1_fused<16>(k, sc, sketchSizeQ, minHits, hg, cutoffs, nCutoffs, sParam, segLength, lane);
}
// one tier of the register sorters: the padded LDS list sc.a[0 .. 64 R), R points per lane, sorted and swept by the fused L1
template <int R, class FuseScratch>
__device__ __forceinline__ int mm_sort_fuse_tier(FuseScratch& sc, int sketchSizeQ, int minHits, int hg, const int32_t* __restrict__ cutoffs, int nCutoffs,
                                                 int sParam, int segLength, int lane) {
  uint64_t k[R];
#pragma unroll
  for (int e = 0; e < R; e++) k[e] = sc.a[lane * R + e];
  mm_wave_bitonic<R>(k, lane);
  return mm_l1_fused<R>(k, sc, sketchSizeQ, minHits, hg, cutoffs, nCutoffs, sParam, segLength, lane);
}
// the ladder of the register sorters for K <= 512 points at the head of sc.a, padded to a tier: the tier that holds them.  (The sixteen-per-lane
// tier stays with its kernel: mm_mid_sort16's call here, the same steps in line in k_lookup_groups.)
template <class FuseScratch>
__device__ __forceinline__ int mm_sort_fuse(FuseScratch& sc, int K, int sketchSizeQ, int minHits, int hg, const int32_t* __restrict__ cutoffs, int nCutoffs,
                                            int sParam, int segLength, int lane) {
  if (K <= 64) return mm_sort_fuse_tier<1>(sc, sketchSizeQ, minHits, hg, cutoffs, nCutoffs, sParam, segLength, lane);
  if (K <= 128) return mm_sort_fuse_tier<2>(sc, sketchSizeQ, minHits, hg, cutoffs, nCutoffs, sParam, segLength, lane);
  if (K <= 256) return mm_sort_fuse_tier<4>(sc, sketchSizeQ, minHits, hg, cutoffs, nCutoffs, sParam, segLength, lane);
  return mm_sort_fuse_tier<8>(sc, sketchSizeQ, minHits, hg, cutoffs, nCutoffs, sParam, segLength, lane);
}

template <bool TAGS>
__global__ void __launch_bounds__(64)
k_lookup_mid(int nList, const unsigned long long* __restrict__ nDev, const int32_t* __restrict__ list, int s, const DFrag* __restrict__ frags,
             const uint64_t* __restrict__ skHash, const uint32_t* __restrict__ skCount, const SeedTable T, const uint64_t* __restrict__ ptKeys,
             const int32_t* __restrict__ readSelf, int seqCounterBase, MapFlags fl, mm_frag_stats* __restrict__ stats, int64_t* __restrict__ ptOff,
             unsigned long long ptsCap, const int32_t* __restrict__ minHitsTab, const int32_t* __restrict__ cutoffs, int nCutoffs, int segLength,
             mm_l1_candidate* __restrict__ l1, unsigned long long regionCap, unsigned long long* __restrict__ l1Cursors, int64_t* __restrict__ l1Off,
             int32_t* __restrict__ bigList, unsigned long long* __restrict__ counters) {
  // LDS of the one wave: the survivors' list (FuseScratch::a) lives through both phases; the seeds' runs, the bins and the contig extents
  // are dead when the sort starts and share their bytes with what mm_l1_fused needs then (FuseScratch::v, ::run)
  typedef FuseScratchT<MM_MID_MAXKEEP> FuseScratch;
  struct Phase1 {
    uint64_t src[MM_MID_MAXSEEDS];                                 // first point of every surviving seed's run
    uint32_t pre[MM_MID_MAXSEEDS + 1];                             // intervals (point pairs) of the seeds before it
    uint32_t binCnt[MM_FILT_SLOTS / 2];                            // two 16-bit counters per word
    int32_t cKey[MM_FILT_CONTIGS]; uint32_t cMin[MM_FILT_CONTIGS], cMax[MM_FILT_CONTIGS];
  };
  constexpr size_t kTail = sizeof(FuseScratch) - offsetof(FuseScratch, v);
  constexpr size_t kBytes = offsetof(FuseScratch, v) + (sizeof(Phase1) > kTail ? sizeof(Phase1) : kTail);
  __shared__ __attribute__((aligned(16))) unsigned char smem[kBytes];
  FuseScratch& sc = *(FuseScratch*)smem;
  Phase1& ph = *(Phase1*)(smem + offsetof(FuseScratch, v));
  const int lane = (int)mm_lane();
  if (nDev) nList = (int)*nDev;
  for (int li = blockIdx.x; li < nList; li += gridDim.x) {
    const int f = list[li];
    const int cnt = (int)skCount[f];
    const size_t fo = (size_t)f * s;
    const int readId = frags[f].readId;
    const int self = readSelf[readId], seqCounter = seqCounterBase + readId;
    const mm_frag_stats st0 = stats[f];
    const int outIdx = st0.sketchSize;
    const int minHits = outIdx > 0 ? minHitsTab[outIdx] : 0;
    for (int i = lane; i < MM_FILT_SLOTS / 2; i += 64) ph.binCnt[i] = 0u;
    for (int i = lane; i < MM_FILT_CONTIGS; i += 64) { ph.cKey[i] = -1; ph.cMin[i] = 0xFFFFFFFFu; ph.cMax[i] = 0u; }
    // the seeds once more; those with points are listed densely: run start + intervals before it
    int nSeeds = 0, nPairs = 0, P = 0; bool giveUp = false;
    for (int base = 0; base < cnt; base += 256) {
      uint64_t h[4], val[4]; bool act[4], found[4];
      mm_probe4<TAGS>(T, skHash, fo, cnt, base, lane, h, act, found, val);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const bool kf = act[u] && found[u] && !(val[u] & 1ull);
        const int c = kf ? (int)((val[u] >> 1) & 0x7fffffull) : 0;
        if (c & 1) giveUp = true;                                  // (never: a hash's points are its intervals' two ends)
        const uint64_t m = mm_ballot(c > 0);
        const int at = nSeeds + (int)mm_popc_below(m);
        const int before = nPairs + mm_wave_excl_scan(c >> 1);
        if (c > 0 && at < MM_MID_MAXSEEDS) { ph.src[at] = val[u] >> 24; ph.pre[at] = (uint32_t)before; }
        nSeeds += (int)__popcll(m); nPairs += mm_wave_sum(c >> 1); P += mm_wave_sum(c);
      }
    }
    if (nSeeds > MM_MID_MAXSEEDS) { giveUp = true; nSeeds = MM_MID_MAXSEEDS; nPairs = 0; }
    if (lane == 0) ph.pre[nSeeds] = (uint32_t)nPairs;
    __threadfence_block();
    // interval g of the fragment = pair (g - pre[j]) of seed j's run, j by binary search: every lane of every round has one
    auto pairAt = [&](int g, uint64_t& O, uint64_t& C) {
      int lo = 0, hi = nSeeds - 1;
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int)ph.pre[mid] <= g) lo = mid; else hi = mid - 1; }
      const ulonglong2 oc = *(const ulonglong2*)(ptKeys + ph.src[lo] + 2 * (uint64_t)(g - (int)ph.pre[lo]));
      O = oc.x; C = oc.y;
    };
    auto dropped = [&](uint64_t key) {
      const int seqId = (int)(key >> 33);
      return (fl.skipSelf && seqId == self) || (fl.lowerTri && !(seqCounter > seqId));
    };
    // sweep 1: intervals per 4 096-position bin, first / last position per contig
    int nValid = 0;
    for (int g0 = 0; g0 < nPairs; g0 += 128) {
      uint64_t O[2], C[2]; bool on[2];
#pragma unroll
      for (int u = 0; u < 2; u++) { const int g = g0 + u * 64 + lane; on[u] = g < nPairs; O[u] = C[u] = MM_EMPTY; if (on[u]) pairAt(g, O[u], C[u]); }
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (!on[u] || dropped(O[u])) continue;
        nValid += 2;
        const uint32_t seq = (uint32_t)(O[u] >> 33), o = (uint32_t)(O[u] >> 1), c = (uint32_t)(C[u] >> 1);
        const uint32_t b0 = o >> MM_FILT_SHIFT, b1 = (c - 1u) >> MM_FILT_SHIFT;
        if (c <= o || b1 - b0 >= (uint32_t)MM_FILT_MAXSPAN || (uint32_t)(C[u] >> 33) != seq) { giveUp = true; continue; }
        for (uint32_t b = b0; b <= b1; b++) { const uint32_t sl = mm_bin_slot(seq, b); atomicAdd(&ph.binCnt[sl >> 1], 1u << (16 * (sl & 1u))); }
        uint32_t sl = (seq * 0x9E3779B1u) >> 25;
        int tries = 0;
        for (; tries < MM_FILT_CONTIGS; tries++) {
          const int32_t prev = atomicCAS(&ph.cKey[sl], -1, (int32_t)seq);
          if (prev == -1 || prev == (int32_t)seq) { atomicMin(&ph.cMin[sl], o); atomicMax(&ph.cMax[sl], c); break; }
          sl = (sl + 1u) & (MM_FILT_CONTIGS - 1);
        }
        if (tries == MM_FILT_CONTIGS) giveUp = true;
      }
    }
    __threadfence_block();
    nValid = mm_wave_sum(nValid);
    bool fallback = mm_ballot(giveUp) != 0ull;
    // sweep 2: the intervals that can matter (k_filter_points' rule), into the LDS list
    int cursor = 0;                                                // pairs kept so far (wave-uniform)
    for (int g0 = 0; g0 < nPairs && !fallback; g0 += 128) {
      uint64_t O[2], C[2]; bool keep[2];
#pragma unroll
      for (int u = 0; u < 2; u++) { const int g = g0 + u * 64 + lane; keep[u] = g < nPairs; O[u] = C[u] = MM_EMPTY; if (keep[u]) pairAt(g, O[u], C[u]); }
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (keep[u]) keep[u] = !dropped(O[u]);
        if (keep[u]) {
          const uint32_t seq = (uint32_t)(O[u] >> 33), o = (uint32_t)(O[u] >> 1), c = (uint32_t)(C[u] >> 1);
          const uint32_t b0 = o >> MM_FILT_SHIFT, b1 = (c - 1u) >> MM_FILT_SHIFT;
          bool k = false;
          for (uint32_t b = b0; b <= b1; b++) { const uint32_t sl = mm_bin_slot(seq, b); k = k || ((ph.binCnt[sl >> 1] >> (16 * (sl & 1u))) & 0xFFFFu) >= (uint32_t)minHits; }
          uint32_t sl = (seq * 0x9E3779B1u) >> 25;
          while (ph.cKey[sl] != (int32_t)seq) sl = (sl + 1u) & (MM_FILT_CONTIGS - 1);
          keep[u] = k || o == ph.cMin[sl] || c == ph.cMax[sl];
        }
        const uint64_t m = mm_ballot(keep[u]);
        const int k = (int)__popcll(m);
        if (cursor + k > MM_MID_MAXKEEP / 2) { fallback = true; break; }
        if (keep[u]) { const int at = cursor + (int)mm_popc_below(m); sc.a[2 * at] = O[u]; sc.a[2 * at + 1] = C[u]; }
        cursor += k;
      }
    }
    __threadfence_block();                                         // phase 1's LDS is free from here on
    int nOut = -1;
    if (!fallback) {
      const int K = 2 * cursor;
      if (K == 0) nOut = 0;
      else {
        const int padTo = K <= 64 ? 64 : K <= 128 ? 128 : K <= 256 ? 256 : K <= 512 ? 512 : 1024;
        for (int j = K + lane; j < padTo; j += 64) sc.a[j] = MM_EMPTY;
        __threadfence_block();
        if (K > 512) nOut = mm_mid_sort16(sc, outIdx, minHits, fl.hg, cutoffs, nCutoffs, s, segLength, lane);
        else nOut = mm_sort_fuse(sc, K, outIdx, minHits, fl.hg, cutoffs, nCutoffs, s, segLength, lane);
      }
    }
    if (nOut < 0) {                                                // to the HBM path after all, as k_lookup_l1 queues a fragment
      int slots = 128; while (slots < P) slots <<= 1;
      if (lane == 0) {
        const unsigned long long off = atomicAdd(&counters[MM_PC_POINT_CURSOR], (unsigned long long)slots);
        bool ok = true;
        if (off + (unsigned long long)slots > ptsCap) { ok = false; atomicOr(&counters[MM_PC_POINT_OVERFLOW], MM_OVERFLOWED); }
        ptOff[2 * f] = (int64_t)off; ptOff[2 * f + 1] = ok ? (int64_t)slots : 0; l1Off[f] = 0;
        if (ok) bigList[atomicAdd(&counters[MM_PC_BIG_LEN], 1ull)] = f;
      }
    } else {
      const unsigned long long base = mm_region_emit(f, nOut, sc.run, l1, regionCap, l1Cursors, counters, lane);
      if (lane == 0) {
        mm_frag_stats st = st0;
        st.nPoints = nValid; st.nL1 = nOut; stats[f] = st;
        ptOff[2 * f] = 0; ptOff[2 * f + 1] = 0; l1Off[f] = (int64_t)base;
      }
    }
    __threadfence_block();
  }
}

// k_lookup_groups (MM_OPT_L1_GROUP_FUSED): the fragments k_lookup_l1 queued under -Y reference groups (MM_FLAG_SKIP_PREFIX) -- every
// fragment with a point -- WITHOUT the trip through HBM (k_gather_points -> block-wide sort -> k_l1_stream_groups).  Map::doL1Mapping calls
// computeL1CandidateRegions once per run of sorted points whose contigs share a reference group (computeMap.hpp:1146-1165), and the groups
// number runs of consecutive contigs (Map::setRefGroups, :144-161; the host has checked that the array is non-decreasing), so one call's
// points are exactly "the fragment's points of one group": a few hundred, which the register sorters and mm_l1_fused take.  One wave per
// queued fragment: the seeds are probed once more and their point runs listed in LDS (as k_lookup_mid does); one sweep over the interval
// pairs applies the seqId filters of :891-896, notes every kept pair's group in a table of distinct groups with counts and leaves a
// one-byte group slot per pair; the groups are then taken in ascending order (= the order of their extents in the sorted list), each
// one's pairs copied to the sort list by their tags, sorted in registers and swept by mm_l1_fused with the fragment's minimumHits -- the
// HG step then works on this extent's own best count, and a position shared by the last point of one group and the first of the next
// lies in two calls, as in the reference.  The candidates of all extents collect in LDS, are claimed once from the fragment's region
// cursor and written in extent order, exactly as k_lookup_mid leaves a fragment.
// Handed over (list `handList`, which stands in for dBigList for the rest of the pass; the point slots are those k_lookup_l1 reserved):
// more than MM_GRP_MAXPTS points, MM_GRP_MAXGROUPS groups, MM_GRP_MAXKEEP kept points in one group or MM_GRP_MAXCAND candidates;
// mm_l1_fused's -1 for any extent (a position group across two contigs inside it, more than MM_FUSE_MAXRUNS runs); minimumHits <= 0.
// LDS per wave: 13 312 (FuseScratch) + 4 096 + 2 052 (seed runs) + 4 096 (tags) + 512 (groups) + 2 048 (candidates), 26 128 bytes with
// alignment: six waves per CU of 160 KB.  The compiler reports (gfx950, -O3) 148 VGPRs (150 with the tagged seed table), 26 128 bytes of
// LDS and no scratch; the 16-per-lane tier is in line for that (a call to mm_mid_sort16 brings 12 bytes of register saves).
#define MM_GRP_MAXSEEDS MM_MID_MAXSKETCH   // seeds with points: every sketch the kernel is launched for fits
#define MM_GRP_MAXPTS 8192                 // interval points of the fragment's runs, before the filters (4 096 tag bytes)
#define MM_GRP_MAXGROUPS 64                // distinct groups among the kept points (one per lane when they are ordered)
#define MM_GRP_MAXKEEP MM_MID_MAXKEEP      // kept points of one group (the 16-per-lane sorter)
#define MM_GRP_MAXCAND 128                 // candidates of the fragment (2 KB of LDS)
#define MM_GRP_NOTAG 0xFFu                 // tag of a pair the filters dropped
template <bool TAGS>
__global__ void __launch_bounds__(64)
k_lookup_groups(const unsigned long long* __restrict__ nDev, const int32_t* __restrict__ list, int s, const DFrag* __restrict__ frags,
                const uint64_t* __restrict__ skHash, const uint32_t* __restrict__ skCount, const SeedTable T, const uint64_t* __restrict__ ptKeys,
                const int32_t* __restrict__ refGroup, const int32_t* __restrict__ readGroup, const int32_t* __restrict__ readSelf, int seqCounterBase,
                MapFlags fl, mm_frag_stats* __restrict__ stats, int64_t* __restrict__ ptOff, const int32_t* __restrict__ minHitsTab,
                const int32_t* __restrict__ cutoffs, int nCutoffs, int segLength, mm_l1_candidate* __restrict__ l1, unsigned long long regionCap,
                unsigned long long* __restrict__ l1Cursors, int64_t* __restrict__ l1Off, int32_t* __restrict__ handList,
                unsigned long long* __restrict__ counters) {
  typedef FuseScratchT<MM_GRP_MAXKEEP> FuseScratch;
  __shared__ FuseScratch sc;
  __shared__ uint64_t src[MM_GRP_MAXSEEDS];                        // first point of every surviving seed's run
  __shared__ uint32_t pre[MM_GRP_MAXSEEDS + 1];                    // intervals (point pairs) of the seeds before it
  __shared__ uint8_t tag[MM_GRP_MAXPTS / 2];                       // per interval: slot of its group in gKey, MM_GRP_NOTAG when dropped
  __shared__ int32_t gKey[MM_GRP_MAXGROUPS], gCnt[MM_GRP_MAXGROUPS];   // distinct groups of the kept intervals (-1: free) and their intervals
  __shared__ L1Run out[MM_GRP_MAXCAND];                            // the fragment's candidates, extent by extent
  const int lane = (int)mm_lane();
  const int nList = (int)*nDev;
  for (int li = blockIdx.x; li < nList; li += gridDim.x) {
    const int f = list[li];
    const int cnt = (int)skCount[f];
    const size_t fo = (size_t)f * s;
    const int readId = frags[f].readId;
    const int rg = readGroup[readId], self = readSelf[readId], seqCounter = seqCounterBase + readId;
    const mm_frag_stats st0 = stats[f];
    const int outIdx = st0.sketchSize;
    const int minHits = outIdx > 0 ? minHitsTab[outIdx] : 0;
    bool hand = minHits <= 0;                                      // wave-uniform: the fragment goes to the HBM point path
    gKey[lane] = -1; gCnt[lane] = 0;
    // the seeds once more; those with points are listed densely: run start + intervals before it
    int nSeeds = 0, nPairs = 0, P = 0; bool giveUp = false;
    for (int base = 0; base < cnt; base += 256) {
      uint64_t h[4], val[4]; bool act[4], found[4];
      mm_probe4<TAGS>(T, skHash, fo, cnt, base, lane, h, act, found, val);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const bool kf = act[u] && found[u] && !(val[u] & 1ull);
        const int c = kf ? (int)((val[u] >> 1) & 0x7fffffull) : 0;
        if (c & 1) giveUp = true;                                  // (never: a hash's points are its intervals' two ends)
        const uint64_t m = mm_ballot(c > 0);
        const int at = nSeeds + (int)mm_popc_below(m);
        const int before = nPairs + mm_wave_excl_scan(c >> 1);
        if (c > 0 && at < MM_GRP_MAXSEEDS) { src[at] = val[u] >> 24; pre[at] = (uint32_t)before; }
        nSeeds += (int)__popcll(m); nPairs += mm_wave_sum(c >> 1); P += mm_wave_sum(c);
      }
    }
    if (nSeeds > MM_GRP_MAXSEEDS) { hand = true; nSeeds = MM_GRP_MAXSEEDS; }
    if (P > MM_GRP_MAXPTS || mm_ballot(giveUp) != 0ull) hand = true;
    if (lane == 0) pre[nSeeds] = (uint32_t)nPairs;
    __threadfence_block();
    // interval g of the fragment = pair (g - pre[j]) of seed j's run, j by binary search
    auto pairAt = [&](int g, uint64_t& O, uint64_t& C) {
      int lo = 0, hi = nSeeds - 1;
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int)pre[mid] <= g) lo = mid; else hi = mid - 1; }
      const ulonglong2 oc = *(const ulonglong2*)(ptKeys + src[lo] + 2 * (uint64_t)(g - (int)pre[lo]));
      O = oc.x; C = oc.y;
    };
    // the one sweep over the intervals: filters, the group table, the tags
    int nValid = 0;
    giveUp = false;
    for (int g0 = 0; g0 < nPairs && !hand; g0 += 64) {
      const int g = g0 + lane;
      if (g < nPairs) {
        uint64_t O, C; pairAt(g, O, C);
        const int seqId = (int)(O >> 33);
        const int grp = refGroup[seqId];
        uint32_t t = MM_GRP_NOTAG;
        const bool drop = (fl.skipSelf && seqId == self) || (fl.skipPrefix && grp == rg) || (fl.lowerTri && !(seqCounter > seqId));
        if ((int)(C >> 33) != seqId || grp < 0) giveUp = true;
        else if (!drop) {
          uint32_t sl = ((uint32_t)grp * 0x9E3779B1u) >> 26;       // 6 bits
          int tries = 0;
          for (; tries < MM_GRP_MAXGROUPS; tries++) {
            const int32_t prev = atomicCAS(&gKey[sl], -1, grp);
            if (prev == -1 || prev == grp) { atomicAdd(&gCnt[sl], 1); t = sl; nValid += 2; break; }
            sl = (sl + 1u) & (MM_GRP_MAXGROUPS - 1);
          }
          if (tries == MM_GRP_MAXGROUPS) giveUp = true;            // a 65th group
        }
        tag[g] = (uint8_t)t;                                       // g < nPairs <= MM_GRP_MAXPTS / 2: checked above (P)
      }
    }
    __threadfence_block();
    if (mm_ballot(giveUp) != 0ull) hand = true;
    nValid = mm_wave_sum(nValid);
    // the groups in ascending order: (group, slot) sorted across the lanes
    int total = 0;                                                 // candidates in out[] so far (wave-uniform)
    if (!hand) {
      const int32_t myKey = gKey[lane];
      uint64_t ord[1] = {myKey >= 0 ? (((uint64_t)(uint32_t)myKey << 8) | (uint64_t)lane) : MM_EMPTY};
      mm_wave_bitonic<1>(ord, lane);
      const int nG = (int)__popcll(mm_ballot(ord[0] != MM_EMPTY));
      for (int gi = 0; gi < nG && !hand; gi++) {
        const int slot = __shfl((int)(uint32_t)ord[0], gi) & 0xff;
        const int K = 2 * gCnt[slot];
        if (K > MM_GRP_MAXKEEP) { hand = true; break; }
        int cursor = 0;                                            // pairs of this group copied so far (wave-uniform)
        for (int g0 = 0; g0 < nPairs; g0 += 64) {
          const int g = g0 + lane;
          const bool mine = g < nPairs && (int)tag[g] == slot;
          const uint64_t m = mm_ballot(mine);
          if (!m) continue;
          const int at = cursor + (int)mm_popc_below(m);
          if (mine && at < MM_GRP_MAXKEEP / 2) { uint64_t O, C; pairAt(g, O, C); sc.a[2 * at] = O; sc.a[2 * at + 1] = C; }
          cursor += (int)__popcll(m);
        }
        const int padTo = K <= 64 ? 64 : K <= 128 ? 128 : K <= 256 ? 256 : K <= 512 ? 512 : 1024;
        for (int j = K + lane; j < padTo; j += 64) sc.a[j] = MM_EMPTY;
        __threadfence_block();
        int nOut;
        if (K > 512) {                                             // mm_mid_sort16's form, in line: a call would bring the callee's register saves (scratch) with it
          uint64_t k[16];
#pragma unroll
          for (int e = 0; e < 16; e++) k[e] = sc.a[lane * 16 + e];
          mm_wave_bitonic<16>(k, lane); nOut = mm_l1_fused<16>(k, sc, outIdx, minHits, fl.hg, cutoffs, nCutoffs, s, segLength, lane);
        }
        else nOut = mm_sort_fuse(sc, K, outIdx, minHits, fl.hg, cutoffs, nCutoffs, s, segLength, lane);
        if (nOut < 0 || total + nOut > MM_GRP_MAXCAND) { hand = true; break; }
        for (int i = lane; i < nOut; i += 64) out[total + i] = sc.run[i];
        total += nOut;
        __threadfence_block();
      }
    }
    if (hand) {                                                    // the HBM point path takes it, in the slots k_lookup_l1 reserved
      if (lane == 0) handList[atomicAdd(&counters[MM_PC_GRP_LEN], 1ull)] = f;
    } else {
      int nOut = total;
      const unsigned long long base = mm_region_emit(f, nOut, out, l1, regionCap, l1Cursors, counters, lane);
      if (lane == 0) {
        mm_frag_stats st = st0;
        st.nPoints = nValid; st.nL1 = nOut; stats[f] = st;
        ptOff[2 * f] = 0; ptOff[2 * f + 1] = 0; l1Off[f] = (int64_t)base;
      }
    }
    __threadfence_block();
  }
}

// closes the gaps between the 64 regions of the L1 buffer: region r moves to its prefix position (into a second buffer), and
// the fragments' first-candidate offsets follow
struct L1Regions { unsigned long long prefix[MM_L1_REGIONS]; unsigned long long count[MM_L1_REGIONS]; };
// the regions' fill counts -> their prefix positions in the dense buffer (device-resident: no host round trip between the lookup kernel
// and the compaction) and the number of fused candidates (counters[MM_PC_L1_CAND])
__global__ void __launch_bounds__(64)
k_l1_regions(const unsigned long long* __restrict__ l1Cursors, unsigned long long regionCap, L1Regions* __restrict__ R, unsigned long long* __restrict__ counters) {
  const int r = threadIdx.x;
  unsigned long long n = l1Cursors[(size_t)r * MM_L1_CURSOR_STRIDE];
  if (n > regionCap) n = regionCap;                              // an overflowed region (counters[MM_PC_L1_OVERFLOW] is set): what was written
  const int ex = mm_wave_excl_scan((int)n);
  R->count[r] = n; R->prefix[r] = (unsigned long long)ex;
  if (r == 63) counters[MM_PC_L1_CAND] = (unsigned long long)ex + n;
}
__global__ void __launch_bounds__(256)
k_l1_compact(const mm_l1_candidate* __restrict__ src, mm_l1_candidate* __restrict__ dst, unsigned long long regionCap, const L1Regions* __restrict__ R) {
  const int r = blockIdx.y;
  const unsigned long long n = R->count[r], at = R->prefix[r];
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256)
    dst[at + i] = src[(unsigned long long)r * regionCap + i];
}
__global__ void __launch_bounds__(256)
k_l1_fix_offsets(int nFrags, const mm_frag_stats* __restrict__ stats, int64_t* __restrict__ l1Off, unsigned long long regionCap, const L1Regions* __restrict__ R) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= nFrags || stats[f].nL1 <= 0) return;
  const int r = f & (MM_L1_REGIONS - 1);
  l1Off[f] = l1Off[f] - (int64_t)((unsigned long long)r * regionCap) + (int64_t)R->prefix[r];
}

// Steady-state passes read the L1 stage's overflow flags (counters[MM_PC_POINT_OVERFLOW] interval points, counters[MM_PC_L1_OVERFLOW] L1 candidates) only when the whole
// pass is over, so the L2 stage must be kept off what an overflowed L1 stage left behind: a region that overflowed has never-written
// slots below its clamped count, the sweep path may have counted past the dense buffer, and more candidates than the previous pass
// sized the candidate-indexed buffers for (candCap) do not fit them either.  One thread, behind the last L1 kernel: any of these zeroes
// the candidate count -- every kernel of the L2 stage covers [0, counters[MM_PC_L1_CAND]) and k_l2_select returns on a set flag -- and leaves (or
// sets) the flag that makes the host redo the pass the sized way.
__global__ void k_l1_gate(unsigned long long* __restrict__ counters, unsigned long long candCap) {
  if (counters[MM_PC_POINT_OVERFLOW] | counters[MM_PC_L1_OVERFLOW]) counters[MM_PC_L1_CAND] = 0ull;
  else if (counters[MM_PC_L1_CAND] > candCap) { counters[MM_PC_L1_OVERFLOW] = MM_OVERFLOWED; counters[MM_PC_L1_CAND] = 0ull; }
}

// ---------------------------------------------------------------------------------------------
// point sorters for the queued fragments (ascending packed key == ascending (seqId, pos, CLOSE-before-OPEN))
// ---------------------------------------------------------------------------------------------
// <= 512 points: one wave per fragment, bitonic network over the lanes' registers
#define MM_SORT_WAVECAP 512
// The kernels over the queued fragments take the list's length from the device when nDev is given (the launcher then has not read it
// back: steady-state passes, one host synchronisation per pass) and walk the list with whatever grid they were given.
__global__ void __launch_bounds__(256)
k_sort_points_wave(int nList, const unsigned long long* __restrict__ nDev, const int32_t* __restrict__ list, const int64_t* __restrict__ ptOff, uint64_t* __restrict__ pts) {
  if (nDev) nList = (int)*nDev;
  for (int li = blockIdx.x * 4 + (threadIdx.x >> 6); li < nList; li += gridDim.x * 4) {
    const int f = list[li];
    const int64_t off = ptOff[2 * f]; const int n = (int)ptOff[2 * f + 1];
    if (n <= 1 || n > MM_SORT_WAVECAP) continue;
    const int lane = (int)mm_lane();
    // up to 512 points in the registers of one wave (the network of the fused kernel): no LDS, no barrier.  What k_filter_points leaves of
    // a repeat-rich fragment's list is a few hundred points; the workgroup-per-fragment LDS sorter below took 16 ms per 0.6 M such lists
    if (n <= 64) {
      uint64_t k[1] = {lane < n ? pts[off + lane] : MM_EMPTY};
      mm_wave_bitonic<1>(k, lane);
      if (lane < n) pts[off + lane] = k[0];
    } else if (n <= 128) {
      uint64_t k[2];
#pragma unroll
      for (int r = 0; r < 2; r++) k[r] = lane * 2 + r < n ? pts[off + lane * 2 + r] : MM_EMPTY;
      mm_wave_bitonic<2>(k, lane);
#pragma unroll
      for (int r = 0; r < 2; r++) if (lane * 2 + r < n) pts[off + lane * 2 + r] = k[r];
    } else if (n <= 256) {
      uint64_t k[4];
#pragma unroll
      for (int r = 0; r < 4; r++) k[r] = lane * 4 + r < n ? pts[off + lane * 4 + r] : MM_EMPTY;
      mm_wave_bitonic<4>(k, lane);
#pragma unroll
      for (int r = 0; r < 4; r++) if (lane * 4 + r < n) pts[off + lane * 4 + r] = k[r];
    } else {
      uint64_t k[8];
#pragma unroll
      for (int r = 0; r < 8; r++) k[r] = lane * 8 + r < n ? pts[off + lane * 8 + r] : MM_EMPTY;
      mm_wave_bitonic<8>(k, lane);
#pragma unroll
      for (int r = 0; r < 8; r++) if (lane * 8 + r < n) pts[off + lane * 8 + r] = k[r];
    }
  }
}

// 65..LDSCAP points (power of two): one 256-thread workgroup per fragment, bitonic sort staged in LDS
#define MM_SORT_LDSCAP 4096
// ids (may be null): a 16-bit payload that travels with its key (windowed mode: the seed of every point)
__global__ void __launch_bounds__(256)
k_sort_points_block(const unsigned int* __restrict__ nListDev, const int64_t* __restrict__ ptOff, uint64_t* __restrict__ pts, const int32_t* __restrict__ list, uint16_t* __restrict__ ids) {
  __shared__ uint64_t sk[MM_SORT_LDSCAP];
  __shared__ uint16_t si[MM_SORT_LDSCAP];
  const int nList = (int)*nListDev;
  for (int li = blockIdx.x; li < nList; li += gridDim.x) {
    const int f = list[li];
    const int64_t off = ptOff[2 * f]; const int n = (int)ptOff[2 * f + 1];
    for (int i = threadIdx.x; i < n; i += 256) { sk[i] = pts[off + i]; if (ids) si[i] = ids[off + i]; }
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = threadIdx.x; i < n; i += 256) {
          const int p = i ^ j;
          if (p > i) {
            const uint64_t a = sk[i], b = sk[p];
            if ((a > b) == ((i & k) == 0)) { sk[i] = b; sk[p] = a; if (ids) { const uint16_t t = si[i]; si[i] = si[p]; si[p] = t; } }
          }
        }
        __syncthreads();
      }
    for (int i = threadIdx.x; i < n; i += 256) { pts[off + i] = sk[i]; if (ids) ids[off + i] = si[i]; }
    __syncthreads();
  }
}

// > LDSCAP points: one 1024-thread workgroup per fragment, bitonic sort in global memory (rare: very repetitive seeds)
__global__ void __launch_bounds__(1024)
k_sort_points_global(const unsigned int* __restrict__ nListDev, const int64_t* __restrict__ ptOff, uint64_t* __restrict__ pts, const int32_t* __restrict__ list, uint16_t* __restrict__ ids) {
  const int nList = (int)*nListDev;
  for (int li = blockIdx.x; li < nList; li += gridDim.x) {
    const int f = list[li];
    const int64_t off = ptOff[2 * f]; const int64_t n = ptOff[2 * f + 1];
    uint64_t* a = pts + off;
    uint16_t* d = ids ? ids + off : nullptr;
    for (int64_t k = 2; k <= n; k <<= 1)
      for (int64_t j = k >> 1; j > 0; j >>= 1) {
        for (int64_t i = threadIdx.x; i < n; i += 1024) {
          const int64_t p = i ^ j;
          if (p > i) { const uint64_t x = a[i], y = a[p]; if ((x > y) == ((i & k) == 0)) { a[i] = y; a[p] = x; if (d) { const uint16_t t = d[i]; d[i] = d[p]; d[p] = t; } } }
        }
        __threadfence_block();
        __syncthreads();
      }
  }
}

// splits the queued fragments into the block / global sorter lists (wave-aggregated cursors)
__global__ void k_classify_sort(int nList, const unsigned long long* __restrict__ nDev, const int32_t* __restrict__ list, const int64_t* __restrict__ ptOff,
                                int32_t* __restrict__ listB, int32_t* __restrict__ listC, unsigned int* __restrict__ lens /* dCounters + MM_CW_SORT_LENS, 32-bit words */, int minB /* lists longer than this go to the LDS sorter */) {
  if (nDev) nList = (int)*nDev;
  for (int base = blockIdx.x * blockDim.x; base < nList; base += gridDim.x * blockDim.x) {
    const int li = base + threadIdx.x;
    int f = -1; int64_t n = 0;
    if (li < nList) { f = list[li]; n = ptOff[2 * f + 1]; }
    const bool isC = n > MM_SORT_LDSCAP, isB = !isC && n > minB;
    const uint64_t mB = __ballot(isB), mC = __ballot(isC);
    unsigned int bB = 0, bC = 0;
    if (mB && mm_lane() == (uint32_t)__builtin_ctzll(mB)) bB = atomicAdd(&lens[MM_SL_BLOCK], (unsigned int)__popcll(mB));
    if (mC && mm_lane() == (uint32_t)__builtin_ctzll(mC)) bC = atomicAdd(&lens[MM_SL_GLOBAL], (unsigned int)__popcll(mC));
    if (mB) bB = __shfl(bB, __builtin_ctzll(mB));
    if (mC) bC = __shfl(bC, __builtin_ctzll(mC));
    if (isB) listB[bB + mm_popc_below(mB)] = f;
    if (isC) listC[bC + mm_popc_below(mC)] = f;
  }
}

// ---------------------------------------------------------------------------------------------
// k_l1_stream: the L1 stage of a queued fragment by one WAVE, streaming its sorted points from HBM 64 at a time (coalesced) -- any
// number of points.  Same formulation as mm_l1_fused: the overlap count after a position group is the running sum of +1 (OPEN) / -1
// (CLOSE) up to its last point; pass 1 finds the best count (computeMap.hpp:948-999), pass 2 folds the groups whose count reaches
// minimumHits -- the last group never does, :1024-1098 -- into runs per contig and joins runs closer than segLength (:1102-1115).  The
// fold is sequential, as in the reference, but wave-uniform and only over the groups that start a run or end one (everything between
// two of those extends the run: a masked wave maximum).  A position group that spans two contigs or minimumHits <= 0 leaves the fragment to the literal k_l1_sweep
// (list `lit`).  Fragments with many points are the rule in repeat families (segmental duplications: every locus x copies), where the
// one-thread-per-fragment kernel costs 50-170 ns per fragment (profiles/r03j_repeat_probe.txt).
// ---------------------------------------------------------------------------------------------
#define MM_STREAM_BUF 64            // candidates kept in LDS by the counting pass (more: the writing pass runs again)
// What k_l1_stream and k_l1_stream_groups share, all in line.  L1Stream: the wave's view of a sorted point list, over an extent [b, e) of it
// (the whole list: 0, nPts) -- nothing outside the extent is a neighbour, and the carried overlap count starts at 0 at b.
struct L1Stream {
  const uint64_t* p; int lane;
  // one chunk of 64 points of the extent: key, overlap count after the point, whether it ends a position group
  __device__ __forceinline__ void chunk(int b, int e, int i0, int carry, uint64_t& k, int& run, bool& gLast, bool& mixed, int& sum) const {
    const int idx = i0 + lane;
    const bool valid = idx < e;
    k = valid ? p[idx] : MM_EMPTY;
    const uint64_t prv = (valid && idx > b) ? p[idx - 1] : MM_EMPTY;
    const uint64_t nxt = (idx + 1 < e) ? p[idx + 1] : MM_EMPTY;
    mixed = valid && prv != MM_EMPTY && (uint32_t)(prv >> 1) == (uint32_t)(k >> 1) && (prv >> 33) != (k >> 33);
    const int delta = valid ? ((k & 1ull) ? 1 : -1) : 0;
    run = carry + mm_wave_excl_scan(delta) + delta;
    gLast = valid && (nxt == MM_EMPTY || (uint32_t)(nxt >> 1) != (uint32_t)(k >> 1));
    sum = mm_wave_sum(delta);
  }
  // ---- pass 1 over the extent: best overlap count, number of groups, the mixed-group test ----
  __device__ __forceinline__ void pass1(int b, int e, int& best, int& G, bool& anyMixed) const {
    int carry = 0;
    for (int i0 = b; i0 < e; i0 += 64) {
      uint64_t k; int run, sum; bool gLast, mixed;
      chunk(b, e, i0, carry, k, run, gLast, mixed, sum);
      if (gLast && run > best) best = run;
      G += (int)__popcll(__ballot(gLast));
      anyMixed = anyMixed || __ballot(mixed) != 0;
      carry += sum;
    }
    best = mm_wave_max(best);
  }
};
// computeMap.hpp:984-998 for a call whose pass 1 found `best` over G groups: false when the call yields nothing; under --hg minimumHits is
// raised to the cutoff of the best count
__device__ __forceinline__ bool mm_l1_raise_min_hits(int best, int G, int S, int hg, int sParam, const int32_t* __restrict__ cutoffs, int nCutoffs, int& minHits) {
  bool go = G > 0;
  if (go && hg) {
    if (best < minHits) go = false;
    else {
      const double div = (double)sParam / 1000.0 > 1.0 ? (double)sParam / 1000.0 : 1.0;
      int ci = (int)((double)(best < S ? best : S) / div);
      if (ci >= nCutoffs) ci = nCutoffs - 1;
      const int cut = cutoffs[ci];
      minHits = cut > minHits ? cut : minHits;
    }
  }
  return go;
}
// the pending-candidate joiner of one pass over a fragment (L1Emit::run inside one computeL1CandidateRegions call): runs of one contig closer
// than segLength become one candidate; the counting pass keeps the first MM_STREAM_BUF in LDS, the writing pass stores from `base` on
struct L1Join {
  mm_l1_candidate* l1; L1Run* buf; long long base; int f, lane, segLength; bool write;
  int count = 0; bool have = false; L1Run pend{0, 0, 0, 0};
  __device__ __forceinline__ void flush() {
    if (have) {
      if (lane == 0) {
        if (write) mm_store_candidate(l1, base + count, f, pend);
        else if (count < MM_STREAM_BUF) buf[count] = pend;
      }
      count++; have = false;
    }
  }
  __device__ __forceinline__ void emit(int seq, int start, int end, int isize) {
    if (have && seq == pend.seq && !(start > pend.end + segLength)) { pend.end = end; pend.isize = isize > pend.isize ? isize : pend.isize; }
    else { flush(); pend.seq = seq; pend.start = start; pend.end = end; pend.isize = isize; have = true; }
  }
};
__global__ void __launch_bounds__(256)
k_l1_stream(int nList, const int32_t* __restrict__ list, const int64_t* __restrict__ ptOff, const uint64_t* __restrict__ pts,
            mm_frag_stats* __restrict__ stats, const int32_t* __restrict__ minHitsTab, const int32_t* __restrict__ cutoffs, int nCutoffs,
            int sParam, int segLength, int hg, mm_l1_candidate* __restrict__ l1, unsigned long long l1Cap, int64_t* __restrict__ l1Off,
            int32_t* __restrict__ lit, unsigned int* __restrict__ litCount, unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS: the L1 cursor and its overflow flag */,
            const unsigned long long* __restrict__ nDev, const int32_t* __restrict__ ptKept /* points at the head of the sorted list (k_gather_points / k_filter_points) */) {
  __shared__ L1Run bufAll[4][MM_STREAM_BUF];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  L1Run* buf = bufAll[wave];
  if (nDev) nList = (int)*nDev;
  auto one = [&](const int f) {
  const int nPts = ptKept[f], S = stats[f].sketchSize;
  if (nPts <= 0 || S <= 0) { if (lane == 0) { stats[f].nL1 = 0; l1Off[f] = 0; } return; }
  const L1Stream st{pts + ptOff[2 * f], lane};
  int minHits = minHitsTab[S];
  // pass 1 once, over the whole list
  int best = 0, G = 0; bool anyMixed = false;
  st.pass1(0, nPts, best, G, anyMixed);
  const bool go = mm_l1_raise_min_hits(best, G, S, hg, sParam, cutoffs, nCutoffs, minHits);
  if (anyMixed || minHits <= 0) {                                 // the literal kernel's business
    if (lane == 0) lit[atomicAdd(litCount, 1u)] = f;
    return;
  }

  // ---- pass 2: runs of flagged groups -> joined candidates; counted (the first MM_STREAM_BUF kept in LDS), then written ----
  int total = 0; long long base = 0;
  for (int pass = 0; pass < 2; pass++) {
    const bool write = pass == 1;
    L1Join jn{l1, buf, base, f, lane, segLength, write};
    if (go) {
      bool inRun = false; int rSeq = 0, rStart = 0, rEnd = 0, rSize = 0;
      int carry = 0, gBase = 0;
      bool prevFlagC = false; int prevSeqC = 0;                   // the last group of the chunks so far: flagged?, its contig
      for (int i0 = 0; i0 < nPts; i0 += 64) {
        uint64_t k; int run, sum; bool gLast, mixed;
        st.chunk(0, nPts, i0, carry, k, run, gLast, mixed, sum);
        carry += sum;
        const uint64_t GM = __ballot(gLast);
        if (!GM) continue;
        const int gidx = gBase + (int)mm_popc_below(GM);
        gBase += (int)__popcll(GM);
        const bool flag = gLast && gidx < G - 1 && run >= minHits;
        const uint64_t FM = __ballot(flag);
        const int gseq = (int)(k >> 33), gpos = (int)(uint32_t)(k >> 1);
        const int lastG = 63 - (int)__builtin_clzll(GM);
        const bool lastFlag = (FM >> lastG) & 1ull; const int lastSeq = __builtin_amdgcn_readlane(gseq, lastG);
        if (FM || prevFlagC) {
          // the group before this lane's: in the chunk, or the carried one
          const uint64_t below = GM & ((1ull << lane) - 1ull);
          const int pl = below ? 63 - (int)__builtin_clzll(below) : lane;
          const int sseq = __shfl(gseq, pl);
          const bool pf = below ? (((FM >> pl) & 1ull) != 0) : prevFlagC;
          const int ps = below ? sseq : prevSeqC;
          // a flagged group continues the run of a flagged predecessor on the same contig; the groups that matter are the others:
          // flagged ones that start a run, and unflagged ones right behind a flagged one, which end it.  Between two of those every
          // flagged group just extends the run: its end is the last one's position, its size the largest count.
          const uint64_t startM = __ballot(flag && !(pf && ps == gseq));
          const uint64_t breakM = __ballot(gLast && !flag && pf);
          auto extend = [&](int lo, int hi) {                       // flagged groups of the lanes [lo, hi) join the open run
            if (lo >= 64) return;
            const uint64_t m = FM & ~((1ull << lo) - 1ull) & (hi >= 64 ? ~0ull : ((1ull << hi) - 1ull));
            if (!m) return;
            rEnd = __builtin_amdgcn_readlane(gpos, 63 - (int)__builtin_clzll(m));
            const int mx = mm_wave_max((flag && lane >= lo && lane < hi) ? run : 0);
            rSize = mx > rSize ? mx : rSize;
          };
          uint64_t ev = startM | breakM;
          int segLo = 0;
          while (ev) {
            const int bpos = (int)__builtin_ctzll(ev);
            ev &= ev - 1ull;
            if (inRun) extend(segLo, bpos);
            if ((breakM >> bpos) & 1ull) { if (inRun) jn.emit(rSeq, rStart, rEnd, rSize); inRun = false; }
            else {
              if (inRun) jn.emit(rSeq, rStart, rEnd, rSize);
              rSeq = __builtin_amdgcn_readlane(gseq, bpos); rStart = __builtin_amdgcn_readlane(gpos, bpos); rEnd = rStart;
              rSize = __builtin_amdgcn_readlane(run, bpos); inRun = true;
            }
            segLo = bpos + 1;
          }
          if (inRun) extend(segLo, 64);
        }
        prevFlagC = lastFlag; prevSeqC = lastSeq;
      }
      if (inRun) jn.emit(rSeq, rStart, rEnd, rSize);
      jn.flush();
    }
    if (!write) {
      total = jn.count;
      if (total > 0) {
        long long b0 = 0;
        if (lane == 0) b0 = (long long)atomicAdd(&counters[MM_PC_L1_CAND], (unsigned long long)total);
        base = (long long)mm_bcast64_readfirstlane((uint64_t)b0);
        if ((unsigned long long)base + (unsigned long long)total > l1Cap) { if (lane == 0) atomicOr(&counters[MM_PC_L1_OVERFLOW], MM_OVERFLOWED); total = 0; }
      }
      if (total > 0 && total <= MM_STREAM_BUF) {                   // the counting pass kept them all
        __threadfence_block();
        if (lane < total) mm_store_candidate(l1, base + lane, f, buf[lane]);
        break;
      }
      if (total == 0) break;
    }
  }
  if (lane == 0) { stats[f].nL1 = total; l1Off[f] = total > 0 ? base : 0; }
  };
  for (int li = blockIdx.x * 4 + wave; li < nList; li += gridDim.x * 4) { one(list[li]); __threadfence_block(); }
}

// ---------------------------------------------------------------------------------------------
// k_l1_stream_groups: k_l1_stream under -Y reference groups (MM_OPT_L1_GROUP_STREAM).  Map::doL1Mapping calls
// computeL1CandidateRegions once per run of points whose contigs share a reference group (computeMap.hpp:1146-1165).  The wave walks the sorted list in those extents [b, e) -- the next one
// found 64 points at a time by a ballot of "group differs"; a group whose contigs are not adjacent comes back as an extent of its own,
// as in the reference -- and runs k_l1_stream's body on each: its own best count, its own copy of minimumHits, its last position group
// never flagged, the carried count starting at 0, no neighbour across its ends, runs joined inside it only.  The candidates of all
// extents are counted together, claimed once and written in extent order.  A position group across two contigs INSIDE an extent (one
// shared by the last point of an extent and the first of the next is none: those are two calls) or minimumHits <= 0 leaves the whole
// fragment to k_l1_sweep.  A kernel of its own, built from what k_l1_stream is built from: the chunk and pass 1 over an extent (L1Stream; the
// plain kernel's extent is 0, nPts), the minimum-hits raise, the pending-candidate joiner (L1Join) and the candidate store.  The fold of an
// extent and the claim-and-write tail of the counting pass stand in both kernels: as functions they raise the VGPR count of k_l1_stream,
// which sits at the SGPR limit, and that kernel keeps its registers.  A change to either copy goes into the other.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_l1_stream_groups(int nList, const int32_t* __restrict__ list, const int64_t* __restrict__ ptOff, const uint64_t* __restrict__ pts,
            mm_frag_stats* __restrict__ stats, const int32_t* __restrict__ minHitsTab, const int32_t* __restrict__ cutoffs, int nCutoffs,
            int sParam, int segLength, int hg, mm_l1_candidate* __restrict__ l1, unsigned long long l1Cap, int64_t* __restrict__ l1Off,
            int32_t* __restrict__ lit, unsigned int* __restrict__ litCount, unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS: the L1 cursor and its overflow flag */,
            const unsigned long long* __restrict__ nDev, const int32_t* __restrict__ ptKept /* points at the head of the sorted list (k_gather_points / k_filter_points) */,
            const int32_t* __restrict__ refGroup) {
  __shared__ L1Run bufAll[4][MM_STREAM_BUF];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  L1Run* buf = bufAll[wave];
  if (nDev) nList = (int)*nDev;
  auto one = [&](const int f) {
  const int nPts = ptKept[f], S = stats[f].sketchSize;
  if (nPts <= 0 || S <= 0) { if (lane == 0) { stats[f].nL1 = 0; l1Off[f] = 0; } return; }
  const L1Stream st{pts + ptOff[2 * f], lane};
  int minHits = minHitsTab[S];
  auto toLiteral = [&]() { if (lane == 0) lit[atomicAdd(litCount, 1u)] = f; };   // the literal kernel's business

  if (minHits <= 0) { toLiteral(); return; }

  // ---- pass 2: runs of flagged groups -> joined candidates; counted (the first MM_STREAM_BUF kept in LDS), then written ----
  int total = 0; long long base = 0;
  for (int pass = 0; pass < 2; pass++) {
    const bool write = pass == 1;
    L1Join jn{l1, buf, base, f, lane, segLength, write};
    // the extent [b, e) with its G groups and its minimumHits; ends with the pending candidate flushed (L1Emit::run's firstOfGroup)
    auto pass2 = [&](int b, int e, int G, int minHits) {
      bool inRun = false; int rSeq = 0, rStart = 0, rEnd = 0, rSize = 0;
      int carry = 0, gBase = 0;
      bool prevFlagC = false; int prevSeqC = 0;                   // the last group of the chunks so far: flagged?, its contig
      for (int i0 = b; i0 < e; i0 += 64) {
        uint64_t k; int run, sum; bool gLast, mixed;
        st.chunk(b, e, i0, carry, k, run, gLast, mixed, sum);
        carry += sum;
        const uint64_t GM = __ballot(gLast);
        if (!GM) continue;
        const int gidx = gBase + (int)mm_popc_below(GM);
        gBase += (int)__popcll(GM);
        const bool flag = gLast && gidx < G - 1 && run >= minHits;
        const uint64_t FM = __ballot(flag);
        const int gseq = (int)(k >> 33), gpos = (int)(uint32_t)(k >> 1);
        const int lastG = 63 - (int)__builtin_clzll(GM);
        const bool lastFlag = (FM >> lastG) & 1ull; const int lastSeq = __builtin_amdgcn_readlane(gseq, lastG);
        if (FM || prevFlagC) {
          // the group before this lane's: in the chunk, or the carried one
          const uint64_t below = GM & ((1ull << lane) - 1ull);
          const int pl = below ? 63 - (int)__builtin_clzll(below) : lane;
          const int sseq = __shfl(gseq, pl);
          const bool pf = below ? (((FM >> pl) & 1ull) != 0) : prevFlagC;
          const int ps = below ? sseq : prevSeqC;
          // a flagged group continues the run of a flagged predecessor on the same contig; the groups that matter are the others:
          // flagged ones that start a run, and unflagged ones right behind a flagged one, which end it.  Between two of those every
          // flagged group just extends the run: its end is the last one's position, its size the largest count.
          const uint64_t startM = __ballot(flag && !(pf && ps == gseq));
          const uint64_t breakM = __ballot(gLast && !flag && pf);
          auto extend = [&](int lo, int hi) {                       // flagged groups of the lanes [lo, hi) join the open run
            if (lo >= 64) return;
            const uint64_t m = FM & ~((1ull << lo) - 1ull) & (hi >= 64 ? ~0ull : ((1ull << hi) - 1ull));
            if (!m) return;
            rEnd = __builtin_amdgcn_readlane(gpos, 63 - (int)__builtin_clzll(m));
            const int mx = mm_wave_max((flag && lane >= lo && lane < hi) ? run : 0);
            rSize = mx > rSize ? mx : rSize;
          };
          uint64_t ev = startM | breakM;
          int segLo = 0;
          while (ev) {
            const int bpos = (int)__builtin_ctzll(ev);
            ev &= ev - 1ull;
            if (inRun) extend(segLo, bpos);
            if ((breakM >> bpos) & 1ull) { if (inRun) jn.emit(rSeq, rStart, rEnd, rSize); inRun = false; }
            else {
              if (inRun) jn.emit(rSeq, rStart, rEnd, rSize);
              rSeq = __builtin_amdgcn_readlane(gseq, bpos); rStart = __builtin_amdgcn_readlane(gpos, bpos); rEnd = rStart;
              rSize = __builtin_amdgcn_readlane(run, bpos); inRun = true;
            }
            segLo = bpos + 1;
          }
          if (inRun) extend(segLo, 64);
        }
        prevFlagC = lastFlag; prevSeqC = lastSeq;
      }
      if (inRun) jn.emit(rSeq, rStart, rEnd, rSize);
      jn.flush();
    };
    {
      for (int b = 0; b < nPts;) {
        // the extent's end: the first point behind b whose contig is of another group
        const int g0 = refGroup[(int)(st.p[b] >> 33)];
        int e = nPts;
        for (int i0 = b; i0 < nPts; i0 += 64) {
          const int idx = i0 + lane;
          const uint64_t D = __ballot(idx < nPts && refGroup[(int)(st.p[idx < nPts ? idx : b] >> 33)] != g0);
          if (D) { e = i0 + (int)__builtin_ctzll(D); break; }
        }
        int bestE = 0, GE = 0; bool mixedE = false;
        st.pass1(b, e, bestE, GE, mixedE);
        if (mixedE) { toLiteral(); return; }                      // (found by the counting pass: nothing of the fragment is out yet)
        int mh = minHits;
        if (mm_l1_raise_min_hits(bestE, GE, S, hg, sParam, cutoffs, nCutoffs, mh)) pass2(b, e, GE, mh);
        b = e;
      }
    }
    if (!write) {
      total = jn.count;
      if (total > 0) {
        long long b0 = 0;
        if (lane == 0) b0 = (long long)atomicAdd(&counters[MM_PC_L1_CAND], (unsigned long long)total);
        base = (long long)mm_bcast64_readfirstlane((uint64_t)b0);
        if ((unsigned long long)base + (unsigned long long)total > l1Cap) { if (lane == 0) atomicOr(&counters[MM_PC_L1_OVERFLOW], MM_OVERFLOWED); total = 0; }
      }
      if (total > 0 && total <= MM_STREAM_BUF) {                   // the counting pass kept them all
        __threadfence_block();
        if (lane < total) mm_store_candidate(l1, base + lane, f, buf[lane]);
        break;
      }
      if (total == 0) break;
    }
  }
  if (lane == 0) { stats[f].nL1 = total; l1Off[f] = total > 0 ? base : 0; }
  };
  for (int li = blockIdx.x * 4 + wave; li < nList; li += gridDim.x * 4) { one(list[li]); __threadfence_block(); }
}

// ---------------------------------------------------------------------------------------------
// k_l1_sweep: one thread per queued fragment over its sorted points (windowLen == 0, i.e. split mode): the literal two-pointer
// restatement of computeMap.hpp:916-1116 in mm_l1_core.h, which the CPU suite checks against the oracle.
// ---------------------------------------------------------------------------------------------
struct L1Claim {                                      // nOut slots of the pass's L1 buffer: the cursor, and its overflow flag when they do not fit
  unsigned long long* counters; unsigned long long l1Cap;
  __device__ __forceinline__ bool operator()(int nOut, long long& base) const {
    base = (long long)atomicAdd(&counters[MM_PC_L1_CAND], (unsigned long long)nOut);
    if ((unsigned long long)base + nOut <= l1Cap) return true;
    atomicOr(&counters[MM_PC_L1_OVERFLOW], MM_OVERFLOWED);
    return false;
  }
};
__global__ void __launch_bounds__(256)
k_l1_sweep(int nList, const int32_t* __restrict__ list, const int64_t* __restrict__ ptOff, const uint64_t* __restrict__ pts,
           mm_frag_stats* __restrict__ stats,
           const int32_t* __restrict__ minHitsTab, const int32_t* __restrict__ cutoffs, int nCutoffs, int sParam, int segLength,
           MapFlags fl, const int32_t* __restrict__ refGroup, mm_l1_candidate* __restrict__ l1, unsigned long long l1Cap,
           int64_t* __restrict__ l1Off, unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS: the L1 cursor and its overflow flag */,
           const unsigned int* __restrict__ nListDev /* non-null: the list's length lives on the device (what k_l1_stream left over) */,
           const unsigned long long* __restrict__ nDev64 /* non-null: the same as a 64-bit counter (the hand-over count of k_lookup_l1) */,
           const int32_t* __restrict__ ptKept) {
  if (nListDev) nList = (int)*nListDev;
  if (nDev64) nList = (int)*nDev64;
  for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < nList; li += gridDim.x * blockDim.x) {
    const int f = list[li];
    const int nPts = ptKept[f], S = stats[f].sketchSize;
    L1Stored r{0, 0};
    if (nPts > 0 && S > 0) {
      const L1Frag q{pts + ptOff[2 * f], nPts, nullptr, 0, nullptr, 0, S, minHitsTab[S], cutoffs, nCutoffs, sParam, segLength, fl.hg, fl.skipPrefix, refGroup};
      r = mm_l1_literal_store<false>(q, f, l1, L1Claim{counters, l1Cap});
    }
    stats[f].nL1 = r.nOut;
    l1Off[f] = r.base;
  }
}

// ---------------------------------------------------------------------------------------------
// k_l1_window: the same for fragments LONGER than segLength (--noSplit: Q.len > segLength, windowLen = Q.len - segLength != 0,
// computeMap.hpp:933): the WINDOWED form of mm_l1_literal_fragment.  `ptIds` numbers the seeds of a fragment (mm_gather_points);
// `freqAll` gives every thread nFreq counters.  Handles windowLen == 0 as well (a batch may mix short and long reads).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_l1_window(int nList, const int32_t* __restrict__ list, const DFrag* __restrict__ frags, const int64_t* __restrict__ ptOff, const uint64_t* __restrict__ pts,
            const uint16_t* __restrict__ ptIds, mm_frag_stats* __restrict__ stats, const int32_t* __restrict__ minHitsTab, const int32_t* __restrict__ cutoffs,
            int nCutoffs, int sParam, int segLength, MapFlags fl, const int32_t* __restrict__ refGroup, int32_t* __restrict__ freqAll, int nFreq,
            mm_l1_candidate* __restrict__ l1, unsigned long long l1Cap, int64_t* __restrict__ l1Off, unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS: the L1 cursor and its overflow flag */) {
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= nList) return;
  const int f = list[li];
  const int nPts = stats[f].nPoints, S = stats[f].sketchSize;
  L1Stored r{0, 0};
  if (nPts > 0 && S > 0) {
    int W = frags[f].len - segLength; if (W < 0) W = 0;
    const L1Frag q{pts + ptOff[2 * f], nPts, ptIds + ptOff[2 * f], W, freqAll + (size_t)li * nFreq, nFreq, S, minHitsTab[S], cutoffs, nCutoffs, sParam, segLength,
                   fl.hg, fl.skipPrefix, refGroup};
    r = mm_l1_literal_store<true>(q, f, l1, L1Claim{counters, l1Cap});
  }
  stats[f].nL1 = r.nOut;
  l1Off[f] = r.base;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// One pass of seed lookup + L1 + L2 + selection over the resident sketches.
//   steady == false: every stage is sized from the counts of the one before it, read back from the device (and grown + retried when a
//                    buffer overflows): five to seven host synchronisations per pass.
//   steady == true : the previous pass of this context has sized every buffer; everything is launched against those capacities with
//                    the counts left on the device (kernels over lists take their lengths from there, kernels over candidates cover the
//                    buffers' capacity), and one block of counters is read back at the end: ONE synchronisation per pass.  A pass that
//                    outgrew a buffer has its overflow flag set there and is redone the sized way (MM_PASS_REDO).
// What the stages of a pass hand on (map_pass calls them in order; each one is a sequence of operations on c->stream).
struct MapPass {
  bool steady, windowed, useMid;
  bool useGroups = false;                  // k_lookup_groups runs behind k_lookup_l1 (MM_OPT_L1_GROUP_FUSED under -Y): bigList is what it handed over
  const int32_t* bigList = nullptr;        // the fragments of the HBM point path: dBigList, or dGrpList behind k_lookup_groups
  unsigned long long nOffered = 0;         // sized pass with useGroups: fragments k_lookup_l1 queued (all of them offered to k_lookup_groups)
  int nF, s;
  MapFlags fl;
  SeedTable seedTab;
  unsigned long long* cnt;                 // dCounters + MM_CW_PASS (MM_PC_*)
  unsigned int* lens;                      // dCounters + MM_CW_SORT_LENS, 32-bit words (MM_SL_*)
  const unsigned long long* nBigDev;       // steady-state pass: the length of dBigList where the kernels read it
  unsigned long long regionCap = 0;        // candidates per output region of the fused kernels
  size_t denseCap = 0;                     // candidates the dense L1 buffer holds
  // what a sized pass has read back (a steady-state pass never reads them: all zero)
  unsigned long long hc[MM_PC_READ] = {0}, hMid = 0, hcur[MM_L1_REGIONS * MM_L1_CURSOR_STRIDE] = {0};
  int nBig = 0;                            // sized pass: fragments queued for the HBM point path
  unsigned long long nLit = 0;             // sized pass: of those, the fragments the literal k_l1_sweep took
  unsigned gWave = 0, gThread = 0;         // grids over those: a wave / a thread per fragment
};

// stage 1: what the pass is, and the buffers that are sized by the number of fragments
static int pass_prepare(mm_ctx* c, MapPass& p) {
  const DeviceIndex& I = c->idx;
  p.nF = (int)c->nFrags; p.s = c->P.sketchSize;
  p.fl = MapFlags{(c->P.flags & MM_FLAG_HG_FILTER) ? 1 : 0, (c->P.flags & MM_FLAG_SKIP_SELF) ? 1 : 0,
                  (c->P.flags & MM_FLAG_SKIP_PREFIX) ? 1 : 0, (c->P.flags & MM_FLAG_LOWER_TRIANGULAR) ? 1 : 0};
  // fragments longer than segLength (--noSplit): windowLen != 0 -- every fragment takes the literal path with its points (and their
  // seeds' numbers) in HBM: k_l1_window here, k_l2_window in mm_l2.hip
  p.windowed = c->windowed;
  const bool pointsInHbm = mm_points_in_hbm(c->opt, p.fl.skipPrefix, p.windowed);
  const size_t cF = mm_frag_cap(c, (size_t)p.nF);
  if (c->ptsCap == 0) c->ptsCap = mm_pts_cap0(cF, pointsInHbm);
  c->l1Cap = std::max(c->l1Cap, mm_l1_cap0(cF));
  MM_HIP(c, c->dListB.ensure(cF * 4 + 16)); MM_HIP(c, c->dListC.ensure(cF * 4 + 16)); MM_HIP(c, c->dBigList.ensure(cF * 4 + 16));
  // fragments with more interval points than k_lookup_l1 sorts go through k_lookup_mid first
  p.useMid = !pointsInHbm && p.s <= MM_MID_MAXSKETCH;
  if (p.useMid) MM_HIP(c, c->dMidList.ensure(cF * 4 + 16));
  // -Y reference groups with MM_OPT_L1_GROUP_FUSED: the queued fragments go through k_lookup_groups first.  Not for a windowed batch, not
  // when the points are to stay in HBM, not for a sketch its seed list does not hold, and only where an extent of the sorted points is
  // a whole group (refGroup non-decreasing).  Such a pass is never a steady-state one (mm_never_steady)
  p.useGroups = c->opt.l1GroupFused && p.fl.skipPrefix && !p.steady && !p.windowed && !c->opt.keepPoints && p.s <= MM_GRP_MAXSEEDS && c->refGroupMonotone;
  if (p.useGroups) MM_HIP(c, c->dGrpList.ensure(cF * 4 + 16));
  p.bigList = p.useGroups ? c->dGrpList.as<int32_t>() : c->dBigList.as<int32_t>();
  MM_HIP(c, c->dL1Regions.ensure(sizeof(L1Regions)));
  p.cnt = c->dCounters.as<unsigned long long>() + MM_CW_PASS;
  p.lens = (unsigned int*)(c->dCounters.as<unsigned long long>() + MM_CW_SORT_LENS);
  p.nBigDev = p.steady ? p.cnt + MM_PC_BIG_LEN : nullptr;
  p.seedTab = SeedTable{I.htSlots.as<HtSlot>(), (uint64_t)(I.htCap - 1), I.filter.as<uint64_t>(), (uint64_t)I.filterMask, I.tagged ? I.htTags.as<uint8_t>() : (const uint8_t*)nullptr};
  return MM_OK;
}

// stage 2: the counters' reset, k_lookup_l1 and k_lookup_mid; a sized pass reads the counts back and grows + retries when the
// interval points or a region of L1 candidates did not fit
static int pass_lookup(mm_ctx* c, MapPass& p) {
  const DeviceIndex& I = c->idx;
  const int nF = p.nF, s = p.s;
  unsigned long long* const cnt = p.cnt;
  unsigned long long* const all = c->dCounters.as<unsigned long long>();
  for (int attempt = 0; attempt < 10; attempt++) {          // grow-and-retry on capacity overflow (points or L1 candidates)
    p.regionCap = mm_region_cap(c->l1Cap, MM_L1_REGIONS);
    MM_HIP(c, c->dPts.ensure(c->ptsCap * 8 + 64));
    MM_HIP(c, c->dPtIds.ensure(p.windowed ? c->ptsCap * 2 + 64 : 64));
    MM_HIP(c, c->dL1.ensure(mm_l1_bytes(p.regionCap, MM_L1_REGIONS, sizeof(mm_l1_candidate))));
    MM_HIP(c, c->dL1b.ensure(mm_l1_bytes(p.regionCap, MM_L1_REGIONS, sizeof(mm_l1_candidate))));
    MM_HIP(c, c->dL1Cursors.ensure(sizeof p.hcur));
    // the sketch launcher's hard-list length (32 bits of its first word) survives the reset below
    if (attempt == 0) MM_HIP(c, hipMemcpyAsync(all + MM_CW_HARD_COPY, all + MM_CW_SKETCH, 8, hipMemcpyDeviceToDevice, c->stream));
    MM_HIP(c, hipMemsetAsync(all, 0, (size_t)MM_CW_MAP * 8, c->stream));
    MM_HIP(c, hipMemsetAsync(all + MM_CW_MAP, 0, (size_t)(MM_CW_MAP_END - MM_CW_MAP) * 8, c->stream));
    MM_HIP(c, hipMemsetAsync(c->dL1Cursors.p, 0, sizeof p.hcur, c->stream));
    {
      KernelTimer t(c, MM_K_LOOKUP);
      // the fused path holds a fragment's interval points in LDS + registers: up to 128 of them for the default sketch, 256 / 512 for
      // larger ones (points come in proportion to the sketch: s = 310 averages ~176 per fragment with a long tail)
      const int fuse = s > 256 ? 512 : s > 160 ? 256 : 128;
      auto kern = I.tagged ? (fuse == 512 ? k_lookup_l1<512, true> : fuse == 256 ? k_lookup_l1<256, true> : k_lookup_l1<128, true>)
                           : (fuse == 512 ? k_lookup_l1<512, false> : fuse == 256 ? k_lookup_l1<256, false> : k_lookup_l1<128, false>);
      hipLaunchKernelGGL(kern, dim3((nF + MM_LOOKUP_WPB - 1) / MM_LOOKUP_WPB), dim3(MM_LOOKUP_WPB * 64), 0, c->stream, nF, s, c->dFrags.as<DFrag>(),
                         c->dSkHash.as<uint64_t>(), c->dSkStrand.as<int8_t>(), c->dSkCount.as<uint32_t>(), p.seedTab, I.ptKeys.as<uint64_t>(),
                         c->dReadSelf.as<int32_t>(), c->seqCounterBase, p.fl, p.windowed ? 2 : (c->opt.keepPoints ? 1 : 0),
                         c->dQHash.as<uint64_t>(), c->dQStrand.as<int8_t>(),
                         c->dStats.as<mm_frag_stats>(), c->dPtOff.as<int64_t>(), (unsigned long long)c->ptsCap,
                         c->dMinHits.as<int32_t>(), c->dCutoffs.as<int32_t>(), (int)c->nCutoffs, c->P.segLength,
                         c->dL1.as<mm_l1_candidate>(), p.regionCap, c->dL1Cursors.as<unsigned long long>(), c->dL1Off.as<int64_t>(),
                         c->dBigList.as<int32_t>(), p.useMid ? c->dMidList.as<int32_t>() : (int32_t*)nullptr, cnt);
      MM_HIP(c, hipGetLastError());
    }
    if (p.useMid) {
      // its list's length stays on the device (MM_PC_MID_LEN); the grid is what the last sized pass saw plus a half (the kernel walks the
      // list with whatever grid it gets), every fragment when nothing is known yet
      KernelTimer t(c, MM_K_SORT);
      const unsigned grid = (unsigned)mm_mid_grid_guess(c->sized.seen, (size_t)nF);
      auto mk = I.tagged ? k_lookup_mid<true> : k_lookup_mid<false>;
      hipLaunchKernelGGL(mk, dim3(grid), dim3(64), 0, c->stream, 0, cnt + MM_PC_MID_LEN, c->dMidList.as<int32_t>(), s, c->dFrags.as<DFrag>(), c->dSkHash.as<uint64_t>(),
                         c->dSkCount.as<uint32_t>(), p.seedTab, I.ptKeys.as<uint64_t>(), c->dReadSelf.as<int32_t>(), c->seqCounterBase, p.fl, c->dStats.as<mm_frag_stats>(),
                         c->dPtOff.as<int64_t>(), (unsigned long long)c->ptsCap, c->dMinHits.as<int32_t>(), c->dCutoffs.as<int32_t>(), (int)c->nCutoffs, c->P.segLength,
                         c->dL1.as<mm_l1_candidate>(), p.regionCap, c->dL1Cursors.as<unsigned long long>(), c->dL1Off.as<int64_t>(), c->dBigList.as<int32_t>(), cnt);
      MM_HIP(c, hipGetLastError());
    }
    if (p.useGroups) {
      // a wave per fragment k_lookup_l1 queued (their number stays on the device: MM_PC_BIG_LEN); what it hands over is counted in
      // MM_PC_GRP_LEN, the word k_lookup_mid's list would use and the read-back below fetches anyway (hMid)
      KernelTimer t(c, MM_K_SORT);
      const unsigned grid = (unsigned)std::max(1, std::min(nF, 1 << 16));
      auto gk = I.tagged ? k_lookup_groups<true> : k_lookup_groups<false>;
      hipLaunchKernelGGL(gk, dim3(grid), dim3(64), 0, c->stream, cnt + MM_PC_BIG_LEN, c->dBigList.as<int32_t>(), s, c->dFrags.as<DFrag>(), c->dSkHash.as<uint64_t>(),
                         c->dSkCount.as<uint32_t>(), p.seedTab, I.ptKeys.as<uint64_t>(), I.refGroup.as<int32_t>(), c->dReadGroup.as<int32_t>(), c->dReadSelf.as<int32_t>(),
                         c->seqCounterBase, p.fl, c->dStats.as<mm_frag_stats>(), c->dPtOff.as<int64_t>(), c->dMinHits.as<int32_t>(), c->dCutoffs.as<int32_t>(),
                         (int)c->nCutoffs, c->P.segLength, c->dL1.as<mm_l1_candidate>(), p.regionCap, c->dL1Cursors.as<unsigned long long>(), c->dL1Off.as<int64_t>(),
                         c->dGrpList.as<int32_t>(), cnt);
      MM_HIP(c, hipGetLastError());
    }
    if (p.steady) return MM_OK;                               // the overflow flags are looked at when the pass is over
    MM_HIP(c, hipMemcpyAsync(p.hc, cnt, sizeof p.hc, hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipMemcpyAsync(&p.hMid, cnt + MM_PC_MID_LEN, 8, hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipMemcpyAsync(p.hcur, c->dL1Cursors.p, sizeof p.hcur, hipMemcpyDeviceToHost, c->stream));
    unsigned long long* hPass = c->hPass.as<unsigned long long>();
    MM_HIP(c, hipMemcpyAsync(hPass + MM_CW_HARD_COPY, all + MM_CW_HARD_COPY, 8, hipMemcpyDeviceToHost, c->stream));
    MM_SYNC(c);
    c->rep.lastHard = (size_t)(hPass[MM_CW_HARD_COPY] & 0xffffffffull);
    if (p.hc[MM_PC_POINT_OVERFLOW]) { c->ptsCap = mm_pts_cap_grown(mm_scaled(c, (size_t)p.hc[MM_PC_POINT_CURSOR], 16)); continue; }
    if (p.hc[MM_PC_L1_OVERFLOW]) {                            // some region overflowed: size for the largest one seen
      unsigned long long mx = 0;
      for (int r = 0; r < MM_L1_REGIONS; r++) mx = std::max(mx, p.hcur[(size_t)r * MM_L1_CURSOR_STRIDE]);
      c->l1Cap = mm_l1_cap_grown(mm_scaled(c, (size_t)mx, sizeof(mm_l1_candidate) * MM_L1_REGIONS), MM_L1_REGIONS); continue;
    }
    break;
  }
  if (p.hc[MM_PC_POINT_OVERFLOW]) { c->err = "interval-point buffer overflow"; return MM_ERR_CAPACITY; }
  if (p.hc[MM_PC_L1_OVERFLOW]) { c->err = "L1 candidate buffer overflow"; return MM_ERR_CAPACITY; }
  return MM_OK;
}

// stage 3: the fused kernels' candidates, one region per cursor, become one dense array.  The regions' prefix positions and the number
// of fused candidates (MM_PC_L1_CAND) are computed on the device; the sized pass knows them from the cursors it has read
static int pass_compact(mm_ctx* c, MapPass& p) {
  unsigned long long* const cnt = p.cnt;
  unsigned long long tot = 0;
  for (int r = 0; r < MM_L1_REGIONS; r++) tot += p.hcur[(size_t)r * MM_L1_CURSOR_STRIDE];
  p.hc[MM_PC_L1_CAND] = p.steady ? 0 : tot;
  if (p.steady || tot) {
    KernelTimer t(c, MM_K_L1);
    hipLaunchKernelGGL(k_l1_regions, dim3(1), dim3(64), 0, c->stream, c->dL1Cursors.as<unsigned long long>(), p.regionCap, c->dL1Regions.as<L1Regions>(), cnt);
    hipLaunchKernelGGL(k_l1_compact, dim3(64, MM_L1_REGIONS), dim3(256), 0, c->stream, c->dL1.as<mm_l1_candidate>(), c->dL1b.as<mm_l1_candidate>(), p.regionCap, c->dL1Regions.as<L1Regions>());
    hipLaunchKernelGGL(k_l1_fix_offsets, dim3((p.nF + 255) / 256), dim3(256), 0, c->stream, p.nF, c->dStats.as<mm_frag_stats>(), c->dL1Off.as<int64_t>(), p.regionCap, c->dL1Regions.as<L1Regions>());
    MM_HIP(c, hipGetLastError());
  }
  std::swap(c->dL1, c->dL1b);                               // dL1 is the dense buffer from here on
  p.denseCap = c->dL1.bytes / sizeof(mm_l1_candidate) - 4;  // room behind the fused candidates for the sweep path's
  p.nBig = (int)p.hc[MM_PC_BIG_LEN];
  if (p.useGroups) {                                        // the point path is left with what k_lookup_groups handed over (MM_PC_GRP_LEN, read back as hMid)
    p.nOffered = p.hc[MM_PC_BIG_LEN]; p.nBig = (int)p.hMid; p.hMid = 0;
    if (c->env.debug) fprintf(stderr, "[mm] reference groups: %llu fragments offered to k_lookup_groups, %llu fused, %d handed over\n", p.nOffered, p.nOffered - (unsigned long long)p.nBig, p.nBig);
  }
  if (c->env.debug) {
    if (p.steady) fprintf(stderr, "[mm] lookup+L1: %d fragments, steady-state pass (the counts stay on the device)\n", p.nF);
    else fprintf(stderr, "[mm] lookup+L1: %d fragments, %llu through k_lookup_mid, %d to the sort+sweep path, %llu fused candidates\n", p.nF, p.hMid, p.nBig, p.hc[MM_PC_L1_CAND]);
  }
  return MM_OK;
}

// stage 4, the HBM point path: the queued fragments' interval points gathered, filtered and sorted (by the sorter their number asks for)
static int pass_point_path(mm_ctx* c, MapPass& p) {
  const DeviceIndex& I = c->idx;
  const int nBig = p.nBig, s = p.s;
  // grids over the queued fragments: exact when their number is known, otherwise sized by what the previous pass saw (the kernels
  // walk the list with whatever grid they get)
  const int nB = p.steady ? (int)mm_big_grid_guess(c->sized.seen, (size_t)p.nF) : nBig;
  p.gWave = (unsigned)((nB + 3) / 4); p.gThread = (unsigned)((nB + 255) / 256);
  KernelTimer t(c, MM_K_SORT);
  uint16_t* sortIds = p.windowed ? c->dPtIds.as<uint16_t>() : (uint16_t*)nullptr;
  auto gk = I.tagged ? k_gather_points<true> : k_gather_points<false>;
  hipLaunchKernelGGL(gk, dim3(p.gWave), dim3(256), 0, c->stream, nBig, p.bigList, s, c->dFrags.as<DFrag>(), c->dSkHash.as<uint64_t>(),
                     c->dSkCount.as<uint32_t>(), p.seedTab, I.ptKeys.as<uint64_t>(), I.refGroup.as<int32_t>(),
                     c->dReadGroup.as<int32_t>(), c->dReadSelf.as<int32_t>(), c->seqCounterBase, p.fl, c->dStats.as<mm_frag_stats>(), c->dPtOff.as<int64_t>(),
                     c->dPts.as<uint64_t>(), sortIds, c->dPtKept.as<int32_t>(), p.nBigDev);
  MM_HIP(c, hipGetLastError());
  // split mode, plain L1: the points that cannot reach minimumHits go before the sort (k_filter_points)
  if (!p.windowed && (!c->opt.keepPoints || c->opt.keepFiltered) && !p.fl.skipPrefix) {
    hipLaunchKernelGGL(k_filter_points, dim3(p.gWave), dim3(256), 0, c->stream, nBig, p.bigList, c->dStats.as<mm_frag_stats>(), c->dMinHits.as<int32_t>(),
                       c->dPtOff.as<int64_t>(), c->dPts.as<uint64_t>(), c->dPtKept.as<int32_t>(), p.nBigDev);
    MM_HIP(c, hipGetLastError());
  }
  if (!p.windowed) hipLaunchKernelGGL(k_sort_points_wave, dim3(p.gWave), dim3(256), 0, c->stream, nBig, p.nBigDev, p.bigList, c->dPtOff.as<int64_t>(), c->dPts.as<uint64_t>());
  hipLaunchKernelGGL(k_classify_sort, dim3(p.gThread), dim3(256), 0, c->stream, nBig, p.nBigDev, p.bigList, c->dPtOff.as<int64_t>(),
                     c->dListB.as<int32_t>(), c->dListC.as<int32_t>(), p.lens, p.windowed ? 1 : MM_SORT_WAVECAP);
  MM_HIP(c, hipGetLastError());
  unsigned int hLens[MM_SL_LITERAL] = {1024u, 16u};         // the two sorter lists (the words before MM_SL_LITERAL).  steady: fixed grids over the two lists (their lengths stay on the device)
  if (!p.steady) {
    MM_HIP(c, hipMemcpyAsync(hLens, p.lens, sizeof hLens, hipMemcpyDeviceToHost, c->stream));
    MM_SYNC(c);
    if (c->env.debug) fprintf(stderr, "[mm] point path: %d queued fragments, after the filter %u lists of more than %d points (LDS sorter), %u beyond the LDS sorter\n", nBig, hLens[MM_SL_BLOCK], MM_SORT_WAVECAP, hLens[MM_SL_GLOBAL]);
  }
  if (hLens[MM_SL_BLOCK]) hipLaunchKernelGGL(k_sort_points_block, dim3(hLens[MM_SL_BLOCK]), dim3(256), 0, c->stream, p.lens + MM_SL_BLOCK, c->dPtOff.as<int64_t>(), c->dPts.as<uint64_t>(), c->dListB.as<int32_t>(), sortIds);
  if (hLens[MM_SL_GLOBAL]) hipLaunchKernelGGL(k_sort_points_global, dim3(hLens[MM_SL_GLOBAL]), dim3(1024), 0, c->stream, p.lens + MM_SL_GLOBAL, c->dPtOff.as<int64_t>(), c->dPts.as<uint64_t>(), c->dListC.as<int32_t>(), sortIds);
  MM_HIP(c, hipGetLastError());
  return MM_OK;
}

// stage 5: L1 over the sorted points.  The candidates of the fused path sit at [0, fusedL1) of the dense buffer; the sweeps append
// behind them, so a sized pass whose buffer was too small grows it and rewinds to fusedL1 only
static int pass_l1_sweeps(mm_ctx* c, MapPass& p) {
  const DeviceIndex& I = c->idx;
  const int nBig = p.nBig, s = p.s;
  unsigned long long* const cnt = p.cnt;
  const unsigned long long fusedL1 = p.hc[MM_PC_L1_CAND];
  // a wave per fragment streams the sorted points; what it cannot take (a position group across two contigs, minimumHits 0) and
  // every fragment under -Y reference groups goes to the literal one-thread-per-fragment kernel -- unless MM_OPT_L1_GROUP_STREAM: then
  // the grouped form of the wave kernel comes first there too
  const bool stream = (!p.fl.skipPrefix || c->opt.l1GroupStream) && !c->env.l1Literal && !p.windowed;
  for (int attempt = 0; attempt < 8; attempt++) {
    if (!p.steady) {
      MM_HIP(c, hipMemcpyAsync(cnt + MM_PC_L1_CAND, &fusedL1, 8, hipMemcpyHostToDevice, c->stream));
      MM_HIP(c, hipMemsetAsync(cnt + MM_PC_L1_OVERFLOW, 0, 8, c->stream));
    }
    {
      KernelTimer t(c, MM_K_L1);
      const int32_t* sweepList = p.bigList; const unsigned int* sweepCount = nullptr;
      if (p.windowed) {
        const int nFreq = s > 256 ? s : 256;                                     // seeds are numbered by their index in the raw sketch
        MM_HIP(c, c->dWinFreq.ensure((size_t)nBig * nFreq * 4 + 64));
        hipLaunchKernelGGL(k_l1_window, dim3((nBig + 63) / 64), dim3(64), 0, c->stream, nBig, p.bigList, c->dFrags.as<DFrag>(), c->dPtOff.as<int64_t>(),
                           c->dPts.as<uint64_t>(), c->dPtIds.as<uint16_t>(), c->dStats.as<mm_frag_stats>(), c->dMinHits.as<int32_t>(), c->dCutoffs.as<int32_t>(),
                           (int)c->nCutoffs, s, c->P.segLength, p.fl, I.refGroup.as<int32_t>(), c->dWinFreq.as<int32_t>(), nFreq, c->dL1.as<mm_l1_candidate>(),
                           (unsigned long long)p.denseCap, c->dL1Off.as<int64_t>(), cnt);
        MM_HIP(c, hipGetLastError());
      } else {
        unsigned int* lit = p.lens + MM_SL_LITERAL;
        if (stream) {
          MM_HIP(c, hipMemsetAsync(lit, 0, (size_t)(MM_SL_END - MM_SL_LITERAL) * 4, c->stream));
          if (p.fl.skipPrefix) hipLaunchKernelGGL(k_l1_stream_groups, dim3(p.gWave), dim3(256), 0, c->stream, nBig, p.bigList, c->dPtOff.as<int64_t>(),
                             c->dPts.as<uint64_t>(), c->dStats.as<mm_frag_stats>(), c->dMinHits.as<int32_t>(), c->dCutoffs.as<int32_t>(),
                             (int)c->nCutoffs, s, c->P.segLength, p.fl.hg, c->dL1.as<mm_l1_candidate>(), (unsigned long long)p.denseCap,
                             c->dL1Off.as<int64_t>(), c->dListB.as<int32_t>(), lit, cnt, p.nBigDev, c->dPtKept.as<int32_t>(), I.refGroup.as<int32_t>());
          else hipLaunchKernelGGL(k_l1_stream, dim3(p.gWave), dim3(256), 0, c->stream, nBig, p.bigList, c->dPtOff.as<int64_t>(),
                             c->dPts.as<uint64_t>(), c->dStats.as<mm_frag_stats>(), c->dMinHits.as<int32_t>(), c->dCutoffs.as<int32_t>(),
                             (int)c->nCutoffs, s, c->P.segLength, p.fl.hg, c->dL1.as<mm_l1_candidate>(), (unsigned long long)p.denseCap,
                             c->dL1Off.as<int64_t>(), c->dListB.as<int32_t>(), lit, cnt, p.nBigDev, c->dPtKept.as<int32_t>());
          MM_HIP(c, hipGetLastError());
          sweepList = c->dListB.as<int32_t>(); sweepCount = lit;
        }
        hipLaunchKernelGGL(k_l1_sweep, dim3(stream && p.steady ? 64u : p.gThread), dim3(256), 0, c->stream, nBig, sweepList, c->dPtOff.as<int64_t>(),
                           c->dPts.as<uint64_t>(), c->dStats.as<mm_frag_stats>(), c->dMinHits.as<int32_t>(), c->dCutoffs.as<int32_t>(),
                           (int)c->nCutoffs, s, c->P.segLength, p.fl, I.refGroup.as<int32_t>(), c->dL1.as<mm_l1_candidate>(),
                           (unsigned long long)p.denseCap, c->dL1Off.as<int64_t>(), cnt, sweepCount, sweepCount ? (const unsigned long long*)nullptr : p.nBigDev, c->dPtKept.as<int32_t>());
        MM_HIP(c, hipGetLastError());
      }
    }
    if (p.steady) return MM_OK;
    MM_HIP(c, hipMemcpyAsync(p.hc + MM_PC_L1_CAND, cnt + MM_PC_L1_CAND, 16, hipMemcpyDeviceToHost, c->stream));   // the cursor and its overflow flag
    // ... and, with them, the length of the list k_l1_stream left for k_l1_sweep (the 64-bit word that holds MM_SL_LITERAL)
    constexpr int litWord = MM_CW_SORT_LENS + MM_SL_LITERAL / 2;
    unsigned long long* hPass = c->hPass.as<unsigned long long>();
    MM_HIP(c, hipMemcpyAsync(hPass + litWord, c->dCounters.as<unsigned long long>() + litWord, 8, hipMemcpyDeviceToHost, c->stream));
    MM_SYNC(c);
    // (set again by every attempt of this loop: the last one, whose candidates stand, is the one that counts)
    p.nLit = p.windowed ? 0ull : stream ? (unsigned long long)((const unsigned int*)(hPass + MM_CW_SORT_LENS))[MM_SL_LITERAL] : (unsigned long long)nBig;
    if (c->env.debug && stream && p.fl.skipPrefix) fprintf(stderr, "[mm] point path: of %d queued fragments the literal L1 kernel took %llu (reference groups on the wave kernel)\n", nBig, p.nLit);
    if (!p.hc[MM_PC_L1_OVERFLOW]) return MM_OK;
    // grow, keeping the fused candidates already in the buffer
    const size_t newCap = mm_cand_cap((size_t)p.hc[MM_PC_L1_CAND]);
    DevBuf nb; MM_HIP(c, nb.ensure(newCap * sizeof(mm_l1_candidate) + 64));
    if (fusedL1) MM_HIP(c, hipMemcpyAsync(nb.p, c->dL1.p, (size_t)fusedL1 * sizeof(mm_l1_candidate), hipMemcpyDeviceToDevice, c->stream));
    MM_SYNC(c);
    c->dL1 = std::move(nb); p.denseCap = newCap;
    if (c->l1Cap < newCap) c->l1Cap = newCap;                  // the next pass sizes both candidate buffers for it: no retry, no reallocation
  }
  c->err = "L1 candidate buffer overflow"; return MM_ERR_CAPACITY;
}

// stage 6: gate (steady), L2, selection; a steady-state pass then reads its counters back -- the pass's one synchronisation -- and
// says whether it stands
static int pass_finish(mm_ctx* c, MapPass& p) {
  if (p.steady) {
    // candidates the buffers of this pass hold: what the previous (sized) pass left of candidate-indexed staging, and the dense L1 buffer itself
    const unsigned long long cap = (unsigned long long)std::min(c->sized.steady.candCap, p.denseCap);
    hipLaunchKernelGGL(k_l1_gate, dim3(1), dim3(1), 0, c->stream, p.cnt, cap);
    MM_HIP(c, hipGetLastError());
  }
  int rc = mm_launch_l2(c, p.cnt, p.steady);
  if (rc != MM_OK) return rc;
  rc = mm_launch_select(c, p.steady);
  if (rc != MM_OK || !p.steady) return rc;
  // the pass is over: the parts of the counter block it has written come back, each to its place in the mirror
  const unsigned long long* all = c->dCounters.as<unsigned long long>();
  unsigned long long* hPass = c->hPass.as<unsigned long long>();
  MM_HIP(c, hipMemcpyAsync(hPass + MM_CW_PASS, all + MM_CW_PASS, (size_t)MM_PC_READ * 8, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipMemcpyAsync(hPass + MM_CW_MAP, all + MM_CW_MAP, (size_t)(MM_CW_MAP_END - MM_CW_MAP) * 8, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipMemcpyAsync(hPass + MM_CW_HARD_COPY, all + MM_CW_HARD_COPY, 8, hipMemcpyDeviceToHost, c->stream));
  MM_SYNC(c);
  const unsigned long long* h = hPass + MM_CW_PASS; const unsigned long long* hm = hPass + MM_CW_MAP;
  PassReport& r = c->rep;
  r.lastHard = (size_t)(hPass[MM_CW_HARD_COPY] & 0xffffffffull);
  if (mm_pass_incomplete(h) || hm[MM_MC_OVERFLOW]) { r.redoCause = mm_redo_cause(h, hm); return MM_PASS_REDO; }   // some buffer was too small for this batch: the sized pass grows it
  r.nL1 = (size_t)h[MM_PC_L1_CAND]; r.nL2 = (size_t)h[MM_PC_L2_LOCI]; r.nMappings = c->haveReplayTables ? (size_t)hm[MM_MC_MAPPINGS] : 0;
  r.lastOps = (size_t)hm[MM_MC_L2_OPS]; r.lastBig = c->sized.seen.prevBig;        // (MM_PC_BIG_LEN holds MM_PC_L2_WIDE_LEN by now: the sized pass's figure stands in)
  return MM_OK;
}

static int map_pass(mm_ctx* c, const bool steady) {
  MapPass p; p.steady = steady;
  int rc = pass_prepare(c, p);
  if (rc == MM_OK) rc = pass_lookup(c, p);
  if (rc == MM_OK) rc = pass_compact(c, p);
  if (rc == MM_OK && (steady || p.nBig > 0)) {
    rc = pass_point_path(c, p);
    if (rc == MM_OK) rc = pass_l1_sweeps(c, p);
  }
  if (rc != MM_OK) return rc;
  if (!steady) {
    c->rep.nL1 = (size_t)p.hc[MM_PC_L1_CAND]; c->rep.lastBig = (size_t)p.nBig; c->rep.lastMid = (size_t)p.hMid;
    // as of this sized pass; the four L2 figures are zero until mm_launch_l2_window counts its candidates
    SizedPass::Seen seen;
    seen.prevBig = (size_t)p.nBig; seen.prevLit = (size_t)p.nLit; seen.prevMid = (size_t)p.hMid; seen.midKnown = p.useMid;
    seen.grpOffered = (size_t)p.nOffered; seen.grpFused = p.useGroups ? (size_t)p.nOffered - (size_t)p.nBig : 0;
    c->sized.seen = seen;
    if (c->rep.nL1 == 0) return MM_OK;
  }
  return pass_finish(c, p);
}

int mm_launch_map(mm_ctx* c) {
  const int nF = (int)c->nFrags, s = c->P.sketchSize;
  const size_t cF = mm_frag_cap(c, (size_t)nF);
  MM_HIP(c, c->dQHash.ensure(cF * s * 8 + 64)); MM_HIP(c, c->dQStrand.ensure(cF * s + 64));
  MM_HIP(c, c->dStats.ensure(cF * sizeof(mm_frag_stats) + 64));
  MM_HIP(c, c->dPtOff.ensure(cF * 16 + 64)); MM_HIP(c, c->dL1Off.ensure(cF * 8 + 64)); MM_HIP(c, c->dPtKept.ensure(cF * 4 + 64));
  MM_HIP(c, c->dCounters.ensure(MM_COUNTER_BYTES));
  MM_HIP(c, c->hPass.ensure(MM_COUNTER_BYTES));
  c->rep = PassReport{};
  if (nF == 0) return MM_OK;
  const bool neverSteady = mm_never_steady(c->opt, (c->P.flags & MM_FLAG_SKIP_PREFIX) != 0, c->windowed, s);
  if (mm_may_try_steady(c->sized.steady, (size_t)nF, neverSteady)) {
    const int rc = map_pass(c, true);
    if (rc == MM_OK) { mm_steady_stood(c->sized.steady, c->rep); return MM_OK; }
    if (rc != MM_PASS_REDO) return rc;
    mm_steady_redone(c->sized.steady, c->tot);
  }
  const int rc = map_pass(c, false);
  mm_sized_pass_done(c->sized.steady, mm_frag_cap(c, (size_t)nF), rc == MM_OK, neverSteady, c->rep.nL1);
  return rc;
}

// ---------------------------------------------------------------------------------------------
// downloads
// ---------------------------------------------------------------------------------------------
extern "C" {

int mm_results_download(mm_ctx* c, mm_frag_stats* stats, mm_l1_candidate* l1, mm_l2_locus* l2) {
  if (!c->mapped) { c->err = "mm_results_download: nothing mapped"; return MM_ERR_STATE; }
  MM_HIP(c, hipSetDevice(c->device));
  const size_t nF = c->nFrags;
  std::vector<int64_t> l1off(nF);
  std::vector<mm_frag_stats> st(nF);
  if (nF) {
    MM_HIP(c, hipMemcpyAsync(st.data(), c->dStats.p, nF * sizeof(mm_frag_stats), hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipMemcpyAsync(l1off.data(), c->dL1Off.p, nF * 8, hipMemcpyDeviceToHost, c->stream));
  }
  const size_t nL1 = c->rep.nL1, nL2 = c->rep.nL2;
  std::vector<mm_l1_candidate> h1(nL1); std::vector<mm_l2_locus> h2(nL2);
  if (nL1) MM_HIP(c, hipMemcpyAsync(h1.data(), c->dL1.p, nL1 * sizeof(mm_l1_candidate), hipMemcpyDeviceToHost, c->stream));
  if (nL2) MM_HIP(c, hipMemcpyAsync(h2.data(), c->dL2.p, nL2 * sizeof(mm_l2_locus), hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipStreamSynchronize(c->stream));
  if (stats && nF) std::memcpy(stats, st.data(), nF * sizeof(mm_frag_stats));
  // fragment-major order: candidates of fragment f are contiguous on the device at l1off[f]
  std::vector<int64_t> newBase(nF, 0);
  size_t w = 0;
  for (size_t f = 0; f < nF; f++) {
    newBase[f] = (int64_t)w;
    for (int i = 0; i < st[f].nL1; i++) { if (l1) l1[w] = h1[(size_t)l1off[f] + i]; w++; }
  }
  if (l2 && nL2) {
    // device order keeps every candidate's loci contiguous and in emission order; a stable sort by (frag, cand) finishes the job
    std::vector<uint32_t> ord(nL2);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
      if (h2[a].frag != h2[b].frag) return h2[a].frag < h2[b].frag;
      return h2[a].cand < h2[b].cand; });
    for (size_t i = 0; i < nL2; i++) { mm_l2_locus o = h2[ord[i]]; o.cand = (int32_t)(newBase[o.frag] + o.cand); l2[i] = o; }
  }
  return MM_OK;
}

int mm_query_sketch_download(mm_ctx* c, mm_minmer* out) {
  if (!c->mapped) { c->err = "mm_query_sketch_download: nothing mapped"; return MM_ERR_STATE; }
  MM_HIP(c, hipSetDevice(c->device));
  const size_t nF = c->nFrags, s = (size_t)c->P.sketchSize;
  if (!nF) return MM_OK;
  std::vector<uint64_t> h(nF * s); std::vector<int8_t> st(nF * s); std::vector<mm_frag_stats> fs(nF);
  MM_HIP(c, hipMemcpyAsync(h.data(), c->dQHash.p, nF * s * 8, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipMemcpyAsync(st.data(), c->dQStrand.p, nF * s, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipMemcpyAsync(fs.data(), c->dStats.p, nF * sizeof(mm_frag_stats), hipMemcpyDeviceToHost, c->stream));
  // fragments that lost no seed were not copied to dQHash/dQStrand: their sketch is the raw one (k_lookup_l1)
  std::vector<uint64_t> rh(nF * s); std::vector<int8_t> rst(nF * s);
  MM_HIP(c, hipMemcpyAsync(rh.data(), c->dSkHash.p, nF * s * 8, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipMemcpyAsync(rst.data(), c->dSkStrand.p, nF * s, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipStreamSynchronize(c->stream));
  for (size_t f = 0; f < nF; f++) {
    const bool raw = fs[f].rawSketchSize == fs[f].sketchSize;
    for (int r = 0; r < fs[f].sketchSize; r++) {
      const size_t o = f * s + r;
      out[o] = mm_minmer{raw ? rh[o] : h[o], 0, 0, c->hFrags[f].readId + c->seqCounterBase, (int16_t)(raw ? rst[o] : st[o]), 0};
    }
  }
  return MM_OK;
}

int mm_points_download(mm_ctx* c, size_t frag, mm_interval_point* out, size_t cap, size_t* n) {
  if (!c->mapped || frag >= c->nFrags) { c->err = "mm_points_download: bad state / fragment"; return MM_ERR_STATE; }
  if (!c->opt.keepPoints && !(c->P.flags & MM_FLAG_SKIP_PREFIX)) { c->err = "mm_points_download: interval points are not kept in HBM (mm_set_option MM_OPT_KEEP_POINTS)"; return MM_ERR_STATE; }
  if (!c->opt.keepPoints && c->opt.l1GroupFused) { c->err = "mm_points_download: with MM_OPT_L1_GROUP_FUSED the interval points of a fused fragment never reach HBM (mm_set_option MM_OPT_KEEP_POINTS keeps them)"; return MM_ERR_STATE; }
  MM_HIP(c, hipSetDevice(c->device));
  int64_t po[2]; mm_frag_stats fs;
  MM_HIP(c, hipMemcpy(po, c->dPtOff.as<int64_t>() + 2 * frag, 16, hipMemcpyDeviceToHost));
  MM_HIP(c, hipMemcpy(&fs, c->dStats.as<mm_frag_stats>() + frag, sizeof fs, hipMemcpyDeviceToHost));
  size_t np = (size_t)fs.nPoints;
  if (c->opt.keepFiltered) {                                            // the head of the sorted list k_filter_points left (dropped points sort behind it)
    int32_t kept = 0;
    MM_HIP(c, hipMemcpy(&kept, c->dPtKept.as<int32_t>() + frag, 4, hipMemcpyDeviceToHost));
    if (po[1] > 0) np = (size_t)kept;
  }
  if (n) *n = np;
  if (np > cap) { c->err = "mm_points_download: capacity"; return MM_ERR_ARG; }
  std::vector<uint64_t> k(np);
  if (np) MM_HIP(c, hipMemcpy(k.data(), c->dPts.as<uint64_t>() + po[0], np * 8, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < np; i++) {
    std::memset(&out[i], 0, sizeof out[i]);
    out[i].seqId = (int32_t)(k[i] >> 33); out[i].pos = (int32_t)(uint32_t)(k[i] >> 1); out[i].side = (k[i] & 1ull) ? 1 : -1;
  }
  return MM_OK;
}


}  // extern "C"
