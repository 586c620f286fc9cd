// mashmap_amd/csrc/mm_l2.hip -- L2 stage on the device (gfx950).
//
//   computeL2MappedRegions   src/map/include/computeMap.hpp:1276-1451
//   SlideMapper              src/map/include/slidingMap.hpp:28-212
//
// The reference walks minmerIndex once per L1 candidate, keeps the open reference minmers in a heap ordered
// by wpos_end and, for every record, binary-searches the query sketch twice (insert + eviction).  Here the index already
// holds, per contig, the merged stream of insert and eviction events (mm_build_device_index), so a candidate is a slice of it:
//
//   k_l2_extents   thread / candidate : the slice [e0, eMid, ub) of the event stream (three searches, each bracketed to one block of
//                                       positions by evBlock) and the block's list of records open at its start
//   scan           exclusive scan of the per-candidate entry counts
//   k_l2_locate    wave / candidate   : streams the open-record list and the slice (coalesced 16 B per event), locates every hash in
//                                       the query sketch (LDS bucket table + short scan) and writes a compact 4-byte entry per event
//                                       that can matter: pre-load inserts still open at rangeStart, inserts, evictions of hashes inside
//                                       the sketch's range; positions are delta-coded against the previous insert
//   k_l2_sweep     lane / candidate   : the sequential SlideMapper sweep over that stream; 64 bytes (16 entries) per lane
//                                       are fetched per step and the next step is prefetched while the current one is
//                                       consumed; per-lane SlideMapper state sits in LDS as 8-bit cells (16-bit for the rare
//                                       candidate that overflows them) laid out so that a lane always hits its own bank; the state
//                                       update runs on integer lane masks, without branches
//
// so the latency-bound pointer chasing of the reference (two dependent 8-step searches per record plus a heap) becomes a
// streaming pre-pass followed by a sweep whose only memory traffic is one sequential stream per lane.
#include "mm_internal.h"
#include "mm_device.h"
#include "mm_heap.h"
#include "mm_l2_window_core.h"
#include "mm_l2_plan.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#define MM_LOCAP0 8         // private L2 locus slots per candidate before the final compaction (doubled and re-run on overflow)

struct L2Info { int64_t e0; int32_t nPre; int32_t nAll;         // slice [e0, e0+nAll) of the contig's events, the first nPre before rangeStart
                int32_t sketch;                                 // the fragment's sketchSize, bit 31: no seed was removed (take the raw sketch)
                int32_t nOpen; int64_t open0;                   // records open at the block boundary before rangeStart: op*[open0, open0+nOpen)
                int32_t target; int32_t pad; };                 // pre-load takes records with wpos >= target = rangeStart - segLength - 1 (:1290)
struct L2Tmp { int32_t start, end, shared, strand; };
// The SlideMapper state of a candidate once the pre-load (computeMap.hpp:1323-1338: the records still open at rangeStart) is in, in closed
// form.  With inserts only the state does not depend on their order -- cell counts add up, the pivot is the largest p with
// p + #{reference-only hashes below q[p]} <= S (slidingMap.hpp:155-160 keeps exactly that), shared / votes are sums over the active cells
// up to it -- so k_l2_locate, which has the candidate's sketch in LDS anyway, builds it in parallel instead of writing ~s pre-load entries
// that the sweep then applies one by one (a fifth to a third of a stream).  Cells: 16 bit each, count (12) | active << 12 | (vote + 1) << 13
// = the wide sweep's cell format; row of s + 2 cells per candidate of a chunk.  flags: 1 = a query hash was open twice in the pre-load (the
// 2-bit vote cannot hold it: k_l2_sweep_exact replays the pre-load from the index), 2 = a pre-load of 4000 records or more,
// which the 12-bit counts might not hold (likewise).
struct L2Init { int32_t pivot, pivRank, shared, votes; };
#define L2INIT_FLAG_SHIFT 24        // flags travel in the top byte of `pivot` (pivot <= 8190)

// stream entry (uint32), JB = width of the sketch-position field (11 for sketches of up to 2046 entries, 13 beyond):
//   bits 0..JB-1        1-based position j of the hash in the query sketch (0: beyond the sketch -> no effect on the state)
//   bit  JB             hash equals q[j]
//   bits JB+1..JB+2     strand vote of a matching insert + 1 (query strand x reference strand)
//   bits JB+3..26       insert / end: wpos minus the running position (previous insert's wpos, rangeStart at first)
//   bits 27..31         kind, one bit each (the sweep turns a bit into a lane mask with one v_bfe_i32):
//                       insert + evaluate, eviction, pre-load insert (computeMap.hpp:1323-1338), end of stream, skip
//   skip: adds its low 27 bits to the running position (a gap that does not fit the delta field)
#define E_INS_BIT 27
#define E_DEL_BIT 28
#define E_PRE_BIT 29
#define E_END_BIT 30
#define E_SKIP_BIT 31
#define E_SKIP_MAX ((1u << 27) - 1u)
#define E_STEP 16           // entries per 64-byte sweep step
template <int JB> struct EF {
  static constexpr uint32_t JMASK = (1u << JB) - 1u;
  static constexpr int MATCH_BIT = JB, VOTE_SHIFT = JB + 1, DELTA_SHIFT = JB + 3, DELTA_BITS = 27 - (JB + 3);
  static constexpr uint32_t MAXDELTA = (1u << DELTA_BITS) - 1u;
};

// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_l2_extents(int nCand, int segLength, int deltaBits, const mm_l1_candidate* __restrict__ l1, const mm_frag_stats* __restrict__ stats, const uint32_t* __restrict__ evKey,
             const int64_t* __restrict__ contigBlock, const int64_t* __restrict__ blockOff,
             const int64_t* __restrict__ evBlock, L2Info* __restrict__ info, int32_t* __restrict__ cnt, const unsigned long long* __restrict__ nDev,
             unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS: MM_L2F_CANDS */) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (nDev) {                                                     // steady state: the launch covers the buffers' capacity, the count is on the device
    const long long n = (long long)*nDev;
    if (c == 0 && n > nCand) atomicOr(&counters[MM_PC_L2_FLAGS], MM_L2F_CANDS);
    if (c >= n) { if (c < nCand) { cnt[c] = 0; info[c].e0 = 0; } return; }
  }
  if (c >= nCand) return;
  const mm_l1_candidate cand = l1[c];
  const mm_frag_stats fst = stats[cand.frag];
  auto lowerIn = [&](int64_t lo, int64_t hi, uint32_t key) { while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (evKey[mid] < key) lo = mid + 1; else hi = mid; } return lo; };
  // std::lower_bound(minmerIndex, (seqId, rangeStart - segLength - 1))  (computeMap.hpp:1290-1293): inserts with wpos >= target are
  // pre-loaded if still open at rangeStart.  Those that start before the block boundary B <= rangeStart come from the block's
  // list of open records, the rest from the events in [max(B, target), rangeStart).  evBlock brackets every search to one block.
  const int target = cand.rangeStartPos - segLength - 1;
  const int64_t blk0 = contigBlock[cand.seqId], nBlk = contigBlock[cand.seqId + 1] - blk0;
  const int64_t blk = blk0 + (cand.rangeStartPos >> MM_OPEN_BLOCK_SHIFT);
  const int64_t ob = blockOff[blk], oe = blockOff[blk + 1];
  const int64_t evB = evBlock[blk], evN = evBlock[blk + 1];
  const int B = (cand.rangeStartPos >> MM_OPEN_BLOCK_SHIFT) << MM_OPEN_BLOCK_SHIFT;
  const int64_t e0 = target > B ? lowerIn(evB, evN, (uint32_t)target * 2u) : evB;
  const int64_t eMid = lowerIn(e0, evN, (uint32_t)cand.rangeStartPos * 2u + 1u);   // first event of the slide: insert at rangeStart or anything later
  int64_t bE = cand.rangeEndPos >> MM_OPEN_BLOCK_SHIFT; if (bE > nBlk - 1) bE = nBlk - 1;
  const int64_t evE = evBlock[blk0 + bE], evEn = evBlock[blk0 + bE + 1];
  const int64_t ub = lowerIn(evE > eMid ? evE : eMid, evEn, (uint32_t)cand.rangeEndPos * 2u + 2u);   // records are visited while wpos <= rangeEnd (:1340)
  L2Info o; o.e0 = e0; o.nPre = (int32_t)(eMid - e0); o.nAll = (int32_t)(ub - e0);
  o.open0 = ob; o.nOpen = (int32_t)(oe - ob); o.target = target;
  o.sketch = fst.sketchSize | (fst.rawSketchSize == fst.sketchSize ? (int32_t)0x80000000 : 0); o.pad = 0;
  info[c] = o;
  // upper bound of the stream: every event, the end marker, one skip per 2^deltaBits of range, slack for the end marker's own skips
  // (the record behind the last insert may be anywhere in the contig: up to 2^31 / 2^27 of them)
  // (the pre-load is not part of the stream: it reaches the sweeps as a ready-made state, L2Init)
  const int n = (o.nAll - o.nPre) + 1 + ((cand.rangeEndPos - cand.rangeStartPos) >> deltaBits) + 20;
  cnt[c] = (n + E_STEP - 1) & ~(E_STEP - 1);
}

// ---------------------------------------------------------------------------------------------
// exclusive scan int32 -> int64 (three small kernels; n up to a few hundred million)
// ---------------------------------------------------------------------------------------------
#define SCAN_ITEMS 8
#define SCAN_TILE (256 * SCAN_ITEMS)
__global__ void __launch_bounds__(256)
k_scan_tiles(int64_t n, const int32_t* __restrict__ in, int64_t* __restrict__ out, int64_t* __restrict__ tileSum) {
  __shared__ int64_t sm[256];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  int64_t v[SCAN_ITEMS]; int64_t acc = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) { v[i] = acc; acc += (base + i < n) ? (int64_t)in[base + i] : 0; }
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int64_t t = (int)threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
    __syncthreads();
    sm[threadIdx.x] += t;
    __syncthreads();
  }
  const int64_t excl = sm[threadIdx.x] - acc;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) if (base + i < n) out[base + i] = excl + v[i];
  if (threadIdx.x == 255) tileSum[blockIdx.x] = sm[255];
}
__global__ void __launch_bounds__(1024)
k_scan_top(int64_t nTiles, int64_t* __restrict__ tileSum, int64_t* __restrict__ total) {
  __shared__ int64_t sm[1024];
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nTiles; b0 += 1024) {
    const int64_t i = b0 + threadIdx.x;
    const int64_t x = i < nTiles ? tileSum[i] : 0;
    sm[threadIdx.x] = x;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int64_t t = (int)threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
      __syncthreads();
      sm[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nTiles) tileSum[i] = carry + sm[threadIdx.x] - x;
    const int64_t blockTotal = sm[1023];
    __syncthreads();
    carry += blockTotal;
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ void __launch_bounds__(256)
k_scan_add(int64_t n, int64_t* __restrict__ out, const int64_t* __restrict__ tileSum) {
  const int64_t add = tileSum[blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) if (base + i < n) out[base + i] += add;
}

// steady-state passes: the streams' total (the scan's last word) against the buffer as the previous pass left it; a batch that does not
// fit is flagged and its candidate count zeroed, so that the kernels behind this one do nothing (the pass is then redone with the
// host's sizing)
__global__ void k_l2_gate(const int64_t* __restrict__ total, int64_t opsCap, unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS */) {
  if (*total > opsCap) { counters[MM_PC_L2_FLAGS] |= MM_L2F_OPS; counters[MM_PC_L1_CAND] = 0ull; }
}

// ---------------------------------------------------------------------------------------------
// Sort keys that put the candidates of a chunk in REFERENCE order (the event index where a candidate's slice starts, coarsened).
// k_l2_locate streams ~3 segment lengths of the index per candidate and the reads cover the reference several times over, in random
// order: taken as they come, every slice is fetched from HBM (16 B per event: the kernel sits on the HBM roofline against a human-scale
// index); taken in reference order, the waves in flight at any moment read one neighbourhood of the index, which the Infinity Cache holds.
__global__ void __launch_bounds__(256)
k_l2_pos_keys(int c0, int n, int shift, const L2Info* __restrict__ info, uint32_t* __restrict__ kOut, int32_t* __restrict__ vOut, const unsigned long long* __restrict__ nDev) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool real = !nDev || c0 + i < (int)*nDev;                 // steady state: n is the buffer's capacity, the entries behind the real ones sort last
  kOut[i] = real ? (uint32_t)(info[c0 + i].e0 >> shift) : 0xFFFFu;
  vOut[i] = c0 + i;
}

// ---------------------------------------------------------------------------------------------
// k_l2_locate: one wave per candidate (4 per workgroup, no workgroup barrier).  LDS per wave: the fragment's query sketch
// (hash + strand) and a table of NB >= s equal-width buckets over [0, qmax] that turns the lower_bound of a hash into one table read
// plus a walk of ~1 entry (the hashes of a sketch are uniform, so equal-width buckets are balanced).
// ---------------------------------------------------------------------------------------------
template <int JB>
__global__ void __launch_bounds__(256)
k_l2_locate(int cBase, int nCand, int64_t opsBase, int s, int NB, const mm_l1_candidate* __restrict__ l1, const mm_frag_stats* __restrict__ stats,
            const uint64_t* __restrict__ qHash, const int8_t* __restrict__ qStrand,
            const uint64_t* __restrict__ skHash, const int8_t* __restrict__ skStrand,
            const uint32_t* __restrict__ evKey, const uint32_t* __restrict__ evAux, const uint64_t* __restrict__ evHash,
            const uint32_t* __restrict__ opKey, const uint32_t* __restrict__ opAux, const uint64_t* __restrict__ opHash,
            const int64_t* __restrict__ contigOff, const L2Info* __restrict__ info, const int64_t* __restrict__ opOff,
            const int32_t* __restrict__ opCnt, uint32_t* __restrict__ ops, const int32_t* __restrict__ order /* candidates in reference order, or null */,
            unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS: MM_L2F_STREAM */,
            const unsigned long long* __restrict__ nDev, uint16_t* __restrict__ initCells, L2Init* __restrict__ initState, int initStride, int preLimit) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;   // (readfirstlane: the candidate's extents then live in scalar registers)
  unsigned char* base = smem + (size_t)wave * mm_locate_lds_per_wave(s, NB);
  uint64_t* q = (uint64_t*)base;                                   // the query sketch + one sentinel
  uint32_t* qhi = (uint32_t*)(base + (size_t)(s + 1) * 8);         // its high words (the bucket walk compares these)
  uint16_t* bkt = (uint16_t*)(base + (size_t)(s + 1) * 8 + (size_t)(s + 2) / 2 * 8);   // bkt[b] = #query hashes whose bucket is < b, b = 0..NB
  int8_t* qs = (int8_t*)(base + (size_t)(s + 1) * 8 + (size_t)(s + 2) / 2 * 8 + (size_t)(NB + 4) * 2);
  uint32_t* ic = (uint32_t*)(base + (size_t)(s + 1) * 8 + (size_t)(s + 2) / 2 * 8 + (size_t)(NB + 4) * 2 + (((size_t)s + 15) & ~(size_t)15));   // pre-load state: two 16-bit cells per dword
  const int wpb = (int)(blockDim.x >> 6);                          // waves per workgroup: 4, fewer when a sketch's LDS share is large
  if (nDev) { const int nd = (int)*nDev - cBase; if (nd < nCand) nCand = nd; }   // steady state: the count stayed on the device (k_l2_gate has zeroed it if the streams do not fit)
  for (int ci = blockIdx.x * wpb + wave; ci < nCand; ci += gridDim.x * wpb) {
    const int c = order ? order[ci] : cBase + ci;                  // this launch covers the candidates [cBase, cBase + nCand): their streams start at ops[opOff - opsBase]
    const mm_l1_candidate cand = l1[c];
    const int f = cand.frag;
    const L2Info in = info[c];
    const int S = in.sketch & 0x7fffffff;
    uint32_t* out = ops + (opOff[c] - opsBase);
    const int cap = opCnt[c];
    const int nOpen = in.nOpen, nPre = in.nPre, nAll = in.nAll;
    // The kernel is bound by the latency of its global reads, not by their volume (the slices come from the Infinity Cache) nor by
    // instruction issue: round 3 walked a chain of ~20 dependent round trips per candidate (sketch, tail scan, the record behind the
    // tail, then one per 64 events).  Everything that depends only on the candidate's extents is therefore requested up front -- the
    // last 64 events of the slice, the 64 behind it, the first chunk of the stream -- and every later chunk while its predecessor
    // is being processed.
    const int64_t ce = contigOff[cand.seqId + 1];
    const int iT = nAll - 64 + lane;
    const uint32_t tailKey = (iT >= nPre && iT < nAll) ? evKey[in.e0 + iT] : 0u;           // insert flag = bit 0; 0 outside the slide
    const uint32_t behindKey = in.e0 + nAll + lane < ce ? evKey[in.e0 + nAll + lane] : 0u;
    // the stream in chunks of 64: the block's open records (all inserts, all before rangeStart), then the events [0, nPre) before
    // rangeStart, then the slide [nPre, nEv).  A chunk reads from wave-uniform arrays (one loop over a concatenation cost a per-lane
    // choice between two sets of three 64-bit pointers in every chunk)
    const int nChO = (nOpen + 63) >> 6, nChPre = nChO + ((nPre + 63) >> 6);
    auto loadChunk = [&](int ch, uint32_t& key, uint32_t& aux, uint64_t& h) {
      key = 0; aux = 0; h = 0;                                       // a lane without a record: no insert flag, nothing kept
      if (ch < nChO) { const int i = ch * 64 + lane; if (i < nOpen) { key = opKey[in.open0 + i]; aux = opAux[in.open0 + i]; h = opHash[in.open0 + i]; } }
      else {
        const int i = ch < nChPre ? (ch - nChO) * 64 + lane : nPre + (ch - nChPre) * 64 + lane;
        if (i < (ch < nChPre ? nPre : nAll)) { key = evKey[in.e0 + i]; aux = evAux[in.e0 + i]; h = evHash[in.e0 + i]; }
      }
    };
    uint32_t nKey, nAux; uint64_t nHash;
    loadChunk(0, nKey, nAux, nHash);
    __threadfence_block();                                         // previous candidate's LDS reads are done
    // a fragment that lost no frequent seed has no copy in qHash/qStrand: its sketch is the raw one (k_lookup_l1)
    const bool raw = in.sketch < 0;
    const uint64_t* srcH = (raw ? skHash : qHash) + (size_t)f * s;
    const int8_t* srcS = (raw ? skStrand : qStrand) + (size_t)f * s;
    for (int p = lane; p < S; p += 64) { const uint64_t h = srcH[p]; q[p] = h; qhi[p] = (uint32_t)(h >> 32); qs[p] = srcS[p]; }
    if (lane == 0) { q[S] = ~0ull; qhi[S] = ~0u; }                 // sentinel: a walk for h <= qmax needs no end test
    for (int d = lane; d <= (S + 1) / 2; d += 64) {                // cells 0 and S + 1: empty; 1 .. S: count 1, inactive, vote 0 (SlideMapper::init, slidingMap.hpp:103-121)
      const int p0 = 2 * d, p1 = 2 * d + 1;
      ic[d] = ((p0 >= 1 && p0 <= S) ? 0x2001u : 0u) | (((p1 >= 1 && p1 <= S) ? 0x2001u : 0u) << 16);
    }
    __threadfence_block();
    const uint64_t qmax = q[S - 1];
    // bucket(h): monotone map of [0, qmax] onto 0..NB-1: the top 24 significant bits times M >> 32, M <= 2^32 * NB / (top24(qmax) + 1)
    // (any smaller M stays monotone and below NB; the float estimate is shaded down)
    const int sh = qmax ? (int)__builtin_clzll(qmax) : 63;
    // (NB <= 16384 and the top bit of top24(qmax) is set, so M < 2^24 as well: a 24 x 24-bit multiply, which issues at full rate)
    const uint32_t bM = (uint32_t)((float)NB * 4294967296.0f / ((float)(uint32_t)((qmax << sh) >> 40) + 1.0f) * 0.99999f) & 0xFFFFFFu;
    auto bucket = [&](uint64_t h) -> int { return (int)(((uint64_t)((uint32_t)((h << sh) >> 40) & 0xFFFFFFu) * (uint64_t)bM) >> 32); };
    // bkt[b] = #{p : bucket(q[p]) < b}.  q is sorted, so entry p owns the buckets (bucket(q[p-1]), bucket(q[p])] and the
    // sentinel p = S owns the rest up to NB: a scatter of ~NB/S stores per lane instead of NB + 1 binary searches
    for (int p0 = 0; p0 <= S; p0 += 64) {
      const int p = p0 + lane;
      if (p <= S) {
        const int from = p == 0 ? 0 : bucket(q[p - 1]) + 1;
        const int to = p == S ? NB : bucket(q[p]);
        for (int b = from; b <= to; b++) bkt[b] = (uint16_t)p;
      }
    }
    __threadfence_block();
    auto locate = [&](uint64_t h) -> uint32_t {
      if (h > qmax) return 0u;
      const int b = bucket(h);
      // lower_bound(q, h): everything in earlier buckets is smaller and h <= qmax < sentinel, so the walk from the bucket's first entry
      // ends by itself; it runs on the 32-bit high words (32-bit LDS reads and compares) and only a tie there looks at all 64 bits.
      // One induction variable (the byte offset into qhi), made opaque behind the loop: left to itself the optimiser carries four
      // (index, index - 1 and two addresses), each with its own add and copy per step of a loop every lane of the wave waits for
      uint32_t off = (uint32_t)bkt[b] * 4u;
      const uint32_t hh = (uint32_t)(h >> 32);
      const unsigned char* qhiB = (const unsigned char*)qhi;
      uint32_t v = *(const uint32_t*)(qhiB + off);
      while (v < hh) { off += 4u; v = *(const uint32_t*)(qhiB + off); }
      asm volatile("" : "+v"(off));
      int lo = (int)(off >> 2);
      if (v == hh) { while (q[lo] < h) lo++; }
      return (uint32_t)(lo + 1) | (q[lo] == h ? (1u << EF<JB>::MATCH_BIT) : 0u) | ((uint32_t)((int)qs[lo] + 1) << EF<JB>::VOTE_SHIFT);   // query strand + 1
    };
    // the slide ends with the last insert at or before rangeEnd (evictions behind it are never reached, :1340); nextW: the wpos of the
    // record after it in the same contig, else its own (:1387-1390)
    int lastRel = -1, nextW = 0;                                   // lastRel: index of that insert relative to e0
    {
      const uint64_t m = mm_ballot((tailKey & 1u) != 0);
      if (m) { const int l = 63 - (int)__builtin_clzll(m); lastRel = nAll - 64 + l; nextW = (int)((uint32_t)__shfl((int)tailKey, l) >> 1); }
    }
    for (int hiEnd = nAll - 64; hiEnd > nPre && lastRel < 0; hiEnd -= 64) {               // (rare: 64 evictions at the end of a slice)
      const int i = hiEnd - 64 + lane;
      const uint32_t k2 = (i >= nPre && i < hiEnd) ? evKey[in.e0 + i] : 0u;
      const uint64_t m = mm_ballot((k2 & 1u) != 0);
      if (m) { const int l = 63 - (int)__builtin_clzll(m); lastRel = hiEnd - 64 + l; nextW = (int)((uint32_t)__shfl((int)k2, l) >> 1); }
    }
    if (lastRel >= 0) {                                            // everything of the slice behind lastRel is an eviction: go on behind the slice
      const uint64_t m0 = mm_ballot((behindKey & 1u) != 0);
      if (m0) nextW = (int)((uint32_t)__shfl((int)behindKey, (int)__builtin_ctzll(m0)) >> 1);
      else for (int64_t e = in.e0 + nAll + 64; e < ce; e += 64) {
        const uint32_t k2 = e + lane < ce ? evKey[e + lane] : 0u;
        const uint64_t m = mm_ballot((k2 & 1u) != 0);
        if (m) { nextW = (int)((uint32_t)__shfl((int)k2, (int)__builtin_ctzll(m)) >> 1); break; }
      }
    }
    int outN = 0;                                                  // entries written so far (wave-uniform)
    uint32_t preFlags = nOpen + nPre >= preLimit ? 2u : 0u;                    // a cell counts in 12 bits, and no cell can receive more than the pre-load holds: beyond that the exact kernel (32-bit counts) takes the candidate
    int posAcc = cand.rangeStartPos;                               // running position of the delta code (wave-uniform)
    bool tooWide = false;
    const int nEv = lastRel + 1;                                   // events [0, nEv) of the slice are streamed
    const int nCh = nChPre + ((nEv > nPre ? nEv - nPre : 0) + 63) / 64;
    asm volatile("" : "+v"(nKey), "+v"(nAux), "+v"(nHash));        // chunk 0 has arrived (no wait is then needed at the loop's head, where it would also cover the previous chunk's writes)
    for (int ch = 0; ch < nCh; ch++) {
      const uint32_t key = nKey, aux = nAux; const uint64_t h = nHash;
      if (ch + 1 < nCh) loadChunk(ch + 1, nKey, nAux, nHash);       // in flight while this chunk is located
      const bool isIns = (key & 1u) != 0;
      const int pos = (int)(key >> 1);
      const bool slide = ch >= nChPre;                               // wave-uniform
      bool keep, evalIns = false;
      if (!slide) keep = isIns && (int)(aux & 0x7fffffffu) > cand.rangeStartPos && pos >= in.target;   // still open at rangeStart (:1323-1338)
      else {
        const bool live = nPre + (ch - nChPre) * 64 + lane < nEv;
        keep = live && (isIns || h <= qmax);                         // an eviction outside the sketch's range changes nothing
        evalIns = live && isIns;
      }
      uint32_t op = 0;
      if (keep) {
        op = locate(h);
        // vote of a matching insert = query strand x reference strand: a REV record (aux bit 31) mirrors the field around 1
        if (isIns && (aux >> 31)) op = (op & ~(3u << EF<JB>::VOTE_SHIFT)) | ((2u - ((op >> EF<JB>::VOTE_SHIFT) & 3u)) << EF<JB>::VOTE_SHIFT);
        op |= 1u << (!slide ? E_PRE_BIT : (isIns ? E_INS_BIT : E_DEL_BIT));
      }
      if (!slide) {
        // the pre-load (records still open at rangeStart) goes into the cell state, not into the stream: a reference-only hash raises the
        // count of the cell it falls before, a matching one activates its cell with its vote (LDS atomics: the lanes of a chunk hit
        // arbitrary cells; two cells share a dword)
        asm volatile("" : "+v"(nKey), "+v"(nAux), "+v"(nHash));      // (the next chunk's reads are waited for here)
        const uint32_t j = op & EF<JB>::JMASK;
        if (keep && j) {
          const uint32_t sh = (j & 1u) * 16u;
          uint32_t* w = ic + (j >> 1);
          if (op & (1u << EF<JB>::MATCH_BIT)) {
            const uint32_t old = atomicOr(w, 0x1000u << sh);
            if ((old >> sh) & 0x1000u) preFlags |= 1u;               // open twice: only the exact kernel can follow that
            else atomicXor(w, ((1u ^ ((op >> EF<JB>::VOTE_SHIFT) & 3u)) << 13) << sh);   // vote + 1: from 1 (vote 0) to this record's
          } else atomicAdd(w, 1u << sh);                             // (nothing comes back; nPre bounds the count, see preFlags)
        }
        continue;
      }
      const uint64_t mKeep = mm_ballot(keep);
      // delta against the previous evaluated insert (lower lanes of this chunk, else the carry)
      const uint64_t mIns = mm_ballot(evalIns);
      int prevPos = posAcc;
      {
        const uint64_t below = mIns & ((1ull << lane) - 1ull);
        const int src = below ? 63 - (int)__builtin_clzll(below) : lane;
        const int p2 = __shfl(pos, src);
        if (below) prevPos = p2;
      }
      const int delta = evalIns ? pos - prevPos : 0;
      const bool needSkip = evalIns && delta > (int)EF<JB>::MAXDELTA;
      const uint64_t mSkip = mm_ballot(needSkip);                                  // slots before this lane: one per kept event, one more per skip
      const bool bigSkip = mm_ballot(needSkip && (uint32_t)(delta - (int)EF<JB>::MAXDELTA) > E_SKIP_MAX) != 0;
      asm volatile("" : "+v"(nKey), "+v"(nAux), "+v"(nHash));
      if (bigSkip) {
        // a gap that one skip entry (27 bits) cannot carry -- two reference minmers of one candidate more than 2^27 bases apart: the gap
        // is spread over as many skip entries as it takes (the reservation holds one per 2^DELTA_BITS bases of the range).  Round 3
        // failed the batch here.
        const uint32_t extra = needSkip ? (uint32_t)(delta - (int)EF<JB>::MAXDELTA) : 0u;
        const int nSkip = (int)((extra + E_SKIP_MAX - 1u) / E_SKIP_MAX);
        const int mineW = keep ? 1 + nSkip : 0;
        int at = outN + mm_wave_excl_scan(mineW);
        if (keep && at + mineW <= cap) {
          uint32_t left = extra;
          for (int i2 = 0; i2 < nSkip; i2++) { const uint32_t part = left > E_SKIP_MAX ? E_SKIP_MAX : left; out[at++] = (1u << E_SKIP_BIT) | part; left -= part; }
          out[at] = op | ((needSkip ? EF<JB>::MAXDELTA : (uint32_t)delta) << EF<JB>::DELTA_SHIFT);
        } else if (keep) tooWide = true;                                          // cannot happen: see the reservation in k_l2_extents
        outN += mm_wave_sum(mineW);
      } else {
        const int mine = keep ? (needSkip ? 2 : 1) : 0;
        const int at = outN + (int)mm_popc_below(mKeep) + (int)mm_popc_below(mSkip);
        if (keep && at + mine <= cap) {
          if (needSkip) {
            const uint32_t extra = (uint32_t)(delta - (int)EF<JB>::MAXDELTA);
            out[at] = (1u << E_SKIP_BIT) | (extra & E_SKIP_MAX);
            out[at + 1] = op | (EF<JB>::MAXDELTA << EF<JB>::DELTA_SHIFT);
          } else out[at] = op | ((uint32_t)delta << EF<JB>::DELTA_SHIFT);
        }
        outN += __popcll(mKeep) + __popcll(mSkip);
      }
      if (mIns) posAcc = __shfl(pos, 63 - (int)__builtin_clzll(mIns));
    }
    if (lane == 0) {                                               // end marker: carries the wpos behind the last insert
      int at = outN;
      uint32_t delta = lastRel >= 0 ? (uint32_t)(nextW - posAcc) : 0u;
      while (delta > EF<JB>::MAXDELTA) {                           // that record may be far away: as many skips as it takes
        const uint32_t extra = delta - EF<JB>::MAXDELTA > E_SKIP_MAX ? E_SKIP_MAX : delta - EF<JB>::MAXDELTA;
        if (at < cap) out[at] = (1u << E_SKIP_BIT) | extra;
        at++; delta -= extra;
      }
      if (at < cap) out[at] = (1u << E_END_BIT) | (delta << EF<JB>::DELTA_SHIFT);
      else tooWide = true;                                         // cannot happen: the reservation covers every event + skips
    }
    if (mm_ballot(tooWide) && lane == 0) atomicOr(&counters[MM_PC_L2_FLAGS], MM_L2F_STREAM);
    // ---- the state after the pre-load, in closed form (see L2Init): pivot = number of cells p with count(1) + .. + count(p) <= S (the sums
    // grow with p), pivRank = that sum at the pivot, shared / votes over the active cells up to it
    __threadfence_block();
    {
      int carry = 0, pivot = 0, pivRank = 0, shared = 0, votes = 0;
      for (int p0 = 1; p0 <= S; p0 += 64) {
        const int p = p0 + lane;
        const uint32_t w = p <= S ? (ic[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu : 0u;
        const int cnt = (int)(w & 0xFFFu);
        const int incl = carry + mm_wave_excl_scan(cnt) + cnt;
        const bool ok = p <= S && incl <= S;
        const uint64_t m = mm_ballot(ok);
        if (m) { pivot += (int)__popcll(m); pivRank = __shfl(incl, 63 - (int)__builtin_clzll(m)); }
        const bool act = ok && (w & 0x1000u);
        shared += (int)__popcll(mm_ballot(act));
        votes += mm_wave_sum(act ? (int)((w >> 13) & 3u) - 1 : 0);
        carry = __shfl(incl, 63);
      }
      const uint64_t fl = mm_ballot(preFlags != 0);
      uint32_t flags = 0;
      if (fl) flags = (mm_ballot((preFlags & 1u) != 0) ? 1u : 0u) | (mm_ballot((preFlags & 2u) != 0) ? 2u : 0u);
      // (16-bit stores: writing the row as the dwords it occupies in LDS made the kernel 10 % slower -- profiles/NOTES.md, r13s)
      uint16_t* row = initCells + (size_t)(c - cBase) * (size_t)initStride;
      for (int p = lane; p < S + 2; p += 64) row[p] = (uint16_t)((ic[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu);
      if (lane == 0) initState[c - cBase] = L2Init{pivot | (int32_t)(flags << L2INIT_FLAG_SHIFT), pivRank, shared, votes};
    }
  }
}

// ---------------------------------------------------------------------------------------------
// bit B of x as a lane mask (all ones / zero): one v_bfe_i32, opaque to the optimiser (see k_l2_sweep)
template <int B> __device__ __forceinline__ int mm_bit_mask(uint32_t x) { int m; asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(x), "n"(B)); return m; }

// k_l2_sweep<WIDE>: one lane per candidate.  Per-lane SlideMapper state in LDS, one cell per query position p:
//   num_before_inc (CB bits) | active (1 bit) | strand_vote + 1 (2 bits)
// The LDS that 64 such states need is what limits the waves per CU, and the kernel is latency bound, so the first pass uses
// 8-bit cells (CB = 5: 18 waves/CU at s = 130).  num_before_inc counts the open reference-only hashes between two neighbouring
// query hashes -- about one on average; a candidate where one exceeds 31 is queued and redone with 16-bit cells (CB = 12).
// Cell p of lane l sits at p * LPW + l (16-bit cells of a full wave: half l >> 5 of dword p * 32 + (l & 31)), so that a cell's LDS
// address is one shift-add of its position, the pivot's right neighbour is the same address with an immediate offset, and no address
// arithmetic is left in the per-entry instruction budget -- the kernel is bound by VALU issue, not by LDS: four lanes share a bank of
// the 8-bit layout, which costs the DS pipe a second pass now and then and the SIMDs nothing (round 4; until then every lane owned a
// bank, byte p & 3 of dword (p >> 2) * 64 + l, at five more VALU instructions per cell access).  One cell of padding behind position S
// lets the neighbour be read without clamping (its value is masked when the pivot is at S).
// ---------------------------------------------------------------------------------------------
// one locus of candidate `candLocal` of fragment f as the record the selection reads
__device__ __forceinline__ mm_l2_locus mm_l2_record(int f, int candLocal, int seqId, int start, int end, int shared, int strand) {
  mm_l2_locus o;
  o.frag = f; o.cand = candLocal; o.seqId = seqId; o.optimalStart = start; o.optimalEnd = end;
  o.meanOptimalPos = (start + end) / 2; o.sharedSketchSize = shared; o.strand = strand;
  return o;
}
// LPW lanes of a wave carry a candidate (64; fewer for sketches whose 64 states would not fit a CU's LDS: 32, 16 or 8 -- the other
// lanes leave at once); JB: width of the stream entries' sketch-position field.
template <bool WIDE, int JB, int LPW>
__global__ void __launch_bounds__(64)
k_l2_sweep(int cBase, int nCand, int64_t opsBase, const int32_t* __restrict__ candList, int segLength, const mm_l1_candidate* __restrict__ l1, const mm_frag_stats* __restrict__ stats,
           const int64_t* __restrict__ opOff, const int32_t* __restrict__ opCnt, const uint32_t* __restrict__ ops,
           const int64_t* __restrict__ l1Off, L2Tmp* __restrict__ tmp, int locap, mm_l2_locus* __restrict__ l2, unsigned long long l2Cap,
           int32_t* __restrict__ wideList, int32_t* __restrict__ exactList, int64_t* __restrict__ l2First, int32_t* __restrict__ l2Num,
           unsigned long long* __restrict__ counters /* dCounters + MM_CW_PASS: the L2 words and the two lists' lengths */,
           const unsigned long long* __restrict__ nDev /* non-null: the number of candidates (minus cBase) or of list entries lives there */, int listCap,
           const uint16_t* __restrict__ initCells, const L2Init* __restrict__ initState, int initStride, int initBase /* rows of the chunk: candidate - initBase */) {
  typedef typename std::conditional<WIDE, uint16_t, uint8_t>::type CellT;
  constexpr int CB = WIDE ? 12 : 5;
  constexpr uint32_t CMASK = (1u << CB) - 1u;
#define CELL_CNT(x) ((int)((x) & CMASK))
#define CELL_ACT(x) ((int)(((x) >> CB) & 1u))
#define CELL_VOTE(x) ((int)(((x) >> (CB + 1)) & 3u) - 1)
  extern __shared__ __attribute__((aligned(16))) unsigned char cellRaw[];
  CellT* cell = (CellT*)cellRaw;
  const int lane = threadIdx.x;
  const int li = blockIdx.x * LPW + lane;
  if (nDev) {
    const long long nd = (long long)*nDev - (listCap ? 0 : cBase);
    if (listCap && nd > listCap && li == 0) atomicOr(&counters[MM_PC_L2_FLAGS], MM_L2F_LIST);   // more listed candidates than this launch covers: the pass is redone with the host's sizing
    nCand = (int)(nd < (listCap ? listCap : nCand) ? nd : (listCap ? listCap : nCand));
  }
  const bool live = lane < LPW && li < nCand;          // (the other lanes of the wave only help with the initial state)
  int cIdx = 0, S = 0, f = 0;
  mm_l1_candidate cand{0, 0, 0, 0, 0};
  if (live) {
    cIdx = candList ? candList[li] : cBase + li;       // candidates [cBase, cBase + nCand), or the listed ones (absolute indices); ops holds the streams from opsBase on
    cand = l1[cIdx]; f = cand.frag; S = stats[f].sketchSize;
  }
  auto lbaseOf = [](int l) -> int { return WIDE && LPW == 64 ? (l & 31) * 2 + (l >> 5) : l; };
  const int lbase = lbaseOf(lane);
#define CELL(p) cell[(p) * LPW + lbase]
  // The state after the pre-load comes ready-made from k_l2_locate (L2Init): every candidate's row of s + 2 16-bit cells is read by the whole
  // wave, 64 consecutive cells at a time, into that candidate's column of the LDS block; a count the 8-bit cells cannot hold flags the
  // candidate for the 16-bit re-run, as an insert into a full cell would have
  int cntOverflow = 0, doubleOpen = 0;
  {
    uint64_t rows = __ballot(live), over = 0;
    while (rows) {
      const int r = (int)__builtin_ctzll(rows); rows &= rows - 1ull;
      const int cR = __shfl(cIdx, r), sR = __shfl(S, r);
      const uint16_t* row = initCells + (size_t)(cR - initBase) * (size_t)initStride;
      const int lb = lbaseOf(r);
      bool tooBig = false;
      for (int p = (int)threadIdx.x; p < sR + 2; p += 64) {
        const uint32_t w = row[p];
        if (WIDE) cell[p * LPW + lb] = (CellT)w;
        else {
          const uint32_t cnt = w & 0xFFFu;
          tooBig |= cnt > CMASK;
          cell[p * LPW + lb] = (CellT)((cnt & CMASK) | (((w >> 12) & 1u) << CB) | (((w >> 13) & 3u) << (CB + 1)));
        }
      }
      if (__ballot(tooBig)) over |= 1ull << r;
    }
    __threadfence_block();
    if (!live) return;
    if ((over >> lane) & 1ull) cntOverflow = -1;
  }
  const L2Init ist = initState[cIdx - initBase];
  const int iflags = (int)((uint32_t)ist.pivot >> L2INIT_FLAG_SHIFT);
  if (iflags & 1) doubleOpen = -1;                     // a query hash open twice in the pre-load: k_l2_sweep_exact
  if (iflags & 2) cntOverflow = -1;                    // a pre-load too long for 12-bit counts: likewise (through the 16-bit re-run's own overflow)
  const uint4* src = (const uint4*)(ops + (opOff[cIdx] - opsBase));
  const int nSteps = opCnt[cIdx] / E_STEP;             // 16 entries = 4 x 16 bytes per step
  int posAcc = cand.rangeStartPos;                     // running position of the delta code
  int pivot = ist.pivot & ((1 << L2INIT_FLAG_SHIFT) - 1), pivRank = ist.pivRank, shared = ist.shared, votes = ist.votes;

  // Lane masks.  The 64 lanes of a wave are at different candidates and take different cases at every entry, so the cases are
  // not branches (measured 5x slower) but all-ones / zero integers combined with and/or/add: a kind bit of the entry becomes
  // a mask with one v_bfe_i32, a comparison of two small non-negative numbers with a subtract and an arithmetic shift, and
  // "x += c ? a : 0" is "x += a & m".  These are 32-bit-encoded VALU instructions, which issue about twice as fast on this
  // part as the v_cmp + v_cndmask pairs (64-bit encodings) the bool form compiles to.  The mask
  // producers are inline asm so that the optimiser does not turn "mask & value" back into compare + select.
#define BITM(x, b) mm_bit_mask<b>((uint32_t)(x))
  auto neg = [](int x) -> int { int m; asm("v_ashrrev_i32 %0, 31, %1" : "=v"(m) : "v"(x)); return m; };   // x < 0 ? ~0 : 0
  auto sel = [](int m, int a, int b2) -> int { return (a & m) | (b2 & ~m); };                               // v_bfi_b32

  // SlideMapper::insert_minmer / delete_minmer (slidingMap.hpp:125-211): the four cases (insert or delete x hash matches a
  // query hash or not) as masks IM, IN, DM, DN.  The cell of the hash, of the pivot and of its right neighbour are read up
  // front, independent of the case.  insM: the entry inserts (insert or pre-load), delM: it evicts.
  auto apply = [&](uint32_t e, int insM, int delM) {
    const int j = (int)(e & EF<JB>::JMASK) & (insM | delM);   // 0: no hash / hash beyond the query sketch -> no effect (cell 0 is a dummy)
    const int valid = neg(-j) & ~cntOverflow;          // after a counter overflow the lane only idles to the end
    const int mt = BITM(e, EF<JB>::MATCH_BIT);
    const int ltS = neg(pivot - S);                    // pivot + 1 <= S
    const int pn = pivot + 1;                          // at pivot == S: the padding cell, masked by ltS below
    const uint32_t cw = CELL(j), pw = CELL(pivot), nw = CELL(pn);
    const int vi = valid & insM, vd = valid & delM;
    const int IM = vi & mt, IN = vi & ~mt, DM = vd & mt, DN = vd & ~mt;
    const int vf = (int)((e >> EF<JB>::VOTE_SHIFT) & 3u);   // vote + 1; a query hash normally has one open reference window at a time (windowLen == 0):
    doubleOpen |= IM & BITM(cw, CB);                   // the 2-bit vote relies on it; a candidate that violates it is handed to k_l2_sweep_exact
    cntOverflow |= IN & neg((int)(CMASK - 1u) - (int)(cw & CMASK));   // the counter of this cell is full: redo the candidate with wide cells
    const int repl = (int)(cw & CMASK) | sel(IM, (int)((1u << CB) | ((uint32_t)vf << (CB + 1))), (int)(1u << (CB + 1)));
    const int ncw = sel(IM | DM, repl, (int)cw - IN + DN);            // IN: count + 1, DN: count - 1 (the masks are -1)
    CELL(j) = (CellT)ncw;
    const int ip = ~neg(pivot - j);                    // j <= pivot
    const int IMp = IM & ip, DMp = DM & ip;
    shared += DMp - IMp;
    votes += ((vf - 1) & IMp) - (CELL_VOTE(cw) & DMp);
    pivRank += (DN & ip) - (IN & ip);
    // insert of a non-shared hash can push the pivot one cell left (:155-160)
    const int pwp = sel(neg((pivot ^ j) - 1), ncw, (int)pw);          // pivot == j: the cell just written
    const int left = IN & neg(S - pivRank);                           // pivRank > S
    // delete of a non-shared hash can let it move one cell right (:201-207)
    const int nwp = sel(neg((pn ^ j) - 1), ncw, (int)nw);
    const int right = DN & ltS & ~neg(S - pivRank - CELL_CNT(nwp));   // pivRank + count(next) <= S
    shared += (CELL_ACT(nwp) & right) - (CELL_ACT(pwp) & left);
    votes += (CELL_VOTE(nwp) & right) - (CELL_VOTE(pwp) & left);
    pivRank += (CELL_CNT(nwp) & right) - (CELL_CNT(pwp) & left);
    pivot += left - right;
  };

  // best-position bookkeeping (:1376-1449)
  int bestShared = 1, inRun = 0;
  int curStart = 0, curEnd = 0, curShared = 0;
  int nFlushed = 0, havePend = 0; L2Tmp pend{0, 0, 0, 0};
  L2Tmp* mySlots = tmp + (size_t)cIdx * locap;
  bool slotOverflow = false;
  auto close_run = [&](int strand) {                   // :1417-1426 / :1440-1449
    if (!havePend || pend.end + segLength < curStart) {
      if (havePend) { if (nFlushed < locap) mySlots[nFlushed] = pend; else slotOverflow = true; nFlushed++; }
      pend.start = curStart; pend.end = curEnd; pend.shared = curShared; pend.strand = strand; havePend = -1;
    } else {
      pend.end = curEnd;
    }
  };
  // the evaluation of insert i needs the wpos of record i+1, so it is carried until the next insert / end entry arrives
  // lastVotes = strand_votes right after the most recent insert (pre-load included): the reference samples it before the
  // evictions that precede the next insert (:1342)
  int evalPending = 0, evW = 0, evShared = 0, evPrevVotes = 0, lastVotes = votes;      // (votes right after the last pre-load insert)
  // the three outcomes of an evaluation (:1376-1430) as masks; only the closing of a run -- rare -- is a branch
  auto evaluate = [&](int on, int nextW) {
    const int gt = on & neg(bestShared - evShared), lt = on & neg(evShared - bestShared), ge = on & ~lt;
    if (lt & inRun) { curEnd = nextW; close_run(evPrevVotes >= 0 ? 1 : -1); curStart = 0; curEnd = 0; curShared = 0; }
    const int startNew = gt | (ge & ~inRun);
    nFlushed &= ~gt; havePend &= ~gt;                  // l2_vec_out.clear()
    bestShared = sel(gt, evShared, bestShared);
    curShared = sel(startNew, evShared, curShared);
    curStart = sel(startNew, evW, curStart);
    curEnd = sel(ge, nextW, curEnd);
    inRun = sel(on, ge, inRun);
  };

  int done = 0;
  uint4 cur[4], nxt[4];
  if (nSteps > 0) {
#pragma unroll
    for (int k = 0; k < 4; k++) cur[k] = src[k];
  }
  for (int step = 0; step < nSteps && !done; step++) {
    if (step + 1 < nSteps) {
#pragma unroll
      for (int k = 0; k < 4; k++) nxt[k] = src[(size_t)(step + 1) * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < E_STEP; k++) {
      const uint4 v = cur[k >> 2];
      const uint32_t eRaw = (k & 3) == 0 ? v.x : (k & 3) == 1 ? v.y : (k & 3) == 2 ? v.z : v.w;
      const uint32_t e = eRaw & (uint32_t)~done;         // a finished lane reads on behind its end marker: no kind bit, no effect
      // straight-line per entry: the entry kinds are masks, not branches
      const int mIns = BITM(e, 27), mDel = BITM(e, 28), mEnd = BITM(e, 30);              // (no pre-load entries: the state starts behind them)
      const int mSkip = neg((int)e);
      const int ie = mIns | mEnd;
      posAcc += ((int)((e >> EF<JB>::DELTA_SHIFT) & EF<JB>::MAXDELTA) & ie) | ((int)(e & E_SKIP_MAX) & mSkip);
      const int wpos = posAcc;
      evaluate(ie & evalPending, wpos);
      evalPending = (evalPending & ~ie) | mIns;
      done |= mEnd;
      evPrevVotes = sel(mIns, lastVotes, evPrevVotes);
      apply(e, mIns, mDel);
      lastVotes = sel(mIns, votes, lastVotes);
      evW = sel(mIns, wpos, evW); evShared = sel(mIns, shared, evShared);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) cur[k] = nxt[k];
  }
  if (inRun) close_run(votes >= 0 ? 1 : -1);
#undef CELL
#undef CELL_CNT
#undef CELL_ACT
#undef CELL_VOTE
  int total = nFlushed + (havePend ? 1 : 0);
  if (cntOverflow) {
    total = 0;
    if (WIDE) exactList[atomicAdd(&counters[MM_PC_L2_EXACT_LEN], 1ull)] = cIdx;   // > 4094 open reference-only hashes between two query hashes: the literal kernel counts in 32 bits
    else wideList[atomicAdd(&counters[MM_PC_L2_WIDE_LEN], 1ull)] = cIdx;
  }
  if (doubleOpen && !cntOverflow) {                    // a query hash with two reference windows open at once: the 2-bit vote cell cannot hold it;
    total = 0; slotOverflow = false;                   // the candidate is redone by k_l2_sweep_exact
    exactList[atomicAdd(&counters[MM_PC_L2_EXACT_LEN], 1ull)] = cIdx;
  }
  if (slotOverflow && !cntOverflow) { atomicOr(&counters[MM_PC_L2_FLAGS], MM_L2F_SLOTS); total = 0; }
  // one reservation per wave (64 candidates): exclusive scan of the lanes' counts, lane 63 of the active lanes asks
  int incl = total;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(incl, o); if (lane >= o) incl += y; }
  const uint64_t activeMask = __ballot(1);
  const int lastLane = 63 - __builtin_clzll(activeMask);
  const int waveTotal = __shfl(incl, lastLane);
  unsigned long long wbase = 0;
  if (lane == lastLane && waveTotal > 0) wbase = atomicAdd(&counters[MM_PC_L2_LOCI], (unsigned long long)waveTotal);
  wbase = mm_bcast64_shfl(wbase, lastLane);
  if (waveTotal > 0 && wbase + (unsigned long long)waveTotal > l2Cap) { if (lane == lastLane) atomicOr(&counters[MM_PC_L2_OVERFLOW], MM_OVERFLOWED); return; }
  l2First[cIdx] = (int64_t)(wbase + (unsigned long long)(incl - total)); l2Num[cIdx] = total;   // where k_l2_select finds this candidate's loci
  if (total > 0) {
    const unsigned long long base = wbase + (unsigned long long)(incl - total);
    const int candLocal = (int)(cIdx - l1Off[f]);
    for (int k = 0; k < total; k++) {
      const L2Tmp t = (k < nFlushed) ? mySlots[k] : pend;
      l2[base + k] = mm_l2_record(f, candLocal, cand.seqId, t.start, t.end, t.shared, t.strand);   // a candidate's loci are contiguous and in emission order
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_l2_sweep_exact: the SlideMapper sweep of one candidate per thread, literally (slidingMap.hpp:125-211), for the candidates the fast
// kernels hand over: an index in which two windows of one hash overlap (addMinmers only removes ADJACENT duplicates,
// commonFunc.hpp:560; an index written by another program may hold anything) makes a query hash active twice.  The reference's state
// then keeps `active` a boolean, accumulates strand_vote, and counts sharedSketchElements once per insert and once per delete -- which
// is what this kernel does, cell by cell, with the state in global memory (count, active, accumulated vote per query position).
// Rare by construction, so nothing here is tuned.
// ---------------------------------------------------------------------------------------------
struct ExactCell { int32_t cnt; int16_t vote; int16_t active; };
// The end of candidate c for a kernel that gives it one THREAD: its `total` loci (the first nFlushed in mySlots, then the pending one) are
// claimed from the pass's cursor and written, l2First / l2Num say where k_l2_select finds them.  Where they do not fit the buffer,
// MM_PC_L2_OVERFLOW is raised and nothing is written.
__device__ __forceinline__ void mm_l2_emit_thread(int c, const mm_l1_candidate& cand, int total, int nFlushed, const L2Tmp* __restrict__ mySlots, const L2Tmp& pend,
                                                  const int64_t* __restrict__ l1Off, mm_l2_locus* __restrict__ l2, unsigned long long l2Cap,
                                                  int64_t* __restrict__ l2First, int32_t* __restrict__ l2Num, unsigned long long* __restrict__ counters) {
  unsigned long long base = 0;
  if (total > 0) {
    base = atomicAdd(&counters[MM_PC_L2_LOCI], (unsigned long long)total);
    if (base + (unsigned long long)total > l2Cap) { atomicOr(&counters[MM_PC_L2_OVERFLOW], MM_OVERFLOWED); return; }
  }
  l2First[c] = (int64_t)base; l2Num[c] = total;
  const int candLocal = (int)(c - l1Off[cand.frag]);
  for (int k = 0; k < total; k++) {
    const L2Tmp t = (k < nFlushed) ? mySlots[k] : pend;
    l2[base + k] = mm_l2_record(cand.frag, candLocal, cand.seqId, t.start, t.end, t.shared, t.strand);
  }
}
__global__ void __launch_bounds__(64)
k_l2_sweep_exact(int jb, int nList, int64_t opsBase, const int32_t* __restrict__ list, int segLength, const mm_l1_candidate* __restrict__ l1, const mm_frag_stats* __restrict__ stats,
                 const int64_t* __restrict__ opOff, const int32_t* __restrict__ opCnt, const uint32_t* __restrict__ ops,
                 const int64_t* __restrict__ l1Off, ExactCell* __restrict__ cells, int cellStride, L2Tmp* __restrict__ tmp, int locap,
                 mm_l2_locus* __restrict__ l2, unsigned long long l2Cap, int64_t* __restrict__ l2First, int32_t* __restrict__ l2Num,
                 unsigned long long* __restrict__ counters, const unsigned long long* __restrict__ nDev,
                 const L2Info* __restrict__ info, int s, const uint64_t* __restrict__ qHash, const int8_t* __restrict__ qStrand,
                 const uint64_t* __restrict__ skHash, const int8_t* __restrict__ skStrand,
                 const uint32_t* __restrict__ evKey, const uint32_t* __restrict__ evAux, const uint64_t* __restrict__ evHash,
                 const uint32_t* __restrict__ opKey, const uint32_t* __restrict__ opAux, const uint64_t* __restrict__ opHash) {
  const int li = blockIdx.x * 64 + threadIdx.x;
  if (nDev) {                                          // steady state: the launch covers nList entries, the list's length is on the device
    const long long nd = (long long)*nDev;
    if (nd > nList && li == 0) atomicOr(&counters[MM_PC_L2_FLAGS], MM_L2F_LIST);
    if (nd < nList) nList = (int)nd;
  }
  if (li >= nList) return;
  const int cIdx = list[li];
  const mm_l1_candidate cand = l1[cIdx];
  const int f = cand.frag;
  const int S = stats[f].sketchSize;
  const uint32_t jmask = (1u << jb) - 1u; const int deltaShift = jb + 3; const uint32_t maxDelta = (1u << (27 - deltaShift)) - 1u;
  ExactCell* cell = cells + (size_t)li * cellStride;
  cell[0] = ExactCell{0, 0, 0};
  for (int p = 1; p <= S; p++) cell[p] = ExactCell{1, 0, 0};                   // SlideMapper::init (:103-121)
  int pivot = S, pivRank = S, shared = 0, votes = 0;
  const uint32_t* src = ops + (opOff[cIdx] - opsBase);
  const int nEnt = opCnt[cIdx];
  int posAcc = cand.rangeStartPos;
  int bestShared = 1; bool inRun = false;
  int curStart = 0, curEnd = 0, curShared = 0;
  int nFlushed = 0; bool havePend = false; L2Tmp pend{0, 0, 0, 0};
  L2Tmp* mySlots = tmp + (size_t)cIdx * locap;
  bool slotOverflow = false;
  auto close_run = [&](int strand) {                                             // computeMap.hpp:1417-1426 / :1440-1449
    if (!havePend || pend.end + segLength < curStart) {
      if (havePend) { if (nFlushed < locap) mySlots[nFlushed] = pend; else slotOverflow = true; nFlushed++; }
      pend.start = curStart; pend.end = curEnd; pend.shared = curShared; pend.strand = strand; havePend = true;
    } else pend.end = curEnd;
  };
  bool evalPending = false; int evW = 0, evShared = 0, evPrevVotes = 0, lastVotes = 0;
  // insert_minmer (slidingMap.hpp:125-165) for the hash at 1-based sketch position j (0: beyond the sketch, no effect)
  auto insert = [&](int j, bool match, int vote) {
    if (j <= 0) return;
    ExactCell c = cell[j];
    if (match) {
      c.active = 1; c.vote = (int16_t)(c.vote + vote);
      if (j <= pivot) { shared++; votes += c.vote; }
      cell[j] = c;
    } else {
      c.cnt++; cell[j] = c;
      if (j <= pivot) pivRank++;
      if (pivRank > S) { const ExactCell pc = cell[pivot]; shared -= pc.active; votes -= pc.vote; pivRank -= pc.cnt; pivot--; }
    }
  };
  {
    // The pre-load (computeMap.hpp:1323-1338) is not in the stream (the fast kernels get its result in closed form, L2Init): it is replayed
    // here from the index, record by record in index order -- the block's list of open records, then the events before rangeStart --, with
    // k_l2_locate's rule for what is still open at rangeStart and a binary search of the query sketch in place of its LDS table
    const L2Info in = info[cIdx];
    const bool raw = in.sketch < 0;
    const uint64_t* qh = (raw ? skHash : qHash) + (size_t)f * s;
    const int8_t* qv = (raw ? skStrand : qStrand) + (size_t)f * s;
    const uint64_t qmax = S > 0 ? qh[S - 1] : 0ull;
    auto one = [&](uint32_t key, uint32_t aux, uint64_t h) {
      const bool isInsert = (key & 1u) != 0; const int pos = (int)(key >> 1);
      if (!(isInsert && (int)(aux & 0x7fffffffu) > cand.rangeStartPos && pos >= in.target)) return;
      if (S > 0 && h <= qmax) {
        int lo = 0, hi = S;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (qh[mid] < h) lo = mid + 1; else hi = mid; }
        const bool match = qh[lo] == h;
        insert(lo + 1, match, (aux >> 31) ? -(int)qv[lo] : (int)qv[lo]);        // vote = query strand x reference strand
      }
      lastVotes = votes;
    };
    for (int i = 0; i < in.nOpen; i++) one(opKey[in.open0 + i], opAux[in.open0 + i], opHash[in.open0 + i]);
    for (int i = 0; i < in.nPre; i++) one(evKey[in.e0 + i], evAux[in.e0 + i], evHash[in.e0 + i]);
  }
  for (int i = 0; i < nEnt; i++) {
    const uint32_t e = src[i];
    const bool isIns = (e >> E_INS_BIT) & 1u, isDel = (e >> E_DEL_BIT) & 1u, isPre = (e >> E_PRE_BIT) & 1u, isEnd = (e >> E_END_BIT) & 1u, isSkip = (e >> E_SKIP_BIT) & 1u;
    if (isSkip) { posAcc += (int)(e & E_SKIP_MAX); continue; }
    if (isIns || isEnd) posAcc += (int)((e >> deltaShift) & maxDelta);
    const int wpos = posAcc;
    if ((isIns || isEnd) && evalPending) {                                       // the evaluation behind the previous insert (:1376-1430): it needed this wpos
      if (evShared > bestShared) {
        nFlushed = 0; havePend = false; bestShared = evShared;
        curShared = evShared; curStart = evW; curEnd = wpos; inRun = true;
      } else if (evShared == bestShared) {
        if (!inRun) { curShared = evShared; curStart = evW; }
        curEnd = wpos; inRun = true;
      } else {
        if (inRun) { curEnd = wpos; close_run(evPrevVotes >= 0 ? 1 : -1); curStart = curEnd = curShared = 0; }
        inRun = false;
      }
      evalPending = false;
    }
    if (isEnd) break;
    if (isIns) { evalPending = true; evPrevVotes = lastVotes; }
    const int j = (int)(e & jmask);
    if (j > 0 && (isIns || isPre || isDel)) {
      const bool match = (e >> jb) & 1u;
      ExactCell c = cell[j];
      if (isIns || isPre) {                                                      // insert_minmer (:125-165)
        if (match) {
          c.active = 1; c.vote = (int16_t)(c.vote + ((int)((e >> (jb + 1)) & 3u) - 1));
          if (j <= pivot) { shared++; votes += c.vote; }
          cell[j] = c;
        } else {
          c.cnt++; cell[j] = c;
          if (j <= pivot) pivRank++;
          if (pivRank > S) { const ExactCell pc = cell[pivot]; shared -= pc.active; votes -= pc.vote; pivRank -= pc.cnt; pivot--; }
        }
      } else {                                                                   // delete_minmer (:171-211)
        if (match) {
          if (j <= pivot) { shared--; votes -= c.vote; }
          c.active = 0; c.vote = 0; cell[j] = c;
        } else {
          c.cnt--; cell[j] = c;
          if (j <= pivot) pivRank--;
          if (pivot + 1 <= S && pivRank + cell[pivot + 1].cnt <= S) { pivot++; const ExactCell pc = cell[pivot]; shared += pc.active; votes += pc.vote; pivRank += pc.cnt; }
        }
      }
    }
    if (isIns || isPre) lastVotes = votes;
    if (isIns) { evW = wpos; evShared = shared; }
  }
  if (inRun) close_run(votes >= 0 ? 1 : -1);
  int total = nFlushed + (havePend ? 1 : 0);
  if (slotOverflow) { atomicOr(&counters[MM_PC_L2_FLAGS], MM_L2F_SLOTS); total = 0; }
  mm_l2_emit_thread(cIdx, cand, total, nFlushed, mySlots, pend, l1Off, l2, l2Cap, l2First, l2Num, counters);
}


// ---------------------------------------------------------------------------------------------
// windowLen != 0 (--noSplit with a read longer than segLength; computeMap.hpp:1276-1451 with Q.len > segLength): the L2 stage literally, one
// thread per candidate.  minmerIndex is walked as the insert events of the contig's stream (they are its records, in index order); the
// open records sit in a heap ordered by wpos_end with libstdc++'s element movements (std::push_heap / std::pop_heap, mm_heap.h); a
// count of open windows per hash (hash_to_freq, :1310) decides, as in the reference, whether a record enters the SlideMapper and whether
// the position is evaluated at all -- including the reference's way of retiring a record whose hash was counted more than once
// (:1344-1357: the front is decremented until its count reaches zero, then popped).  State per candidate in HBM scratch: SlideMapper
// cells, the heap, an open-addressing table for the counts.  A slow path by design: correctness for the one mode the fast kernels
// cannot express; split mode never comes here.
// ---------------------------------------------------------------------------------------------
struct WinExt { int64_t e0, e1; };                               // events [e0, e1) of the contig: from lower_bound(rangeStart - segLength - 1) to the last wpos <= rangeEnd + windowLen
__global__ void __launch_bounds__(256)
k_l2_window_extents(int nCand, int segLength, const mm_l1_candidate* __restrict__ l1, const DFrag* __restrict__ frags, const uint32_t* __restrict__ evKey,
                    const int64_t* __restrict__ contigOff, WinExt* __restrict__ ext, int32_t* __restrict__ cntH, int32_t* __restrict__ cntT) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nCand) return;
  const mm_l1_candidate cand = l1[c];
  int W = frags[cand.frag].len - segLength; if (W < 0) W = 0;
  const int64_t cb = contigOff[cand.seqId], ce = contigOff[cand.seqId + 1];
  auto lowerIn = [&](int64_t lo, int64_t hi, uint64_t key) { while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((uint64_t)evKey[mid] < key) lo = mid + 1; else hi = mid; } return lo; };
  const long long target = (long long)cand.rangeStartPos - segLength - 1;
  const int64_t e0 = target <= 0 ? cb : lowerIn(cb, ce, (uint64_t)target * 2ull);
  const long long last = (long long)cand.rangeEndPos + W;
  const int64_t e1 = last < 0 ? e0 : lowerIn(e0, ce, (uint64_t)last * 2ull + 2ull);
  ext[c] = WinExt{e0, e1 < e0 ? e0 : e1};
  const int64_t n = (e1 < e0 ? 0 : e1 - e0) + 2;
  int64_t t = 16; while (t < 2 * n) t <<= 1;
  cntH[c] = (int32_t)n; cntT[c] = (int32_t)t;
}

__global__ void __launch_bounds__(64)
k_l2_window(int nCand, int s, int segLength, const mm_l1_candidate* __restrict__ l1, const mm_frag_stats* __restrict__ stats, const DFrag* __restrict__ frags,
            const uint64_t* __restrict__ qHash, const int8_t* __restrict__ qStrand, const uint64_t* __restrict__ skHash, const int8_t* __restrict__ skStrand,
            const uint32_t* __restrict__ evKey, const uint32_t* __restrict__ evAux, const uint64_t* __restrict__ evHash, const int64_t* __restrict__ contigOff,
            const WinExt* __restrict__ ext, const int64_t* __restrict__ offH, const int64_t* __restrict__ offT, const int32_t* __restrict__ cntT,
            int32_t* __restrict__ heapAll, uint64_t* __restrict__ tabKeys, int32_t* __restrict__ tabVals, ExactCell* __restrict__ cells,
            const int64_t* __restrict__ l1Off, L2Tmp* __restrict__ tmp, int locap, mm_l2_locus* __restrict__ l2, unsigned long long l2Cap,
            int64_t* __restrict__ l2First, int32_t* __restrict__ l2Num, unsigned long long* __restrict__ counters,
            const int32_t* __restrict__ list /* null: every candidate; else the candidates k_l2_window_wave handed over ... */,
            const unsigned long long* __restrict__ nListDev /* ... whose number stays on the device */) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nCand) return;
  if (list) { if ((unsigned long long)c >= *nListDev) return; c = list[c]; }
  const mm_l1_candidate cand = l1[c];
  const int f = cand.frag;
  const mm_frag_stats fst = stats[f];
  const int S = fst.sketchSize;
  int W = frags[f].len - segLength; if (W < 0) W = 0;
  const bool raw = fst.rawSketchSize == fst.sketchSize;                         // no seed was removed: the sketch is the raw one (k_lookup_l1)
  const uint64_t* q = (raw ? skHash : qHash) + (size_t)f * s;                  // Q.minmerTableQuery, ascending
  const int8_t* qs = (raw ? skStrand : qStrand) + (size_t)f * s;
  ExactCell* cell = cells + (size_t)c * (s + 1);
  cell[0] = ExactCell{0, 0, 0};
  for (int p = 1; p <= S; p++) cell[p] = ExactCell{1, 0, 0};                   // SlideMapper::init (slidingMap.hpp:103-121)
  int pivot = S, pivRank = S, shared = 0, votes = 0;
  int32_t* heap = heapAll + offH[c]; int nHeap = 0;                             // event indices relative to e0
  uint64_t* tk = tabKeys + offT[c]; int32_t* tv = tabVals + offT[c];
  const uint32_t tmask = (uint32_t)cntT[c] - 1u;
  for (uint32_t i = 0; i <= tmask; i++) { tk[i] = ~0ull; tv[i] = 0; }
  const WinExt X = ext[c];
  const int64_t ce = contigOff[cand.seqId + 1];
  auto wposOf = [&](int64_t e) { return (int)(evKey[e] >> 1); };
  auto wendOf = [&](int64_t e) { return (int)(evAux[e] & 0x7fffffffu); };
  auto freqOf = [&](uint64_t h) -> int32_t* {                                    // hash_to_freq[h] (created at 0 on first access, like operator[])
    uint32_t i = (uint32_t)(h * 0x9E3779B97F4A7C15ull >> 40) & tmask;
    while (tk[i] != h) { if (tk[i] == ~0ull) { tk[i] = h; break; } i = (i + 1) & tmask; }
    return &tv[i];
  };
  auto locate = [&](uint64_t h, bool& match) -> int {                            // 1-based lower_bound in the sketch; 0: beyond its last hash
    int lo = 0, hi = S;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (q[mid] < h) lo = mid + 1; else hi = mid; }
    if (lo >= S) { match = false; return 0; }
    match = q[lo] == h; return lo + 1;
  };
  auto insertMinmer = [&](int64_t e) {                                           // slidingMap.hpp:125-165
    bool match; const int j = locate(evHash[e], match);
    if (j == 0) return;
    ExactCell x = cell[j];
    if (match) {
      x.active = 1; x.vote = (int16_t)(x.vote + (int)qs[j - 1] * ((evAux[e] >> 31) ? -1 : 1));
      cell[j] = x;
      if (j <= pivot) { shared++; votes += x.vote; }
    } else {
      x.cnt++; cell[j] = x;
      if (j <= pivot) pivRank++;
      if (pivRank > S) { const ExactCell pc = cell[pivot]; shared -= pc.active; votes -= pc.vote; pivRank -= pc.cnt; pivot--; }
    }
  };
  auto deleteMinmer = [&](int64_t e) {                                           // slidingMap.hpp:171-211
    bool match; const int j = locate(evHash[e], match);
    if (j == 0) return;
    ExactCell x = cell[j];
    if (match) {
      if (j <= pivot) { shared--; votes -= x.vote; }
      x.active = 0; x.vote = 0; cell[j] = x;
    } else {
      x.cnt--; cell[j] = x;
      if (j <= pivot) pivRank--;
      if (pivot + 1 <= S && pivRank + cell[pivot + 1].cnt <= S) { pivot++; const ExactCell pc = cell[pivot]; shared += pc.active; votes += pc.vote; pivRank += pc.cnt; }
    }
  };
  auto later = [&](int32_t a, int32_t b) { return wendOf(X.e0 + a) > wendOf(X.e0 + b); };   // heap_cmp (:1299): min-heap on wpos_end
  auto nextIns = [&](int64_t e) { while (e < ce && !(evKey[e] & 1u)) e++; return e; };       // minmerIndex records = insert events
  // wpos of the record behind `e` in the same contig, else its own (:1387-1390)
  auto nextWpos = [&](int64_t e) { const int64_t n = nextIns(e + 1); return n < ce ? wposOf(n) : wposOf(e); };

  int bestShared = 1; bool inRun = false;
  int curStart = 0, curEnd = 0, curShared = 0;
  int nFlushed = 0; bool havePend = false; L2Tmp pend{0, 0, 0, 0};
  L2Tmp* mySlots = tmp + (size_t)c * locap;
  bool slotOverflow = false;
  auto close_run = [&](int strand) {                                             // :1417-1426 / :1440-1449
    if (!havePend || pend.end + segLength < curStart) {
      if (havePend) { if (nFlushed < locap) mySlots[nFlushed] = pend; else slotOverflow = true; nFlushed++; }
      pend.start = curStart; pend.end = curEnd; pend.shared = curShared; pend.strand = strand; havePend = true;
    } else pend.end = curEnd;
  };

  int64_t it = nextIns(X.e0);
  while (it < ce && wposOf(it) < cand.rangeStartPos) {                           // set up the window (:1323-1338)
    if (wendOf(it) > cand.rangeStartPos) {
      int32_t* fq = freqOf(evHash[it]);
      if (W > 0) (*fq)++;
      if (W == 0 || *fq == 1) {
        heap[nHeap] = (int32_t)(it - X.e0); nHeap++;
        mm_heap_push(heap, nHeap - 1, 0, heap[nHeap - 1], later);
        insertMinmer(it);
      }
    }
    it = nextIns(it + 1);
  }
  while (it < ce && (long long)wposOf(it) <= (long long)cand.rangeEndPos + W) {  // the slide (:1340-1434)
    const int prevVotes = votes;
    while (nHeap > 0 && wendOf(X.e0 + heap[0]) <= wposOf(it) - W) {
      const int64_t fr = X.e0 + heap[0];
      int32_t* fq = freqOf(evHash[fr]);
      if (W > 0) (*fq)--;
      if (W == 0 || *fq == 0) {
        deleteMinmer(fr);
        mm_pop_heap(heap, nHeap, later); nHeap--;
      }
    }
    int32_t* fq = freqOf(evHash[it]);
    if (W > 0) (*fq)++;
    if (W == 0 || *fq == 1) {
      insertMinmer(it);
      heap[nHeap] = (int32_t)(it - X.e0); nHeap++;
      mm_heap_push(heap, nHeap - 1, 0, heap[nHeap - 1], later);
    } else { it = nextIns(it + 1); continue; }
    if (shared > bestShared) {
      nFlushed = 0; havePend = false;
      inRun = true; bestShared = shared; curShared = shared;
      curStart = wposOf(it);                                                     // (no "- windowLen" here in the reference, :1384)
      curEnd = nextWpos(it) - W;
    } else if (shared == bestShared) {
      if (!inRun) { curShared = shared; curStart = wposOf(it) - W; }
      inRun = true;
      curEnd = nextWpos(it) - W;
    } else {
      if (inRun) { curEnd = nextWpos(it) - W; close_run(prevVotes >= 0 ? 1 : -1); curStart = curEnd = curShared = 0; }
      inRun = false;
    }
    it = nextIns(it + 1);
  }
  if (inRun) close_run(votes >= 0 ? 1 : -1);
  int total = nFlushed + (havePend ? 1 : 0);
  if (slotOverflow) { atomicOr(&counters[MM_PC_L2_FLAGS], MM_L2F_SLOTS); total = 0; }
  mm_l2_emit_thread(c, cand, total, nFlushed, mySlots, pend, l1Off, l2, l2Cap, l2First, l2Num, counters);
}

// ---------------------------------------------------------------------------------------------
// k_l2_window_wave (MM_OPT_L2_WINDOW_WAVE): the windowLen != 0 L2 stage with one WAVE per candidate.  k_l2_window above gives a candidate to
// one thread, whose every step -- a binary search of the sketch in HBM, a probe of its count table, the heap, the cells, all in per-candidate
// HBM scratch -- waits for the one before it, 64 unrelated chains per wave.  Here the candidate's state is in LDS -- its query sketch, its
// SlideMapper cells, its heap of open records (each carries its located form, so an eviction searches nothing) -- and the wave takes 64
// consecutive events of the candidate's slice [e0, e1) per step:
//   - coalesced loads of evKey / evAux / evHash (the next step's are in flight meanwhile);
//   - per lane with an index record (an insert event: about half of a step's events, the others are evictions, which the heap replaces here): the binary search of the sketch in LDS, the wpos of the record behind it, the wpos
//     of the slide record before it, and the probe of the presence table (mm_l2_window_core.h: "absent" or "present with record R" per
//     hash; the candidate's slice of dWinKeys / dWinVals in HBM, 64 probes at a time);
//   - then the records the table lets in go through mm_win_enter one by one, in index order, the whole wave running the one sequential
//     step on LDS: the evictions due, the insert, the push, the evaluation.  A record that enters hands its wpos_end to the later lanes of
//     the step that carry the same hash, which look at the rule again when their turn comes: same-hash records of one step are resolved
//     in record order;
//   - the entries of the records that entered go to the table, one lane each (compare-and-swap on the key: two hashes may want one slot).
// windowLen == 0 fragments of a windowed batch take the same steps with the gate off.  Loci, l2First / l2Num and the cursor as k_l2_window
// writes them.  A candidate this state cannot hold is appended to handList (its length in MM_PC_L2_WIDE_LEN, which the split sweeps use for
// their list and a windowed batch does not) and swept by k_l2_window behind this kernel; each is checked before the write it guards:
//   - a heap that would outgrow MM_WW_HEAP open records;
//   - more tied loci at the best count than MM_LOCAP0 slots and the pending one (WinRuns::overflow);
//   - a fragment sketch larger than the launch's LDS layout (cannot happen: Q.sketchSize <= sketchSize).
// LDS per wave: MM_WW_HEAP x 8 B + 17 B per sketch entry -- 18.7 KB at s = 130: 8 waves per CU (two per SIMD), against the 2 560 per-lane
// chains the literal kernel keeps per CU; the heap's share is what a read of 30 kbp at segLength 5000 needs (about 0.05 records per base
// over windowLen + segLength stay open: 1 300 - 1 600).
// ---------------------------------------------------------------------------------------------
#define MM_WW_HEAP 2048            // open records the LDS heap holds
#define MM_WW_MAX_SKETCH 2046      // sketchSize up to which the option applies (51 KB of LDS per wave there)
__host__ __device__ static inline size_t mm_ww_lds(int s) {
  return (size_t)MM_WW_HEAP * 8 + (size_t)(s + 1) * 8 + (size_t)(s + 2) * sizeof(WinCell) + (size_t)MM_LOCAP0 * sizeof(WinLocus) + (((size_t)s + 15) & ~(size_t)15);
}
// The end of candidate c for a kernel that gives it one WAVE: the loci rn holds are claimed from the pass's cursor by lane 0 and written
// 64 at a time, l2First / l2Num say where k_l2_select finds them.  Where they do not fit the buffer, MM_PC_L2_OVERFLOW is raised and
// nothing is written.
__device__ __forceinline__ void mm_l2_emit_wave(int c, const mm_l1_candidate& cand, const WinRuns& rn, const int64_t* __restrict__ l1Off, mm_l2_locus* __restrict__ l2,
                                                unsigned long long l2Cap, int64_t* __restrict__ l2First, int32_t* __restrict__ l2Num,
                                                unsigned long long* __restrict__ counters, int lane) {
  const int total = rn.total();
  unsigned long long at = 0;
  if (total > 0) {
    if (lane == 0) at = atomicAdd(&counters[MM_PC_L2_LOCI], (unsigned long long)total);
    at = mm_bcast64_readlane(at, 0);
    if (at + (unsigned long long)total > l2Cap) { if (lane == 0) atomicOr(&counters[MM_PC_L2_OVERFLOW], MM_OVERFLOWED); return; }
  }
  if (lane == 0) { l2First[c] = (int64_t)at; l2Num[c] = total; }
  const int candLocal = (int)(c - l1Off[cand.frag]);
  for (int k = lane; k < total; k += 64) {
    const WinLocus t = rn.locus(k);
    l2[at + k] = mm_l2_record(cand.frag, candLocal, cand.seqId, t.start, t.end, t.shared, t.strand);
  }
}
__global__ void __launch_bounds__(64)
k_l2_window_wave(int nCand, int s, int segLength, const mm_l1_candidate* __restrict__ l1, const mm_frag_stats* __restrict__ stats, const DFrag* __restrict__ frags,
                 const uint64_t* __restrict__ qHash, const int8_t* __restrict__ qStrand, const uint64_t* __restrict__ skHash, const int8_t* __restrict__ skStrand,
                 const uint32_t* __restrict__ evKey, const uint32_t* __restrict__ evAux, const uint64_t* __restrict__ evHash, const int64_t* __restrict__ contigOff,
                 const WinExt* __restrict__ ext, const int64_t* __restrict__ offT, const int32_t* __restrict__ cntT, uint64_t* __restrict__ tabKeys, int32_t* __restrict__ tabVals,
                 const int64_t* __restrict__ l1Off, mm_l2_locus* __restrict__ l2, unsigned long long l2Cap, int64_t* __restrict__ l2First, int32_t* __restrict__ l2Num,
                 unsigned long long* __restrict__ counters, int32_t* __restrict__ handList) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wsm[];
  uint64_t* heap = (uint64_t*)wsm;
  uint64_t* q = heap + MM_WW_HEAP;                                 // the query sketch, ascending
  WinCell* cells = (WinCell*)(q + (s + 1));                        // cells 0 .. S
  WinLocus* slots = (WinLocus*)(cells + (s + 2));
  int8_t* qs = (int8_t*)(slots + MM_LOCAP0);
  const int lane = (int)threadIdx.x;
  for (int c = blockIdx.x; c < nCand; c += gridDim.x) {
    const mm_l1_candidate cand = l1[c];
    const int f = cand.frag;
    const mm_frag_stats fst = stats[f];
    const int S = fst.sketchSize;
    int W = frags[f].len - segLength; if (W < 0) W = 0;
    const WinExt X = ext[c];
    const int64_t ce = contigOff[cand.seqId + 1];
    uint64_t* tk = tabKeys + offT[c]; int32_t* tv = tabVals + offT[c];
    const uint32_t tmask = (uint32_t)cntT[c] - 1u;
    bool hand = S > s;
    __threadfence_block();                                         // the previous candidate's LDS reads are done
    if (!hand) {
      const bool raw = fst.rawSketchSize == fst.sketchSize;        // no seed was removed: the sketch is the raw one (k_lookup_l1)
      const uint64_t* srcH = (raw ? skHash : qHash) + (size_t)f * s;
      const int8_t* srcS = (raw ? skStrand : qStrand) + (size_t)f * s;
      for (int p = lane; p < S; p += 64) { q[p] = srcH[p]; qs[p] = srcS[p]; }
      for (int p = lane; p <= S; p += 64) cells[p] = WinCell{p ? 1 : 0, 0, 0};             // SlideMapper::init (slidingMap.hpp:103-121)
      if (W > 0) for (uint32_t i = (uint32_t)lane; i <= tmask; i += 64u) tk[i] = ~0ull;    // no hash has an entry
      __threadfence();                                             // ... before the first probe and the first compare-and-swap
    }
    WinSlide sm; sm.start(cells, S);
    WinRuns rn; rn.start(segLength, W, slots, MM_LOCAP0);
    int nHeap = 0, lastSlideW = MM_WIN_NONE;
    auto load = [&](int64_t e, uint32_t& key, uint32_t& aux, uint64_t& h) { key = 0; aux = 0; h = 0; if (e < ce) { key = evKey[e]; aux = evAux[e]; h = evHash[e]; } };
    uint32_t nKey, nAux; uint64_t nH;
    load(X.e0 + lane, nKey, nAux, nH);
    for (int64_t base = X.e0; base < X.e1 && !hand; base += 64) {
      const uint32_t key = nKey, aux = nAux; const uint64_t h = nH;
      load(base + 64 + lane, nKey, nAux, nH);                      // in flight during this step; to the contig's end, not e1: the record behind the last one
      const bool isIns = (key & 1u) != 0;                          // minmerIndex records = insert events
      const int pos = (int)(key >> 1), wend = (int)(aux & 0x7fffffffu);
      const bool walked = base + lane < X.e1 && isIns;
      const bool setup = pos < cand.rangeStartPos;                 // the set-up loop (:1323-1338) takes the records still open at rangeStart
      const bool cons = walked && (!setup || wend > cand.rangeStartPos);
      // wpos of the record behind this one in the same contig, else its own (:1387-1390)
      const uint64_t above = mm_ballot(isIns) & ~((2ull << lane) - 1ull);
      int nextW = __shfl(pos, above ? (int)__builtin_ctzll(above) : lane);
      if (mm_ballot(cons && !above)) {                             // the last record of the step: the first one behind it
        uint64_t m = mm_ballot((nKey & 1u) != 0);
        int tailW = m ? mm_rl((int)(nKey >> 1), (int)__builtin_ctzll(m)) : 0;
        for (int64_t e2 = base + 128; !m && e2 < ce; e2 += 64) {   // (rare: 64 evictions in a row)
          const uint32_t k2 = e2 + lane < ce ? evKey[e2 + lane] : 0u;
          m = mm_ballot((k2 & 1u) != 0);
          if (m) tailW = mm_rl((int)(k2 >> 1), (int)__builtin_ctzll(m));
        }
        if (!above && m) nextW = tailW;
      }
      // wpos of the slide record before this one, entering or not: its evictions come before this record's votes are sampled
      const uint64_t mSl = mm_ballot(walked && !setup);
      int prevSlideW = lastSlideW;
      {
        const uint64_t below = mSl & ((1ull << lane) - 1ull);
        const int p2 = __shfl(pos, below ? 63 - (int)__builtin_clzll(below) : lane);
        if (below) prevSlideW = p2;
      }
      uint32_t loc = 0, slot = 0; bool exists = false; int entryEnd = 0;
      if (cons) {
        loc = mm_win_locate(q, qs, S, h, (aux >> 31) != 0);
        if (W > 0) {                                               // the presence table: h -> wpos_end of the record that is in
          slot = (uint32_t)(h * 0x9E3779B97F4A7C15ull >> 40) & tmask;
          uint64_t k2;
          while ((k2 = __hip_atomic_load(&tk[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != h && k2 != ~0ull) slot = (slot + 1u) & tmask;
          if (k2 == h) { exists = true; entryEnd = __hip_atomic_load(&tv[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        }
      }
      // records the table lets in, in index order; the others are final: an earlier record of this step cannot make a hash absent
      uint64_t todo = mm_ballot(cons && !(W > 0 && mm_win_present(exists, entryEnd, setup, pos, W)));
      bool writer = false;
      while (todo) {
        const int l = (int)__builtin_ctzll(todo); todo &= todo - 1ull;
        const bool setupL = mm_rl(setup ? 1 : 0, l) != 0;
        const int posL = mm_rl(pos, l), wendL = mm_rl(wend, l);
        if (W > 0 && mm_win_present(mm_rl(exists ? 1 : 0, l) != 0, mm_rl(entryEnd, l), setupL, posL, W)) continue;   // a record of this step entered with its hash
        if (!mm_win_enter(sm, heap, nHeap, MM_WW_HEAP, rn, setupL, posL, wendL, (uint32_t)mm_rl((int)loc, l), mm_rl(nextW, l), mm_rl(prevSlideW, l))) { hand = true; break; }
        if (W > 0) {
          const uint64_t hL = mm_bcast64_readlane(h, l);
          if (cons && h == hL) { writer = lane == l; if (lane > l) { exists = true; entryEnd = wendL; } }
        }
      }
      if (writer) {                                                // the last record of its hash that entered in this step
        uint32_t i = slot;
        while (true) {
          const unsigned long long old = atomicCAS((unsigned long long*)&tk[i], ~0ull, (unsigned long long)h);
          if (old == ~0ull || old == (unsigned long long)h) break;
          i = (i + 1u) & tmask;
        }
        __hip_atomic_store(&tv[i], wend, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (W > 0) __threadfence();                                  // the entries are there before the next step's probes
      if (mSl) lastSlideW = mm_rl(pos, 63 - (int)__builtin_clzll(mSl));
    }
    if (!hand) { mm_win_finish(sm, heap, nHeap, rn, lastSlideW); hand = rn.overflow; }
    if (hand) { if (lane == 0) handList[atomicAdd(&counters[MM_PC_L2_WIDE_LEN], 1ull)] = c; continue; }
    mm_l2_emit_wave(c, cand, rn, l1Off, l2, l2Cap, l2First, l2Num, counters, lane);
  }
}

// ---------------------------------------------------------------------------------------------
// k_l2_large_wave (MM_OPT_L2_LARGE_WAVE): the L2 stage of a SPLIT batch (windowLen == 0 for every fragment) on the literal route -- a
// sketch beyond MM_LDS_MAX_SKETCH, which neither k_l2_locate's LDS tables nor the located stream's 13-bit position field hold -- with one
// WAVE per candidate.  The candidate's slice of the index is k_l2_extents' (L2Info): the block's open records, the events before rangeStart,
// the slide.  The wave takes 64 consecutive events of one of the three ranges per step, as k_l2_locate's chunk loop does (the next chunk's
// three loads in flight):
//   - per lane: k_l2_locate's keep rule, and the hash located in the fragment's query sketch with mm_win_locate.  The sketch is read
//     where it lies in HBM -- 160 KB of hashes at s = 20 000 would leave no LDS for the cells --: 64 searches at a time against one array
//     that stays cache-resident, instead of one chain per candidate;
//   - then, in event order, the whole wave applies the located events to WinSlide (mm_l2_window_core.h: 32-bit counts, boolean `active`,
//     accumulated vote, the literal insert_minmer / delete_minmer) in LDS.  Evictions come from the stream -- at windowLen == 0 its order is
//     the heap's order, which k_l2_sweep and k_l2_sweep_exact rely on as well -- and a lane whose hash lies beyond the sketch is skipped by
//     the ballot mask, unless it is an insert: its position is still evaluated.
// The pre-load is applied the same way, serially (its inserts commute, so LDS atomics and a wave scan would do; not done here).  The
// evaluation is k_l2_sweep_exact's, stated by WinRuns with W = 0: an insert is evaluated when the next insert's wpos is known, the strand of
// a closing run comes from the votes as they stood after the previous insert, the last insert uses k_l2_locate's nextW.  Every loop is
// bounded by the slice's length (the two tail scans by the contig's); no wave waits for another.  Loci, l2First / l2Num and the cursor as
// k_l2_window_wave writes them.  Handed over to k_l2_window through handList (length in MM_PC_L2_LARGE_LEN), each checked before the write
// it guards: more tied loci at the best count than MM_LOCAP0 slots and the pending one (WinRuns::overflow); a fragment sketch larger than
// the launch's LDS layout (cannot happen: Q.sketchSize <= sketchSize).
// LDS per wave: (s + 2) cells of 8 B and MM_LOCAP0 loci -- 160 112 B of a CU's 163 840 at s = 19 998: one wave per CU there.
// ---------------------------------------------------------------------------------------------
#define MM_LW_MAX_SKETCH 20460     // the largest sketchSize whose cells and locus slots fit a CU's 160 KB of LDS
__host__ __device__ static inline size_t mm_lw_lds(int s) { return (size_t)(s + 2) * sizeof(WinCell) + (size_t)MM_LOCAP0 * sizeof(WinLocus); }
static_assert((size_t)(MM_LW_MAX_SKETCH + 2) * sizeof(WinCell) + (size_t)MM_LOCAP0 * sizeof(WinLocus) <= 160 * 1024, "k_l2_large_wave's state in one CU's LDS");
__global__ void __launch_bounds__(64)
k_l2_large_wave(int nCand, int s, int segLength, const mm_l1_candidate* __restrict__ l1, const L2Info* __restrict__ info,
                const uint64_t* __restrict__ qHash, const int8_t* __restrict__ qStrand, const uint64_t* __restrict__ skHash, const int8_t* __restrict__ skStrand,
                const uint32_t* __restrict__ evKey, const uint32_t* __restrict__ evAux, const uint64_t* __restrict__ evHash,
                const uint32_t* __restrict__ opKey, const uint32_t* __restrict__ opAux, const uint64_t* __restrict__ opHash, const int64_t* __restrict__ contigOff,
                const int64_t* __restrict__ l1Off, mm_l2_locus* __restrict__ l2, unsigned long long l2Cap, int64_t* __restrict__ l2First, int32_t* __restrict__ l2Num,
                unsigned long long* __restrict__ counters, int32_t* __restrict__ handList) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lwsm[];
  WinCell* cells = (WinCell*)lwsm;                                 // cells 0 .. S (+ one unused)
  WinLocus* slots = (WinLocus*)(cells + (s + 2));
  const int lane = (int)threadIdx.x;
  for (int c = blockIdx.x; c < nCand; c += gridDim.x) {
    const mm_l1_candidate cand = l1[c];
    const int f = cand.frag;
    const L2Info in = info[c];
    const int S = in.sketch & 0x7fffffff;
    const int nOpen = in.nOpen, nPre = in.nPre, nAll = in.nAll;
    const int64_t ce = contigOff[cand.seqId + 1];
    bool hand = S > s;
    __threadfence_block();                                         // the previous candidate's LDS reads are done
    if (!hand) for (int p = lane; p <= S; p += 64) cells[p] = WinCell{p ? 1 : 0, 0, 0};      // SlideMapper::init (slidingMap.hpp:103-121)
    __threadfence_block();
    // a fragment that lost no frequent seed has no copy in qHash/qStrand: its sketch is the raw one (k_lookup_l1)
    const bool raw = in.sketch < 0;
    const uint64_t* q = (raw ? skHash : qHash) + (size_t)f * s;
    const int8_t* qs = (raw ? skStrand : qStrand) + (size_t)f * s;
    const uint64_t qmax = S > 0 && !hand ? q[S - 1] : 0ull;
    // the slide ends with the last insert at or before rangeEnd; nextW: the wpos of the record behind it in the same contig, else its own
    // (k_l2_locate's rule, a slice that ends in 64 evictions included)
    int lastRel = -1, nextW = 0;
    if (!hand) {
      const int iT = nAll - 64 + lane;
      const uint32_t tailKey = (iT >= nPre && iT < nAll) ? evKey[in.e0 + iT] : 0u;
      const uint32_t behindKey = in.e0 + nAll + lane < ce ? evKey[in.e0 + nAll + lane] : 0u;
      const uint64_t m = mm_ballot((tailKey & 1u) != 0);
      if (m) { const int l = 63 - (int)__builtin_clzll(m); lastRel = nAll - 64 + l; nextW = (int)((uint32_t)mm_rl((int)tailKey, l) >> 1); }
      for (int hiEnd = nAll - 64; hiEnd > nPre && lastRel < 0; hiEnd -= 64) {
        const int i = hiEnd - 64 + lane;
        const uint32_t k2 = (i >= nPre && i < hiEnd) ? evKey[in.e0 + i] : 0u;
        const uint64_t m2 = mm_ballot((k2 & 1u) != 0);
        if (m2) { const int l = 63 - (int)__builtin_clzll(m2); lastRel = hiEnd - 64 + l; nextW = (int)((uint32_t)mm_rl((int)k2, l) >> 1); }
      }
      if (lastRel >= 0) {
        const uint64_t m0 = mm_ballot((behindKey & 1u) != 0);
        if (m0) nextW = (int)((uint32_t)mm_rl((int)behindKey, (int)__builtin_ctzll(m0)) >> 1);
        else for (int64_t e = in.e0 + nAll + 64; e < ce; e += 64) {
          const uint32_t k2 = e + lane < ce ? evKey[e + lane] : 0u;
          const uint64_t m2 = mm_ballot((k2 & 1u) != 0);
          if (m2) { nextW = (int)((uint32_t)mm_rl((int)k2, (int)__builtin_ctzll(m2)) >> 1); break; }
        }
      }
    }
    const int nEv = lastRel + 1;                                   // events [0, nEv) of the slice are walked
    const int nChO = (nOpen + 63) >> 6, nChPre = nChO + ((nPre + 63) >> 6);
    const int nCh = hand ? 0 : nChPre + ((nEv > nPre ? nEv - nPre : 0) + 63) / 64;
    auto loadChunk = [&](int ch, uint32_t& key, uint32_t& aux, uint64_t& h) {
      key = 0; aux = 0; h = 0;                                       // a lane without a record: no insert flag, nothing kept
      if (ch < nChO) { const int i = ch * 64 + lane; if (i < nOpen) { key = opKey[in.open0 + i]; aux = opAux[in.open0 + i]; h = opHash[in.open0 + i]; } }
      else {
        const int i = ch < nChPre ? (ch - nChO) * 64 + lane : nPre + (ch - nChPre) * 64 + lane;
        if (i < (ch < nChPre ? nPre : nEv)) { key = evKey[in.e0 + i]; aux = evAux[in.e0 + i]; h = evHash[in.e0 + i]; }
      }
    };
    WinSlide sm; sm.start(cells, S);
    WinRuns rn; rn.start(segLength, 0, slots, MM_LOCAP0);
    bool evalPending = false; int evW = 0, evShared = 0, evPrevVotes = 0, lastVotes = 0;
    uint32_t nKey = 0, nAux = 0; uint64_t nHash = 0;
    if (nCh > 0) loadChunk(0, nKey, nAux, nHash);
    for (int ch = 0; ch < nCh; ch++) {
      const uint32_t key = nKey, aux = nAux; const uint64_t h = nHash;
      if (ch + 1 < nCh) loadChunk(ch + 1, nKey, nAux, nHash);       // in flight while this chunk is located and applied
      const bool isIns = (key & 1u) != 0;
      const int pos = (int)(key >> 1);
      const bool slide = ch >= nChPre;                               // wave-uniform
      bool keep, evalIns = false;
      if (!slide) keep = isIns && (int)(aux & 0x7fffffffu) > cand.rangeStartPos && pos >= in.target;   // still open at rangeStart (:1323-1338)
      else {
        const bool live = nPre + (ch - nChPre) * 64 + lane < nEv;
        keep = live && (isIns || h <= qmax);                         // an eviction outside the sketch's range changes nothing
        evalIns = live && isIns;
      }
      const uint32_t loc = keep ? mm_win_locate(q, qs, S, h, (aux >> 31) != 0) : 0u;
      uint64_t todo = mm_ballot(evalIns || (keep && mm_win_loc_j(loc) != 0));
      while (todo) {
        const int l = (int)__builtin_ctzll(todo); todo &= todo - 1ull;
        const uint32_t locL = (uint32_t)mm_rl((int)loc, l);
        if (!slide) sm.insert(locL);
        else if (mm_rl(isIns ? 1 : 0, l) != 0) {
          const int posL = mm_rl(pos, l);
          if (evalPending) rn.evaluate(evShared, evW, posL, evPrevVotes);       // the insert before this one: its nextW is this wpos
          evPrevVotes = lastVotes;
          sm.insert(locL);
          lastVotes = sm.votes; evW = posL; evShared = sm.shared; evalPending = true;
        } else sm.remove(locL);
      }
      if (!slide) lastVotes = sm.votes;                              // (votes right after the last pre-load insert)
    }
    if (!hand) {
      if (evalPending) rn.evaluate(evShared, evW, nextW, evPrevVotes);
      if (rn.inRun) rn.close_run(sm.votes >= 0 ? 1 : -1);
      hand = rn.overflow;
    }
    if (hand) { if (lane == 0) handList[atomicAdd(&counters[MM_PC_L2_LARGE_LEN], 1ull)] = c; continue; }
    mm_l2_emit_wave(c, cand, rn, l1Off, l2, l2Cap, l2First, l2Num, counters, lane);
  }
}

// the end of a sized L2 stage: the counters as last read back (MM_PC_*) become the number of loci, or the reason there is none
// (MM_L2F_STREAM is raised by k_l2_locate alone: the literal launcher never sees it)
static int mm_l2_verdict(mm_ctx* c, const unsigned long long* hc) {
  if (hc[MM_PC_L2_FLAGS] & MM_L2F_STREAM) { c->err = "internal: an L2 stream outgrew the reservation k_l2_extents made for it"; return MM_ERR_CAPACITY; }
  if (hc[MM_PC_L2_FLAGS] & MM_L2F_SLOTS) { c->err = "an L1 candidate with more tied L2 loci than 64 GiB of staging can hold"; return MM_ERR_CAPACITY; }
  if (hc[MM_PC_L2_OVERFLOW]) { c->err = "L2 locus buffer overflow"; return MM_ERR_CAPACITY; }
  c->rep.nL2 = (size_t)hc[MM_PC_L2_LOCI];
  return MM_OK;
}

// What a sized L2 stage does about the counters it has just read back.  MoreSlots: a candidate tied in more loci than it has staging slots
// (tandem repeats), locap is doubled -- unless twice the slots would need more than 64 GiB (GiveUp: mm_l2_verdict names the reason).
// MoreLoci: the locus buffer is full, l2Cap follows the demand the cursor ran up to.  Slots come first, except (lociFirst) on the literal
// route behind a wave kernel: a moved locus buffer has both kernels run again there, more slots the literal kernel alone.
enum class L2Retry { Done, MoreSlots, MoreLoci, GiveUp };
static L2Retry l2_after_readback(mm_ctx* c, const unsigned long long* hc, int nC, int& locap, bool lociFirst) {
  const bool slots = (hc[MM_PC_L2_FLAGS] & MM_L2F_SLOTS) != 0, over = hc[MM_PC_L2_OVERFLOW] != 0;
  if (slots && !(lociFirst && over)) {
    if ((size_t)nC * (size_t)locap * 2 * sizeof(L2Tmp) > ((size_t)64 << 30)) return L2Retry::GiveUp;
    locap *= 2;
    return L2Retry::MoreSlots;
  }
  if (!over) return L2Retry::Done;
  c->l2Cap = mm_loci_cap_grown(mm_scaled(c, (size_t)hc[MM_PC_L2_LOCI], sizeof(mm_l2_locus)));
  return L2Retry::MoreLoci;
}

// k_l2_extents over nC candidates (nDev: their number on the device, steady-state pass); the caller holds the timer
static void l2_launch_extents(mm_ctx* c, unsigned long long* cnt, int nC, int deltaBits, const unsigned long long* nDev) {
  const DeviceIndex& I = c->idx;
  hipLaunchKernelGGL(k_l2_extents, dim3((nC + 255) / 256), dim3(256), 0, c->stream, nC, c->P.segLength, deltaBits, c->dL1.as<mm_l1_candidate>(), c->dStats.as<mm_frag_stats>(),
                     I.evKey.as<uint32_t>(), I.contigBlock.as<int64_t>(), I.blockOff.as<int64_t>(), I.evBlock.as<int64_t>(),
                     c->dL2Info.as<L2Info>(), c->dL2Cnt.as<int32_t>(), nDev, cnt);
}

// ---- the literal route: mm_launch_l2_window and its stages ----------------------------------------------------------------------------------
// stage 1: the per-candidate buffers, every candidate's window of the event stream (k_l2_window_extents), the scans of the two counts it
// leaves and the scratch they size
static int l2w_extents(mm_ctx* c, int nC) {
  const DeviceIndex& I = c->idx;
  MM_HIP(c, c->dWinExt.ensure((size_t)nC * sizeof(WinExt) + 64));
  MM_HIP(c, c->dWinCntH.ensure((size_t)nC * 4 + 64)); MM_HIP(c, c->dWinCntT.ensure((size_t)nC * 4 + 64));
  MM_HIP(c, c->dWinOffH.ensure((size_t)nC * 8 + 64)); MM_HIP(c, c->dWinOffT.ensure((size_t)nC * 8 + 64));
  MM_HIP(c, c->dL2First.ensure((size_t)nC * 8 + 64)); MM_HIP(c, c->dL2Num.ensure((size_t)nC * 4 + 64));
  int64_t totH = 0, totT = 0;
  {
    KernelTimer t(c, MM_K_L2_LOCATE);
    hipLaunchKernelGGL(k_l2_window_extents, dim3((nC + 255) / 256), dim3(256), 0, c->stream, nC, c->P.segLength, c->dL1.as<mm_l1_candidate>(), c->dFrags.as<DFrag>(),
                       I.evKey.as<uint32_t>(), I.contigOff.as<int64_t>(), c->dWinExt.as<WinExt>(), c->dWinCntH.as<int32_t>(), c->dWinCntT.as<int32_t>());
    MM_HIP(c, hipGetLastError());
    int rc = mm_scan_i32_to_i64(c, nC, c->dWinCntH.as<int32_t>(), c->dWinOffH.as<int64_t>(), &totH); if (rc != MM_OK) return rc;
    rc = mm_scan_i32_to_i64(c, nC, c->dWinCntT.as<int32_t>(), c->dWinOffT.as<int64_t>(), &totT); if (rc != MM_OK) return rc;
  }
  if ((size_t)totT * 12 + (size_t)totH * 4 > ((size_t)96 << 30)) { c->err = "windowLen != 0: the candidates of this batch need more than 96 GiB of scratch; use smaller batches (MASHMAP_HIP_BATCH_MBP)"; return MM_ERR_CAPACITY; }
  MM_HIP(c, c->dWinHeap.ensure((size_t)totH * 4 + 64)); MM_HIP(c, c->dWinKeys.ensure((size_t)totT * 8 + 64)); MM_HIP(c, c->dWinVals.ensure((size_t)totT * 4 + 64));
  MM_HIP(c, c->dL2Cells.ensure((size_t)nC * (size_t)(c->P.sketchSize + 1) * sizeof(ExactCell) + 64));
  c->l2Cap = std::max(c->l2Cap, mm_loci_cap0(c->rep.nL1));
  return MM_OK;
}

static void l2w_launch_large_wave(mm_ctx* c, unsigned long long* cnt, int nC, int blocks) {
  const DeviceIndex& I = c->idx;
  const int s = c->P.sketchSize; const size_t lds = mm_lw_lds(s);
  (void)hipFuncSetAttribute((const void*)k_l2_large_wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k_l2_large_wave, dim3((unsigned)blocks), dim3(64), lds, c->stream, nC, s, c->P.segLength, c->dL1.as<mm_l1_candidate>(), c->dL2Info.as<L2Info>(),
                     c->dQHash.as<uint64_t>(), c->dQStrand.as<int8_t>(), c->dSkHash.as<uint64_t>(), c->dSkStrand.as<int8_t>(),
                     I.evKey.as<uint32_t>(), I.evAux.as<uint32_t>(), I.evHash.as<uint64_t>(), I.opKey.as<uint32_t>(), I.opAux.as<uint32_t>(), I.opHash.as<uint64_t>(),
                     I.contigOff.as<int64_t>(), c->dL1Off.as<int64_t>(), c->dL2.as<mm_l2_locus>(), (unsigned long long)c->l2Cap, c->dL2First.as<int64_t>(),
                     c->dL2Num.as<int32_t>(), cnt, c->dL2Wide.as<int32_t>());
}

static void l2w_launch_window_wave(mm_ctx* c, unsigned long long* cnt, int nC, int blocks) {
  const DeviceIndex& I = c->idx;
  const int s = c->P.sketchSize;
  hipLaunchKernelGGL(k_l2_window_wave, dim3((unsigned)blocks), dim3(64), mm_ww_lds(s), c->stream, nC, s, c->P.segLength, c->dL1.as<mm_l1_candidate>(), c->dStats.as<mm_frag_stats>(),
                     c->dFrags.as<DFrag>(), c->dQHash.as<uint64_t>(), c->dQStrand.as<int8_t>(), c->dSkHash.as<uint64_t>(), c->dSkStrand.as<int8_t>(),
                     I.evKey.as<uint32_t>(), I.evAux.as<uint32_t>(), I.evHash.as<uint64_t>(), I.contigOff.as<int64_t>(), c->dWinExt.as<WinExt>(),
                     c->dWinOffT.as<int64_t>(), c->dWinCntT.as<int32_t>(), c->dWinKeys.as<uint64_t>(), c->dWinVals.as<int32_t>(), c->dL1Off.as<int64_t>(),
                     c->dL2.as<mm_l2_locus>(), (unsigned long long)c->l2Cap, c->dL2First.as<int64_t>(), c->dL2Num.as<int32_t>(), cnt, c->dL2Wide.as<int32_t>());
}

// the wave kernel that takes every candidate first and leaves a list (dL2Wide) of those it cannot hold: its list-length word, the kernel,
// and the cursor behind it -- where a repeated literal sweep (more locus slots) starts again (MM_PC_L2_EXACT_LEN: the exact sweep's list
// length on the split route, unused here)
static int l2w_first_kernel(mm_ctx* c, unsigned long long* cnt, int nC, bool large) {
  MM_HIP(c, hipMemsetAsync(cnt + (large ? MM_PC_L2_LARGE_LEN : MM_PC_L2_WIDE_LEN), 0, 8, c->stream));   // (the L1 stage is done with the word)
  KernelTimer t(c, MM_K_L2);
  const int blocks = std::min(nC, 256 * 32);
  if (large) l2w_launch_large_wave(c, cnt, nC, blocks); else l2w_launch_window_wave(c, cnt, nC, blocks);
  MM_HIP(c, hipGetLastError());
  MM_HIP(c, hipMemcpyAsync(cnt + MM_PC_L2_EXACT_LEN, cnt + MM_PC_L2_LOCI, 8, hipMemcpyDeviceToDevice, c->stream));
  return MM_OK;
}

// the literal kernel: every candidate, or (list) the ones the wave kernel handed over
static void l2w_launch_window(mm_ctx* c, unsigned long long* cnt, int nC, int locap, bool list) {
  const DeviceIndex& I = c->idx;
  const int s = c->P.sketchSize;
  hipLaunchKernelGGL(k_l2_window, dim3((nC + 63) / 64), dim3(64), 0, c->stream, nC, s, c->P.segLength, c->dL1.as<mm_l1_candidate>(), c->dStats.as<mm_frag_stats>(),
                     c->dFrags.as<DFrag>(), c->dQHash.as<uint64_t>(), c->dQStrand.as<int8_t>(), c->dSkHash.as<uint64_t>(), c->dSkStrand.as<int8_t>(),
                     I.evKey.as<uint32_t>(), I.evAux.as<uint32_t>(), I.evHash.as<uint64_t>(), I.contigOff.as<int64_t>(), c->dWinExt.as<WinExt>(),
                     c->dWinOffH.as<int64_t>(), c->dWinOffT.as<int64_t>(), c->dWinCntT.as<int32_t>(), c->dWinHeap.as<int32_t>(), c->dWinKeys.as<uint64_t>(),
                     c->dWinVals.as<int32_t>(), c->dL2Cells.as<ExactCell>(), c->dL1Off.as<int64_t>(), c->dL2Tmp.as<L2Tmp>(), locap, c->dL2.as<mm_l2_locus>(),
                     (unsigned long long)c->l2Cap, c->dL2First.as<int64_t>(), c->dL2Num.as<int32_t>(), cnt,
                     list ? c->dL2Wide.as<int32_t>() : (const int32_t*)nullptr, list ? cnt + MM_PC_L2_WIDE_LEN : (const unsigned long long*)nullptr);
}

static int mm_launch_l2_window(mm_ctx* c, unsigned long long* cnt) {
  const int s = c->P.sketchSize;
  const int nC = (int)c->rep.nL1;
  { const int rc = l2w_extents(c, nC); if (rc != MM_OK) return rc; }
  // MM_OPT_L2_WINDOW_WAVE: k_l2_window_wave takes every candidate first and leaves a list of those it cannot hold; k_l2_window then walks
  // that list, whose length stays on the device (the launch covers every candidate), so the stage waits for the host as often as without
  // the option.  A sketch beyond the wave kernel's LDS layout, or a batch without a long fragment (a sketch beyond MM_LDS_MAX_SKETCH comes
  // here as well), is the literal kernel's alone.
  // MM_OPT_L2_LARGE_WAVE, bit 0: a split batch (it is here for its sketch size, or for bit 1 of the option) goes to k_l2_large_wave first, in
  // the same place and with the same hand-over, from the slices k_l2_extents computes; beyond MM_LW_MAX_SKETCH the literal kernel alone.
  const bool winWave = c->opt.l2WindowWave && c->windowed && s <= MM_WW_MAX_SKETCH && nC > 0;
  const bool large = (c->opt.l2LargeWave & 1) && !c->windowed && s <= MM_LW_MAX_SKETCH && nC > 0;
  const bool wave = winWave || large;
  if (wave) MM_HIP(c, c->dL2Wide.ensure((size_t)nC * 4 + 64));
  if (large) {
    MM_HIP(c, c->dL2Info.ensure((size_t)nC * sizeof(L2Info) + 64)); MM_HIP(c, c->dL2Cnt.ensure((size_t)nC * 4 + 64));
    KernelTimer t(c, MM_K_L2_LOCATE);
    l2_launch_extents(c, cnt, nC, EF<13>::DELTA_BITS, nullptr);
    MM_HIP(c, hipGetLastError());
  }
  unsigned long long hc[MM_PC_READ];
  int locap = MM_LOCAP0;
  bool waveDone = false;
  for (int attempt = 0; attempt < 24; attempt++) {
    MM_HIP(c, c->dL2.ensure(c->l2Cap * sizeof(mm_l2_locus) + 64));
    MM_HIP(c, c->dL2Tmp.ensure((size_t)nC * locap * sizeof(L2Tmp) + 64));
    if (!wave || !waveDone) MM_HIP(c, hipMemsetAsync(cnt + MM_PC_L2_LOCI, 0, (size_t)(MM_PC_L2_FLAGS + 1 - MM_PC_L2_LOCI) * 8, c->stream));   // cursor, overflow, flags
    if (wave && !waveDone) {
      const int rc = l2w_first_kernel(c, cnt, nC, large); if (rc != MM_OK) return rc;
      waveDone = true;
    } else if (wave) {                                                     // again with more slots, the literal kernel alone: from the cursor behind the wave kernel
      MM_HIP(c, hipMemcpyAsync(cnt + MM_PC_L2_LOCI, cnt + MM_PC_L2_EXACT_LEN, 8, hipMemcpyDeviceToDevice, c->stream));
      MM_HIP(c, hipMemsetAsync(cnt + MM_PC_L2_OVERFLOW, 0, (size_t)(MM_PC_L2_FLAGS + 1 - MM_PC_L2_OVERFLOW) * 8, c->stream));
    }
    {
      KernelTimer t(c, MM_K_L2);
      l2w_launch_window(c, cnt, nC, locap, wave);
      MM_HIP(c, hipGetLastError());
    }
    MM_HIP(c, hipMemcpyAsync(hc, cnt, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipStreamSynchronize(c->stream));
    const L2Retry r = l2_after_readback(c, hc, nC, locap, /*lociFirst=*/wave);
    if (r == L2Retry::MoreLoci) waveDone = false;                          // the locus buffer moves: the wave kernel runs again as well
    if (r == L2Retry::Done || r == L2Retry::GiveUp) break;
  }
  SizedPass::Seen& seen = c->sized.seen;
  seen.winCands = c->windowed ? (size_t)nC : 0;
  seen.winLit = !c->windowed ? 0 : wave ? (size_t)hc[MM_PC_L2_WIDE_LEN] : (size_t)nC;
  if (c->env.debug && c->windowed) fprintf(stderr, "[mm] L2: of %d windowed candidates the literal L2 kernel took %zu\n", nC, seen.winLit);
  seen.lwCands = c->windowed ? 0 : (size_t)nC;
  seen.lwLit = c->windowed ? 0 : large ? (size_t)hc[MM_PC_L2_LARGE_LEN] : (size_t)nC;
  if (c->env.debug && !c->windowed) fprintf(stderr, "[mm] L2: of %d candidates of a split batch on the literal route k_l2_window took %zu\n", nC, seen.lwLit);
  return mm_l2_verdict(c, hc);
}

// ---------------------------------------------------------------------------------------------
// exclusive scan; the total stays on the device at *dTotal (a word of dScanTmp, valid until the next scan of this context)
int mm_scan_i32_to_i64_dev(mm_ctx* c, int64_t n, const int32_t* dIn, int64_t* dOut, const int64_t** dTotal) {
  const int64_t nTiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  MM_HIP(c, c->dScanTmp.ensure((size_t)(nTiles + 2) * 8));
  int64_t* tileSum = c->dScanTmp.as<int64_t>();
  hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)nTiles), dim3(256), 0, c->stream, n, dIn, dOut, tileSum);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, c->stream, nTiles, tileSum, tileSum + nTiles);
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nTiles), dim3(256), 0, c->stream, n, dOut, tileSum);
  MM_HIP(c, hipGetLastError());
  if (dTotal) *dTotal = tileSum + nTiles;
  return MM_OK;
}
int mm_scan_i32_to_i64(mm_ctx* c, int64_t n, const int32_t* dIn, int64_t* dOut, int64_t* total) {
  const int64_t* dTotal = nullptr;
  const int rc = mm_scan_i32_to_i64_dev(c, n, dIn, dOut, &dTotal);
  if (rc != MM_OK) return rc;
  MM_HIP(c, hipMemcpyAsync(total, dTotal, 8, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipStreamSynchronize(c->stream));
  return MM_OK;
}

#define MM_WIDE_CAP 4096     // steady-state passes: candidates the 16-bit re-run / the exact kernel are launched for without knowing their number
#define MM_EXACT_CAP 1024

// ---- the split route: what the stages of mm_launch_l2 hand on (it calls them in order; each one is a sequence of operations on c->stream)
struct L2Pass {
  bool steady;
  unsigned long long* cnt;                 // dCounters + MM_CW_PASS (MM_PC_*)
  L2Geom geom;                             // LDS geometry of the locate and sweep kernels at this sketch size (mm_l2_plan.h)
  int nC = 0, nCbuf = 0;                   // candidates the launches cover; candidates the candidate-indexed buffers hold (candCap)
  const unsigned long long* nDev = nullptr;   // steady-state pass: the number of candidates, where the kernels read it
  int64_t totalOps = 0;                    // sized pass: stream entries of all candidates
  std::vector<L2Chunk> chunks;             // consecutive candidates whose located streams share dL2Ops
  bool oneChunk = true;                    // ... all of them: located once, the streams stay put over the retries
  int posShift = 0;                        // event number -> the 16 bits of key the reference-order sort of k_l2_locate's candidates takes
  int preLimit = 0;                        // pre-loads of this many records or more go to the exact kernel (MM_L2_PRE_LIMIT)
  int locap = MM_LOCAP0;                   // staging slots per candidate
  unsigned long long hc[MM_PC_READ] = {0}; // the counters as a sized pass last read them back
};

// stage 1: the candidate-indexed buffers, every candidate's slice of the event stream (k_l2_extents) and the scan of the stream lengths --
// read back by a sized pass, left on the device (and checked against dL2Ops by k_l2_gate) by a steady-state one
static int l2_extents(mm_ctx* c, L2Pass& p) {
  // sized pass: the candidates are counted (rep.nL1) and the candidate-indexed buffers get an eighth of head room, which is what a
  // steady-state pass (count on the device: MM_PC_L1_CAND) launches against
  size_t& candCap = c->sized.steady.candCap;
  if (!p.steady) candCap = mm_cand_cap(mm_scaled(c, c->rep.nL1, 96 + 2 * (size_t)((c->P.sketchSize + 3) & ~1)));
  p.nC = p.steady ? (int)candCap : (int)c->rep.nL1;
  p.nCbuf = (int)candCap;
  p.nDev = p.steady ? p.cnt + MM_PC_L1_CAND : nullptr;
  MM_HIP(c, c->dL2Info.ensure((size_t)p.nCbuf * sizeof(L2Info) + 64));
  MM_HIP(c, c->dL2Cnt.ensure((size_t)p.nCbuf * 4 + 64));
  MM_HIP(c, c->dL2Off.ensure((size_t)p.nCbuf * 8 + 64));
  MM_HIP(c, hipMemsetAsync(p.cnt + MM_PC_L2_LOCI, 0, (size_t)(MM_PC_L2_FLAGS + 1 - MM_PC_L2_LOCI) * 8, c->stream));   // cursor, overflow, flags
  KernelTimer t(c, MM_K_L2_LOCATE);
  l2_launch_extents(c, p.cnt, p.nC, p.geom.JB == 13 ? EF<13>::DELTA_BITS : EF<11>::DELTA_BITS, p.nDev);
  MM_HIP(c, hipGetLastError());
  if (p.steady) {
    const int64_t* dTotal = nullptr;
    const int rc = mm_scan_i32_to_i64_dev(c, p.nC, c->dL2Cnt.as<int32_t>(), c->dL2Off.as<int64_t>(), &dTotal); if (rc != MM_OK) return rc;
    MM_HIP(c, hipMemcpyAsync(c->dCounters.as<unsigned long long>() + MM_CW_MAP + MM_MC_L2_OPS, dTotal, 8, hipMemcpyDeviceToDevice, c->stream));   // read back with the pass's counters
    hipLaunchKernelGGL(k_l2_gate, dim3(1), dim3(1), 0, c->stream, dTotal, (int64_t)(c->dL2Ops.bytes / 4) - 64, p.cnt);
    MM_HIP(c, hipGetLastError());
    return MM_OK;
  }
  const int rc = mm_scan_i32_to_i64(c, p.nC, c->dL2Cnt.as<int32_t>(), c->dL2Off.as<int64_t>(), &p.totalOps); c->rep.nSyncs++; if (rc != MM_OK) return rc;
  c->rep.lastOps = (size_t)p.totalOps;
  return MM_OK;
}

// stream entries (4 bytes each) a chunk may hold: 24 GiB, MM_L2_STREAM_MIB where it is set
static int64_t l2_stream_budget(const mm_ctx* c) {
  if (c->env.l2StreamMiB > 0) return (int64_t)(c->env.l2StreamMiB * 262144.0);
  int64_t budget = (int64_t)24 << 28;
  // ... or half of the device memory that is free (counting what the stream buffer already holds), up to 128 GiB: on a 288 GB part the
  // streams of a configs[4] batch (57 GB: 2.7 M candidates at s = 498) then stay in one chunk, and the passes behind this one are
  // steady-state passes instead of being sized, chunk by chunk, every time
  size_t freeB = 0, totalB = 0;
  if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
    const size_t half = (freeB + c->dL2Ops.bytes) / 2;
    budget = std::max<int64_t>(budget, (int64_t)(std::min<size_t>(half, (size_t)128 << 30) / 4));
  }
  return budget;
}

// stage 2: the chunks, and the buffers sized by them.  The located streams (4 bytes per event a candidate touches: ~5 KB per candidate at
// s = 130) live in HBM only between the locate and the sweep kernels; a batch with very many candidates -- reads out of repeat families --
// is taken through the two in chunks, so the buffer does not grow with the repeat content.  A steady-state pass is one chunk: its streams
// must fit the buffer as it is (k_l2_gate flags it otherwise).
static int l2_plan(mm_ctx* c, L2Pass& p) {
  const int s = c->P.sketchSize;
  if (p.steady) p.chunks.push_back(L2Chunk{0, p.nC, 0});
  else {
    const int64_t* dOff = c->dL2Off.as<int64_t>();
    const int nC = p.nC; const int64_t totalOps = p.totalOps;
    auto offAt = [c, dOff, nC, totalOps](int i, int64_t& v) -> int {         // opOff[i], opOff[nC] = totalOps
      if (i >= nC) { v = totalOps; return MM_OK; }
      MM_HIP(c, hipMemcpy(&v, dOff + i, 8, hipMemcpyDeviceToHost));
      return MM_OK;
    };
    int64_t maxChunkOps = 0;
    const int rc = mm_l2_plan_chunks(nC, totalOps, l2_stream_budget(c), offAt, p.chunks, maxChunkOps); if (rc != MM_OK) return rc;
    if (c->env.debug && p.chunks.size() > 1) fprintf(stderr, "[mm] L2: %lld stream entries of %d candidates in %zu chunks of at most %lld\n", (long long)totalOps, nC, p.chunks.size(), (long long)maxChunkOps);
    const size_t opsFor = p.chunks.size() == 1 ? mm_scaled(c, (size_t)maxChunkOps, 4) : (size_t)maxChunkOps;
    MM_HIP(c, c->dL2Ops.ensure(mm_l2_ops_bytes(opsFor)));
    c->sized.steady.l2Chunks = p.chunks.size();                                                       // a batch that needs several chunks stays with the sized passes
  }
  if (p.steady && c->dL2Ops.bytes == 0) { c->rep.redoCause = MM_REDO_NO_STREAM_BUFFER; return MM_PASS_REDO; }
  p.oneChunk = p.chunks.size() == 1;
  // the pre-load states k_l2_locate leaves for the sweeps: a row of s + 2 cells and four integers per candidate of a chunk
  size_t rows = 0;
  for (const L2Chunk& ch : p.chunks) rows = std::max(rows, (size_t)ch.n);
  if (p.oneChunk) rows = std::max(rows, (size_t)p.nCbuf);
  MM_HIP(c, c->dL2InitCells.ensure(rows * (size_t)((s + 3) & ~1) * 2 + 64));
  MM_HIP(c, c->dL2InitState.ensure(rows * sizeof(L2Init) + 64));
  // total events of the index -> a shift that leaves 16 bits of key (two radix passes)
  { const int64_t nEv = (int64_t)(c->idx.evKey.bytes / 4); while ((nEv >> p.posShift) > 0xFFFF) p.posShift++; }
  p.preLimit = c->env.l2PreLimit;
  return MM_OK;
}

// k_l2_locate over a chunk; above 4096 candidates they are taken in reference order (k_l2_pos_keys)
static int l2_locate(mm_ctx* c, L2Pass& p, const L2Chunk& ch) {
  const DeviceIndex& I = c->idx;
  const L2Geom& g = p.geom;
  KernelTimer t(c, MM_K_L2_LOCATE);
  const int32_t* order = nullptr;
  if (ch.n > 4096) {
    MM_HIP(c, c->dL2OrderPos.ensure((size_t)p.nCbuf * 4 + 64));
    MM_HIP(c, c->dL2Sort[0].ensure((size_t)p.nCbuf * 4 + 64)); MM_HIP(c, c->dL2Sort[2].ensure((size_t)p.nCbuf * 4 + 64));
    hipLaunchKernelGGL(k_l2_pos_keys, dim3((unsigned)((ch.n + 255) / 256)), dim3(256), 0, c->stream, ch.c0, ch.n, p.posShift, c->dL2Info.as<L2Info>(),
                       c->dL2Sort[0].as<uint32_t>(), c->dL2Sort[2].as<int32_t>(), p.nDev);
    MM_HIP(c, hipGetLastError());
    const int rc = mm_order_pairs(c, ch.n, 16u, c->dL2OrderPos.as<int32_t>());
    if (rc != MM_OK) return rc;
    order = c->dL2OrderPos.as<int32_t>();
  }
  const int blocks = std::min((ch.n + g.wpb - 1) / g.wpb, 256 * 32);
  auto kern = k_l2_locate<13>; if (g.JB != 13) kern = k_l2_locate<11>;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.ldsLoc);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(g.wpb * 64), g.ldsLoc, c->stream, ch.c0, ch.n, ch.base, c->P.sketchSize, g.NB, c->dL1.as<mm_l1_candidate>(),
                     c->dStats.as<mm_frag_stats>(), c->dQHash.as<uint64_t>(), c->dQStrand.as<int8_t>(), c->dSkHash.as<uint64_t>(), c->dSkStrand.as<int8_t>(),
                     I.evKey.as<uint32_t>(),
                     I.evAux.as<uint32_t>(), I.evHash.as<uint64_t>(), I.opKey.as<uint32_t>(), I.opAux.as<uint32_t>(), I.opHash.as<uint64_t>(),
                     I.contigOff.as<int64_t>(),
                     c->dL2Info.as<L2Info>(), c->dL2Off.as<int64_t>(), c->dL2Cnt.as<int32_t>(), c->dL2Ops.as<uint32_t>(), order, p.cnt, p.nDev,
                     c->dL2InitCells.as<uint16_t>(), c->dL2InitState.as<L2Init>(), g.initStride, p.preLimit);
  MM_HIP(c, hipGetLastError());
  return MM_OK;
}

// one launch of a sweep kernel (8-bit cells, or 16-bit cells: wide): n candidates starting at c0, or the n listed ones (countDev: their
// number lives on the device, the launch covers listCap of them); the caller holds the timer
static void l2_sweep(mm_ctx* c, const L2Pass& p, bool wide, int c0, int n, int64_t opsBase, const int32_t* list, const unsigned long long* countDev, int listCap, int initBase) {
  const L2Geom& g = p.geom;
  const int lpw = wide ? g.lpwW : g.lpwN;
  const size_t lds = wide ? g.ldsWide : g.ldsNarrow;
  auto kern = k_l2_sweep<false, 11, 64>;                                  // (named in this order, the instantiations keep their places in the code object)
  if (!wide && g.JB == 13) { if (lpw == 32) kern = k_l2_sweep<false, 13, 32>; else kern = k_l2_sweep<false, 13, 16>; }
  if (wide && g.JB == 11) { if (lpw == 64) kern = k_l2_sweep<true, 11, 64>; else kern = k_l2_sweep<true, 11, 32>; }
  if (wide && g.JB == 13) { if (lpw == 16) kern = k_l2_sweep<true, 13, 16>; else kern = k_l2_sweep<true, 13, 8>; }
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)((n + lpw - 1) / lpw)), dim3(64), lds, c->stream, c0, n, opsBase, list, c->P.segLength,
                     c->dL1.as<mm_l1_candidate>(), c->dStats.as<mm_frag_stats>(), c->dL2Off.as<int64_t>(), c->dL2Cnt.as<int32_t>(), c->dL2Ops.as<uint32_t>(),
                     c->dL1Off.as<int64_t>(), c->dL2Tmp.as<L2Tmp>(), p.locap, c->dL2.as<mm_l2_locus>(), (unsigned long long)c->l2Cap,
                     c->dL2Wide.as<int32_t>(), c->dL2Exact.as<int32_t>(), c->dL2First.as<int64_t>(), c->dL2Num.as<int32_t>(), p.cnt, countDev, listCap,
                     c->dL2InitCells.as<uint16_t>(), c->dL2InitState.as<L2Init>(), g.initStride, initBase);
}

// k_l2_sweep_exact over the first n candidates of its list (countDev: their number lives on the device); dL2Cells holds n rows, the
// caller holds the timer
static void l2_sweep_exact(mm_ctx* c, const L2Pass& p, int n, int64_t opsBase, const unsigned long long* countDev) {
  const DeviceIndex& I = c->idx;
  const int s = c->P.sketchSize;
  hipLaunchKernelGGL(k_l2_sweep_exact, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, p.geom.JB, n, opsBase, c->dL2Exact.as<int32_t>(), c->P.segLength,
                     c->dL1.as<mm_l1_candidate>(), c->dStats.as<mm_frag_stats>(), c->dL2Off.as<int64_t>(), c->dL2Cnt.as<int32_t>(), c->dL2Ops.as<uint32_t>(),
                     c->dL1Off.as<int64_t>(), c->dL2Cells.as<ExactCell>(), s + 1, c->dL2Tmp.as<L2Tmp>(), p.locap, c->dL2.as<mm_l2_locus>(),
                     (unsigned long long)c->l2Cap, c->dL2First.as<int64_t>(), c->dL2Num.as<int32_t>(), p.cnt, countDev,
                     c->dL2Info.as<L2Info>(), s, c->dQHash.as<uint64_t>(), c->dQStrand.as<int8_t>(), c->dSkHash.as<uint64_t>(), c->dSkStrand.as<int8_t>(),
                     I.evKey.as<uint32_t>(), I.evAux.as<uint32_t>(), I.evHash.as<uint64_t>(), I.opKey.as<uint32_t>(), I.opAux.as<uint32_t>(), I.opHash.as<uint64_t>());
}

// a chunk's narrow sweep, behind its locate where the chunks take turns in dL2Ops, with the two lists it may queue candidates on emptied
static int l2_chunk_narrow(mm_ctx* c, L2Pass& p, const L2Chunk& ch) {
  if (!p.oneChunk) { const int rc = l2_locate(c, p, ch); if (rc != MM_OK) return rc; }
  MM_HIP(c, hipMemsetAsync(p.cnt + MM_PC_L2_WIDE_LEN, 0, 8, c->stream));
  MM_HIP(c, hipMemsetAsync(p.cnt + MM_PC_L2_EXACT_LEN, 0, 8, c->stream));   // (the L1 stage is done with both words)
  KernelTimer t(c, MM_K_L2);
  // lane-per-candidate sweep: candidates in order of descending stream length, so that the 64 streams of a wave end together
  // (a wave runs as long as its longest; lengths spread ~ +-10 % around 45 steps: max of 64 is ~15 % above the mean)
  const int32_t* order = nullptr;
  if (ch.n > 64) {
    MM_HIP(c, c->dL2Order.ensure((size_t)p.nCbuf * 4 + 64));
    const int rc = mm_order_desc(c, c->dL2Cnt.as<int32_t>(), ch.c0, ch.n, 4, c->dL2Order.as<int32_t>());
    if (rc != MM_OK) return rc;
    order = c->dL2Order.as<int32_t>();
  }
  l2_sweep(c, p, false, ch.c0, ch.n, ch.base, order, p.nDev, 0, ch.c0);
  MM_HIP(c, hipGetLastError());
  return MM_OK;
}

// steady-state pass: the 16-bit re-run and the exact kernel for however many candidates the narrow sweep has queued (usually none),
// launched for a fixed number of them; the lists' lengths are read on the device
static int l2_chunk_steady(mm_ctx* c, L2Pass& p, const L2Chunk& ch) {
  { const int rc = l2_chunk_narrow(c, p, ch); if (rc != MM_OK) return rc; }
  KernelTimer t(c, MM_K_L2);
  l2_sweep(c, p, true, 0, MM_WIDE_CAP, ch.base, c->dL2Wide.as<int32_t>(), p.cnt + MM_PC_L2_WIDE_LEN, MM_WIDE_CAP, ch.c0);
  MM_HIP(c, hipGetLastError());
  MM_HIP(c, c->dL2Cells.ensure((size_t)MM_EXACT_CAP * (size_t)(c->P.sketchSize + 1) * sizeof(ExactCell) + 64));
  l2_sweep_exact(c, p, MM_EXACT_CAP, ch.base, p.cnt + MM_PC_L2_EXACT_LEN);
  MM_HIP(c, hipGetLastError());
  return MM_OK;
}

// sized pass: the counters are read back behind the narrow sweep, and behind each of the two re-runs that its lists ask for (neither runs
// once the slots or the locus buffer have run out: the attempt is repeated anyway)
static int l2_chunk_sized(mm_ctx* c, L2Pass& p, const L2Chunk& ch) {
  { const int rc = l2_chunk_narrow(c, p, ch); if (rc != MM_OK) return rc; }
  const unsigned long long* const hc = p.hc;
  const auto spent = [hc]() { return (hc[MM_PC_L2_FLAGS] & MM_L2F_SLOTS) || hc[MM_PC_L2_OVERFLOW]; };
  MM_HIP(c, hipMemcpyAsync(p.hc, p.cnt, sizeof p.hc, hipMemcpyDeviceToHost, c->stream));
  MM_SYNC(c);
  if (hc[MM_PC_L2_WIDE_LEN] && !spent()) {                                  // the few candidates whose 5-bit counters overflowed
    const int nWide = (int)hc[MM_PC_L2_WIDE_LEN];
    if (c->env.debug) fprintf(stderr, "[mm] L2 sweep: %d of %d candidates redone with 16-bit cells\n", nWide, ch.n);
    KernelTimer t(c, MM_K_L2);
    l2_sweep(c, p, true, 0, nWide, ch.base, c->dL2Wide.as<int32_t>(), nullptr, 0, ch.c0);
    MM_HIP(c, hipGetLastError());
    MM_HIP(c, hipMemcpyAsync(p.hc, p.cnt, sizeof p.hc, hipMemcpyDeviceToHost, c->stream));
    MM_SYNC(c);
  }
  if (hc[MM_PC_L2_EXACT_LEN] && !spent()) {                                 // candidates with a doubly open query hash: the literal sweep
    const int nExact = (int)hc[MM_PC_L2_EXACT_LEN];
    if (c->env.debug) fprintf(stderr, "[mm] L2 sweep: %d of %d candidates redone by the exact kernel (overlapping windows of one hash)\n", nExact, ch.n);
    MM_HIP(c, c->dL2Cells.ensure((size_t)nExact * (size_t)(c->P.sketchSize + 1) * sizeof(ExactCell) + 64));
    KernelTimer t(c, MM_K_L2);
    l2_sweep_exact(c, p, nExact, ch.base, nullptr);
    MM_HIP(c, hipGetLastError());
    MM_HIP(c, hipMemcpyAsync(p.hc, p.cnt, sizeof p.hc, hipMemcpyDeviceToHost, c->stream));
    MM_SYNC(c);
  }
  return MM_OK;
}

int mm_launch_l2(mm_ctx* c, unsigned long long* cnt, bool steady) {
  if (mm_l2_literal_route(c->opt, c->windowed, c->P.sketchSize)) return mm_launch_l2_window(c, cnt);
  L2Pass p;
  p.steady = steady; p.cnt = cnt; p.geom = mm_l2_geom(c->P.sketchSize);
  int rc = l2_extents(c, p); if (rc != MM_OK) return rc;
  rc = l2_plan(c, p); if (rc != MM_OK) return rc;
  if (p.oneChunk) { rc = l2_locate(c, p, p.chunks[0]); if (rc != MM_OK) return rc; }      // its streams stay put over the retries below
  MM_HIP(c, c->dL2Wide.ensure((size_t)p.nCbuf * 4 + 64)); MM_HIP(c, c->dL2Exact.ensure((size_t)p.nCbuf * 4 + 64));
  MM_HIP(c, c->dL2First.ensure((size_t)p.nCbuf * 8 + 64)); MM_HIP(c, c->dL2Num.ensure((size_t)p.nCbuf * 4 + 64));
  c->l2Cap = std::max(c->l2Cap, mm_loci_cap0((size_t)p.nCbuf));
  if (steady && c->sized.steady.prevLocap) p.locap = c->sized.steady.prevLocap;
  for (int attempt = 0; attempt < 24; attempt++) {
    MM_HIP(c, c->dL2.ensure(c->l2Cap * sizeof(mm_l2_locus) + 64));
    MM_HIP(c, c->dL2Tmp.ensure((size_t)p.nCbuf * p.locap * sizeof(L2Tmp) + 64));
    MM_HIP(c, hipMemsetAsync(cnt + MM_PC_L2_LOCI, 0, (size_t)(MM_PC_L2_FLAGS - MM_PC_L2_LOCI) * 8, c->stream));   // cursor, overflow; MM_PC_L2_FLAGS keeps the locate kernel's
    for (const L2Chunk& ch : p.chunks) {
      rc = steady ? l2_chunk_steady(c, p, ch) : l2_chunk_sized(c, p, ch); if (rc != MM_OK) return rc;
      if (p.hc[MM_PC_L2_FLAGS] & MM_L2F_SLOTS) break;                       // slots ran out: everything is redone below with more of them (a full locus
                                                                           // buffer lets the other chunks run on, so that the cursor ends at the total demand)
    }
    if (steady) return MM_OK;                                              // the flags and the count are read when the pass is over
    const L2Retry r = l2_after_readback(c, p.hc, p.nC, p.locap, /*lociFirst=*/false);
    if (r == L2Retry::MoreSlots) {                                         // the flag comes down on the device as well; the locate kernel's stay
      const unsigned long long flags = p.hc[MM_PC_L2_FLAGS] & ~MM_L2F_SLOTS;
      MM_HIP(c, hipMemcpyAsync(cnt + MM_PC_L2_FLAGS, &flags, 8, hipMemcpyHostToDevice, c->stream));
    }
    if (r == L2Retry::Done || r == L2Retry::GiveUp) break;
  }
  rc = mm_l2_verdict(c, p.hc);
  if (rc == MM_OK) c->sized.steady.prevLocap = p.locap;
  return rc;
}
