// mashmap_amd/csrc/mm_sketch_dev.h -- the device steps that more than one sketch kernel takes (k_sketch_fast, k_hash_only, k_sketch_hard:
// mm_sketch.hip; k_sketch_global, k_sketch_large; k_ref_hash: mm_index.hip), each stated once.  Everything here is inlined into its callers.
//
// The head of the file -- the fast kernel's cut as a high word and its drain's keep / drop decision -- is plain C++ and compiles for the host
// too (tests/hostlogic/sketch_drain_check.cpp); everything behind it is for hipcc alone.
#pragma once
#include "mm_sketch_plan.h"

// ---------------------------------------------------------------------------------------------
// k_sketch_fast tests a position against its cut on the high words of the two hashes alone, so its cut is a multiple of 2^32: T rounded
// up (any cut is exact as long as s distinct hashes survive it, and a larger one only lets more through), or no cut where that leaves the
// 64 bits.  mm_sketch_fast_cut makes T from a float: 24 significant bits, so at T >= 2^55 (n <= 256 wantFast) the low word is zero already
// and the value -- hence the fragments that go to the hard list -- is what it was.  A position passes when min(hf.hi, hr.hi) <=
// mm_sketch_cut_last_hi(cut).
// ---------------------------------------------------------------------------------------------
MM_SK_HD uint64_t mm_sketch_cut_hiword(uint64_t T) {
  if (T == MM_SK_HASH_MAX) return T;
  const uint32_t hi = (uint32_t)(T >> 32) + ((uint32_t)T != 0u ? 1u : 0u);
  return hi ? (uint64_t)hi << 32 : MM_SK_HASH_MAX;
}
MM_SK_HD uint32_t mm_sketch_cut_last_hi(uint64_t cut) { return cut == MM_SK_HASH_MAX ? 0xFFFFFFFFu : (uint32_t)(cut >> 32) - 1u; }

// The fast kernel's hash loop queues every position under the cut, whether or not it has a k-mer; the drain sees each queued position once
// and keeps it if it lies inside the fragment (pos < n = len - K + 1: the last strip runs past the end) and its k-mer holds no N.
// maskWords: the fragment's N mask, bit i of word j = base 32 j + i is an N, with two words of run-off behind base len - 1; null when the
// read holds no N.
template <int K>
MM_SK_HD bool mm_sk_drain_keep(uint32_t pos, uint32_t n, const uint32_t* maskWords) {
  static_assert(K >= 1 && K <= 64, "a k-mer's mask bits span at most three words");
  if (pos >= n) return false;
  if (!maskWords) return true;
  const uint32_t j = pos >> 5, sh = pos & 31u;
  uint64_t m = ((uint64_t)maskWords[j] | ((uint64_t)maskWords[j + 1] << 32)) >> sh;      // mask bits of bases pos .. pos + 63 - sh
  if (K > 33 && sh) m |= (uint64_t)maskWords[j + 2] << (64 - sh);                           // K + sh <= 64 otherwise
  return (m & (K >= 64 ? ~0ull : ((1ull << (K & 63)) - 1ull))) == 0ull;
}

#ifdef __HIPCC__
#include "mm_device.h"

// ---------------------------------------------------------------------------------------------
// The cut of an ordered LDS table (SkTable, SkFast: mm_sketch.hip).  The home slot is a monotone function of the hash: hashes below the
// cut T are spread over [0, HT), collisions probe linearly WITHOUT wrap-around into spare slots behind.
//   x = top 32 bits of h after normalising T to bit 63, home = x * M >> 32 with M <= 2^32 * HT / (x_max + 1)
//   (any smaller M keeps home < HT and monotone; the float estimate is shaded down)
// ---------------------------------------------------------------------------------------------
struct SkCut {
  uint32_t M; int sh;
  __device__ __forceinline__ void set_cut(uint64_t T, uint32_t HT) {
    sh = (T == MM_HASH_MAX) ? 0 : __clzll((long long)T);
    const uint64_t t32 = ((T << sh) >> 32) + 1ull;
    M = (uint32_t)((float)HT * 4294967296.0f / (float)t32 * 0.99999f);
  }
  __device__ __forceinline__ uint32_t home(uint64_t h) const { return __umulhi((uint32_t)((h << sh) >> 32), M); }
};

// ---------------------------------------------------------------------------------------------
// The fragment out of the packed batch, re-aligned to its first base.  Word j of `words` as if the array began at bit `sh` of word w0:
//   code words (16 bases each):  w0 = base >> 4, sh = (base & 15) * 2;     N-mask words (32 bases each):  w0 = base >> 5, sh = base & 31
// (the run-off words behind the batch are there and zero)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mm_sk_word_at(const uint32_t* __restrict__ words, int64_t w0, int sh, int j) {
  const uint32_t a = words[w0 + j], b = words[w0 + j + 1];
  return sh ? __builtin_amdgcn_alignbit(b, a, sh) : a;
}
// ... staged: dst[j] = word j, for j < n, by the whole workgroup
__device__ __forceinline__ void mm_sk_stage(uint32_t* dst, int n, const uint32_t* __restrict__ words, int64_t w0, int sh, int tid, int nthr) {
  for (int j = tid; j < n; j += nthr) dst[j] = mm_sk_word_at(words, w0, sh, j);
}

// bit j: the k-mer at position 16 * strip + j holds an N.  maskAt(i): word i of the (re-aligned) N mask; 16 + K - 1 mask bits are looked
// at, two words for k-mers of up to 32 bases (and up to 49 bits), four beyond
template <int K, class I, class MaskAt>
__device__ __forceinline__ uint32_t mm_sk_strip_has_n(I strip, MaskAt&& maskAt) {
  const uint64_t m64 = (uint64_t)maskAt(strip >> 1) | ((uint64_t)maskAt((strip >> 1) + 1) << 32);
  if constexpr (MMWideK<K>::value) {
    const uint64_t h64 = (uint64_t)maskAt((strip >> 1) + 2) | ((uint64_t)maskAt((strip >> 1) + 3) << 32);
    const int sh = (int)(strip & 1) * 16;
    return mm_window_or_wide<K>(sh ? ((m64 >> sh) | (h64 << (64 - sh))) : m64, sh ? (h64 >> sh) : h64);
  } else return (uint32_t)mm_window_or<K>(m64 >> ((strip & 1) * 16));
}

// ---------------------------------------------------------------------------------------------
// Occupancy of an ordered table of NS slots (NS and the workgroup multiples of 64: a wave is in or out as a whole): occW = one bit per
// slot, occP = the words' exclusive prefix counts (wave 0: one DPP scan per 64 words); thread 0 hands the number of occupied slots to
// onTotal.  Two barriers inside, none behind: the caller's comes after what onTotal stores.
// ---------------------------------------------------------------------------------------------
template <class OnTotal>
__device__ __forceinline__ void mm_sk_occupancy(const uint64_t* key, uint64_t* occW, uint32_t* occP, int NS, int nOcc, int tid, int nthr, OnTotal&& onTotal) {
  for (int base = 0; base < NS; base += nthr) {
    const int slot = base + tid;
    if (slot < NS) {
      const uint64_t m = __ballot(key[slot] != MM_HASH_MAX);
      if (mm_lane() == 0) occW[slot >> 6] = m;
    }
  }
  __syncthreads();
  if (tid < 64) {
    int carry = 0;
    for (int w0 = 0; w0 < nOcc; w0 += 64) {
      const int w = w0 + tid;
      const int v = w < nOcc ? (int)__popcll(occW[w]) : 0;
      const int ex = mm_wave_excl_scan(v);
      if (w < nOcc) occP[w] = (uint32_t)(carry + ex);
      carry += mm_wave_sum(v);
    }
    if (tid == 0) onTotal(carry);
  }
}

// The cluster (maximal run of occupied slots) around an occupied slot holding k: returns how many of its keys are smaller than k, q =
// its first slot.  MM_SK_GUARD neighbours on either side are fetched at once (independent LDS reads, one latency); only a cluster that
// reaches further is walked slot by slot.  The guard slots beyond the table are always empty.
__device__ __forceinline__ uint32_t mm_sk_cluster_smaller(const uint64_t* key, int slot, uint64_t k, int NS, int& q) {
  uint64_t L[MM_SK_GUARD], Rr[MM_SK_GUARD];
#pragma unroll
  for (int i = 0; i < MM_SK_GUARD; i++) { L[i] = key[slot - 1 - i]; Rr[i] = key[slot + 1 + i]; }
  uint32_t smaller = 0;
  q = slot;
  bool openL = true, openR = true;
#pragma unroll
  for (int i = 0; i < MM_SK_GUARD; i++) {
    openL = openL && L[i] != MM_HASH_MAX;
    openR = openR && Rr[i] != MM_HASH_MAX;
    if (openL) { smaller += L[i] < k ? 1u : 0u; q = slot - 1 - i; }
    if (openR) smaller += Rr[i] < k ? 1u : 0u;
  }
  if (openL) { while (q > 0) { const uint64_t o = key[q - 1]; if (o == MM_HASH_MAX) break; smaller += o < k ? 1u : 0u; q--; } }
  if (openR) { for (int r = slot + 1 + MM_SK_GUARD; r < NS; r++) { const uint64_t o = key[r]; if (o == MM_HASH_MAX) break; smaller += o < k ? 1u : 0u; } }
  return smaller;
}

// the strand of a sketch entry: the sign of the sum of its occurrences' strands, which the reference accumulates in an int16
// (base_types.hpp:24, commonFunc.hpp:268)
__device__ __forceinline__ int8_t mm_sk_strand(int sum) {
  const int16_t acc = (int16_t)sum;
  return acc > 0 ? 1 : (acc == 0 ? 0 : -1);
}

// ---------------------------------------------------------------------------------------------
// The global-memory kernels (k_sketch_global, k_sketch_large): one entry of the sort -- the hash, then position << 1 | (forward strand
// is the smaller one) --, its order, the entry a slice is padded with, and what the two kernels do alike before and behind their sorts.
// ---------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) SkEnt { uint64_t h; uint32_t m; uint32_t pad; };
__device__ __forceinline__ bool mm_sk_ent_less(const SkEnt& a, const SkEnt& b) { return a.h != b.h ? a.h < b.h : a.m < b.m; }
__device__ __forceinline__ SkEnt mm_sk_ent_padding() { SkEnt x; x.h = MM_HASH_MAX; x.m = 0xFFFFFFFFu; x.pad = 0; return x; }

// appends the entries (h, m) of the lanes that keep theirs to the slice e, behind *cursor (an LDS word): one atomic per wave.  Whole
// waves come here together.
__device__ __forceinline__ void mm_sk_append(SkEnt* e, int* cursor, bool keep, uint64_t h, uint32_t m32) {
  const uint64_t m = mm_ballot(keep);
  int base = 0;
  if (m && mm_lane() == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(cursor, (int)__popcll(m));
  if (m) base = __shfl(base, (int)__builtin_ctzll(m));
  if (keep) { SkEnt x; x.h = h; x.m = m32; x.pad = 0; e[base + (int)mm_popc_below(m)] = x; }
}

// Behind the sort of e[0, N2) (ascending, padding last): one output entry per distinct hash in order -- first = smallest position, last =
// largest, strand (commonFunc.hpp:242-270) --, the s smallest (:278-286), and skCount[f].  Every thread owns a contiguous chunk; a run
// belongs to the chunk its first entry lies in.  sCount: one LDS word per thread, sTotal: one more.  Returns true, and writes nothing, when
// fewer than s distinct hashes are there although a cut was applied: the fragment is to be done once more without one.  Barriers inside;
// the caller's comes behind whatever it adds.
__device__ __forceinline__ bool mm_sk_emit_sorted(const SkEnt* e, int64_t N2, int s, bool cut, int f, int* sCount, int* sTotal,
                                                  uint64_t* __restrict__ skHash, int2* __restrict__ skPos, int8_t* __restrict__ skStrand, uint32_t* __restrict__ skCount) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int64_t chunk = (N2 + nthr - 1) / nthr;
  const int64_t c0 = (int64_t)tid * chunk < N2 ? (int64_t)tid * chunk : N2, c1 = c0 + chunk < N2 ? c0 + chunk : N2;
  int mine = 0;
  for (int64_t i = c0; i < c1; i++) { const uint64_t h = e[i].h; if (h != MM_HASH_MAX && (i == 0 || e[i - 1].h != h)) mine++; }
  sCount[tid] = mine;
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int t = 0; t < nthr; t++) { const int v = sCount[t]; sCount[t] = acc; acc += v; } *sTotal = acc; }
  __syncthreads();
  const int total = *sTotal;
  if (total < s && cut) return true;
  int rank = sCount[tid];
  for (int64_t i = c0; i < c1 && rank < s; i++) {
    const uint64_t h = e[i].h;
    if (h == MM_HASH_MAX || (i != 0 && e[i - 1].h == h)) continue;
    int first = (int)(e[i].m >> 1), last = first, sum = 0;
    for (int64_t r = i; r < N2 && e[r].h == h; r++) { last = (int)(e[r].m >> 1); sum += (e[r].m & 1u) ? 1 : -1; }
    const size_t o = (size_t)f * s + rank;
    skHash[o] = h; skPos[o] = make_int2(first, last);
    skStrand[o] = mm_sk_strand(sum);
    rank++;
  }
  if (tid == 0) skCount[f] = (uint32_t)(total < s ? total : s);
  return false;
}
#endif  // __HIPCC__
