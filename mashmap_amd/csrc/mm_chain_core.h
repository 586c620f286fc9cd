// mashmap_amd/csrc/mm_chain_core.h -- the tail of Map::mapModule for ONE read, from its candidate mappings, literally.
//
//   Map::mapSingleQueryFrag    kmerComplexity gate, sort by (refSeqId, refStartPos)     src/map/include/computeMap.hpp:799-800, :830-831, :1137
//   Map::mapModule             coordinates of a split read                              :632-636
//   Map::mergeMappingsInRange  sort, pair loop, union-find, extents, the two averages   :1580-1702   (src/common/dset64.hpp:93-125)
//   Map::filterWeakMappings                                                             :423-432
//   Map::filterByGroup         both sorts, the query-axis plane sweep                   :504-561, src/map/include/filter.hpp:36-160
//
// i.e. MapPost::finishRead (mashmap_amd/host/skch_map_post.hpp) up to and including filterByGroup, on the integers of mm_mapping.
// Shared by the kernel (k_chain_reads, mm_chain.hip) and by the CPU check (tests/hostlogic/chain_check.cpp), which runs it beside
// MapPost on generated reads and compares every field bit for bit.  Compiles for the host (g++) and for the device (hipcc).
//
// Why the result is the host's, bit for bit:
//   sorts     The function takes a read only when it has at most MM_CHAIN_MAX_RECORDS (16) records.  libstdc++'s std::sort of 16 or
//             fewer elements is __insertion_sort alone (_S_threshold), which is stable; mm_chain_sort is a stable insertion sort by
//             the same key from the same input order, so all five sorts of the tail come out the same -- including the one by
//             splitMappingId, whose first member of every chain becomes the chain's representative (conservedSketches of the PAF
//             line).  The 2n events of the sweep and the (dist + score, id) pairs are totally ordered tuples: any sort does.
//   status    The sweep's std::set finds two mappings equivalent when identity, queryStartPos and refSeqId agree: insert is then a
//             no-op and erase(id) removes whichever element is equivalent.  A sorted array of at most 16 ids with the same two rules.
//   identity  a function of (sketchSize, conservedSketches): the host's own floats arrive as a table.
//   chaining  chainGap <= 1 << 25 (mm_chain_params_ok).  A pair that passes dist < max_dist has |query_dist|, |ref_dist| < 2^25, their
//             squares and the sum are integers below 2^53, (query_dist - ref_dist)^2 one below 2^52: exact in a double, with or without
//             a contracted multiply-add.  Only sqrt and dist + score round, both correctly (IEEE; the library is not built with
//             fast-math).  For a pair that fails the test nothing computed is used.
//   averages  accumulated in double from 0.0 in member order, as std::accumulate does.  The identity's sum is double + float on the host
//             too.  The complexity's is not: the host's lambda adds the long double member kmerComplexity in 80 bits and rounds the sum
//             to double, this function adds in double.  ASSUMPTION, not enforced: the complexities of one chain's members lie within a
//             factor 2^24 of each other.  They are floats, at most 16 of them, so every partial sum then spans at most 24 + 24 + 4 = 52
//             bits and is exact in a double and in an 80-bit long double alike; the one rounding is the division.  Beyond that factor a
//             sum rounds once here and twice on the host, and the two can differ in the last bit.  Complexity is
//             rawSketchSize / (maxHash / 2^64) / (2 (len - k + 1)): a factor 2^24 between two fragments of a read needs a bottom-s sketch
//             whose LARGEST hash lies below 2^40 -- s hashes out of 2^64 all that small -- which no sequence a sketch is taken of yields.
//             tests/hostlogic/chain_check.cpp draws maxHash over the whole assumed range (2^40 .. 2^64).
//   kmerComplexity  (double)((long double)maxHash / UINT64_MAX) without an 80-bit type: mm_chain_hash01.
#pragma once
#include <math.h>
#include "mm_heap.h"
#include "../../include/mashmap_hip.h"

// what the function needs beside the caller's parameter block
struct mm_chain_env {
  mm_chain_params p;
  int32_t kmerSize, segLength, stride;       // stride of `identity` (sketchSize + 1)
  const float* identity;                     // identity[Qs * stride + shared]
};

// secondaryShort / secondarySegment are numMappingsFor... - 1 of an unsigned count: -1 (a count of 0) is what the reference and MapPost
// turn into 65535 by their cast to uint16_t (filterByGroup: filterQueryAxis(tmp, (uint16_t)n_mappings)), and so does mm_chain_read;
// anything below -1 is no count at all
MM_HD bool mm_chain_params_ok(const mm_chain_params& p) {
  return p.chainGap >= 0 && p.chainGap <= MM_CHAIN_MAX_GAP && (p.filter == MM_CHAIN_FILTER_NONE || p.filter == MM_CHAIN_FILTER_QUERY) &&
         p.secondaryShort >= -1 && p.secondarySegment >= -1 && p.minMerged >= 0;
}
#define MM_CHAIN_BAD_RECORD (-2)             // mm_chain_read: a record outside the identity table (an error, not a hand-over)

// (double)((long double)maxHash / UINT64_MAX), getSeedHits' max_hash_01 (:830), in integers.  With D = 2^64 - 1 and m' = maxHash << clz
// in [2^63, 2^64): m' * 2^64 = m' * D + m', so the quotient's 64-bit mantissa is m' with remainder m' -- more than D / 2, never a tie (D
// is odd) --: the x87 division rounds it up to m' + 1.  (maxHash == D is the quotient 1.)  Then 64 -> 53 bits, to nearest even.
MM_HD double mm_chain_hash01(uint64_t maxHash) {
  if (maxHash == 0) return 0.0;
  if (maxHash == ~0ull) return 1.0;
  int s = 0;
  while (!((maxHash << s) >> 63)) s++;
  const uint64_t M = (maxHash << s) + 1;     // m' <= 2^64 - 2 here (m' == 2^64 - 1 only for maxHash == D): no wrap
  uint64_t M53 = M >> 11;
  const uint64_t rem = M & 0x7FFull;
  if (rem > 0x400ull || (rem == 0x400ull && (M53 & 1))) M53++;
  return ldexp((double)M53, 11 - 64 - s);    // M53 <= 2^53: exact
}

// getSeedHits (:830-831): the ratio above -> double -> float
MM_HD float mm_chain_kmer_complexity(uint64_t maxHash, int rawSketchSize, int Qlen, int k) {
  const double max_hash_01 = mm_chain_hash01(maxHash);
  return (float)(((double)rawSketchSize / max_hash_01) / (double)((Qlen - k + 1) * 2));
}

MM_HD double mm_chain_sqrt(double x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dsqrt_rn(x);
#else
  return sqrt(x);
#endif
}

// one read's working set: the MappingResult fields the tail reads and writes, per record
struct mm_chain_work {
  int32_t qs[MM_CHAIN_MAX_RECORDS], qe[MM_CHAIN_MAX_RECORDS], rs[MM_CHAIN_MAX_RECORDS], re[MM_CHAIN_MAX_RECORDS];
  int32_t sid[MM_CHAIN_MAX_RECORDS], cons[MM_CHAIN_MAX_RECORDS], sk[MM_CHAIN_MAX_RECORDS], blk[MM_CHAIN_MAX_RECORDS], approx[MM_CHAIN_MAX_RECORDS];
  int32_t nm[MM_CHAIN_MAX_RECORDS], smid[MM_CHAIN_MAX_RECORDS];
  float ident[MM_CHAIN_MAX_RECORDS];
  double kc[MM_CHAIN_MAX_RECORDS];
  int8_t strand[MM_CHAIN_MAX_RECORDS], discard[MM_CHAIN_MAX_RECORDS];
};

// stable insertion sort of ids v[b, e) by less(x, y) -- what std::sort is for at most 16 elements
template <class Less>
MM_HD void mm_chain_sort(int8_t* v, int b, int e, Less less) {
  for (int i = b + 1; i < e; i++) {
    const int8_t x = v[i];
    int j = i;
    while (j > b && less(x, v[j - 1])) { v[j] = v[j - 1]; j--; }
    v[j] = x;
  }
}

// res.approxMatches = std::round(res.nucIdentity * res.blockLength / 100.0): a float product, a double quotient (:1247, :1661)
MM_HD int32_t mm_chain_approx(float ident, int32_t blk) { return (int32_t)round((double)(ident * (float)blk) / 100.0); }

// Finishes the read of length readLen whose records are recs[0, n), in mm_mappings_download's order.  Writes the surviving mappings to
// out (when non-null; up to n of them), in the order filterByGroup leaves them, and returns their number; -1 for n above
// MM_CHAIN_MAX_RECORDS (the read is not taken: the single hand-over cause), MM_CHAIN_BAD_RECORD for a record outside the identity table.
MM_HD int mm_chain_read(const mm_chain_env& E, const mm_mapping* recs, int n, int32_t readLen, mm_chain_row* out) {
  if (n > MM_CHAIN_MAX_RECORDS) return -1;
  if (n <= 0) return 0;
  mm_chain_work W;
  int8_t v[MM_CHAIN_MAX_RECORDS];
  int m = 0;
  const bool split = readLen > E.segLength;                       // :583 (MM_FLAG_NO_SPLIT is refused by the caller)
  const int32_t querySeqId = recs[0].querySeqId;

  // ---- per fragment: mapSingleQueryFrag's gate and sort, then the read's coordinates
  for (int p = 0; p < n;) {
    int q = p;
    while (q < n && recs[q].fragStart == recs[p].fragStart) q++;
    const int32_t Qlen = recs[p].fragLen;
    const float kc = mm_chain_kmer_complexity(recs[p].maxHash, recs[p].rawSketchSize, Qlen, E.kmerSize);
    if (!(kc < E.p.kmerComplexityThreshold)) {                    // :1137
      const int b = m;
      for (int i = p; i < q; i++) {
        const mm_mapping& r = recs[i];
        // a record that names an entry outside the identity table is not a hand-over cause but an error (k_l2_select writes shared <= Qs <=
        // sketchSize): nothing is read outside the table, and the caller reports it (mm_chain_reads: MM_ERR_STATE, "corrupt record")
        if ((uint32_t)r.sketchSize >= (uint32_t)E.stride || (uint32_t)r.conservedSketches >= (uint32_t)E.stride) return MM_CHAIN_BAD_RECORD;
        const int x = m++;
        v[x] = (int8_t)x;
        W.ident[x] = E.identity[(size_t)r.sketchSize * (size_t)E.stride + (size_t)r.conservedSketches];
        W.rs[x] = r.refStartPos; W.re[x] = r.refStartPos + Qlen; W.qs[x] = 0; W.qe[x] = Qlen;
        W.sid[x] = r.refSeqId; W.sk[x] = r.sketchSize; W.cons[x] = r.conservedSketches;
        W.blk[x] = Qlen;                                           // max(refEnd - refStart, queryEnd - queryStart)
        W.approx[x] = mm_chain_approx(W.ident[x], Qlen);
        W.strand[x] = (int8_t)r.strand; W.kc[x] = (double)kc;
        W.nm[x] = 0; W.smid[x] = 0; W.discard[x] = 0;
      }
      mm_chain_sort(v, b, m, [&W](int x, int y) { return W.sid[x] != W.sid[y] ? W.sid[x] < W.sid[y] : W.rs[x] < W.rs[y]; });   // :799-800
      if (split) for (int i = b; i < m; i++) { W.qs[v[i]] = recs[p].fragStart; W.qe[v[i]] = recs[p].fragStart + Qlen; }          // :632-636
    }
    p = q;
  }
  const int32_t queryLen = split ? readLen : recs[0].fragLen;     // (a read that is one fragment: Qlen == len)

  // ---- mergeMappingsInRange + filterWeakMappings
  if (split && E.p.merge) {
    if (m >= 2) {
      const int max_dist = E.p.chainGap;
      mm_chain_sort(v, 0, m, [&W](int x, int y) {
        if (W.sid[x] != W.sid[y]) return W.sid[x] < W.sid[y];
        if (W.rs[x] != W.rs[y]) return W.rs[x] < W.rs[y];
        return W.qs[x] < W.qs[y]; });
      int8_t parent[MM_CHAIN_MAX_RECORDS], rnk[MM_CHAIN_MAX_RECORDS];
      for (int i = 0; i < m; i++) { parent[i] = (int8_t)i; rnk[i] = 0; W.smid[v[i]] = i; }
      auto find = [&parent](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
      for (int i = 0; i < m; i++) {
        const int a = v[i];
        bool have = false; double bestKey = 0; int bestJ = 0;
        for (int j = i + 1; j < m; j++) {
          const int b = v[j];
          if (W.sid[b] != W.sid[a] || W.rs[b] > W.re[a] + max_dist) break;
          if (W.strand[b] != W.strand[a]) continue;
          const int ref_dist = W.rs[b] - W.re[a];
          int query_dist;
          if (W.strand[a] == 1 && W.qs[a] <= W.qs[b]) query_dist = W.qs[b] - W.qe[a];
          else if (W.strand[a] != 1 && W.qe[a] >= W.qe[b]) query_dist = W.qs[a] - W.qe[b];
          else continue;                                           // dist stays at the double's maximum
          const double qd = (double)query_dist, rd = (double)ref_dist, df = (double)(query_dist - ref_dist);
          const double dist = mm_chain_sqrt(qd * qd + rd * rd);
          const double score = df * df;
          if (dist < (double)max_dist) {
            const double key = dist + score;
            if (!have || key < bestKey) { have = true; bestKey = key; bestJ = j; }     // the front of the sorted (key, id) pairs: ids ascend with j
          }
        }
        if (have) {                                                // DisjointSets::unite (dset64.hpp:93-125)
          int x = find(i), y = find(bestJ);
          if (x != y) {
            if (rnk[x] > rnk[y] || (rnk[x] == rnk[y] && x < y)) { const int t = x; x = y; y = t; }     // x goes under y
            parent[x] = (int8_t)y;
            if (rnk[x] == rnk[y]) rnk[y]++;
          }
        }
      }
      for (int i = 0; i < m; i++) W.smid[v[i]] = find(W.smid[v[i]]);
      mm_chain_sort(v, 0, m, [&W](int x, int y) { return W.smid[x] < W.smid[y]; });
      int w = 0;
      for (int it = 0; it < m;) {
        const int rep = v[it];
        int end = it;
        while (end < m && W.smid[v[end]] == W.smid[rep]) end++;
        const float repIdent = W.ident[rep];
        double sumI = 0.0, sumK = 0.0;
        for (int j = it; j < end; j++) {
          const int x = v[j];
          W.qs[rep] = W.qs[x] < W.qs[rep] ? W.qs[x] : W.qs[rep];
          W.rs[rep] = W.rs[x] < W.rs[rep] ? W.rs[x] : W.rs[rep];
          W.qe[rep] = W.qe[x] > W.qe[rep] ? W.qe[x] : W.qe[rep];
          W.re[rep] = W.re[x] > W.re[rep] ? W.re[x] : W.re[rep];
          sumI = sumI + (double)W.ident[x];
          sumK = sumK + W.kc[x];
        }
        const int32_t dr = W.re[rep] - W.rs[rep], dq = W.qe[rep] - W.qs[rep];
        W.blk[rep] = dr > dq ? dr : dq;
        W.approx[rep] = mm_chain_approx(repIdent, W.blk[rep]);
        W.nm[rep] = end - it;
        W.ident[rep] = (float)(sumI / (double)W.nm[rep]);
        W.kc[rep] = sumK / (double)W.nm[rep];
        v[w++] = (int8_t)rep;
        it = end;
      }
      m = w;
    }
    int w = 0;
    for (int i = 0; i < m; i++) if (!(queryLen > W.blk[v[i]] && W.nm[v[i]] < E.p.minMerged)) v[w++] = v[i];     // filterWeakMappings
    m = w;
  }

  // ---- filterByGroup, query axis
  if (E.p.filter == MM_CHAIN_FILTER_QUERY) {
    const int secondaryToKeep = (int)(uint16_t)(readLen < E.segLength ? E.p.secondaryShort : E.p.secondarySegment);
    mm_chain_sort(v, 0, m, [&W](int x, int y) { return W.sid[x] != W.sid[y] ? W.sid[x] < W.sid[y] : W.rs[x] < W.rs[y]; });
    auto byQuery = [&W](int x, int y) {
      if (W.qs[x] != W.qs[y]) return W.qs[x] < W.qs[y];
      if (W.sid[x] != W.sid[y]) return W.sid[x] < W.sid[y];
      return W.rs[x] < W.rs[y]; };
    mm_chain_sort(v, 0, m, byQuery);
    if (m > 1) {                                                   // filterQueryAxis; ids of the sweep are positions in v
      uint64_t ev[2 * MM_CHAIN_MAX_RECORDS];
      for (int i = 0; i < m; i++) {
        W.discard[v[i]] = 1;
        ev[2 * i] = ((uint64_t)((uint32_t)W.qs[v[i]] ^ 0x80000000u) << 8) | (1u << 5) | (uint64_t)i;          // (pos, BEGIN = 1, id)
        ev[2 * i + 1] = ((uint64_t)((uint32_t)W.qe[v[i]] ^ 0x80000000u) << 8) | (2u << 5) | (uint64_t)i;      // (pos, END = 2, id)
      }
      const int nE = 2 * m;
      for (int i = 1; i < nE; i++) { const uint64_t x = ev[i]; int j = i; while (j > 0 && x < ev[j - 1]) { ev[j] = ev[j - 1]; j--; } ev[j] = x; }
      // better(x, y): std::tie(identity as double, queryStartPos, refSeqId) of x > that of y
      auto better = [&W, &v](int x, int y) {
        const int a = v[x], b = v[y];
        if (W.ident[a] != W.ident[b]) return W.ident[a] > W.ident[b];
        if (W.qs[a] != W.qs[b]) return W.qs[a] > W.qs[b];
        return W.sid[a] > W.sid[b]; };
      int8_t status[MM_CHAIN_MAX_RECORDS];
      int nS = 0;
      for (int i = 0; i < nE;) {
        int j = i;
        while (j < nE && (ev[j] >> 8) == (ev[i] >> 8)) j++;
        for (int e = i; e < j; e++) {
          const int id = (int)(ev[e] & 31u);
          int at = 0;
          while (at < nS && better(status[at], id)) at++;          // lower bound
          const bool equivalent = at < nS && !better(id, status[at]);
          if (((ev[e] >> 5) & 7u) == 1u) {
            if (!equivalent) { for (int t = nS; t > at; t--) status[t] = status[t - 1]; status[at] = (int8_t)id; nS++; }
          } else if (equivalent) {
            for (int t = at; t + 1 < nS; t++) status[t] = status[t + 1];
            nS--;
          }
        }
        if (nS > 0) {                                              // markGood (filter.hpp:77-95)
          const float best = W.ident[v[status[0]]];
          int kept = 0;
          for (int t = 0; t < nS; t++) {
            const int x = v[status[t]];
            const bool worseOrSeen = best > W.ident[x] || W.discard[x] == 0;
            if (worseOrSeen && kept > secondaryToKeep) break;
            W.discard[x] = 0;
            ++kept;
          }
        }
        i = j;
      }
      int w = 0;
      for (int i = 0; i < m; i++) if (W.discard[v[i]] == 0) v[w++] = v[i];
      m = w;
    }
    mm_chain_sort(v, 0, m, byQuery);
  }

  if (out)
    for (int i = 0; i < m; i++) {
      const int x = v[i];
      mm_chain_row r;
      r.querySeqId = querySeqId; r.queryLen = queryLen; r.queryStartPos = W.qs[x]; r.queryEndPos = W.qe[x];
      r.refSeqId = W.sid[x]; r.refStartPos = W.rs[x]; r.refEndPos = W.re[x]; r.strand = W.strand[x];
      r.conservedSketches = W.cons[x]; r.sketchSize = W.sk[x]; r.blockLength = W.blk[x]; r.approxMatches = W.approx[x];
      r.n_merged = W.nm[x]; r.splitMappingId = W.smid[x];
      r.nucIdentity = W.ident[x]; r.pad_ = 0; r.kmerComplexity = W.kc[x];
      out[i] = r;
    }
  return m;
}
