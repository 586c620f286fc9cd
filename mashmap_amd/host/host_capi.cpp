// mashmap_amd/host/host_capi.cpp -- C entry points around skch::MapPost (skch_map_post.hpp), the host half of skch::Map that turns
// the device's candidate mappings into reported MappingResult rows (chaining computeMap.hpp:1580, filters filter.hpp:103,334,
// sanity checks :1714).  Built as mashmap_amd/lib/libmashmap_host.so so that bench.py can time the stage a user's run goes through
// after the kernels ("packed bases -> MappingResult rows") with the same code skch::Map runs, on all host cores.
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "skch_map_post.hpp"
#include "../csrc/mm_exchange_plan.h"

extern "C" {

// one reported mapping, integers + the two identities (what the PAF line is printed from)
struct mmh_row {
  int32_t querySeqId, queryLen, queryStartPos, queryEndPos, refSeqId, refStartPos, refEndPos, strand, conservedSketches, blockLength;
  float nucIdentity, kmerComplexity;
};

// per read: mapModule's tail (MapPost::mapModuleFromRecords) on `threads` threads.  recs: the batch's candidate mappings, read-major
// (mm_mappings_download / mm_gathered_download); readLens[r] for querySeqId == firstSeqCounter + r.  Returns the number of reported
// mappings (rows, if non-null, receives the first `cap` of them in input order); *seconds = wall time of the stage.
int64_t mmh_post_batch(int k, int segLength, int sketchSize, float pi, int filterMode, int hgFilter, int numMappings,
                       int nContigs, const int32_t* contigLens, const mm_mapping* recs, size_t nRecs, const int32_t* readLens,
                       size_t nReads, int32_t firstSeqCounter, int threads, double* seconds, mmh_row* rows, size_t cap) {
  skch::Parameters p;
  p.kmerSize = k; p.segLength = segLength; p.block_length = segLength; p.chain_gap = segLength; p.sketchSize = sketchSize;
  p.percentageIdentity = pi; p.filterMode = filterMode; p.stage1_topANI_filter = hgFilter != 0;
  p.numMappingsForSegment = (uint32_t)numMappings; p.numMappingsForShortSequence = (uint32_t)numMappings;
  std::vector<skch::ContigInfo> meta((size_t)nContigs);
  for (int i = 0; i < nContigs; i++) meta[i] = skch::ContigInfo{"c" + std::to_string(i), contigLens[i]};
  std::vector<int> grp((size_t)nContigs, 0);
  skch::MapPost post(p, meta, grp);
  const auto t0 = std::chrono::high_resolution_clock::now();
  std::vector<size_t> recBegin(nReads + 1, nRecs);
  { size_t i = 0; for (size_t r = 0; r <= nReads; r++) { while (i < nRecs && (size_t)(recs[i].querySeqId - firstSeqCounter) < r) i++; recBegin[r] = i; } }
  std::vector<skch::MappingResultsVector_t> perRead(nReads);
  std::atomic<size_t> next(0);
  auto work = [&]() {
    const size_t chunk = 64;
    for (size_t r0 = next.fetch_add(chunk); r0 < nReads; r0 = next.fetch_add(chunk))
      for (size_t r = r0; r < std::min(nReads, r0 + chunk); r++)
        if (readLens[r] >= k && recBegin[r] != recBegin[r + 1]) post.mapModuleFromRecords(recs + recBegin[r], recs + recBegin[r + 1], readLens[r], perRead[r]);
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
  int64_t n = 0;
  for (size_t r = 0; r < nReads; r++)
    for (const auto& e : perRead[r]) {
      if (rows && (size_t)n < cap)
        rows[n] = mmh_row{e.querySeqId, e.queryLen, e.queryStartPos, e.queryEndPos, e.refSeqId, e.refStartPos, e.refEndPos, (int32_t)e.strand,
                          e.conservedSketches, e.blockLength, e.nucIdentity, (float)e.kmerComplexity};
      n++;
    }
  if (seconds) *seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
  return n;
}

// The same stage behind mm_chain_reads: chainRows are the batch's rows (mm_chain_download: the reads the device finished, in read
// order) and recs the left-over records of the reads it handed over (mm_chain_leftover_download), read-major; a read has rows, or
// records, or neither.  Rows go through MapPost::finishRows, records through mapModuleFromRecords, and the reported mappings come out
// in input order.  With no rows at all this is mmh_post_batch with chain_gap, block_length and the two mapping counts given
// explicitly.  nMerged / approxMatches (may be null) receive those two fields of every reported mapping beside `rows`.
static int64_t post_chained(int k, int segLength, int sketchSize, float pi, int filterMode, int hgFilter, int numMappingsShort, int numMappingsSegment,
                            int chainGap, int blockLength, int nContigs, const int32_t* contigLens, const mm_chain_row* chainRows, size_t nChainRows,
                            const mm_mapping* recs, size_t nRecs, const int32_t* readLens, size_t nReads, int32_t firstSeqCounter, int threads,
                            double* seconds, mmh_row* rows, int32_t* nMerged, int32_t* approxMatches, size_t cap, const int32_t* refGroup, int split) {
  skch::Parameters p;
  p.kmerSize = k; p.segLength = segLength; p.block_length = blockLength; p.chain_gap = chainGap; p.sketchSize = sketchSize;
  p.percentageIdentity = pi; p.filterMode = filterMode; p.stage1_topANI_filter = hgFilter != 0;
  p.numMappingsForSegment = (uint32_t)numMappingsSegment; p.numMappingsForShortSequence = (uint32_t)numMappingsShort;
  p.skip_prefix = refGroup != nullptr; p.split = split != 0;
  std::vector<skch::ContigInfo> meta((size_t)nContigs);
  for (int i = 0; i < nContigs; i++) meta[i] = skch::ContigInfo{"c" + std::to_string(i), contigLens[i]};
  std::vector<int> grp((size_t)nContigs, 0);
  if (refGroup) grp.assign(refGroup, refGroup + nContigs);
  skch::MapPost post(p, meta, grp);
  const auto t0 = std::chrono::high_resolution_clock::now();
  std::vector<size_t> recBegin(nReads + 1, nRecs), rowBegin(nReads + 1, nChainRows);
  { size_t i = 0; for (size_t r = 0; r <= nReads; r++) { while (i < nRecs && (size_t)(recs[i].querySeqId - firstSeqCounter) < r) i++; recBegin[r] = i; } }
  { size_t i = 0; for (size_t r = 0; r <= nReads; r++) { while (i < nChainRows && (size_t)(chainRows[i].querySeqId - firstSeqCounter) < r) i++; rowBegin[r] = i; } }
  std::vector<skch::MappingResultsVector_t> perRead(nReads);
  std::atomic<size_t> next(0);
  auto work = [&]() {
    const size_t chunk = 64;
    for (size_t r0 = next.fetch_add(chunk); r0 < nReads; r0 = next.fetch_add(chunk))
      for (size_t r = r0; r < std::min(nReads, r0 + chunk); r++) {
        if (readLens[r] < k) continue;
        if (rowBegin[r] != rowBegin[r + 1]) post.finishRows(chainRows + rowBegin[r], chainRows + rowBegin[r + 1], readLens[r], perRead[r]);
        else if (recBegin[r] != recBegin[r + 1]) post.mapModuleFromRecords(recs + recBegin[r], recs + recBegin[r + 1], readLens[r], perRead[r]);
      }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back(work);
  work();
  for (auto& th : pool) th.join();
  int64_t n = 0;
  for (size_t r = 0; r < nReads; r++)
    for (const auto& e : perRead[r]) {
      if ((size_t)n < cap) {
        if (rows) rows[n] = mmh_row{e.querySeqId, e.queryLen, e.queryStartPos, e.queryEndPos, e.refSeqId, e.refStartPos, e.refEndPos, (int32_t)e.strand,
                                    e.conservedSketches, e.blockLength, e.nucIdentity, (float)e.kmerComplexity};
        if (nMerged) nMerged[n] = e.n_merged;
        if (approxMatches) approxMatches[n] = e.approxMatches;
      }
      n++;
    }
  if (seconds) *seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
  return n;
}

int64_t mmh_post_chained(int k, int segLength, int sketchSize, float pi, int filterMode, int hgFilter, int numMappingsShort, int numMappingsSegment,
                         int chainGap, int blockLength, int nContigs, const int32_t* contigLens, const mm_chain_row* chainRows, size_t nChainRows,
                         const mm_mapping* recs, size_t nRecs, const int32_t* readLens, size_t nReads, int32_t firstSeqCounter, int threads,
                         double* seconds, mmh_row* rows, int32_t* nMerged, int32_t* approxMatches, size_t cap) {
  return post_chained(k, segLength, sketchSize, pi, filterMode, hgFilter, numMappingsShort, numMappingsSegment, chainGap, blockLength, nContigs, contigLens, chainRows,
                      nChainRows, recs, nRecs, readLens, nReads, firstSeqCounter, threads, seconds, rows, nMerged, approxMatches, cap, nullptr, 1);
}
// ... under -Y (refGroup, nContigs entries: skip_prefix and MapPost's refIdGroup; nullptr: none) and --noSplit (split == 0): the stage
// behind mm_chain_reads with MM_OPT_CHAIN_MODES, and with no rows at all the host stage of such a run as it was (scripts/chain_probe.py --groups)
int64_t mmh_post_chained_modes(int k, int segLength, int sketchSize, float pi, int filterMode, int hgFilter, int numMappingsShort, int numMappingsSegment,
                               int chainGap, int blockLength, int nContigs, const int32_t* contigLens, const mm_chain_row* chainRows, size_t nChainRows,
                               const mm_mapping* recs, size_t nRecs, const int32_t* readLens, size_t nReads, int32_t firstSeqCounter, int threads,
                               double* seconds, mmh_row* rows, int32_t* nMerged, int32_t* approxMatches, size_t cap, const int32_t* refGroup, int split) {
  return post_chained(k, segLength, sketchSize, pi, filterMode, hgFilter, numMappingsShort, numMappingsSegment, chainGap, blockLength, nContigs, contigLens, chainRows,
                      nChainRows, recs, nRecs, readLens, nReads, firstSeqCounter, threads, seconds, rows, nMerged, approxMatches, cap, refGroup, split);
}

// What mm_chain_reads must leave, from the host's own code: for every read with 1 .. maxRecords records, MapPost::chainedFromRecords
// (mapModuleFromRecords stopped behind filterByGroup) as mm_chain_row, in read order.  Returns the number of rows (out receives the
// first `cap`).  refGroup (nContigs entries; nullptr: no -Y) sets skip_prefix and MapPost's refIdGroup, split == 0 is --noSplit.  One thread.
static int64_t chain_rows(int k, int segLength, int sketchSize, float pi, int filterMode, int numMappingsShort, int numMappingsSegment, int chainGap,
                          int blockLength, int nContigs, const int32_t* contigLens, const mm_mapping* recs, size_t nRecs, const int32_t* readLens,
                          size_t nReads, int32_t firstSeqCounter, int maxRecords, mm_chain_row* out, size_t cap, const int32_t* refGroup, int split) {
  skch::Parameters p;
  p.kmerSize = k; p.segLength = segLength; p.block_length = blockLength; p.chain_gap = chainGap; p.sketchSize = sketchSize;
  p.percentageIdentity = pi; p.filterMode = filterMode;
  p.numMappingsForSegment = (uint32_t)numMappingsSegment; p.numMappingsForShortSequence = (uint32_t)numMappingsShort;
  p.skip_prefix = refGroup != nullptr; p.split = split != 0;
  std::vector<skch::ContigInfo> meta((size_t)nContigs);
  for (int i = 0; i < nContigs; i++) meta[i] = skch::ContigInfo{"c" + std::to_string(i), contigLens[i]};
  std::vector<int> grp((size_t)nContigs, 0);
  if (refGroup) grp.assign(refGroup, refGroup + nContigs);
  skch::MapPost post(p, meta, grp);
  int64_t n = 0;
  skch::MappingResultsVector_t v;
  for (size_t i = 0; i < nRecs;) {
    size_t j = i;
    while (j < nRecs && recs[j].querySeqId == recs[i].querySeqId) j++;
    const size_t r = (size_t)(recs[i].querySeqId - firstSeqCounter);
    if (r < nReads && j - i <= (size_t)maxRecords) {
      post.chainedFromRecords(recs + i, recs + j, readLens[r], v);
      for (const auto& e : v) {
        if ((size_t)n < cap) {
          mm_chain_row& o = out[n];
          std::memset(&o, 0, sizeof o);
          o.querySeqId = e.querySeqId; o.queryLen = (int32_t)e.queryLen; o.queryStartPos = (int32_t)e.queryStartPos; o.queryEndPos = (int32_t)e.queryEndPos;
          o.refSeqId = e.refSeqId; o.refStartPos = (int32_t)e.refStartPos; o.refEndPos = (int32_t)e.refEndPos; o.strand = e.strand;
          o.conservedSketches = e.conservedSketches; o.sketchSize = e.sketchSize; o.blockLength = e.blockLength; o.approxMatches = e.approxMatches;
          o.n_merged = e.n_merged; o.splitMappingId = (int32_t)e.splitMappingId; o.nucIdentity = e.nucIdentity; o.kmerComplexity = (double)e.kmerComplexity;
        }
        n++;
      }
    }
    i = j;
  }
  return n;
}
// the checker of the device rows in tests/test_gpu_chain.py
int64_t mmh_chain_rows(int k, int segLength, int sketchSize, float pi, int filterMode, int numMappingsShort, int numMappingsSegment, int chainGap,
                       int blockLength, int nContigs, const int32_t* contigLens, const mm_mapping* recs, size_t nRecs, const int32_t* readLens,
                       size_t nReads, int32_t firstSeqCounter, int maxRecords, mm_chain_row* out, size_t cap) {
  return chain_rows(k, segLength, sketchSize, pi, filterMode, numMappingsShort, numMappingsSegment, chainGap, blockLength, nContigs, contigLens, recs, nRecs, readLens,
                    nReads, firstSeqCounter, maxRecords, out, cap, nullptr, 1);
}
// ... and for the modes MM_OPT_CHAIN_MODES adds, in tests/test_gpu_chain_modes.py
int64_t mmh_chain_rows_modes(int k, int segLength, int sketchSize, float pi, int filterMode, int numMappingsShort, int numMappingsSegment, int chainGap,
                             int blockLength, int nContigs, const int32_t* contigLens, const mm_mapping* recs, size_t nRecs, const int32_t* readLens,
                             size_t nReads, int32_t firstSeqCounter, int maxRecords, mm_chain_row* out, size_t cap, const int32_t* refGroup, int split) {
  return chain_rows(k, segLength, sketchSize, pi, filterMode, numMappingsShort, numMappingsSegment, chainGap, blockLength, nContigs, contigLens, recs, nRecs, readLens,
                    nReads, firstSeqCounter, maxRecords, out, cap, refGroup, split);
}

// fakeMapQ over [0, 1] as mm_set_paf_tables takes it, from MapPost's own expression (MapPost::mapqTable): thresholds[cap], text[cap * 8].
// Returns the number of entries, or -1 when cap is too small.
int mmh_paf_mapq_table(float* thresholds, char* text, int cap) {
  std::vector<float> t; std::vector<char> x;
  skch::MapPost::mapqTable(t, x);
  if ((size_t)cap < t.size() || !thresholds || !text) return -1;
  std::memcpy(thresholds, t.data(), t.size() * sizeof(float));
  std::memcpy(text, x.data(), x.size());
  return (int)t.size();
}

// What mm_paf_rows / mm_paf_format must write, from the host's own code: MapPost::finishRows + appendReadMappings of the given rows
// (read-major, querySeqId - firstSeqId in [0, nReads)), read by read.  Names arrive as the device calls take them: bytes end to end and
// n + 1 offsets.  text receives the first `cap` bytes, off[nReads + 1] every read's span, reported[nReads] (may be null) the number of
// lines of every read.  Returns the bytes of the whole text, or -1 for a row outside the reads, the contigs or the sketch size (the
// identity bound is cached per (sketchSize, conservedSketches) up to the parameter's sketch size).  One thread.
int64_t mmh_paf_text(int k, int sketchSize, float pi, int legacy, int aniPercentage, int merge, int filterLengthMismatches, int nContigs,
                     const int32_t* contigLens, const char* refNames, const uint64_t* refNameOff, const mm_chain_row* rows, size_t nRows,
                     const int32_t* readLens, size_t nReads, int32_t firstSeqId, const char* queryNames, const uint64_t* queryNameOff, char* text,
                     size_t cap, int64_t* off, int64_t* reported) {
  skch::Parameters p;
  p.kmerSize = k; p.sketchSize = sketchSize; p.percentageIdentity = pi; p.filterMode = skch::filter::MAP;
  p.legacy_output = legacy != 0; p.report_ANI_percentage = aniPercentage != 0; p.mergeMappings = merge != 0; p.filterLengthMismatches = filterLengthMismatches != 0;
  std::vector<skch::ContigInfo> meta((size_t)nContigs);
  for (int i = 0; i < nContigs; i++) meta[i] = skch::ContigInfo{std::string(refNames + refNameOff[i], refNames + refNameOff[i + 1]), contigLens[i]};
  std::vector<int> grp((size_t)nContigs, 0);
  skch::MapPost post(p, meta, grp);
  for (size_t i = 0; i < nRows; i++) {
    const mm_chain_row& r = rows[i];
    if ((size_t)(uint32_t)(r.querySeqId - firstSeqId) >= nReads || (uint32_t)r.refSeqId >= (uint32_t)nContigs || r.sketchSize < 1 || r.sketchSize > sketchSize ||
        r.conservedSketches < 0 || r.conservedSketches > sketchSize || (i && rows[i - 1].querySeqId > r.querySeqId)) return -1;
  }
  std::string all;
  skch::MappingResultsVector_t v;
  size_t i = 0;
  for (size_t r = 0; r < nReads; r++) {
    off[r] = (int64_t)all.size();
    size_t j = i;
    while (j < nRows && (size_t)(rows[j].querySeqId - firstSeqId) == r) j++;
    v.clear();
    if (j > i) {
      post.finishRows(rows + i, rows + j, readLens[r], v);
      post.appendReadMappings(v, std::string(queryNames + queryNameOff[r], queryNames + queryNameOff[r + 1]), all);
    }
    if (reported) reported[r] = (int64_t)v.size();
    i = j;
  }
  off[nReads] = (int64_t)all.size();
  if (text && cap) std::memcpy(text, all.data(), std::min(cap, all.size()));
  return (int64_t)all.size();
}

// slots of the all-gatherv of candidate mappings (mm_exchange_plan.h, what mm_comm.hip places its RCCL broadcasts by): disp[world + 1]
uint64_t mmh_exchange_plan(const uint64_t* counts, int world, uint64_t* disp) { return mm_exchange_place(counts, world, disp); }

}  // extern "C"
