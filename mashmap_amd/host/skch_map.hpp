// mashmap_amd/host/skch_map.hpp -- skch::Map on top of the C ABI (include/mashmap_hip.h).
//
// Stands in for the reference's class of the same name (src/map/include/computeMap.hpp:53-1820): same constructor
// signature (maps every query and writes param.outFileName in the ctor, :123-141), same optional per-mapping callback
// (:100-101, called once per reported MappingResult, :1802), same PAF text (:1758-1806).
//
// What moved: sketchSequence, getSeedHits, getSeedIntervalPoints, computeL1CandidateRegions and
// computeL2MappedRegions (:818-1451) and the best-first / early-exit walk of doL2Mapping (:1182-1267, k_l2_select on integer tables
// of its two float decisions) run on the GPU for a whole batch of reads at once (mm_map_fragments).  What stays here, on host
// threads, is everything that touches floating point or std:: algorithm order:
//   * the floats of MappingResult (nucIdentity, its upper bound, kmerComplexity) from the candidate mappings' integers,
//   * chaining (mergeMappingsInRange :1580-1702), filterWeakMappings :423, the plane-sweep filters
//     (filter.hpp:103-160 query axis, :334-396 reference axis), filterFalseHighIdentity :441,
//     mappingBoundarySanityCheck :1714, sparsifyMappings :481 and the PAF writer.
// The reference runs one pthread task per read (ThreadPool.hpp); here three stages run concurrently on successive batches
// (MASHMAP_HIP_BATCH_MBP, default 512 Mbp): the reader thread parses batch i+2, the device stage maps batch i+1, the post stage
// chains / filters / prints batch i on param.threads std::threads.  Output order == input order (ThreadPool.hpp:187-211).
// A device PASS covers as many parsed batches as it takes to fill the GPU (MASHMAP_HIP_COALESCE_MBP, default 3072 Mbp; the kernels of a
// 512 Mbp pass run at ~120 Gbp/s, those of a 2 Gbp pass at ~150): the batches of a pass are laid end to end in HBM by
// mm_reads_upload_packed_parts, each from its own page-locked buffer, so the reader's unit (and the memory it locks) stays small.  A
// pass takes what is queued when the GPU falls free and never waits for more.
//
// Device stage.  The kernels report, per fragment, the candidate mappings doL2Mapping would have pushed (mm_mapping, k_l2_select);
// with several contexts (MASHMAP_HIP_DEVICES, one per GPU, index replicated by Sketch) a batch -- 512 Mbp PER CONTEXT -- is cut into
// contiguous blocks of about equal bases, every context maps its block and hands its records to the host (each GPU over its own
// link; rank-major == input order) before the CPU filters, the one-to-one filter (:358-405) included, see them.
// MASHMAP_HIP_EXCHANGE=allgather puts the device-side all-gatherv (mm_allgatherv_mappings_local, RCCL over xGMI) in front instead.
#pragma once
#include <malloc.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/mashmap_hip.h"
#include "mm_stats.hpp"
#include "pass_plan.hpp"
#include "seq_parse.hpp"
#include "skch_map_post.hpp"
#include "skch_sketch.hpp"
#include "skch_types.hpp"

namespace skch {

class Map {
 public:
  struct L1_candidateLocus_t { seqno_t seqId; offset_t rangeStartPos; offset_t rangeEndPos; int intersectionSize; };   // computeMap.hpp:58
  struct L2_mapLocus_t { seqno_t seqId; offset_t meanOptimalPos, optimalStart, optimalEnd; int sharedSketchSize; strand_t strand; };   // :76
  typedef std::function<void(const MappingResult&)> PostProcessResultsFn_t;

 private:
  const skch::Parameters& param;
  const skch::Sketch& refSketch;
  PostProcessResultsFn_t processMappingResults;
  std::vector<ContigInfo> qmetadata;             // only filled for one-to-one filtering (:105)
  std::vector<int> refIdGroup;
  std::unordered_map<std::string, int> refNameToId;
  std::vector<mm_ctx*> ctxs;                     // one per GPU (Sketch::contexts)
  mm_ctx* ctx;                                   // ctxs[0]
  MapPost post;                                  // everything downstream of the device integers (skch_map_post.hpp)
  std::unique_ptr<mmhost::WorkerPool> postPool;  // the post stage's threads
  bool packedUpload = true;                      // batches travel as 2-bit codes + N mask (set in mapQuery)
  // Host-to-device copies run ahead of the kernels: every context has a staging area that takes the blocks of parsed batches in queue
  // order (mm_reads_prefetch_packed_append), up to twice a pass's worth.  Whoever sees room sends the next block -- the reader the moment
  // it has parsed a batch, the device stage right after an upload has emptied part of the area -- so the copies of the batches behind a
  // pass always run under that pass's kernels.  stagedBases[i]: bases of queued batches already sent to context i (guarded by pfMu).
  std::mutex pfMu; std::vector<size_t> stagedBases; size_t stageCapBases = 0, stageReserveBases = 0;
  // MASHMAP_HIP_DEVICE_CHAIN: the device stage runs mm_chain_reads behind mm_map_fragments and brings back the rows of the reads it
  // finished plus the records of the reads it handed over, instead of every record; the post stage finishes both kinds.  Only in a run
  // with one context, split reads, no reference groups (-Y), filter mode map or one-to-one, sketchSize <= MM_CHAIN_MAX_SKETCH and a
  // chain gap the stage takes; anywhere else the switch does nothing.  With the value `long` the context additionally gets
  // MM_OPT_CHAIN_LONG: reads of 17 .. 512 records are chained on the device too, and only reads above 512 are handed over.  With the
  // value `all` it gets MM_OPT_CHAIN_LONG and MM_OPT_CHAIN_MODES, and the condition "split reads, no reference groups" falls away: the
  // stage then runs under -Y and --noSplit as well (the reference-axis filter of one-to-one stays on the host)
  bool deviceChain = false, deviceChainLong = false, deviceChainModes = false;
  // MASHMAP_HIP_DEVICE_PAF: behind mm_chain_reads the device stage runs mm_paf_rows and brings back the PAF text of the reads the device
  // finished, every read's span in it and the left-over records -- rows only when a read was handed over because one of its rows is not
  // formattable; the post stage writes the spans and finishes the other reads as before.  Acts only where MASHMAP_HIP_DEVICE_CHAIN acts
  // -- with this switch set that includes filter mode none --, and then only in a filter mode other than one-to-one (its output is deferred and needs the mappings), without a processMappingResults
  // callback and without a sparsity threshold; anywhere else one line says why it is ignored
  bool devicePaf = false;
  bool exchangeFellBack = false;                 // a default RCCL all-gatherv failed once: per-context downloads for the rest of the run
  skch::Time::time_point tStart = skch::Time::now();   // MASHMAP_HIP_TIMING lines carry the time since the Map was constructed
  // one write per diagnostic line: three stages log at once, and `std::cerr << a << b` from two threads interleaves inside a line
  struct LogLine {
    std::ostringstream os;
    template <class T> LogLine& operator<<(const T& v) { os << v; return *this; }
    ~LogLine() { os << '\n'; const std::string t = os.str(); std::fwrite(t.data(), 1, t.size(), stderr); }
  };
  std::string at() const { char b[48]; snprintf(b, sizeof b, " [t=%.4f]", std::chrono::duration<double>(skch::Time::now() - tStart).count()); return b; }
  struct Batch {
    mmhost::ParsedBatch in;                      // names, offsets, bases (page-locked buffer, recycled through bufferPool)
    seqno_t firstSeqCounter = 0;
    // candidate mappings of the batch, read-major: a slice of the records its device pass brought back (page-locked, skch_types.hpp;
    // shared by the batches of the pass)
    std::shared_ptr<PinnedRecs<mm_mapping>> recOwner; const mm_mapping* recs = nullptr; size_t nRecs = 0;
    // under MASHMAP_HIP_DEVICE_CHAIN: the rows of the reads mm_chain_reads finished (recs are then the handed-over reads' records only)
    std::shared_ptr<PinnedRecs<mm_chain_row>> rowOwner; const mm_chain_row* rows = nullptr; size_t nRows = 0;
    // under MASHMAP_HIP_DEVICE_PAF: the text mm_paf_rows wrote for the pass, every read's span in it (off, nReads of the pass + 1) and
    // the reads handed over for a row that is not formattable; this batch's reads start at pafFirst
    struct PafPass { std::vector<char> text; std::vector<int64_t> off; std::vector<uint8_t> handed; };
    std::shared_ptr<PafPass> paf; size_t pafFirst = 0;
    mutable std::vector<char> prefetched;        // per context: the batch's block is already on its way to that GPU (guarded by pfMu)
    size_t size() const { return in.names.size(); }
    size_t bases() const { return (size_t)in.totalBases(); }
  };
  // page-locked batch buffers come from skch::HostBufferPool (allocated while the index was being built) and are recycled
  [[noreturn]] void die(const char* what, mm_ctx* c = nullptr) const {
    std::cerr << "[mashmap_hip::skch::Map] ERROR: " << what << ": " << mm_last_error(c ? c : ctx) << std::endl;
    exit(1);
  }
  typedef mmhost::BatchChannel<Batch> Channel;     // hand-over between two stages (pass_plan.hpp)

 public:
  Map(const skch::Parameters& p, const skch::Sketch& refsketch, PostProcessResultsFn_t f = nullptr)
      : param(p), refSketch(refsketch), processMappingResults(f),
        refIdGroup(p.skip_prefix ? refsketch.refGroups() : std::vector<int>(refsketch.metadata.size(), 0)), ctxs(refsketch.contexts()),
        ctx(refsketch.ctx()), post(p, refsketch.metadata, refIdGroup) {
    post.qmetadata = &qmetadata;
    for (size_t i = 0; i < refsketch.metadata.size(); i++) refNameToId.emplace(refsketch.metadata[i].name, (int)i);
    // integer tables the kernels consume: estimateMinimumHitsRelaxed per Q.sketchSize (:1144), sketchCutoffs (:178-258), and the two
    // tables of doL2Mapping's walk (acceptance :1221, ANI cut-off :1192-1202)
    std::vector<int32_t> minHits = mmhost::minHitsTable(p.sketchSize, p.kmerSize, p.percentageIdentity);
    std::vector<int> cut = mmhost::sketchCutoffs(p.sketchSize, p.kmerSize, p.ANIDiff, p.ANIDiffConf, p.stage1_topANI_filter);
    std::vector<int32_t> cut32(cut.begin(), cut.end());
    std::vector<uint8_t> accept; std::vector<int16_t> minIsz;
    mmhost::replayTables(p.sketchSize, p.kmerSize, p.percentageIdentity, p.ANIDiff, p.keep_low_pct_id,
                         mmhost::availableCpus(), accept, minIsz);
    for (mm_ctx* c : ctxs) {
      if (mm_set_tables(c, minHits.data(), minHits.size(), cut32.data(), cut32.size()) != MM_OK) die("mm_set_tables", c);
      if (mm_set_replay_tables(c, accept.data(), minIsz.data(), (size_t)p.sketchSize + 1) != MM_OK) die("mm_set_replay_tables", c);
    }
    const char* chainEnv = getenv("MASHMAP_HIP_DEVICE_CHAIN");
    const bool chainAll = chainEnv && std::strcmp(chainEnv, "all") == 0;
    // (filter mode none: mm_chain_reads takes it as MM_CHAIN_FILTER_NONE; the command line asks for the stage there only together with
    // MASHMAP_HIP_DEVICE_PAF, so that a run with the chain switch alone does what it did)
    const bool pafAsked = getenv("MASHMAP_HIP_DEVICE_PAF") != nullptr;
    if (chainEnv && ctxs.size() == 1 && (chainAll || (p.split && !p.skip_prefix)) &&
        (p.filterMode == filter::MAP || p.filterMode == filter::ONETOONE || (pafAsked && p.filterMode == filter::NONE)) &&
        p.sketchSize <= MM_CHAIN_MAX_SKETCH && p.chain_gap >= 0 && p.chain_gap <= MM_CHAIN_MAX_GAP) {
      const size_t stride = (size_t)p.sketchSize + 1;
      std::vector<float> identity(stride * stride);
      if (mm_stat_identity_table(p.sketchSize, p.kmerSize, identity.data()) != MM_OK) die("mm_stat_identity_table");
      const mm_chain_params cp = post.chainParams();
      if (mm_set_chain_tables(ctx, &cp, identity.data(), stride) != MM_OK) die("mm_set_chain_tables");
      deviceChain = true;
      if (std::strcmp(chainEnv, "long") == 0 || chainAll) {
        if (mm_set_option(ctx, MM_OPT_CHAIN_LONG, 1) != MM_OK) die("mm_set_option(MM_OPT_CHAIN_LONG)");
        deviceChainLong = true;
      }
      if (chainAll) {
        if (mm_set_option(ctx, MM_OPT_CHAIN_MODES, 1) != MM_OK) die("mm_set_option(MM_OPT_CHAIN_MODES)");
        deviceChainModes = true;
      }
    }
    if (pafAsked) {
      const char* why = nullptr;
      if (!deviceChain) why = "MASHMAP_HIP_DEVICE_CHAIN is not set, or does not act in this run";
      else if (p.filterMode == filter::ONETOONE) why = "filter mode one-to-one defers its output and needs the mappings";
      else if (processMappingResults) why = "a processMappingResults callback needs the mappings";
      else if (p.sparsity_hash_threshold != std::numeric_limits<uint64_t>::max()) why = "a sparsity threshold is set (sparsifyMappings stays on the host)";
      if (why) LogLine() << "[mashmap_hip::skch::Map] MASHMAP_HIP_DEVICE_PAF ignored: " << why;
      else {
        std::vector<float> thresholds; std::vector<char> mapqText;
        MapPost::mapqTable(thresholds, mapqText);
        std::string names; std::vector<uint64_t> nameOff(1, 0); std::vector<int32_t> lens;
        for (const auto& m : refsketch.metadata) { names += m.name; nameOff.push_back(names.size()); lens.push_back((int32_t)m.len); }
        const mm_paf_params pp = post.pafParams();
        if (mm_set_paf_tables(ctx, &pp, thresholds.data(), mapqText.data(), thresholds.size(), names.data(), nameOff.data(), lens.data(), lens.size()) != MM_OK) die("mm_set_paf_tables");
        devicePaf = true;
      }
    }
    if (getenv("MASHMAP_HIP_TIMING")) LogLine() << "[mashmap_hip::timing] integer tables ready" << (deviceChain ? " (chaining on the device)" : "")
                                                << (devicePaf ? " (PAF text on the device)" : "") << at();
    this->mapQuery();
    if (getenv("MASHMAP_HIP_TIMING")) LogLine() << "[mashmap_hip::timing] mapQuery done" << at();
    if (getenv("MASHMAP_HIP_TIMING")) {
      uint64_t calls = 0, blocks = 0, bytes = 0;                 // reference and query readers together; all zero unless MASHMAP_HIP_DEVICE_INFLATE=1 met BGZF input
      if (mm_inflate_counts(ctxs[0], &calls, &blocks, &bytes) == MM_OK)
        LogLine() << "[mashmap_hip::timing] device inflater: " << calls << " calls, " << blocks << " blocks, " << bytes << " bytes";
      uint64_t scans = 0, records = 0, textBytes = 0;            // all zero unless MASHMAP_HIP_DEVICE_PARSE=1 met a BGZF query file
      if (mm_text_counts(ctxs[0], &scans, &records, &textBytes) == MM_OK)
        LogLine() << "[mashmap_hip::timing] device parser: " << scans << " scans, " << records << " records, " << textBytes << " bytes";
    }
  }

  static void insertL2ResultsToVec(MappingResultsVector_t& v, const MappingResult& reportedL2Result) { v.push_back(reportedL2Result); }

 private:
  std::string prefix(const std::string& s) const { return s.substr(0, s.find_last_of(param.prefix_delim)); }

  int getRefGroup(const std::string& seqName) const {      // :164-176
    const std::string qp = prefix(seqName);
    for (size_t i = 0; i < refSketch.metadata.size(); i++)
      if (qp == prefix(refSketch.metadata[i].name)) return refIdGroup[i];
    return -1;
  }

  // ------------------------------------------------------------------------------------------------------------------
  void mapQuery() {                                         // :263-420
    seqno_t totalReadsPickedForMapping = 0, totalReadsMapped = 0, seqCounter = 0;
    uint64_t totalBp = 0;
    std::ofstream outstrm(param.outFileName);
    MappingResultsVector_t allReadMappings;
    // a batch = MASHMAP_HIP_BATCH_MBP (default 512 Mbp) PER CONTEXT: every GPU of a sharded run gets a block as large as the batch of a
    // single-GPU run (tens of milliseconds of kernels), instead of an n-th of it
    const QueryBatchPlan plan = queryBatchPlan(param.querySequences, ctxs.size());
    const size_t batchBases = plan.batchBases;
    // the reader's workers normalise and pack the bases (2 bit + N mask, pack2bit.hpp) while they drop the line breaks, so that PCIe
    // carries 0.375 bytes per base instead of 1 (mm_reads_upload_packed); MASHMAP_HIP_ASCII_UPLOAD=1 ships ASCII to k_pack2bit instead
    packedUpload = getenv("MASHMAP_HIP_ASCII_UPLOAD") == nullptr;
    // batches per device pass: only with one context (the blocks of a sharded batch are not consecutive reads across batches) and packed
    // uploads; MASHMAP_HIP_COALESCE_MBP=0 maps every batch by itself
    const size_t maxGroup = (ctxs.size() == 1 && packedUpload) ? std::max<size_t>(1, plan.passBases / std::max<size_t>(1, batchBases)) : 1;
    Channel parsed(std::max<size_t>(2, maxGroup)), mapped(std::max<size_t>(2, 2 * maxGroup));
    if (maxGroup > 1) {
      // passes grow from one batch to maxGroup: the first pass sizes the contexts' staging buffers for the largest one (a quarter of head
      // room for the overlapping tail fragments of reads that are not a multiple of segLength long), the others then launch against them
      const uint64_t frags = plan.passBases / (uint64_t)std::max<offset_t>(1, param.segLength);
      const int reserve = (int)std::min<uint64_t>(0x7fffffffu, frags + frags / 4 + 1024);
      for (mm_ctx* c : ctxs) if (mm_set_option(c, MM_OPT_RESERVE_FRAGMENTS, reserve) != MM_OK) die("mm_set_option", c);
    }
    if (!plan.inputKnown || plan.inputBytes > (256u << 20)) {
      // every batch allocates and frees a few megabyte-sized vectors (records, per-read results, PAF text) from three stages at once:
      // keep them on the heap instead of mmap/munmap per batch (each unmap interrupts every thread of the process), and keep the heap
      mallopt(M_MMAP_THRESHOLD, 32 << 20); mallopt(M_TRIM_THRESHOLD, 1 << 30); mallopt(M_TOP_PAD, 256 << 20);
    }
    stagedBases.assign(ctxs.size(), 0);
    stageCapBases = stagingCapBases(plan, ctxs.size());                               // per context: the pass being assembled and the one behind it (skch_types.hpp)
    stageReserveBases = stagingReserveBases(plan, ctxs.size());
    std::thread reader([&]() {
      // multi-threaded ingest (seq_parse.hpp): a window of the file per batch, parsed straight into a page-locked buffer.  8 workers:
      // memchr + memcpy at that width keep up with the device stage, and more of them page-faulting through the same file mapping next
      // to the post stage's threads stall each other for tens of milliseconds at a time (profiles/r03d_e2e_thread_sweep.txt: 32 reader
      // threads 18 Gbp/s end to end, 8 threads 24-26)
      const char* rte = getenv("MASHMAP_HIP_READER_THREADS");
      const unsigned readerThreads = rte ? (unsigned)std::max(1, atoi(rte)) : std::min((unsigned)std::min(12, std::max(1, param.threads)), std::max(1u, mmhost::availableCpus() * 3 / 4));
      mmhost::BatchReader rd(param.querySequences, batchBases, readerThreads, {}, "",
                             [](size_t n) {                       // only when the pool (skch_sketch.hpp) has run dry
                               const auto t0 = skch::Time::now();
                               char* p = (char*)mm_host_alloc(n);
                               if (getenv("MASHMAP_HIP_TIMING")) LogLine() << "[mashmap_hip::timing] reader: page-locked " << n << " bytes itself in "
                                                                           << std::chrono::duration<double>(skch::Time::now() - t0).count() << " s";
                               return p;
                             }, [](char* p) { mm_host_free(p); }, packedUpload);
      rd.setBlockInflater(deviceBlockInflater(ctxs[0]));          // MASHMAP_HIP_DEVICE_INFLATE=1: BGZF blocks of the query go to mm_inflate_blocks (its own stream: it runs beside the device stage)
      // MASHMAP_HIP_DEVICE_PARSE=1, one context, packed uploads: windows of BGZF query files are inflated, parsed and packed on the device
      if (ctxs.size() == 1 && packedUpload) rd.setWindowParser(deviceWindowParser(ctxs[0], stageReserveBases));
      while (true) {
        Batch batch;
        { auto b = HostBufferPool::instance().take(0); batch.in.bases = b.first; batch.in.cap = b.second; }
        const auto tr0 = skch::Time::now();
        const bool more = rd.next(batch.in);
        if (more && getenv("MASHMAP_HIP_TIMING")) LogLine() << "[mashmap_hip::timing] reader: parsed " << batch.size() << " records, " << batch.in.totalBases() << " bases in "
                                                            << std::chrono::duration<double>(skch::Time::now() - tr0).count() << " s" << at();
        if (!more) { HostBufferPool::instance().give(batch.in.bases, batch.in.cap); break; }
        batch.firstSeqCounter = seqCounter;
        for (size_t r = 0; r < batch.size(); r++) {
          if (batch.in.offs[r + 1] - batch.in.offs[r] > kDeviceMaxLen) {       // see Sketch::build: int32 positions on the device
            std::cerr << "[mashmap::skch::Map::mapQuery] ERROR: query sequence " << batch.in.names[r] << " has " << (batch.in.offs[r + 1] - batch.in.offs[r])
                      << " bp; sequences of more than " << kDeviceMaxLen << tooLongAdvice() << std::endl;
            exit(1);
          }
          const offset_t len = (offset_t)(batch.in.offs[r + 1] - batch.in.offs[r]);
          totalBp += (uint64_t)len;
          if (param.filterMode == filter::ONETOONE) qmetadata.push_back(ContigInfo{batch.in.names[r], len});
          if (len < param.kmerSize) {
            std::cerr << std::endl << "WARNING, skch::Map::mapQuery, read " << batch.in.names[r] << " of " << len << "bp "
                      << " is not long enough for mapping at segment length " << param.segLength << std::endl;
          } else {
            totalReadsPickedForMapping++;
          }
          // short reads travel too (they yield no fragment) so that seqCounter == firstSeqCounter + index inside the batch
          seqCounter++;
        }
        if (batch.size()) {
          // room in the staging areas: this batch's blocks start travelling now.  Prefetch and hand-over are ONE step under pfMu -- the
          // device stage tops the areas up from the queue under the same lock, in queue order, so a block is never sent twice or out of
          // order.  The wait for room in the queue comes first: the device stage takes pfMu between two gets, so a put() that blocked
          // while holding it would never be served.
          parsed.waitSpace();
          std::lock_guard<std::mutex> lk(pfMu);
          if (batch.in.staged) {                              // the device parser has put the words into context 0's staging area: on its way already
            batch.prefetched.assign(ctxs.size(), 0); batch.prefetched[0] = 1; stagedBases[0] += batch.bases();
          }
          if (packedUpload) {
            const std::vector<size_t> cut = blocksOf(batch);
            for (size_t i = 0; i < ctxs.size(); i++) issuePrefetch(batch, i, cut);
          }
          parsed.put(std::move(batch));
        }
      }
      parsed.close();
    });
    std::thread poster([&]() {
      Batch cur;
      while (mapped.get(cur)) {
        postStage(cur, allReadMappings, totalReadsMapped, outstrm);
        if (cur.in.bases) { HostBufferPool::instance().give(cur.in.bases, cur.in.cap); cur.in.bases = nullptr; }   // (normally handed back by the device stage, right behind the upload)
        cur = Batch();
      }
    });
    {
      // pass size, greedy: a pass takes whatever the reader has queued when the GPU falls free (at least one batch, at most maxGroup) and
      // never waits for more.  A one-batch pass costs more per base than the reader needs for a batch, so the queue grows and the next pass
      // takes two or three: the sizes balance themselves where the device keeps up with the reader, the post stage gets its work in a
      // steady trickle instead of six batches at a time, and what is left when the input ends is one small pass.
      std::vector<Batch> grp;
      while (parsed.getGroup(grp, maxGroup)) {
        deviceStage(grp, parsed);
        for (auto& b : grp) mapped.put(std::move(b));
        grp.clear();
      }
      mapped.close();
    }
    reader.join();
    poster.join();
    HostBufferPool::instance().stop();                      // nobody asks for page-locked buffers any more

    if (param.filterMode == filter::ONETOONE) {            // :358-406
      const auto tf0 = skch::Time::now();
      const int n_mappings = (int)param.numMappingsForSegment - 1;
      MappingResultsVector_t tmp, filtered;
      auto b = allReadMappings.begin();
      while (b != allReadMappings.end()) {
        auto e = allReadMappings.end();
        if (param.skip_prefix) {
          const int g = getRefGroup(qmetadata[b->querySeqId].name);
          e = std::find_if_not(b, allReadMappings.end(), [&](const MappingResult& m) { return g == getRefGroup(qmetadata[m.querySeqId].name); });
        }
        tmp.assign(b, e);
        post.filterByGroup(tmp, filtered, n_mappings, true);
        tmp.clear();
        b = e;
      }
      allReadMappings = std::move(filtered);
      std::sort(allReadMappings.begin(), allReadMappings.end(), [](const MappingResult& a, const MappingResult& b2) {
        return std::tie(a.querySeqId, a.queryStartPos, a.refSeqId, a.refStartPos) < std::tie(b2.querySeqId, b2.queryStartPos, b2.refSeqId, b2.refStartPos);
      });
      std::string text;
      post.appendReadMappings(allReadMappings, "", text);
      outstrm.write(text.data(), (std::streamsize)text.size());
      if (processMappingResults) for (const auto& e : allReadMappings) processMappingResults(e);
      if (getenv("MASHMAP_HIP_TIMING")) LogLine() << "[mashmap_hip::timing] one-to-one filter + output " << std::chrono::duration<double>(skch::Time::now() - tf0).count() << " s" << at();
    }
    std::cerr << "[mashmap::skch::Map::mapQuery] count of mapped reads = " << totalReadsMapped
              << ", reads qualified for mapping = " << totalReadsPickedForMapping << ", total input reads = " << seqCounter
              << ", total input bp = " << totalBp << std::endl;
  }

  // sends context i's block of `b` ahead into that context's staging area, if there is room (pfMu held)
  void issuePrefetch(const Batch& b, size_t i, const std::vector<size_t>& cut) {
    if (b.prefetched.size() != ctxs.size()) b.prefetched.assign(ctxs.size(), 0);
    if (b.prefetched[i] || !b.in.packed) return;
    const int64_t o0 = b.in.packOffs[cut[i]], o1 = b.in.packEnd(cut[i], cut[i + 1]);
    const size_t blockBases = (size_t)(b.in.offs[cut[i + 1]] - b.in.offs[cut[i]]);
    if (o1 <= o0 || stagedBases[i] + blockBases > stageCapBases) return;
    mm_ctx* c = ctxs[i];
    const size_t reserve = stageReserveBases;                                          // what skch::Sketch has allocated behind the index build
    int staged = 0;
    if (mm_reads_prefetch_packed_append(c, b.in.bases2() + o0 / 16, b.in.nmask() + o0 / 32, (size_t)(o1 - o0), reserve, &staged) != MM_OK) die("mm_reads_prefetch_packed_append", c);
    if (!staged) return;                                    // the ring had no room under the pieces on their way: asked again when an upload has emptied part of it
    b.prefetched[i] = 1; stagedBases[i] += blockBases;
  }

  // ------------------------------------------------------------------------------------------------------------------
  // device stage: the reads of a pass (one batch; several with a single context) -> candidate mappings, on one GPU or sharded over all
  // contexts in contiguous blocks of about equal bases, one per context (a block may be empty)
  std::vector<size_t> blocksOf(const Batch& batch) const {
    const size_t nReads = batch.size(), nCtx = ctxs.size();
    std::vector<size_t> cutAt(nCtx + 1, nReads);
    cutAt[0] = 0;
    const int64_t total = batch.in.offs[nReads];
    size_t r = 0;
    for (size_t i = 1; i < nCtx; i++) {
      const int64_t want = total * (int64_t)i / (int64_t)nCtx;
      while (r < nReads && batch.in.offs[r] < want) r++;
      cutAt[i] = r;
    }
    return cutAt;
  }

  void deviceStage(std::vector<Batch>& grp, Channel& parsed) {
    const size_t nCtx = ctxs.size(), nB = grp.size();
    const bool timing = getenv("MASHMAP_HIP_TIMING") != nullptr;
    const auto t0 = skch::Time::now();
    size_t nReads = 0, passBases = 0;
    for (const auto& b : grp) { nReads += b.size(); passBases += b.bases(); }
    // per read of the pass (batches end to end): the reference group of its name, the reference contig of the same name
    std::vector<int32_t> readGroup, readSelf;
    std::vector<size_t> first(nB + 1, 0);
    for (size_t j = 0; j < nB; j++) first[j + 1] = first[j] + grp[j].size();
    if (param.skip_prefix) { readGroup.resize(nReads); for (size_t j = 0; j < nB; j++) for (size_t r = 0; r < grp[j].size(); r++) readGroup[first[j] + r] = getRefGroup(grp[j].in.names[r]); }
    if (param.skip_self) {
      readSelf.resize(nReads);
      for (size_t j = 0; j < nB; j++) for (size_t r = 0; r < grp[j].size(); r++) { auto it = refNameToId.find(grp[j].in.names[r]); readSelf[first[j] + r] = it == refNameToId.end() ? -1 : it->second; }
    }
    // several batches per pass only with one context (mapQuery): the blocks are then whole batches and the pass's reads are consecutive
    std::vector<std::vector<size_t>> cutAt(nB);
    for (size_t j = 0; j < nB; j++) cutAt[j] = blocksOf(grp[j]);
    // How the blocks' candidate mappings reach the host stage.  With a GPU per context (MASHMAP_HIP_DEVICES names distinct devices) the
    // exchange step is the one north_star describes: the RCCL all-gatherv of the candidate mappings over xGMI
    // (mm_allgatherv_mappings_local: count all-gather + one grouped broadcast per rank) in front of a single download from context 0 --
    // the layout one-process-per-GPU runs use (bench.py --gpus N, mm_allgatherv_mappings_begin/_end).  Contexts that share a GPU cannot
    // form an RCCL communicator: there every context downloads its own block (rank-major concatenation == input order), which serves
    // every filter mode just as well -- the one-to-one filter (:358-405) runs on the host over all records either way.
    // MASHMAP_HIP_EXCHANGE=allgather | download picks one explicitly; a default all-gatherv that RCCL refuses falls back to the
    // downloads with one warning (an explicit one is fatal).
    const char* xe = getenv("MASHMAP_HIP_EXCHANGE");
    const bool gatherAsked = xe && std::string(xe) == "allgather";
    if (gatherAsked && nCtx > 1 && !refSketch.commReady()) die("MASHMAP_HIP_EXCHANGE=allgather, but the contexts have no communicator (mm_comm_init_local failed)");
    bool gatherOnDevice = nCtx > 1 && !exchangeFellBack && refSketch.commReady() && (xe ? gatherAsked : refSketch.distinctDevices());
    std::vector<PinnedRecs<mm_mapping>> blockRecs(nCtx == 1 ? 0 : nCtx);
    auto all = std::make_shared<PinnedRecs<mm_mapping>>();
    auto allRows = std::make_shared<PinnedRecs<mm_chain_row>>();
    size_t nRows = 0;
    double phase[3] = {0, 0, 0};                           // context 0: upload, kernels, download (seconds)
    auto releaseBuffers = [&]() {                           // the bases are in HBM: the page-locked buffers go back to the reader
      for (auto& b : grp) if (b.in.bases) { HostBufferPool::instance().give(b.in.bases, b.in.cap); b.in.bases = nullptr; }
    };
    auto runBlock = [&](size_t i) {
      mm_ctx* c = ctxs[i];
      const auto p0 = skch::Time::now();
      const seqno_t seqBase = grp[0].firstSeqCounter + (seqno_t)cutAt[0][i];
      if (grp[0].in.packed) {
        std::vector<mm_packed_part> parts(nB);
        for (size_t j = 0; j < nB; j++) {
          const Batch& bt = grp[j];
          const size_t b = cutAt[j][i], e = cutAt[j][i + 1];
          const int64_t o = bt.in.packOffs[b];
          parts[j] = mm_packed_part{bt.in.bases2() + o / 16, bt.in.nmask() + o / 32, bt.in.hasN.data() + b, bt.in.lens.data() + b, bt.in.packOffs.data() + b, e - b,
                                    param.skip_prefix ? readGroup.data() + first[j] + b : nullptr, param.skip_self ? readSelf.data() + first[j] + b : nullptr};
        }
        if (mm_reads_upload_packed_parts(c, parts.data(), nB, seqBase) != MM_OK) die("mm_reads_upload_packed_parts", c);
      } else {                                              // MASHMAP_HIP_ASCII_UPLOAD: one batch per pass, packed on the device
        const size_t b = cutAt[0][i], e = cutAt[0][i + 1];
        if (mm_reads_upload(c, grp[0].in.bases, grp[0].in.offs.data() + b, e - b, param.skip_prefix ? readGroup.data() + b : nullptr,
                            param.skip_self ? readSelf.data() + b : nullptr, seqBase) != MM_OK) die("mm_reads_upload", c);
      }
      if (nCtx == 1) releaseBuffers();
      {
        // this context's staging area has room again: the batches the reader has parsed behind this pass start travelling, in queue
        // order, while the pass is mapped; what the reader parses from now on it sends itself
        std::lock_guard<std::mutex> lk(pfMu);
        for (const auto& bt : grp) if (bt.prefetched.size() == nCtx && bt.prefetched[i]) { const auto ct = blocksOf(bt); stagedBases[i] -= (size_t)(bt.in.offs[ct[i + 1]] - bt.in.offs[ct[i]]); }
        if (packedUpload) parsed.forEach([&](Batch& q) { issuePrefetch(q, i, blocksOf(q)); });
      }
      const auto p1 = skch::Time::now();
      if (mm_map_fragments(c) != MM_OK) die("mm_map_fragments", c);
      if (i == 0) { phase[0] = std::chrono::duration<double>(p1 - p0).count(); phase[1] = std::chrono::duration<double>(skch::Time::now() - p1).count(); }
      if (!blockRecs.empty() && !gatherOnDevice) {
        size_t nb = 0;
        if (mm_mappings_count(c, &nb) != MM_OK) die("mm_mappings_count", c);
        blockRecs[i].resize(nb);
        if (nb && mm_mappings_download(c, blockRecs[i].data(), nb, &nb) != MM_OK) die("mm_mappings_download", c);
      }
    };
    if (nCtx == 1) runBlock(0);
    else {
      std::vector<std::thread> th;
      for (size_t i = 1; i < nCtx; i++) th.emplace_back(runBlock, i);
      runBlock(0);
      for (auto& t : th) t.join();
      releaseBuffers();
    }
    size_t n = 0;
    uint64_t longOffered = 0, longFinished = 0, groupReads = 0, groupRuns = 0, pafBytes = 0, pafHanded = 0;
    size_t chainedRows = 0;
    std::shared_ptr<typename Batch::PafPass> pafPass;
    const auto p2 = skch::Time::now();
    if (nCtx == 1 && deviceChain) {
      // rows of the reads the device finished + records of the reads it handed over, instead of every record
      if (mm_chain_reads(ctx) != MM_OK) die("mm_chain_reads");
      if (mm_chain_counts(ctx, nullptr, nullptr, &nRows, &n) != MM_OK) die("mm_chain_counts");
      if (deviceChainLong && mm_chain_long_counts(ctx, &longOffered, &longFinished) != MM_OK) die("mm_chain_long_counts");
      if (deviceChainModes && mm_chain_group_counts(ctx, &groupReads, &groupRuns) != MM_OK) die("mm_chain_group_counts");
      if (devicePaf) {
        // the text of the reads the device finished and every read's span; rows only for reads handed over for a row that is not formattable
        std::string names; std::vector<uint64_t> nameOff(1, 0);
        nameOff.reserve(nReads + 1);
        for (const auto& b : grp) for (const auto& nm : b.in.names) { names += nm; nameOff.push_back(names.size()); }
        if (mm_paf_rows(ctx, names.data(), nameOff.data(), nReads) != MM_OK) die("mm_paf_rows");
        if (mm_paf_counts(ctx, nullptr, nullptr, &pafBytes, nullptr, &pafHanded) != MM_OK) die("mm_paf_counts");
        pafPass = std::make_shared<typename Batch::PafPass>();
        pafPass->text.resize((size_t)pafBytes); pafPass->off.resize(nReads + 1); pafPass->handed.resize(nReads + 1);
        size_t got = 0;
        if (mm_paf_download(ctx, pafPass->text.data(), pafPass->text.size(), &got) != MM_OK) die("mm_paf_download");
        if (mm_paf_offsets_download(ctx, pafPass->off.data(), pafPass->handed.data()) != MM_OK) die("mm_paf_offsets_download");
        chainedRows = nRows;
        if (!pafHanded) nRows = 0;
      }
      allRows->resize(nRows); all->resize(n);
      if (nRows && mm_chain_download(ctx, allRows->data(), nRows, &nRows) != MM_OK) die("mm_chain_download");
      if (n && mm_chain_leftover_download(ctx, all->data(), n, &n) != MM_OK) die("mm_chain_leftover_download");
    } else if (nCtx == 1) {
      if (mm_mappings_count(ctx, &n) != MM_OK) die("mm_mappings_count");
      all->resize(n);
      if (n && mm_mappings_download(ctx, all->data(), n, &n) != MM_OK) die("mm_mappings_download");
    }
    if (nCtx > 1 && gatherOnDevice) {
      if (mm_allgatherv_mappings_local(ctxs.data(), (int)nCtx) != MM_OK) {
        if (gatherAsked) die("mm_allgatherv_mappings_local");
        std::cerr << "[mashmap_hip::skch::Map] WARNING: the RCCL all-gatherv of the candidate mappings failed (" << mm_last_error(ctx)
                  << "); every context downloads its own block from here on" << std::endl;
        exchangeFellBack = true; gatherOnDevice = false;
        for (size_t i = 0; i < nCtx; i++) {
          size_t nb = 0;
          if (mm_mappings_count(ctxs[i], &nb) != MM_OK) die("mm_mappings_count", ctxs[i]);
          blockRecs[i].resize(nb);
          if (nb && mm_mappings_download(ctxs[i], blockRecs[i].data(), nb, &nb) != MM_OK) die("mm_mappings_download", ctxs[i]);
        }
      } else {
        if (mm_gathered_counts(ctx, nullptr, &n) != MM_OK) die("mm_gathered_counts");
        all->resize(n);
        if (n && mm_gathered_download(ctx, all->data(), n) != MM_OK) die("mm_gathered_download");
      }
    }
    if (nCtx > 1 && !gatherOnDevice) {
      for (const auto& v : blockRecs) n += v.size();
      all->resize(n);
      size_t at = 0;
      for (const auto& v : blockRecs) { if (!v.empty()) std::memcpy(all->data() + at, v.data(), v.size() * sizeof(mm_mapping)); at += v.size(); }
    }
    // the records are read-major in input order: every batch of the pass gets its slice
    {
      size_t at = 0, rowAt = 0;
      for (size_t j = 0; j < nB; j++) {
        const seqno_t endId = grp[j].firstSeqCounter + (seqno_t)grp[j].size();
        const size_t b0 = at, r0 = rowAt;
        while (at < n && (*all)[at].querySeqId < endId) at++;
        while (rowAt < nRows && (*allRows)[rowAt].querySeqId < endId) rowAt++;
        grp[j].recOwner = all; grp[j].recs = all->data() + b0; grp[j].nRecs = at - b0;
        grp[j].rowOwner = allRows; grp[j].rows = allRows->data() + r0; grp[j].nRows = rowAt - r0;
        grp[j].paf = pafPass; grp[j].pafFirst = first[j];
      }
      if (at != n || rowAt != nRows) { std::cerr << "[mashmap_hip::skch::Map] ERROR: candidate mappings of a pass are not in input order" << std::endl; exit(1); }
    }
    if (timing) LogLine() << "[mashmap_hip::timing] device stage (upload + pack + kernels" << (gatherOnDevice ? " + all-gatherv" : "") << " + download of " << n
                          << (deviceChain ? " left-over candidate mappings and " + std::to_string(nRows) + " chained rows): " : std::string(" candidate mappings): "))
                          << std::chrono::duration<double>(skch::Time::now() - t0).count() << " s (upload " << phase[0] << ", kernels " << phase[1]
                          << ", download " << std::chrono::duration<double>(skch::Time::now() - p2).count() << ") [bases " << passBases << "] [batches " << nB << "]"
                          << (deviceChainLong ? " [" + std::to_string(longFinished) + " of " + std::to_string(longOffered) + " reads of more than 16 records chained on the device]" : std::string())
                          << (deviceChainModes ? " [" + std::to_string(groupRuns) + " group runs filtered on the device, " + std::to_string(groupReads) + " reads with more than one]" : std::string())
                          << (devicePaf ? " [" + std::to_string(pafBytes) + " bytes of PAF text of " + std::to_string(chainedRows) + " chained rows written on the device, " + std::to_string(pafHanded) + " reads handed over]" : std::string()) << at();
  }

  // post stage under MASHMAP_HIP_DEVICE_PAF: the device's text holds the lines of every read it finished, in read order; a read with
  // left-over records (handed over by mm_chain_reads) or handed over by mm_paf_rows has an empty span there and is finished here as
  // before.  The spans between two such reads are consecutive bytes of the text: each maximal run is written with one call, the host's
  // lines in between.  Filter mode is not one-to-one and there is no callback (the constructor checked), so nothing keeps the mappings.
  void postStagePaf(Batch& batch, const std::vector<size_t>& recBegin, const std::vector<size_t>& rowBegin, seqno_t& totalReadsMapped, std::ofstream& outstrm,
                    skch::Time::time_point t0, bool timing) {
    const size_t nReads = batch.size();
    const typename Batch::PafPass& P = *batch.paf;
    const int64_t* off = P.off.data() + batch.pafFirst;
    const uint8_t* handed = P.handed.data() + batch.pafFirst;
    std::vector<size_t> hostReads;                         // the reads this stage finishes itself
    for (size_t r = 0; r < nReads; r++)
      if (recBegin[r] != recBegin[r + 1] || (handed[r] && batch.nRows && rowBegin[r] != rowBegin[r + 1])) hostReads.push_back(r);
    std::vector<std::string> hostText(hostReads.size());
    const unsigned nThreads = std::min((unsigned)std::max(1, param.threads), mmhost::availableCpus());
    std::atomic<size_t> next(0);
    auto work = [&]() {
      MappingResultsVector_t one;
      for (size_t i = next.fetch_add(1); i < hostReads.size(); i = next.fetch_add(1)) {
        const size_t r = hostReads[i];
        const offset_t len = (offset_t)(batch.in.offs[r + 1] - batch.in.offs[r]);
        if (len < param.kmerSize) continue;
        one.clear();
        if (handed[r]) post.finishRows(batch.rows + rowBegin[r], batch.rows + rowBegin[r + 1], len, one);
        else post.mapModuleFromRecords(batch.recs + recBegin[r], batch.recs + recBegin[r + 1], len, one);
        post.appendReadMappings(one, batch.in.names[r], hostText[i]);
      }
    };
    if (!hostReads.empty()) {
      if (!postPool || postPool->size() != nThreads) postPool.reset(new mmhost::WorkerPool(nThreads));
      postPool->run(nThreads, [&](unsigned) { work(); });
    }
    const auto t1 = skch::Time::now();
    seqno_t mapped = 0;
    for (size_t r = 0; r < nReads; r++) mapped += off[r + 1] > off[r] ? 1 : 0;             // the device's readsWithText, of this batch
    int64_t runStart = off[0];
    for (size_t i = 0; i < hostReads.size(); i++) {
      if (hostText[i].empty()) continue;
      mapped++;
      const int64_t here = off[hostReads[i]];
      if (here > runStart) outstrm.write(P.text.data() + runStart, (std::streamsize)(here - runStart));
      outstrm.write(hostText[i].data(), (std::streamsize)hostText[i].size());
      runStart = here;
    }
    if (off[nReads] > runStart) outstrm.write(P.text.data() + runStart, (std::streamsize)(off[nReads] - runStart));
    totalReadsMapped += mapped;
    if (timing) LogLine() << "[mashmap_hip::timing] post stage: chain + filter + format " << std::chrono::duration<double>(t1 - t0).count()
                          << " s, output " << std::chrono::duration<double>(skch::Time::now() - t1).count() << " s" << at();
  }

  // post stage: per read, chaining + filters + PAF text on param.threads threads; then output in input order
  void postStage(Batch& batch, MappingResultsVector_t& allReadMappings, seqno_t& totalReadsMapped, std::ofstream& outstrm) {
    const size_t nReads = batch.size();
    const bool timing = getenv("MASHMAP_HIP_TIMING") != nullptr;
    const auto t0 = skch::Time::now();
    // the records are read-major: first record of every read
    std::vector<size_t> recBegin(nReads + 1, batch.nRecs);
    {
      size_t i = 0;
      for (size_t r = 0; r <= nReads; r++) {
        while (i < batch.nRecs && (size_t)(batch.recs[i].querySeqId - batch.firstSeqCounter) < r) i++;
        recBegin[r] = i;
      }
    }
    // ... and, under MASHMAP_HIP_DEVICE_CHAIN, first row of every read (a read has rows, or records, or neither)
    std::vector<size_t> rowBegin(batch.nRows ? nReads + 1 : 0, batch.nRows);
    if (batch.nRows) {
      size_t i = 0;
      for (size_t r = 0; r <= nReads; r++) {
        while (i < batch.nRows && (size_t)(batch.rows[i].querySeqId - batch.firstSeqCounter) < r) i++;
        rowBegin[r] = i;
      }
    }
    if (batch.paf) { postStagePaf(batch, recBegin, rowBegin, totalReadsMapped, outstrm, t0, timing); return; }
    // per CHUNK of 64 consecutive reads, not per read: one text buffer, one result vector, one counter (a hundred thousand small
    // allocations and frees per batch on this thread cost as much as the stage's work)
    const bool reportNow = param.filterMode != filter::ONETOONE;
    const bool keepMaps = !reportNow || (bool)processMappingResults;
    const size_t chunk = 64, nChunks = (nReads + chunk - 1) / chunk;
    std::vector<std::string> chunkText(reportNow ? nChunks : 0);
    std::vector<MappingResultsVector_t> chunkMaps(keepMaps ? nChunks : 0);
    std::vector<int32_t> chunkMapped(nChunks, 0);
    // no wider than the CPUs the process may use (a container's quota: seq_parse.hpp availableCpus) -- more threads than that do not
    // finish the batch sooner, they get the whole process throttled
    const unsigned nThreads = std::min((unsigned)std::max(1, param.threads), mmhost::availableCpus());
    std::atomic<size_t> next(0);
    auto work = [&]() {
      std::string text;                                    // the chunk's PAF lines (MapPost::appendReadMappings: std::to_chars, no stream)
      MappingResultsVector_t one;
      for (size_t ci = next.fetch_add(1); ci < nChunks; ci = next.fetch_add(1)) {
        text.clear();
        int mappedHere = 0;
        for (size_t r = ci * chunk; r < std::min(nReads, (ci + 1) * chunk); r++) {
          const offset_t len = (offset_t)(batch.in.offs[r + 1] - batch.in.offs[r]);
          const bool hasRows = batch.nRows && rowBegin[r] != rowBegin[r + 1];
          if (len < param.kmerSize || (recBegin[r] == recBegin[r + 1] && !hasRows)) continue;
          one.clear();
          if (hasRows) post.finishRows(batch.rows + rowBegin[r], batch.rows + rowBegin[r + 1], len, one);
          else post.mapModuleFromRecords(batch.recs + recBegin[r], batch.recs + recBegin[r + 1], len, one);
          if (one.empty()) continue;
          mappedHere++;
          if (reportNow) post.appendReadMappings(one, batch.in.names[r], text);
          if (keepMaps) chunkMaps[ci].insert(chunkMaps[ci].end(), one.begin(), one.end());
        }
        chunkMapped[ci] = mappedHere;
        if (reportNow) chunkText[ci] = text;
      }
    };
    if (!postPool || postPool->size() != nThreads) postPool.reset(new mmhost::WorkerPool(nThreads));   // persistent: a batch is milliseconds of work
    postPool->run(nThreads, [&](unsigned) { work(); });
    const auto t1 = skch::Time::now();
    size_t textBytes = 0;
    for (const auto& t : chunkText) textBytes += t.size();
    std::string all;                                       // the batch's PAF text, input order, written with one call
    all.reserve(textBytes);
    for (size_t ci = 0; ci < nChunks; ci++) {              // mapModuleHandleOutput (:724-752), input order
      totalReadsMapped += chunkMapped[ci];
      if (!reportNow) allReadMappings.insert(allReadMappings.end(), chunkMaps[ci].begin(), chunkMaps[ci].end());
      else {
        all += chunkText[ci];
        if (processMappingResults) for (const auto& e : chunkMaps[ci]) processMappingResults(e);
      }
    }
    if (!all.empty()) outstrm.write(all.data(), (std::streamsize)all.size());
    if (timing) LogLine() << "[mashmap_hip::timing] post stage: chain + filter + format " << std::chrono::duration<double>(t1 - t0).count()
                          << " s, output " << std::chrono::duration<double>(skch::Time::now() - t1).count() << " s" << at();
  }

};

}  // namespace skch
