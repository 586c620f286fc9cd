// mashmap_amd/csrc/mm_internal.h -- shared between the translation units of libmashmap_hip.so.
// gfx950 (MI355X, wave64) only.  No CUDA, no portability macros.
#pragma once
#include <chrono>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include "../../include/mashmap_hip.h"
#include "mm_devbuf.h"
#include "mm_pass_state.h"
#include "mm_stage_plan.h"

#define MM_WAVE 64

// X(K) for every k-mer size the kernels are instantiated for: the switches that pick a launcher by c->P.kmerSize
#define MM_FOR_EACH_K(X) \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
  X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32) \
  X(33) X(34) X(35) X(36) X(37) X(38) X(39) X(40) X(41) X(42) X(43) X(44) X(45) X(46) X(47) X(48) \
  X(49) X(50) X(51) X(52) X(53) X(54) X(55) X(56) X(57) X(58) X(59) X(60) X(61) X(62) X(63) X(64)

// ---------------------------------------------------------------------------------------------
// host-side helpers
// ---------------------------------------------------------------------------------------------
// (DevBuf, DevStream, DevEvent, PinnedBuf -- the owners of every device allocation, stream, event and page-locked block: mm_devbuf.h)

// fragment descriptor on the device
struct DFrag {
  int64_t base;      // absolute index of the fragment's first base in the packed buffer
  int32_t len;       // bases
  int32_t readId;
};

// device index (see DESIGN.md "data layout in HBM")

#define MM_OPEN_BLOCK_SHIFT 10

struct DeviceIndex {
  size_t nRec = 0, nKeys = 0, nPoints = 0, nContigs = 0, htCap = 0, nOpen = 0;
  // minmerIndex as the L2 event stream (see mm_build_device_index): per contig, one insert event per record at wpos and one
  // eviction event at wpos_end, merged by position
  DevBuf evKey;                // uint32 pos*2 + isInsert
  DevBuf evAux;                // uint32 insert: wpos_end | REV<<31 ; eviction: 0
  DevBuf evHash;               // uint64 hash of the record
  DevBuf contigOff;            // int64[nContigs+1] event offsets
  // records still open at every MM_OPEN_BLOCK-th position (wpos < B < wpos_end, index order), as insert events: the L2 pre-load of a
  // candidate starts from the list of its block instead of streaming a whole segLength of events (computeMap.hpp:1323-1338)
  DevBuf opKey, opAux, opHash; // as evKey / evAux / evHash
  DevBuf blockOff;             // int64[nBlocks+1] offsets into op*
  DevBuf evBlock;              // int64[nBlocks+1] first event at or behind the block start (block b of a contig: pos >= b << MM_OPEN_BLOCK_SHIFT)
  DevBuf contigBlock;          // int64[nContigs+1] first block of every contig
  DevBuf contigLen;            // int32[nContigs]
  DevBuf refGroup;             // int32[nContigs] (all 0 when unused)
  DevBuf htSlots;              // {uint64 key, uint64 val}[htCap]; val = offset<<24 | count<<1 | freq (one 16-byte slot per probe)
  DevBuf filter; uint64_t filterMask = 0;   // presence filter in front of htSlots: uint64 words, mm_filter_word / mm_filter_bits (mm_device.h); word mask, 0 = disabled
  // large tables (human-scale index): htSlots is placed in buckets of MM_TAG_BUCKET slots and fronted by one TAG BYTE per slot (0 = empty):
  // a probe reads the 16 tags of the seed's home bucket -- one 16-byte load out of an array 1/16 the size of the table -- and touches
  // the 16-byte slot only where a tag matches (~86 % of query seeds are absent from the index: sequencing errors)
  DevBuf htTags; bool tagged = false;
  DevBuf ptKeys;               // uint64[nPoints]: seqId<<33 | pos<<1 | (side==OPEN)
  DevBuf keys, keyOff, keyFreq; // the lookup map's key table in the order of ptKeys: uint64 key, uint64 first point (nKeys + 1), uint8 isFrequent
  bool ready = false;
};
// what mm_index_replicate copies to another context.  The replica gets the device index only: neither keys / keyOff / keyFreq nor the
// host mirrors behind mm_index_download, which stay with the source
static constexpr DevBuf DeviceIndex::* const MM_REPLICATED_BUFS[] = {
  &DeviceIndex::evKey, &DeviceIndex::evAux, &DeviceIndex::evHash, &DeviceIndex::contigOff, &DeviceIndex::opKey, &DeviceIndex::opAux, &DeviceIndex::opHash,
  &DeviceIndex::blockOff, &DeviceIndex::evBlock, &DeviceIndex::contigBlock, &DeviceIndex::contigLen, &DeviceIndex::refGroup, &DeviceIndex::htSlots,
  &DeviceIndex::htTags, &DeviceIndex::filter, &DeviceIndex::ptKeys};

// ---------------------------------------------------------------------------------------------
// mm_ctx::dCounters: ONE block of MM_CW_WORDS 64-bit words that the sketch launcher, the index build and every stage of a mapping
// pass count in.  MM_CW_*: word indexes from the start of the block -- where each part begins (and, *_END, the word behind it).
// The words inside a part are named relative to the part's first word, because that is the pointer the kernels are handed:
// MM_PC_* under MM_CW_PASS, MM_MC_* under MM_CW_MAP, MM_SL_* (32-bit) under MM_CW_SORT_LENS, MM_IX_* under MM_CW_INDEX_*.
// ---------------------------------------------------------------------------------------------
enum : int {
  MM_CW_SKETCH        = 0,    //  0..7  the sketch launcher's (reset by it before its kernels).  In use: the low 32 bits of word 0, the
  MM_CW_SKETCH_END    = 8,    //        length of the hard list, which the sketch kernels take as a uint32_t* to the start of the block;
                              //        words 1 and 2, k_sketch_large's counts (MM_SKW_*)
  MM_CW_PASS          = 8,    //  8..   the mapping pass: `counters` of its kernels, `cnt` of its launchers, `passCnt` of k_l2_select (MM_PC_*)
  MM_CW_PASS_END      = 16,   //        ... the words a stage reads back in one copy (MM_PC_READ of them)
  MM_CW_SORT_LENS     = 16,   // 16..17 mapping pass, as 32-bit words: the lengths of the point path's lists (MM_SL_*)
  MM_CW_SORT_LENS_END = 18,
  MM_CW_INDEX_BUILD   = 16,   // 16..19 index build only (mm_finalize_index_device): MM_IX_BUILD_*
  MM_CW_INDEX_FLATTEN = 20,   // 20..23 index build only (mm_flatten_device_index): MM_IX_FLAT_*
  MM_CW_INDEX_END     = 24,
  MM_CW_MID_LEN       = 24,   // 24     mapping pass: fragments on k_lookup_mid's list (MM_PC_MID_LEN from MM_CW_PASS), or on k_lookup_groups' hand-over list (MM_PC_GRP_LEN) ...
  MM_CW_SKETCH_PHASES = 24,   // 24..31 ... and, under MM_SKETCH_STATS, the sketch kernel's phase cycles (read and printed by the sketch launcher
  MM_CW_SKETCH_PHASES_END = 32, //      before the pass resets them); word 24 is also the sink of k_hash_only, which never stores to it
  MM_CW_MAP           = 32,   // 32..39 mapping pass: what a steady-state pass reports besides MM_CW_PASS (MM_MC_*); `result` of k_l2_select
  MM_CW_MAP_END       = 40,
  MM_CW_HARD_COPY     = 48,   // 48     copy of word MM_CW_SKETCH (the hard-list length), taken before the pass resets [0, MM_CW_MAP)
  MM_CW_WORDS         = 64
};
#define MM_COUNTER_BYTES ((size_t)MM_CW_WORDS * 8)   // every ensure() of dCounters, and the page-locked mirror mm_ctx::hPass

// Words of the mapping pass, relative to MM_CW_PASS.  Two of them are used twice, by stages that do not overlap in time: the L2 sweep
// launcher resets them when the L1 stage is done with them.  A steady-state pass reads the block back once, at its end, and so sees
// the L2 sweep's values there: it cannot report how many fragments went through the HBM point path, and PassReport::lastBig repeats the
// figure of the last sized pass (SizedPass::Seen::prevBig) instead.
enum : int {
  MM_PC_POINT_CURSOR   = 0,   // L1 stage: interval points handed out in dPts
  MM_PC_L2_EXACT_LEN   = 0,   // L2 sweep: candidates on the list of k_l2_sweep_exact (dL2Exact)
  MM_PC_POINT_OVERFLOW = 1,   // the interval-point buffer overflowed
  MM_PC_L1_CAND        = 2,   // L1 candidates: the fused ones after k_l1_regions, all of them after the sweeps (their cursor behind the fused ones)
  MM_PC_L1_OVERFLOW    = 3,   // the L1 candidate buffer (a region of it, or the dense buffer) overflowed
  MM_PC_L2_LOCI        = 4,   // L2 locus cursor
  MM_PC_L2_OVERFLOW    = 5,   // the L2 locus buffer overflowed
  MM_PC_L2_FLAGS       = 6,   // MM_L2F_* bits
  MM_PC_BIG_LEN        = 7,   // L1 stage: fragments queued for the HBM point path (dBigList)
  MM_PC_L2_WIDE_LEN    = 7,   // L2 sweep: candidates on the list of the 16-bit-cell sweep (dL2Wide)
  MM_PC_L2_LARGE_LEN   = 7,   // literal L2 route, split batch under MM_OPT_L2_LARGE_WAVE: candidates k_l2_large_wave handed over to k_l2_window (dL2Wide; no 16-bit sweep runs there)
  MM_PC_READ           = MM_CW_PASS_END - MM_CW_PASS,
  MM_PC_MID_LEN        = MM_CW_MID_LEN - MM_CW_PASS,
  MM_PC_GRP_LEN        = MM_PC_MID_LEN // L1 stage under MM_OPT_L1_GROUP_FUSED: fragments k_lookup_groups handed over (dGrpList).  k_lookup_mid never runs in such a
                              // pass (-Y: useMid is off), and a sized pass reads the word back behind the lookup kernels either way (mm_pass_l1_group_fused)
};
enum : int {                  // relative to MM_CW_SKETCH: what k_sketch_large counts (mm_sketch_large_counts)
  MM_SKW_LARGE_FRAGS = 1,     // fragments it sketched
  MM_SKW_LARGE_UNCUT = 2      // ... whose final sort ran without a cut
};
static_assert(MM_CW_SKETCH + MM_SKW_LARGE_UNCUT < MM_CW_SKETCH_END, "k_sketch_large counts inside the sketch launcher's words");
constexpr unsigned long long MM_OVERFLOWED = 1ull;   // what the kernels raise an overflow word to
// bits of MM_PC_L2_FLAGS; any of them set in a steady-state pass has it redone the sized way
constexpr unsigned long long MM_L2F_SLOTS  = 1ull;   // a candidate has more tied loci than the staging slots per candidate (the sized pass doubles them)
constexpr unsigned long long MM_L2F_STREAM = 4ull;   // a stream outgrew the reservation k_l2_extents made for it
constexpr unsigned long long MM_L2F_OPS    = 8ull;   // steady-state pass: the streams do not fit dL2Ops as it is
constexpr unsigned long long MM_L2F_LIST   = 16ull;  // steady-state pass: the wide / exact list is longer than the launch covers
constexpr unsigned long long MM_L2F_CANDS  = 32ull;  // steady-state pass: more candidates than the buffers of this pass hold
// "some stage before this one ran out of room": asked by k_l2_select on the device and by map_pass on the host, of the same words
__host__ __device__ inline bool mm_pass_incomplete(const unsigned long long* pc) {
  return (pc[MM_PC_POINT_OVERFLOW] | pc[MM_PC_L1_OVERFLOW] | pc[MM_PC_L2_OVERFLOW] | pc[MM_PC_L2_FLAGS]) != 0;
}
enum : int {                  // relative to MM_CW_MAP
  MM_MC_MAPPINGS = 0,         // candidate mappings k_l2_select<true> found
  MM_MC_OVERFLOW = 1,         // ... more than dMappings holds
  MM_MC_L2_OPS   = 2          // L2 stream entries reserved (copied here by the L2 launcher)
};
// why a steady-state pass is redone, as mm_pass_redo_cause reports it (MM_REDO_*): from the host mirror of the two parts a steady-state
// pass reads back at its end -- pc: the words under MM_CW_PASS, mc: those under MM_CW_MAP.  Nonzero exactly when pass_finish says MM_PASS_REDO:
// every MM_L2F_* bit has its MM_REDO_* bit here (a new flag bit needs one too)
inline uint64_t mm_redo_cause(const unsigned long long* pc, const unsigned long long* mc) {
  const unsigned long long f = pc[MM_PC_L2_FLAGS];
  uint64_t cause = 0;
  if (pc[MM_PC_POINT_OVERFLOW]) cause |= MM_REDO_POINTS;
  if (pc[MM_PC_L1_OVERFLOW]) cause |= MM_REDO_L1;
  if (pc[MM_PC_L2_OVERFLOW]) cause |= MM_REDO_L2_LOCI;
  if (f & MM_L2F_SLOTS) cause |= MM_REDO_L2_SLOTS;
  if (f & MM_L2F_STREAM) cause |= MM_REDO_L2_STREAM;
  if (f & MM_L2F_OPS) cause |= MM_REDO_L2_OPS;
  if (f & MM_L2F_LIST) cause |= MM_REDO_L2_LIST;
  if (f & MM_L2F_CANDS) cause |= MM_REDO_L2_CANDS;
  if (mc[MM_MC_OVERFLOW]) cause |= MM_REDO_MAPPINGS;
  return cause;
}
enum : int {                  // 32-bit words relative to MM_CW_SORT_LENS
  MM_SL_BLOCK   = 0,          // list of k_sort_points_block (listB of k_classify_sort)
  MM_SL_GLOBAL  = 1,          // list of k_sort_points_global (listC)
  MM_SL_LITERAL = 2,          // the fragments k_l1_stream leaves for k_l1_sweep (a word of its own: the two above still feed the sorters
                              // in flight); a sized pass reads it back behind the L1 sweeps, with the L1 cursor (mm_pass_l1_literal)
  MM_SL_END     = 4
};
enum : int {                  // index build diagnostics, relative to MM_CW_INDEX_BUILD / MM_CW_INDEX_FLATTEN
  MM_IX_BUILD_UNSTABLE = 0,   // |= 1: the sort did not keep the records of a hash in minmerIndex order
  MM_IX_BUILD_NFREQ    = 1,   // frequent keys
  MM_IX_BUILD_CURSOR   = 2,   // cursor of the frequent-key list
  MM_IX_BUILD_THRESHOLD = 3,  // int32: the frequency threshold
  MM_IX_FLAT_BAD_REC   = 1,   // a record out of order or with a bad position
  MM_IX_FLAT_MAX_LEN   = 2,   // longest window
  MM_IX_FLAT_TABLE     = 3    // |= 1 value overflow, |= 2 duplicate key
};
static_assert(MM_CW_SKETCH_END <= MM_CW_PASS && MM_CW_PASS_END <= MM_CW_SORT_LENS && MM_CW_SORT_LENS_END <= MM_CW_MID_LEN, "mapping pass: parts overlap");
static_assert(MM_CW_SORT_LENS * 2 + MM_SL_END <= MM_CW_SORT_LENS_END * 2, "the 32-bit list lengths outgrow their words");
static_assert(MM_CW_MID_LEN < MM_CW_MAP && MM_CW_MAP + MM_MC_L2_OPS < MM_CW_MAP_END && MM_CW_MAP_END <= MM_CW_HARD_COPY && MM_CW_HARD_COPY < MM_CW_WORDS, "mapping pass: parts overlap");
static_assert(MM_CW_INDEX_BUILD + 4 == MM_CW_INDEX_FLATTEN && MM_CW_INDEX_FLATTEN + 4 == MM_CW_INDEX_END && MM_CW_SKETCH_END <= MM_CW_INDEX_BUILD, "index build: parts overlap");
static_assert(MM_CW_SKETCH_PHASES >= MM_CW_INDEX_END && MM_CW_SKETCH_PHASES_END <= MM_CW_MAP, "the sketch statistics must stay clear of the words that outlive the sketch launcher");
static_assert(MM_PC_POINT_CURSOR == MM_PC_L2_EXACT_LEN && MM_PC_BIG_LEN == MM_PC_L2_WIDE_LEN, "the words shared by the L1 stage and the L2 sweep");
static_assert(MM_CW_PASS + MM_PC_MID_LEN == MM_CW_SKETCH_PHASES, "k_lookup_mid's list length shares its word with the sketch statistics");
static_assert(MM_PC_L2_LARGE_LEN == MM_PC_L2_WIDE_LEN, "k_l2_large_wave and k_l2_window_wave count their hand-overs in one word: a batch is split or windowed");
static_assert(MM_PC_L2_LOCI + 1 == MM_PC_L2_OVERFLOW && MM_PC_L2_OVERFLOW + 1 == MM_PC_L2_FLAGS && MM_PC_L2_FLAGS < MM_PC_READ, "the L2 words are reset as one range");
static_assert(MM_PC_GRP_LEN == MM_PC_MID_LEN && MM_PC_GRP_LEN != MM_PC_BIG_LEN, "k_lookup_groups counts its hand-overs in the mid list's word, beside the queue it reads");
static_assert(MM_PC_L1_CAND + 1 == MM_PC_L1_OVERFLOW, "the L1 cursor and its flag are read back as one range");

// The device library's environment switches ("Environment switches"), read once per context by mm_create: a switch
// set after a context was created does not reach it
struct mm_env {
  bool debug = false;             // MM_DEBUG: what every stage of a pass did, on stderr
  bool timing = false;            // MASHMAP_HIP_TIMING: wall time of the sized passes (and the RCCL library bound), on stderr
  bool sketchStats = false;       // MM_SKETCH_STATS: phase cycles of the fast sketch kernel, on stderr
  bool l1Literal = false;         // MM_L1_LITERAL: every queued fragment through the literal L1 kernel instead of k_l1_stream
  int l2PreLimit = 4000;          // MM_L2_PRE_LIMIT (0 .. 3999): pre-loads of this many records or more go to the exact L2 kernel
  double l2StreamMiB = 0;         // MM_L2_STREAM_MIB: budget of one chunk of L2 streams; 0 = sized by the free device memory
  bool winnowGsk = false;         // MM_WINNOW_GSK: the HBM form of the window sketch of k_winnow_tiles at any sketch size
  int seedTags = -1;              // MM_SEED_TAGS: 1 / 0 forces the tag layer of the seed table on / off; -1 = by the table's size
  std::string rcclPath;           // MASHMAP_HIP_RCCL: the RCCL library to bind first
  bool noRccl = false;            // MASHMAP_HIP_NO_RCCL: a local group exchanges by peer copies even across distinct GPUs
  bool requireRccl = false;       // MASHMAP_HIP_REQUIRE_RCCL: a local group without a communicator is an error, not a warning
};
mm_env mm_read_env();

// A batch of reads on the device: everything an upload leaves behind.  mm_ctx IS its resident batch (c->nFrags, c->dFrags, ...) and
// parks others beside it; mm_reads_exchange swaps two of these, by pointer.  Movable, not copyable (DevBuf).
struct ReadBatch {
  size_t nReads = 0, nFrags = 0, nPackedBases = 0;
  int32_t seqCounterBase = 0, maxFragLen = 0;
  bool windowed = false;                                // --noSplit: some fragment of the batch is longer than segLength (windowLen != 0, computeMap.hpp:933)
  DevBuf dReadSrcOff, dReadPackOff, dReadLen, dReadGroup, dReadSelf, dReadHasN;
  DevBuf dBases2, dNmask, dFrags;
  std::vector<mm_fragment> hFrags;
};

// A reader thread, the context's own thread and the gather thread all touch mm_ctx.  Two locks guard what they share, and each sits in a
// member of mm_ctx beside exactly the fields it guards: Staging::prefetchMu and DeviceInput::inflateMu.  Where both are taken, inflateMu
// is taken first (mm_text_pack).  Everything else in mm_ctx belongs to the context's own thread, which lends the exchange's fields to the
// gather thread from mm_allgatherv_mappings_begin until it joins it.
//
// What travels ahead of an upload, on a stream of its own while the current batch is mapped (mm_reads_prefetch*): the next batch's ASCII
// bytes, or packed pieces in a ring (mm_stage_plan.h) -- one area, dAsciiNext, holds either.  copyDone always marks the last copy into it.
// mm_reads_prefetch* and mm_text_pack may come from another thread than the uploads, which match and consume this state.
struct Staging {
  std::mutex prefetchMu;
  DevBuf dAsciiNext; DevStream copyStream; DevEvent copyDone;
  const void* prefetchPtr = nullptr; size_t prefetchBytes = 0; bool prefetchValid = false;   // the ASCII bytes sent ahead: their host range
  StageRing ring;                                       // the packed pieces sent ahead: [codes | mask] at dAsciiNext + off
};

struct InflateErr { std::string err; };                 // what MM_HIP writes to on the reader thread's paths (never mm_ctx::err)

// mm_inflate_blocks (mm_inflate.hip) and mm_text_* (mm_text.hip): a stream, a lock and buffers of their own -- a reader thread calls them
// beside the context's own thread
struct DeviceInput {
  mutable std::mutex inflateMu;
  DevStream inflateStream;
  struct Inflate {
    DevBuf dInfComp, dInfOut, dInfDesc, dInfStatus, dInfStats;   // compressed span, payloads packed end to end, descriptors, one status word per block, [next block | blocks, bytes out, bad blocks]
    DevEvent infEvA, infEvB;
    std::vector<mm_inflate_block> infDesc; std::vector<uint32_t> infOrder, infStatus;
    uint64_t infCalls = 0, infBlocks = 0, infBytes = 0, infBad = 0; double infKernelMs = 0; int infGrid = 0;
  } inf;
  // the text buffer (dText, textLen bytes; dTextAlt takes the tail when the consumed bytes leave), per tile its summary and carry-in, the
  // record table with the sequence-byte index at every record start, keep flags, packed start of every record, the totals block, scratch
  // for a piece that is not staged
  struct Text {
    DevBuf dText, dTextAlt, dTextSum, dTextCarry, dTextRecs, dTextSeqStart, dTextKeep, dTextPackOff, dTextTotals, dTextNames, dTextWords;
    size_t textLen = 0; bool textScanned = false; int textFormat = 0, textFinal = 0;
    size_t textRecords = 0, textNameBytes = 0, textConsumed = 0;
    DevEvent textEvA, textEvB, textDone;
    uint64_t textScans = 0, textRecordsTotal = 0, textBytesTotal = 0; double textScanMs = 0, textPackMs = 0;
  } text;
  int ready(int device, InflateErr* e);                 // inflateMu held: the device is set and the stream exists
};

struct mm_ctx : ReadBatch {                             // the resident reads: the base
  int device = 0;
  DevStream stream;
  mm_params P{};
  mm_env env;
  std::string err;
  Options opt;                                          // mm_set_option
  // a mapping pass's bookkeeping, by lifetime (mm_pass_state.h): the last mm_map_fragments, the last sized pass, the context
  PassReport rep;
  SizedPass sized;
  PassTotals tot;

  // host mirrors needed for downloads in reference layout
  std::vector<mm_minmer> hMinmers;
  std::vector<mm_minmer> hMinmersAll;                   // minmerIndex before dropFreqSeedSet (only with Options::keepFullIndex: --saveIndex)
  std::vector<uint64_t> hKeys, hOffsets, hFreq;
  std::vector<mm_interval_point> hPoints;
  bool mirrorMinmers = false, mirrorMap = false;        // the host copies above are filled (a device-built index fills them on request)
  int32_t freqThreshold = 0x7fffffff;

  DeviceIndex idx;
  DevBuf dMinHits, dCutoffs; size_t nMinHits = 0, nCutoffs = 0;

  DevBuf dAscii;                                        // the resident batch's ASCII bytes as uploaded (an upload's scratch: not part of ReadBatch)
  Staging stage;
  DeviceInput input;
  ReadBatch parked[MM_BATCH_SLOTS];                     // batches parked beside the resident one (mm_reads_exchange)

  // sketches: raw (a4) and after frequent-seed removal (a8)
  DevBuf dSkHash, dSkPos, dSkStrand, dSkCount;          // [nFrags*s] u64, int2, i8 ; [nFrags] u32
  DevBuf dHardList, dCounters, dSketchSpill;            // dSketchSpill: first / last / strand-sum arrays of k_sketch_hard<K, true> (large sketches)
  DevBuf dSketchTabs; int sketchTabsK = 0;        // strip-hasher tables for kmerSize sketchTabsK (built once, copied into LDS by every workgroup)
  // MM_OPT_SKETCH_LARGE: the two counts of k_sketch_large as of the last sketch launch -- copied to the page-locked hSkLarge behind the
  // kernel (the mapping pass resets the words they are counted in); mm_sketch_large_counts waits for skLargeDone when the copy is pending
  PinnedBuf hSkLarge; DevEvent skLargeDone;
  int skLargeState = 0; uint64_t skLargeFrags = 0, skLargeUncut = 0;   // MM_SKL_STATE_*
  DevBuf dQHash, dQStrand;                              // post-removal sketch (written only for fragments that lose a frequent seed)
  DevBuf dStats;                                        // mm_frag_stats[nFrags]
  DevBuf dPtOff, dPts; size_t ptsCap = 0;               // per-fragment offset (int64) + sorted keys
  DevBuf dPtKept;                                       // int32[nFrags]: points of a queued fragment that reach the L1 kernels (k_gather_points, k_filter_points)
  // --noSplit with reads longer than segLength (ReadBatch::windowed): the literal kernels' state
  DevBuf dPtIds, dWinFreq, dWinExt, dWinHeap, dWinKeys, dWinVals, dWinOffH, dWinOffT, dWinCntH, dWinCntT;
  DevBuf dL1, dL1b, dL1Cursors; size_t l1Cap = 0;   // dL1b: the region-filled buffer k_l1_compact reads from
  DevBuf dL1Off;                                        // int64[nFrags] first candidate of a fragment
  DevBuf dL1Regions;                                    // L1Regions: fill count + prefix position of the 64 output regions (k_l1_regions)
  DevBuf dL2; size_t l2Cap = 0;
  DevBuf dL2First, dL2Num;                              // per L1 candidate: first locus in dL2 (int64) and count (int32)
  // candidate mappings (mm_select.hip)
  DevBuf dAccept, dMinIsz; bool haveReplayTables = false;
  DevBuf dSelCnt, dSelOff, dSelHeap, dFragTab, dMappings; bool fragTabStale = true;
  // chaining and filtering on the device (mm_chain.hip): the identity table and parameter block of mm_set_chain_tables; per read the
  // record range, row / left-over counts and their scans; the two output arrays; the four counts of the last mm_chain_reads
  DevBuf dChainIdent, dChainBegin, dChainEnd, dChainCntR, dChainCntL, dChainOffR, dChainOffL, dChainRows, dChainLeft, dChainTotals;
  mm_chain_params chainP{}; bool haveChainTables = false;
  uint64_t chainPass = 0;                               // tot.nPasses when mm_chain_reads last went through: its results belong to that pass (0: none)
  size_t chOffered = 0, chFinished = 0, chRows = 0, chLeft = 0;
  // MM_OPT_CHAIN_LONG: the list of reads with 17 .. 512 records (filled by the count pass), the rows k_chain_reads_long leaves at each
  // read's record offset, and the two counts of mm_chain_long_counts
  DevBuf dChainLongList, dChainStage;
  uint64_t chLongOffered = 0, chLongFinished = 0;
  uint64_t chGroupReads = 0, chGroupRuns = 0;           // mm_chain_group_counts: finished reads with more than one run of filterByGroup, and the runs of all of them
  int chainCUs = 0;                                     // compute units of the device (k_chain_reads_long's grid), asked for once
  // the PAF lines on the device (mm_paf.hip): the tables of mm_set_paf_tables (parameter block, mapQ thresholds and texts, the contigs'
  // names, name offsets and lengths); per call the reads' names and offsets, the rows and read lengths mm_paf_format brings; per row its
  // line's length and offset, per read its flag and its offset; the text and the counts.  The results belong to the batch and the pass
  // they were made in (pafGen, pafPass)
  DevBuf dPafMapqT, dPafMapqText, dPafRefNames, dPafRefOff, dPafRefLens, dPafQNames, dPafQOff, dPafRows, dPafReadLens;
  DevBuf dPafLen, dPafRowOff, dPafFlag, dPafOff, dPafText, dPafTotals;
  mm_paf_params pafP{}; bool havePafTables = false; int32_t pafNMapq = 0; size_t pafNContigs = 0; uint64_t pafRefNameBytes = 0;
  bool pafDone = false; uint64_t pafGen = 0, pafPass = 0; size_t pafReads = 0;
  uint64_t pafBytes = 0, pafLines = 0, pafDropped = 0, pafReadsText = 0, pafHanded = 0;
  uint64_t batchGen = 0;                                // counts the changes of the resident batch (mm_batch_changed)
  // multi-GPU exchange (mm_comm.hip)
  void* comm = nullptr; int commRank = 0, commWorld = 0; bool commCopy = false;   // commCopy: local group whose contexts share a device
  DevBuf dCommCounts, dGathered; std::vector<size_t> gatherCounts, gatherDisp; size_t nGathered = 0; bool gathered = false;
  // overlapped exchange (mm_allgatherv_mappings_begin / _end): a snapshot of the records, a stream of its own, the host thread that
  // runs the exchange while the caller maps the next batch
  DevBuf dGatherSrc; DevStream commStream; std::thread gatherThread; int gatherRc = 0; std::string gatherErr;
  DevBuf dL2Info, dL2Cnt, dL2Off, dL2Ops, dScanTmp, dL2Tmp, dL2Wide, dL2Exact, dL2Cells, dListB, dListC, dBigList, dMidList, dGrpList;     // L2 staging: per-candidate stream extents, op counts/offsets, located ops
  DevBuf dL2InitCells, dL2InitState;                                 // per candidate of a chunk: the SlideMapper state after the pre-load, as k_l2_locate leaves it for the sweeps
  DevBuf dL2Sort[4], dL2Order, dL2OrderPos;                          // candidates of a chunk in order of descending stream length (mm_order_desc)
  bool sketched = false, mapped = false;
  PinnedBuf hPass;                                      // page-locked mirror of dCounters (MM_COUNTER_BYTES, word for word): the parts a pass reads back at its end
  bool refGroupMonotone = true;                         // the index's refGroup array is non-decreasing (checked where it arrives: mm_flatten_device_index; mm_index_replicate carries it)

  // profiling
  bool profile = false;
  double kMs[MM_K_COUNT] = {0};
  uint64_t kLaunches[MM_K_COUNT] = {0};
  DevEvent evA, evB;                                    // mm_bench_hash_only's own pair
  std::vector<std::pair<DevEvent, DevEvent>> evPool; size_t evUsed = 0;       // KernelTimer brackets recorded since the last mm_profile_collect
  std::vector<std::pair<int, size_t>> evPending;                              // (kernel, pool index)
};

const char* mm_inflate_take_error(const mm_ctx* c);     // mm_inflate.hip: the text of this thread's failed mm_inflate_blocks / mm_text_* on c, once; else null
void mm_inflate_keep_error(const mm_ctx* c, InflateErr& e, int rc);   // rc != MM_OK: e's text becomes this thread's for c; MM_OK: forgets it
int mm_inflate_run(mm_ctx* c, InflateErr* e, const void* comp, size_t nComp, mm_inflate_block* blocks, size_t nBlocks, void* dst, size_t nDst, size_t* nBad, uint8_t* devOut);
// the staging area of packed pieces (mm_api.hip; prefetchMu held): the area sized and stage.ring.next the place of a piece of nPackedBases
// -- *fits = false: no room under the pieces on their way -- and its entry once its words are on their way there (copyDone recorded behind them)
int mm_stage_place(mm_ctx* c, size_t nPackedBases, size_t reservePackedBases, bool* fits);
void mm_stage_commit(mm_ctx* c, const uint32_t* bases2, const uint32_t* nmask, size_t nPackedBases);
// the resident batch changed (an upload, an exchange): nothing sketched, mapped or gathered belongs to it
inline void mm_batch_changed(mm_ctx* c) { c->sketched = false; c->mapped = false; c->fragTabStale = true; c->gathered = false; c->batchGen++; }

#define MM_HIP(ctx, call)                                                                        \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                           \
      return MM_ERR_DEVICE;                                                                      \
    }                                                                                            \
  } while (0)
inline int DeviceInput::ready(int device, InflateErr* e) {
  MM_HIP(e, hipSetDevice(device));
  MM_HIP(e, inflateStream.ensure());
  return MM_OK;
}
// an entry point of mm_inflate.hip / mm_text.hip: body(InflateErr*) runs under inflateMu, and its error text is kept for the calling thread
template <class F>
int mm_input_call(mm_ctx* c, F&& body) {
  if (!c) return MM_ERR_ARG;
  InflateErr e;
  std::lock_guard<std::mutex> lock(c->input.inflateMu);
  const int rc = body(&e);
  mm_inflate_keep_error(c, e, rc);
  return rc;
}
// a host synchronisation of a mapping pass: counted (mm_pass_syncs)
#define MM_SYNC(c) do { MM_HIP(c, hipStreamSynchronize((c)->stream)); (c)->rep.nSyncs++; } while (0)

// RAII hipEvent bracket on the ctx stream.  The two events are only RECORDED here (a pair out of a pool that grows with the number of
// brackets in flight); their times are read by mm_profile_collect once the stream has been synchronised anyway -- measuring a pass does
// not add host waits to it (a steady-state pass stays at its one synchronisation with the per-kernel timers on).
struct KernelTimer {
  mm_ctx* c; int which; size_t idx = 0; bool on = false;
  KernelTimer(mm_ctx* c_, int w) : c(c_), which(w) {
    if (!c->profile) return;
    if (c->evUsed == c->evPool.size()) {
      // the pool is recycled by mm_profile_collect (every profiled entry point that synchronises calls it); a caller that records
      // thousands of brackets without one gets no more events than this, and a failing event creation switches the timers off
      if (c->evPool.size() >= 8192) return;
      std::pair<DevEvent, DevEvent> pr;
      if (pr.first.ensure() != hipSuccess || pr.second.ensure() != hipSuccess) { c->profile = false; return; }
      c->evPool.push_back(std::move(pr));
    }
    idx = c->evUsed++;
    on = hipEventRecord(c->evPool[idx].first, c->stream) == hipSuccess;
  }
  ~KernelTimer() {
    if (!on) return;
    if (hipEventRecord(c->evPool[idx].second, c->stream) == hipSuccess) c->evPending.emplace_back(which, idx);
  }
};
// adds the recorded brackets to kMs / kLaunches; the stream must have been synchronised behind them
inline void mm_profile_collect(mm_ctx* c) {
  for (const auto& pr : c->evPending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->evPool[pr.second].first, c->evPool[pr.second].second) == hipSuccess) { c->kMs[pr.first] += ms; c->kLaunches[pr.first] += 1; }
  }
  c->evPending.clear(); c->evUsed = 0;
}

// MM_OPT_RESERVE_FRAGMENTS: a sized pass over a small batch sizes every staging buffer for the largest batch the caller has announced, so
// that the larger batches behind it are steady-state passes instead of being sized (and their buffers reallocated) again.
//   mm_frag_cap: fragments to size per-fragment buffers for;  mm_scaled: a count of this pass scaled to what the announced batch would bring
inline size_t mm_frag_cap(const mm_ctx* c, size_t nF) { return mm_frag_cap(c->opt, nF); }
// A scaled count never claims more than an eighth of the device memory that is free when it is asked for (`bytesPer` = bytes the buffer
// holds per counted item): the scaling is a convenience for the passes behind this one -- a repeat-rich first batch must not turn a pass
// that fits into an out-of-memory error; a later, larger batch that outgrows the clamped buffer is redone the sized way, as without scaling.
inline size_t mm_scaled(const mm_ctx* c, size_t count, size_t bytesPer) {
  const size_t nF = c->nFrags ? c->nFrags : 1;
  if (c->opt.reserveFrags <= nF) return count;
  size_t scaled = (size_t)((double)count * (double)c->opt.reserveFrags / (double)nF) + 1;
  size_t freeB = 0, totalB = 0;
  if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); return count; }
  const size_t most = freeB / 8 / (bytesPer ? bytesPer : 1);
  if (scaled > most) scaled = most > count ? most : count;
  return scaled;
}

// launchers implemented in the .hip files
int mm_check_params(const mm_params* p, std::string& err);
int mm_launch_pack(mm_ctx* c);
int mm_launch_pack_raw(mm_ctx* c, const uint8_t* dAscii, const int64_t* dSrcOff, const int64_t* dPackOff, const int32_t* dLen, int nReads,
                       int64_t nChunks, uint32_t* dB, uint32_t* dM, uint32_t* dHasN);
int mm_launch_sketch(mm_ctx* c);
int mm_launch_sketch_global(mm_ctx* c);   // mm_sketch_global.hip: sketches no LDS table holds (sketchSize > MM_LDS_MAX_SKETCH)
int mm_launch_sketch_large(mm_ctx* c);    // mm_sketch_large.hip: the same sketches under MM_OPT_SKETCH_LARGE (strip hashers, LDS tiles)
enum : int { MM_SKL_STATE_NONE = 0, MM_SKL_STATE_KNOWN = 1, MM_SKL_STATE_PENDING = 2 };   // mm_ctx::skLargeState: no sketch launch yet / counts on the host / their copy in flight
// (MM_LDS_MAX_SKETCH, beyond which the global-memory sketch kernel and the literal L2 kernels take over: mm_pass_state.h)
#define MM_WINNOW_LDS_SKETCH 4096          // the device index build keeps a window's sketch as one sorted array in LDS up to here (k_winnow_tiles: an insert shifts half of it), and as
                                           // blocks of 64 entries in HBM under an LDS directory beyond (k_winnow_tiles<.., GSK>: 0.7 s against 8.7 s of index build at sketchSize 9 998,
                                           // profiles/r14_11; LDS itself would hold 10 000 entries)
#define MM_MAX_SKETCH 65535                // seeds are numbered in 16 bits where the literal kernels count windows per seed (mm_map.hip: ptIds); the reference takes any size
int mm_launch_map(mm_ctx* c);
// Steady state: once a pass of a context has sized every staging buffer, the next passes launch everything against
// those capacities with the counts left on the device and read ONE block of counters back at the end (one host synchronisation per
// pass); a pass that outgrows a buffer is detected there and redone the sized way (MM_PASS_REDO from the launchers).
#define MM_PASS_REDO 1
int mm_launch_select(mm_ctx* c, bool steady = false);
void mm_comm_release(mm_ctx* c);
int mm_launch_l2(mm_ctx* c, unsigned long long* cnt, bool steady = false);   // cnt: dCounters + MM_CW_PASS (MM_PC_*)
int mm_build_device_index(mm_ctx* c, const int32_t* contigLen, const int32_t* refGroup, size_t nContigs);   // from the host mirrors
int mm_flatten_device_index(mm_ctx* c, const mm_minmer* dRec, size_t n, size_t nk, size_t np, const int32_t* contigLen, const int32_t* refGroup, size_t nContigs);
int mm_finalize_index_device(mm_ctx* c, const std::vector<std::pair<const mm_minmer*, size_t>>& parts, float kmerPctThreshold, const int32_t* contigLen,
                             const int32_t* refGroup, size_t nContigs);
int mm_mirror_minmers(mm_ctx* c);
int mm_mirror_map(mm_ctx* c);
int mm_scan_i32_to_i64(mm_ctx* c, int64_t n, const int32_t* dIn, int64_t* dOut, int64_t* total);
int mm_scan_i32_to_i64_dev(mm_ctx* c, int64_t n, const int32_t* dIn, int64_t* dOut, const int64_t** dTotal);   // the total stays on the device: no synchronisation
int mm_order_desc(mm_ctx* c, const int32_t* dKey, int c0, int n, int shift, int32_t* dOrder);   // mm_index_dev.hip (rocPRIM radix sort)
int mm_order_pairs(mm_ctx* c, int n, unsigned bits, int32_t* dOrder);                          // same file: pairs already in dL2Sort[0] / dL2Sort[2]
