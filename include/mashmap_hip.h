/*
 * include/mashmap_hip.h -- C ABI of libmashmap_hip.so: MashMap's sketch + L1/L2 hot path as
 * hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (marbl/MashMap v3.1.3) has no FFI: its boundary is the two C++ classes main()
 * constructs (src/map/mash_map.cpp:43,51) and the free functions they call.  Every entry point
 * below names the reference interface it stands in for (file:line relative to the reference
 * tree).  Plain pointers and sizes only; the library owns all device memory; the caller owns
 * every host buffer.  All functions return 0 on success or a negative MM_ERR_* code
 * (mm_last_error() gives the text); nothing here ever falls back to a CPU implementation --
 * if no gfx950 device / kernel image is available mm_create() fails.
 *
 * Thread model: one mm_ctx per GPU (one process per GPU in multi-GPU runs); a ctx is
 * thread-compatible, not thread-safe; all work of a ctx is ordered on its own HIP stream.
 */
#ifndef MASHMAP_HIP_H
#define MASHMAP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_ABI_VERSION 2     /* 2: mm_pass_stats writes 5 counts; mm_reads_prefetch_packed_append reports whether it staged; mm_reads_prefetch_drop */

enum {
  MM_OK = 0,
  MM_ERR_ARG = -1,        /* bad argument / unsupported parameter combination */
  MM_ERR_DEVICE = -2,     /* HIP runtime error (no device, launch failure, out of memory ...) */
  MM_ERR_STATE = -3,      /* call sequence violated (e.g. map before index upload) */
  MM_ERR_CAPACITY = -4    /* an internal device buffer overflowed and could not be grown */
};

/* skch::Parameters fields the hot path reads (map_parameters.hpp:32-80) */
enum {
  MM_FLAG_HG_FILTER = 1,        /* stage1_topANI_filter   (parseCmdArgs.hpp:397) */
  MM_FLAG_SKIP_SELF = 2,        /* skip_self              (parseCmdArgs.hpp:341) */
  MM_FLAG_SKIP_PREFIX = 4,      /* skip_prefix            (parseCmdArgs.hpp:349): L1 runs once per run of interval points whose contigs share a
                                   reference group (computeMap.hpp:1146-1165).  Every fragment's points go through HBM (gather, sort), every
                                   pass is a sized pass, and the L1 stage is the literal one-thread-per-fragment kernel for every queued
                                   fragment (mm_pass_l1_literal: literal == queued) unless MM_OPT_L1_GROUP_STREAM.  With
                                   MM_OPT_L1_GROUP_FUSED the queued fragments first go to a wave-per-fragment kernel that keeps their points
                                   out of HBM; the path above is then left with what that kernel hands over. */
  MM_FLAG_LOWER_TRIANGULAR = 8, /* lower_triangular       (parseCmdArgs.hpp:334) */
  MM_FLAG_NO_SPLIT = 16         /* !split                 (parseCmdArgs.hpp:427): a read longer than segLength is then ONE fragment with
                                   windowLen = len - segLength != 0 (computeMap.hpp:933, :1309); a batch that holds such a read goes through
                                   the literal kernels (k_l1_window, k_l2_window: exact, not fast; MM_OPT_L2_WINDOW_WAVE puts the L2 stage on
                                   a wave per candidate first).  A read of any length: one that does not
                                   fit a CU's LDS (a whole contig as a read) is sketched by the exact kernel from global memory. */
};

typedef struct {
  int32_t kmerSize;       /* Parameters::kmerSize   (1..64; 16..32 take the tuned strip hasher, 19 -- the reference's default -- the tuned tail as well) */
  int32_t segLength;      /* Parameters::segLength  */
  int32_t sketchSize;     /* Parameters::sketchSize (1 .. 65535.  Up to 8190 the sketch and L2 kernels keep their state in a CU's 160 KB of LDS -- mm_create
                             checks the combination with segLength and says what does not fit --; beyond, every fragment takes a global-memory sketch
                             kernel and the literal L2 kernels, and the index build keeps a window's sketch in HBM from 4097 on: exact, not tuned;
                             MM_OPT_L2_LARGE_WAVE puts the L2 stage of such a batch on a wave per candidate first, up to 20460) */
  int32_t flags;          /* MM_FLAG_* */
} mm_params;

/* bit-for-bit skch::MinmerInfo (base_types.hpp:31; 24 bytes) */
typedef struct { uint64_t hash; int32_t wpos, wpos_end, seqId; int16_t strand; int16_t pad_; } mm_minmer;
/* bit-for-bit skch::IntervalPoint (base_types.hpp:66; 24 bytes) */
typedef struct { int32_t pos; int32_t pad0_; uint64_t hash; int32_t seqId; int8_t side; int8_t pad1_[3]; } mm_interval_point;

/* one query fragment, as Map::mapModule cuts them (computeMap.hpp:587-671) */
typedef struct {
  int32_t readId;         /* index of the read in the uploaded batch (InputSeqContainer::seqCounter - first) */
  int32_t fragStart;      /* offset of the fragment inside the read == MappingResult::queryStartPos */
  int32_t len;            /* QueryMetaData::len */
  int32_t pad_;
} mm_fragment;

/* per-fragment integers behind QueryMetaData (base_types.hpp:265) after getSeedHits (computeMap.hpp:818) */
typedef struct {
  int32_t rawSketchSize;  /* |minmerTableQuery| before frequent-seed removal (feeds kmerComplexity, :830) */
  int32_t sketchSize;     /* Q.sketchSize (:839) */
  uint64_t maxHash;       /* minmerTableQuery.back().hash before removal (:830) */
  int32_t nPoints;        /* interval points that survived the seqId filters (:891-896) */
  int32_t nL1;            /* L1 candidates (:916) */
} mm_frag_stats;

/* Map::L1_candidateLocus_t (computeMap.hpp:58) + owning fragment */
typedef struct { int32_t frag; int32_t seqId, rangeStartPos, rangeEndPos, intersectionSize; } mm_l1_candidate;
/* Map::L2_mapLocus_t (computeMap.hpp:76) + owning fragment / candidate.  `cand` as returned by mm_results_download is the index
 * into the L1 array downloaded with it.  In the DEVICE-resident records (mm_results_device / mm_results_copy_device) `cand` is the
 * candidate's rank among the candidates of its own fragment (0 .. stats[frag].nL1-1), and records are grouped by candidate but
 * not sorted by fragment. */
typedef struct {
  int32_t frag, cand;
  int32_t seqId, meanOptimalPos, optimalStart, optimalEnd, sharedSketchSize, strand;
} mm_l2_locus;

/*
 * A candidate mapping: one L2 locus that doL2Mapping reports for a fragment (computeMap.hpp:1221-1250), in integers.  The floats of
 * MappingResult (base_types.hpp:154) are functions of these: nucIdentity / nucIdentityUpperBound of (conservedSketches, sketchSize, k)
 * (map_stats.hpp:45,81), kmerComplexity of (rawSketchSize, maxHash, fragLen, k) (computeMap.hpp:830-831).  This is the record the
 * host side chains and filters, and the record multi-GPU runs exchange (mm_allgatherv_mappings).  48 bytes.
 */
typedef struct {
  int32_t querySeqId;          /* MappingResult::querySeqId == seqCounterBase + index of the read in the batch */
  int32_t fragStart, fragLen;  /* offset of the fragment in the read (queryStartPos after :632-636), Q.len */
  int32_t refSeqId, refStartPos;          /* L2_mapLocus_t::seqId, meanOptimalPos */
  int32_t conservedSketches, sketchSize;  /* sharedSketchSize, Q.sketchSize */
  int32_t strand;
  int32_t rawSketchSize, pad_;
  uint64_t maxHash;
} mm_mapping;

typedef struct mm_ctx mm_ctx;

/* ------------------------------------------------------------------------------------------ */
int  mm_abi_version(void);
/* creates the context on HIP device `device`; fails (MM_ERR_DEVICE) when there is none */
int  mm_create(mm_ctx** out, int device, const mm_params* params);
void mm_destroy(mm_ctx* ctx);
const char* mm_last_error(const mm_ctx* ctx);   /* ctx may be NULL for mm_create failures */

/*
 * Reference index -> device.  Stands in for how Map reads `const skch::Sketch&`:
 *   minmerIndex            (winSketch.hpp:102; read by computeL2MappedRegions, computeMap.hpp:1284-1340)
 *   minmerPosLookupIndex   (winSketch.hpp:101; read by getSeedIntervalPoints, computeMap.hpp:878)
 *   isFreqSeed()           (winSketch.hpp:506; read by getSeedHits, computeMap.hpp:835)
 *   metadata[i].len        (winSketch.hpp:79)
 * `minmers` is minmerIndex *after* dropFreqSeedSet (:497).  The lookup map is passed flattened:
 * keys[i] owns points[offsets[i] .. offsets[i+1]) in the map's own per-key order.
 * refGroup[i] is Map::refIdGroup (computeMap.hpp:113), or NULL when skip_prefix is off.
 */
int mm_index_upload(mm_ctx* ctx,
                    const mm_minmer* minmers, size_t nMinmers,
                    const uint64_t* keys, const uint64_t* offsets, size_t nKeys,
                    const mm_interval_point* points, size_t nPoints,
                    const uint64_t* freqSeeds, size_t nFreq,
                    const int32_t* contigLen, const int32_t* refGroup, size_t nContigs);

/*
 * Host-computed integer tables (they depend on GSL-class floating point, kept on the host):
 *   minHits[q]      = Stat::estimateMinimumHitsRelaxed(q, k, pi, 0.95), q = 0..sketchSize   (computeMap.hpp:1144)
 *   sketchCutoffs[] = Map::sketchCutoffs (computeMap.hpp:109,178-258), nCutoffs entries
 */
int mm_set_tables(mm_ctx* ctx, const int32_t* minHits, size_t nMinHits, const int32_t* sketchCutoffs, size_t nCutoffs);

/*
 * Integer tables for the best-first walk of doL2Mapping (computeMap.hpp:1182-1267) on the device, stride = sketchSize + 1:
 *   accept[Qs*stride + shared] = 1 iff a locus sharing `shared` of Qs sketch elements is reported  (:1221: identity or, with
 *                                keep_low_pct_id, its upper bound reaches percentageIdentity)
 *   minIsz[Qs*stride + best]   = smallest L1 intersectionSize that passes the ANI cut-off (:1192-1202) when the best reported
 *                                locus so far shares `best` elements
 * (mashmap_amd/host/mm_stats.hpp: mmhost::replayTables fills them with the reference's own float expressions.)  Without them
 * mm_map_fragments stops at the L2 loci and the mm_mappings_* calls fail with MM_ERR_STATE.
 */
int mm_set_replay_tables(mm_ctx* ctx, const uint8_t* accept, const int16_t* minIsz, size_t stride);

/* all three tables computed inside the library (mashmap_amd/host/mm_stats.hpp mirrors skch::Stat and Map::setProbs) with the
 * reference's defaults (ANIDiff 0, ANIDiffConf 0.999, keep_low_pct_id on) and uploaded */
int mm_set_tables_default(mm_ctx* ctx, float percentageIdentity);

/*
 * Host-side statistics (no device needed) -- mirrors of skch::Stat (map_stats.hpp:45-262), exported so
 * that parity tests and the C++ host side share one implementation:
 *   j2md :45, md2j :63, md_lower_bound :81, estimateMinimumHitsRelaxed :144 (ci = 0.95),
 *   recommendedSketchSize :234 (p-value 1e-3, ci 0.95, alphabet 4), Map::sketchCutoffs (computeMap.hpp:178-258)
 */
float   mm_stat_j2md(float j, int k);
float   mm_stat_md2j(float d, int k);
float   mm_stat_md_lower_bound(float d, int s, int k, float ci);
int     mm_stat_min_hits_relaxed(int s, int k, float percentageIdentity);
int64_t mm_stat_recommended_sketch_size(int k, float percentageIdentity, int64_t segLength, uint64_t referenceSize);
int     mm_stat_sketch_cutoffs(int sketchSize, int k, int hgFilter, int32_t* out, size_t cap);   /* returns entries written */
/* the tables of mm_set_replay_tables, (sketchSize+1)^2 entries each, from the reference's own float expressions (computeMap.hpp:1192-1222) */
int     mm_stat_replay_tables(int sketchSize, int k, float percentageIdentity, float ANIDiff, int keepLowPctId, uint8_t* accept, int16_t* minIsz);

/*
 * A batch of query reads -> device.  Replaces the `char* seq` handed to sketchSequence
 * (commonFunc.hpp:183): ASCII in, normalised (makeUpperCaseAndValidDNA, :97) and packed to
 * 2 bit/base + N mask on the device.  readOffsets has nReads+1 entries into `bases`.
 * Fragments are cut exactly as mapModule does (computeMap.hpp:587-671).
 * readRefGroup[r] = Map::getRefGroup(name) (computeMap.hpp:164) or NULL;
 * readSelfSeqId[r] = reference seqId whose name equals the read's name, -1 if none, or NULL
 * (this is what the skip_self test `Q.seqName != ref.name` needs, computeMap.hpp:891);
 * seqCounterBase = seqCounter of read 0 (lower_triangular compares seqCounter with seqId, :893).
 */
int mm_reads_upload(mm_ctx* ctx, const char* bases, const int64_t* readOffsets, size_t nReads,
                    const int32_t* readRefGroup, const int32_t* readSelfSeqId, int32_t seqCounterBase);
/* Optional: start the host-to-device copy of the ASCII bytes the NEXT mm_reads_upload will name -- [bases, bases + nBytes) must be exactly
 * the range that call reads, i.e. its `bases + readOffsets[0]` and `readOffsets[nReads] - readOffsets[0]` -- on a stream of the context's
 * own, so that it runs under the kernels of the batch being mapped (call it between mm_reads_upload and mm_map_fragments of the current
 * batch).  mm_reads_upload recognises the range and skips its own copy; any other upload simply discards the prefetch.  The bytes must
 * stay unchanged until that upload returns, and should be page-locked (mm_host_alloc): a copy from pageable memory does not overlap.
 * The two prefetch calls are the one exception to "a ctx is thread-compatible": they may come from another thread (a reader) while the
 * context's own thread is inside any other call; against mm_reads_upload* of the same context they are serialised inside the library. */
int mm_reads_prefetch(mm_ctx* ctx, const char* bases, size_t nBytes);
/* page-locked host memory for the `bases` of mm_reads_upload / mm_index_build: the copy to the GPU is then a single DMA at PCIe rate
 * (pageable memory is staged through a bounce buffer at a fraction of it).  Optional: any host pointer works. */
void* mm_host_alloc(size_t bytes);
void  mm_host_free(void* p);
/* same, from already device-resident ASCII (hipMalloc'ed by the caller, e.g. a torch tensor).  The bytes are read on the context's own
 * stream (mm_stream): work of the caller's stream that produces them must have completed before the call. */
int mm_reads_upload_device(mm_ctx* ctx, const void* dBases, size_t nBases, const int64_t* readOffsets, size_t nReads,
                           const int32_t* readRefGroup, const int32_t* readSelfSeqId, int32_t seqCounterBase);
/*
 * The same batch for a caller that has normalised and packed the reads itself (the layout k_pack2bit produces on the device, DESIGN.md
 * section 2): PCIe then carries 0.375 bytes per base instead of 1.  Read r has readLengths[r] bases and starts at packed base
 * P(r) = sum over earlier reads of ceil(len / 32) * 32 -- or, with readStarts != NULL, at P(r) = readStarts[r] - readStarts[0]: ascending
 * multiples of 32 with P(r+1) >= P(r) + ceil(len / 32) * 32, i.e. gaps between reads are allowed (a parser whose threads pack their
 * pieces of a file independently leaves one between pieces; the words of a gap travel with the rest and are never read as bases).
 * P(nReads) is the end of the last read:
 *   bases2  2 bit/base, A0 C1 G2 T3 (the code of an N is 0), sixteen bases per uint32, first base in the low bits; read r owns the words
 *           [P(r) / 16, P(r+1) / 16), bases behind its end are 0
 *   nmask   1 bit/base, set where makeUpperCaseAndValidDNA (commonFunc.hpp:97) leaves an 'N' (anything but A C G T a c g t); read r owns
 *           the words [P(r) / 32, P(r+1) / 32)
 *   readHasN[r] != 0 iff any mask bit of read r is set; NULL: derived from nmask here
 * mm_pack_read produces the words of one read on the host (AVX2 + BMI2 when the CPU has them; mm_pack_read_portable is the plain loop,
 * same result): 2 * ceil(len / 32) code words and ceil(len / 32) mask words; returns the number of N bases.
 * mm_reads_prefetch_packed is mm_reads_prefetch for the next mm_reads_upload_packed (same two pointers, nPackedBases = P(nReads)).
 * mm_reads_packed_download returns the resident packed batch of any upload (parity tests); any pointer may be NULL.
 */
int mm_reads_upload_packed(mm_ctx* ctx, const uint32_t* bases2, const uint32_t* nmask, const uint8_t* readHasN, const int32_t* readLengths,
                           const int64_t* readStarts, size_t nReads, const int32_t* readRefGroup, const int32_t* readSelfSeqId, int32_t seqCounterBase);
int mm_reads_prefetch_packed(mm_ctx* ctx, const uint32_t* bases2, const uint32_t* nmask, size_t nPackedBases);
/*
 * One resident batch out of several packed pieces.  A reader that hands over its input in pieces of a fixed size (one page-locked buffer
 * each: skch::Map's 512 Mbp) can have several of them mapped by ONE pass -- the kernels of a pass fill the GPU only from a few Gbp
 * on -- without ever holding them in one host buffer: part p is exactly what one mm_reads_upload_packed call takes, the parts are laid
 * end to end in HBM and their reads numbered consecutively (read r of part p has readId = reads of the parts before it + r).
 * mm_reads_prefetch_packed_append is mm_reads_prefetch_packed that ADDS a piece to what has been sent ahead instead of replacing it
 * (same thread exception): the upload takes every part it finds staged from there and copies the others itself; staged pieces an upload
 * does not name stay staged for the next one.  reservePackedBases: packed bases the staging area should hold when it has to be
 * (re)allocated -- it can only grow while nothing is staged; a piece that does not fit is simply not staged: *staged (may be NULL)
 * says which happened, and a piece that was declined travels with its upload.
 * A staged piece is recognised by its two host pointers and its packed length: between the call that stages it and the upload that names
 * it (or mm_reads_prefetch_drop) the host words must neither change nor be handed to another batch -- a caller that recycles page-locked
 * buffers gives a buffer back only after the upload of its batch has returned (skch::Map does), or drops what it staged.  An ASCII upload
 * (mm_reads_upload / _device) and mm_reads_prefetch / mm_reads_prefetch_packed drop every staged piece; mm_reads_prefetch_drop does
 * nothing else.
 */
typedef struct {
  const uint32_t* bases2; const uint32_t* nmask; const uint8_t* readHasN; const int32_t* readLengths; const int64_t* readStarts;
  size_t nReads; const int32_t* readRefGroup; const int32_t* readSelfSeqId;
} mm_packed_part;
int mm_reads_upload_packed_parts(mm_ctx* ctx, const mm_packed_part* parts, size_t nParts, int32_t seqCounterBase);
int mm_reads_prefetch_packed_append(mm_ctx* ctx, const uint32_t* bases2, const uint32_t* nmask, size_t nPackedBases, size_t reservePackedBases, int* staged);
int mm_reads_prefetch_drop(mm_ctx* ctx);
/* allocates the staging area (and the copy stream) for reservePackedBases ahead of the first piece, e.g. while the index is being built:
 * the first mm_reads_prefetch_packed_append then does not stop for a multi-gigabyte hipMalloc.  Only while nothing is staged. */
int mm_reads_prefetch_reserve(mm_ctx* ctx, size_t reservePackedBases);
size_t mm_pack_read(const char* ascii, size_t len, uint32_t* bases2, uint32_t* nmask);
size_t mm_pack_read_portable(const char* ascii, size_t len, uint32_t* bases2, uint32_t* nmask);
int mm_reads_packed_download(mm_ctx* ctx, uint32_t* bases2, uint32_t* nmask, uint32_t* readHasN, size_t* nPackedBases);
/*
 * Batch slots.  A context maps its RESIDENT batch (what the last mm_reads_upload* left); beside it, it can hold MM_BATCH_SLOTS parked
 * batches.  mm_reads_exchange swaps the resident batch with the one in `slot` -- either may be empty; device pointers change hands, nothing
 * is copied -- so that several uploaded batches stay in HBM and take turns (bench.py rotates three; a caller that maps a batch twice with
 * something else in between).  Results of the previous mm_map_fragments belong to the batch that was resident then and are gone after
 * the swap (an overlapped exchange works on its own snapshot of the records and is not affected); the context's staging buffers keep
 * their sizes, so the next pass is a steady-state pass if the incoming batch fits them and is redone the sized way if not
 * (mm_pass_totals counts both).
 */
#define MM_BATCH_SLOTS 4
int mm_reads_exchange(mm_ctx* ctx, int slot);
size_t mm_num_fragments(const mm_ctx* ctx);
int mm_fragments_download(mm_ctx* ctx, mm_fragment* out);

/* a4: CommonFunc::sketchSequence for every resident fragment (commonFunc.hpp:183) */
int mm_sketch_fragments(mm_ctx* ctx);
/* raw sketches (before frequent-seed removal): out[f*sketchSize + r], counts[f]; seqId := readId+seqCounterBase */
int mm_sketch_download(mm_ctx* ctx, mm_minmer* out, uint32_t* counts);

/*
 * The whole hot path for every resident fragment: sketch (a4) -> getSeedHits (a8) ->
 * getSeedIntervalPoints (a9) -> computeL1CandidateRegions (a10) -> computeL2MappedRegions for
 * every L1 candidate (a13) -> doL2Mapping's best-first walk with its early exit and acceptance test
 * (a12, :1182-1267; k_l2_select on the integer tables of mm_set_replay_tables) -> candidate mappings (mm_mapping).
 * Equivalent of the integer part of Map::mapSingleQueryFrag (computeMap.hpp:756); only the floats of MappingResult
 * (identity, upper bound, complexity) are host work on these integers.  Results stay on the device until downloaded.
 */
int mm_map_fragments(mm_ctx* ctx);
/* How the last mm_map_fragments went: the number of times the host waited for the device inside it, and whether it was a steady-state
 * pass -- the first pass of a context sizes every staging buffer from counts it reads back stage by stage (5-7 waits); the passes behind
 * it launch against those capacities with the counts left on the device and wait once, at the end.  A pass that outgrows a buffer is
 * redone the sized way (and counted as such here).  counts (FIVE entries since MM_ABI_VERSION 2 -- the caller's array holds at least 5 --, may be NULL): L1 candidates, L2 loci, fragments whose interval
 * points went through HBM (more than the fused kernel holds; as of the last sized pass), entries reserved for the L2 streams (one per
 * index event a candidate touches: what k_l2_locate reads 16 bytes for and k_l2_sweep at most 4), fragments the fast sketch kernel handed to
 * the exact one (the hard list: fewer than sketchSize distinct survivors below the cut, or an LDS structure overflowed). */
int mm_pass_stats(const mm_ctx* ctx, uint64_t* hostSyncs, int* steady, uint64_t* counts);
/* The context's mm_map_fragments calls so far: all of them, those that went through as steady-state passes (one host wait), and the
 * steady-state attempts that outgrew a buffer and were redone the sized way.  Any pointer may be NULL. */
int mm_pass_totals(const mm_ctx* ctx, uint64_t* passes, uint64_t* steadyPasses, uint64_t* redonePasses);
/* Why the last mm_map_fragments had its steady-state attempt redone the sized way: *cause = MM_REDO_* bits, taken from the one counter
 * block that attempt read back (nothing more is read or waited for); 0 when the last mm_map_fragments went through as a steady-state
 * pass or made no steady-state attempt.  A stage that overflows silences the stages behind it, so the bits name the FIRST stages that
 * ran out of room, not everything the sized pass then had to grow. */
enum {
  MM_REDO_POINTS    = 1,    /* the interval-point buffer of the HBM point path */
  MM_REDO_L1        = 2,    /* the L1 candidate buffer (one of its output regions, or the dense buffer behind them), or more candidates
                               than the staging behind L1 holds: the gate between the two stages raises this bit for that as well */
  MM_REDO_L2_LOCI   = 4,    /* the L2 locus buffer */
  MM_REDO_L2_SLOTS  = 8,    /* a candidate with more tied loci than the staging slots per candidate */
  MM_REDO_L2_STREAM = 16,   /* internal error: an L2 stream outgrew the reservation made for it (never expected) */
  MM_REDO_L2_OPS    = 32,   /* the L2 streams do not fit their buffer as the last sized pass left it */
  MM_REDO_L2_LIST   = 64,   /* more candidates for the 16-bit-cell re-run or the exact L2 kernel than their launches cover */
  MM_REDO_L2_CANDS  = 128,  /* more L1 candidates than the candidate-indexed buffers hold (a second line behind the gate: MM_REDO_L1 comes first) */
  MM_REDO_MAPPINGS  = 256,  /* more candidate mappings than their buffer holds */
  MM_REDO_NO_STREAM_BUFFER = 512   /* there is no L2 stream buffer yet (the attempt ended before its counters were read).  Not reachable
                                      today: an attempt needs a sized pass with candidates before it, and that pass allocates the buffer */
};
int mm_pass_redo_cause(const mm_ctx* ctx, uint64_t* cause);
/* Which L1 kernel took the fragments of the HBM point path, as of the context's last SIZED pass (a steady-state pass leaves both figures
 * as they were): *queued = fragments queued for that path, *literal = those of them the literal one-thread-per-fragment kernel
 * (k_l1_sweep) swept -- every one of them (a batch with a read longer than segLength excepted: 0, k_l1_window takes those) under MM_L1_LITERAL
 * or MM_FLAG_SKIP_PREFIX unless MM_OPT_L1_GROUP_STREAM, otherwise what the wave-per-fragment kernel (k_l1_stream) leaves: a position
 * group across two contigs (of one reference-group extent, in its grouped form) or minimumHits <= 0.  Read back with the words the sized pass reads behind the L1 sweeps anyway: no host wait
 * more.  Either pointer may be NULL.  Purely additive: MM_ABI_VERSION stays 2.  In a pass that ran k_lookup_groups (MM_OPT_L1_GROUP_FUSED)
 * the HBM point path holds only what that kernel handed over: *queued equals offered - fused of mm_pass_l1_group_fused. */
int mm_pass_l1_literal(const mm_ctx* ctx, uint64_t* queued, uint64_t* literal);
/* *mid = fragments k_lookup_l1 passed to k_lookup_mid in the context's last SIZED pass, finished there or handed on to the HBM point path (0 where it did not run). */
int mm_pass_l1_mid(const mm_ctx* ctx, uint64_t* mid);
/* Which L2 kernel took the candidates of a batch with a read longer than segLength (MM_FLAG_NO_SPLIT, windowLen != 0), as of the context's
 * last SIZED pass: *candidates = L1 candidates the windowed L2 stage took, *literal = those of them the literal one-thread-per-candidate
 * kernel (k_l2_window) swept -- every one without MM_OPT_L2_WINDOW_WAVE, otherwise the ones the wave-per-candidate kernel hands over: more
 * open records at once than its LDS heap holds (2048), more than 9 tied loci at the best shared count.  0 / 0 for a batch without such a
 * read.  Read back with the words the stage reads anyway: no host wait more.  Either pointer may be NULL.  Purely additive:
 * MM_ABI_VERSION stays 2. */
int mm_pass_l2_window(const mm_ctx* ctx, uint64_t* candidates, uint64_t* literal);
/* Which L2 kernel took the candidates of a SPLIT batch (no read longer than segLength) that went the literal L2 route -- sketchSize above
 * 8190, or bit 1 of MM_OPT_L2_LARGE_WAVE --, as of the context's last SIZED pass: *candidates = L1 candidates the route took, *literal =
 * those of them the literal one-thread-per-candidate kernel (k_l2_window) swept -- every one without bit 0 of the option or with sketchSize
 * above 20460, otherwise the ones k_l2_large_wave handed over: more than 9 tied loci at the best shared count.  0 / 0 for a batch with a read
 * longer than segLength or one that took the fast kernels.  Read back with the words the stage reads anyway: no host wait more.  Either
 * pointer may be NULL.  Purely additive: MM_ABI_VERSION stays 2. */
int mm_pass_l2_large(const mm_ctx* ctx, uint64_t* candidates, uint64_t* literal);
/* MM_OPT_SKETCH_LARGE, as of the context's last sketch launch (mm_sketch_fragments, or the one inside mm_map_fragments): *fragments =
 * fragments k_sketch_large sketched -- 0 without the option or at sketchSize <= 8190 --, *uncut = those of them whose final sort ran
 * without a cut: a fragment with no more k-mer positions than the s + 5 sqrt(s) + 64 hashes the cut aims for, or one with fewer than s
 * distinct hashes below the cut, which the kernel does again without one.  The kernel's two counts are copied to the host right behind
 * it; this call waits for that copy if it is still in flight, mm_map_fragments never does.  Either pointer may be NULL.  MM_ERR_STATE
 * before the context's first sketch launch.  Purely additive: MM_ABI_VERSION stays 2. */
int mm_sketch_large_counts(mm_ctx* ctx, uint64_t* fragments, uint64_t* uncut);
/* MM_OPT_L1_GROUP_FUSED, as of the context's last SIZED pass: *offered = fragments the lookup kernel queued under MM_FLAG_SKIP_PREFIX (every
 * fragment with an interval point), *fused = those of them k_lookup_groups finished without the HBM point path; the rest it handed over
 * to that path (mm_pass_l1_literal's *queued).  0 / 0 when the kernel was not launched: the option off, no MM_FLAG_SKIP_PREFIX, sketchSize
 * above 512, a batch with a read longer than segLength, MM_OPT_KEEP_POINTS, or a refGroup array that is not non-decreasing.  Read back
 * with the words the sized pass reads behind the lookup kernels anyway: no host wait more.  Either pointer may be NULL.  Purely
 * additive: MM_ABI_VERSION stays 2. */
int mm_pass_l1_group_fused(const mm_ctx* ctx, uint64_t* offered, uint64_t* fused);
int mm_result_counts(const mm_ctx* ctx, size_t* nL1, size_t* nL2);
/* any pointer may be NULL.  l1/l2 are sorted by (frag, emission order of the reference) */
int mm_results_download(mm_ctx* ctx, mm_frag_stats* stats, mm_l1_candidate* l1, mm_l2_locus* l2);
/*
 * The candidate mappings of the batch (needs the replay tables): what mapSingleQueryFrag leaves in l2Mappings for every fragment
 * before its final std::sort (computeMap.hpp:774-800), fragment-major, inside a fragment in doL2Mapping's push order.
 */
int mm_mappings_count(const mm_ctx* ctx, size_t* n);
int mm_mappings_download(mm_ctx* ctx, mm_mapping* out, size_t cap, size_t* n);
/* device address of the same records; valid until the next map call */
int mm_mappings_device(const mm_ctx* ctx, const mm_mapping** dMappings, size_t* n);
/*
 * The tail of Map::mapModule on the device (computeMap.hpp:679-714): for every read of the batch, from its resident candidate mappings,
 * what the host side's MapPost::finishRead computes up to and including filterByGroup -- the kmerComplexity gate and the sort of
 * mapSingleQueryFrag (:799-800, :1137), the coordinates of a split read (:632-636), mergeMappingsInRange (:1580-1702),
 * filterWeakMappings (:423), filterByGroup on the query axis (:504-561) with the plane sweep of filter.hpp:36-160 --, one mm_chain_row per
 * surviving mapping.  The caller starts the stage explicitly after mm_map_fragments; nothing of that call changes.  The restatement is
 * mashmap_amd/csrc/mm_chain_core.h (one function per read, compiled for the host by tests/hostlogic/chain_check.cpp); DESIGN.md
 * section 6 has the argument why rows equal the host's bit for bit.  A read with more than MM_CHAIN_MAX_RECORDS records is not taken
 * by the one-thread-per-read kernel: up to that size libstdc++'s std::sort is a stable insertion sort; beyond, the representative of a
 * chain depends on introsort's moves.  Its records are handed over untouched (the left-over array) and the host finishes it as before
 * -- unless MM_OPT_CHAIN_LONG is set: then a read of 17 .. MM_CHAIN_LONG_MAX_RECORDS (512) records goes to k_chain_reads_long, a wave
 * per read with the working set in LDS, whose sorts are std::sort restated move for move (mashmap_amd/csrc/mm_stdsort.h), and only
 * reads above 512 records are handed over.
 * What stays on the host, applied to the rows: filterFalseHighIdentity, mappingBoundarySanityCheck, sparsifyMappings,
 * nucIdentityUpperBound and the PAF text (MapPost::finishRows).
 *
 * mm_chain_params: chainGap = Parameters::chain_gap (refused above 1 << 25: every accepted pair's squared distances are then exact in
 * a double); minMerged = floor(block_length / segLength); secondaryShort / secondarySegment = numMappingsForShortSequence - 1 /
 * numMappingsForSegment - 1 (secondaryToKeep of a read shorter than segLength / of any other; -1, a count of 0, is 65535 behind the
 * reference's cast to uint16_t, here as there; below -1 the block is refused, as is a negative minMerged); merge = mergeMappings; filter =
 * MM_CHAIN_FILTER_NONE or MM_CHAIN_FILTER_QUERY (filter modes map and one-to-one; the reference-axis filter of one-to-one is global
 * and stays on the host).
 * mm_set_chain_tables uploads the block and identity[Qs * stride + shared] = 1 - j2md(1.0 * shared / Qs, k) as floats (stride =
 * sketchSize + 1, the stride of the replay tables; mm_stat_identity_table fills it with the host's own expression).
 * mm_chain_reads runs the stage on the context's stream and waits once, at its end, for the four counts.  MM_ERR_STATE, with the reason
 * in mm_last_error: nothing mapped or no replay tables; mm_set_chain_tables not called; MM_FLAG_SKIP_PREFIX (its filter runs group by
 * group) and MM_FLAG_NO_SPLIT, unless MM_OPT_CHAIN_MODES is set; sketchSize above MM_CHAIN_MAX_SKETCH (the identity table would pass 16 MB); a record that names a sketch
 * size or shared count outside the identity table ("corrupt record": an error, never a hand-over -- the 16-record limit is the single
 * hand-over cause).  An empty batch, or one
 * without records, is MM_OK with zero counts.
 * mm_chain_counts: *offered = reads with at least one record, *finished = those of them the kernel took, *rows, *leftover = entries of
 * the two arrays.  Rows are in read order, inside a read in the order filterByGroup leaves them; the left-over mm_mapping records are
 * the handed-over reads', read-major, in their original order.  The device addresses are valid until the next mm_chain_reads or map call.
 * mm_chain_long_counts: *offered = reads of the batch with more than MM_CHAIN_MAX_RECORDS records, *finished = those of them
 * k_chain_reads_long wrote rows for (0 without MM_OPT_CHAIN_LONG); MM_ERR_STATE under the conditions of mm_chain_counts.
 * With MM_OPT_CHAIN_MODES (below) the two refusals by flag fall away: under MM_FLAG_SKIP_PREFIX filterByGroup runs reference group by
 * reference group, under MM_FLAG_NO_SPLIT no read is split.  mm_chain_group_counts: *runs = the group runs the filter stage swept or
 * passed through, over all finished reads; *reads = the finished reads with more than one run.  A RUN is a maximal stretch of
 * consecutive mappings of a read, in the order filterByGroup's first sort leaves them (by refSeqId, refStartPos), whose contigs have
 * equal refGroup[refSeqId] -- what the reference's std::find_if_not delimits (computeMap.hpp:524); each run is sorted by the query key
 * and swept on its own, a run of one mapping is passed through.  A group whose contigs are not consecutive in refGroup forms a run
 * per stretch.  In a context without MM_FLAG_SKIP_PREFIX the mappings that reach the filter are one run; a read of which no mapping
 * reaches the filter (the complexity gate or filterWeakMappings dropped them all) counts none, and with MM_CHAIN_FILTER_NONE no read
 * counts any.  The two values come back with the words the stage already reads at its one host wait; MM_ERR_STATE under the
 * conditions of mm_chain_counts.
 * Purely additive: MM_ABI_VERSION stays 2.
 */
#define MM_CHAIN_MAX_RECORDS 16          /* what k_chain_reads (one thread per read, std::sort == __insertion_sort) takes */
#define MM_CHAIN_LONG_MAX_RECORDS 512
#define MM_CHAIN_MAX_SKETCH 2048
#define MM_CHAIN_MAX_GAP (1 << 25)
enum { MM_CHAIN_FILTER_NONE = 0, MM_CHAIN_FILTER_QUERY = 1 };
typedef struct {
  int32_t chainGap, minMerged, secondaryShort, secondarySegment, merge, filter;
  float kmerComplexityThreshold;
  int32_t pad_;
} mm_chain_params;
/* every field of MappingResult (base_types.hpp:154) that finishRead leaves defined behind filterByGroup.  72 bytes.  kmerComplexity is
 * a double: a merged chain's is an average taken in double (:1668), a lone mapping's the float of getSeedHits (:831) widened. */
typedef struct {
  int32_t querySeqId, queryLen, queryStartPos, queryEndPos;
  int32_t refSeqId, refStartPos, refEndPos, strand;
  int32_t conservedSketches, sketchSize, blockLength, approxMatches, n_merged, splitMappingId;
  float nucIdentity;
  int32_t pad_;
  double kmerComplexity;
} mm_chain_row;
int mm_stat_identity_table(int sketchSize, int k, float* identity);   /* (sketchSize+1)^2 floats; row 0 (Qs == 0) is never read */
int mm_set_chain_tables(mm_ctx* ctx, const mm_chain_params* params, const float* identity, size_t stride);
int mm_chain_reads(mm_ctx* ctx);
int mm_chain_counts(const mm_ctx* ctx, size_t* offered, size_t* finished, size_t* rows, size_t* leftover);
int mm_chain_long_counts(const mm_ctx* ctx, uint64_t* offered, uint64_t* finished);
int mm_chain_group_counts(const mm_ctx* ctx, uint64_t* reads, uint64_t* runs);
int mm_chain_download(mm_ctx* ctx, mm_chain_row* out, size_t cap, size_t* n);
int mm_chain_leftover_download(mm_ctx* ctx, mm_mapping* out, size_t cap, size_t* n);
int mm_chain_device(const mm_ctx* ctx, const mm_chain_row** dRows, size_t* nRows, const mm_mapping** dLeftover, size_t* nLeftover);
/*
 * The PAF lines of a pass on the device: what the host side's MapPost::finishRows + appendReadMappings make of the rows of
 * mm_chain_reads -- filterFalseHighIdentity (computeMap.hpp:441), mappingBoundarySanityCheck (:1714) and the text of every line
 * (:1758-1806), byte for byte.  The restatement is mashmap_amd/csrc/mm_paf_core.h (compiled for the host by
 * tests/hostlogic/paf_check.cpp, which holds it against MapPost); DESIGN.md section 6 says why the bytes are the host's.
 *
 * mm_paf_params: legacy = Parameters::legacy_output (separator ' ', ends minus 1, last field nucIdentity * 100); aniPercentage =
 * report_ANI_percentage; merge = mergeMappings (0 adds the jc:f: field); filterLengthMismatches with lenIdThreshold = the host's own
 * std::min(0.7, std::pow(percentageIdentity, 3)); sparsityThreshold = sparsity_hash_threshold, which must be 2^64 - 1: sparsifyMappings
 * hashes through std::hash<float> and is not restated (MM_ERR_ARG otherwise).
 * mm_set_paf_tables uploads the block, the mapQ table and the contigs' names and lengths; it needs no index.  fakeMapQ is not computed
 * on the device (log10f there is not the host's bit for bit): mapqThresholds are nMapq (1 .. MM_PAF_MAX_MAPQ) ascending floats with
 * mapqThresholds[0] == 0 and the last <= 1, mapqText holds MM_PAF_MAPQ_TEXT bytes an entry, NUL-padded with at least one NUL: the text of
 * fakeMapQ for every identity t in thresholds[i] <= t < thresholds[i + 1] (the last entry: up to 1).  The host library builds it from
 * MapPost's own expression (mmh_paf_mapq_table).  refNames are the contigs' names end to end, refNameOff[i] .. refNameOff[i + 1] contig
 * i's (non-decreasing, nContigs + 1 entries).
 * mm_paf_rows formats the rows mm_chain_reads left resident for the mapped batch: nReads must be the batch's read count, read index =
 * querySeqId - seqCounterBase, queryNames / queryNameOff as the reference's.  mm_paf_format does the same for rows the caller brings
 * (host memory, read-major: querySeqId - firstSeqId in [0, nReads), non-decreasing), with readLens[nReads]; it needs neither an index nor
 * a mapped batch.  Both run on the context's stream and wait once, for the counts, before the text is written.
 * The output is the text of all reads in read order, lines in row order inside a read; off[r] .. off[r + 1] is read r's span (empty for a
 * read without rows or whose rows were all dropped).  A read with a row that is NOT FORMATTABLE -- an identity outside [0, 1], or a
 * floating-point field that is inf, NaN or, unless it is +-0, outside 2^-64 <= |v| < 2^64 -- is handed over as a whole: empty span,
 * handed[r] = 1, and the caller finishes it from mm_chain_download's rows; nothing is ever written for a read in part.
 * MM_ERR_STATE / MM_ERR_ARG with the reason in mm_last_error, before anything is launched: tables not set; mm_chain_reads has not run
 * on the mapped batch (mm_paf_rows); nReads mismatch; name offsets not non-decreasing; more than 2^31 - 1 rows; a row of mm_paf_format
 * whose refSeqId lies outside the contigs or whose querySeqId lies outside the reads or breaks read order ("corrupt row").  The rows of
 * mm_paf_rows are on the device: the same test runs in the first kernel, which reads no name or length for such a row, and the call
 * answers MM_ERR_STATE "corrupt row" behind its one wait, before any text is written.  An empty batch or one without rows is MM_OK
 * with zero counts.  A new upload or map call invalidates the results.
 * mm_paf_counts: reads with a non-empty span, lines and bytes of the text, rows the two filters dropped (over all rows, those of
 * handed-over reads included), reads handed over.  mm_paf_download copies the text (*n = its bytes; MM_ERR_ARG when cap is smaller),
 * mm_paf_offsets_download off[nReads + 1] and, when non-NULL, handed[nReads]; mm_paf_device gives the device addresses, valid until the
 * next mm_paf_* or map call.  Any pointer of mm_paf_counts / mm_paf_device may be NULL.
 * Purely additive: MM_ABI_VERSION stays 2.
 */
#define MM_PAF_MAPQ_TEXT 8
#define MM_PAF_MAX_MAPQ 128
typedef struct { int32_t legacy, aniPercentage, merge, filterLengthMismatches; double lenIdThreshold; uint64_t sparsityThreshold; } mm_paf_params;
int mm_set_paf_tables(mm_ctx* ctx, const mm_paf_params* params, const float* mapqThresholds, const char* mapqText, size_t nMapq,
                      const char* refNames, const uint64_t* refNameOff, const int32_t* refLens, size_t nContigs);
int mm_paf_rows(mm_ctx* ctx, const char* queryNames, const uint64_t* queryNameOff, size_t nReads);
int mm_paf_format(mm_ctx* ctx, const mm_chain_row* rows, size_t nRows, const int32_t* readLens, int32_t firstSeqId,
                  const char* queryNames, const uint64_t* queryNameOff, size_t nReads);
int mm_paf_counts(const mm_ctx* ctx, uint64_t* readsWithText, uint64_t* lines, uint64_t* bytes, uint64_t* dropped, uint64_t* handedReads);
int mm_paf_download(mm_ctx* ctx, char* text, size_t cap, size_t* n);
int mm_paf_offsets_download(mm_ctx* ctx, int64_t* off, uint8_t* handed);
int mm_paf_device(const mm_ctx* ctx, const char** dText, size_t* n, const int64_t** dOff);
/* post-removal sketches Q.minmerTableQuery: out[f*sketchSize + r] (valid r < stats[f].sketchSize) */
int mm_query_sketch_download(mm_ctx* ctx, mm_minmer* out);
/*
 * Options.  MM_OPT_KEEP_POINTS (default 0): by default the interval points of a fragment (getSeedIntervalPoints,
 * computeMap.hpp:857) live only in LDS/registers between the seed lookup and the L1 sweep; with 1 every fragment's sorted
 * point list is also kept in HBM so that mm_points_download can return it (parity tests); with 2 the list additionally goes through the
 * interval-point pre-filter the HBM point path applies to the fragments queued for it (k_filter_points: the intervals that cannot reach
 * minimumHits are dropped before the sort -- L1 candidates unchanged), and mm_points_download returns what the filter left.
 * MM_OPT_KEEP_FULL_INDEX (default 0): keep minmerIndex as it is BEFORE dropFreqSeedSet (winSketch.hpp:497) on the host so that
 * mm_index_download_full can return it -- that is what --saveIndex writes (winSketch.hpp:127-134 run before the drop).
 * MM_OPT_RESERVE_FRAGMENTS (default 0): the number of fragments of the largest batch the caller is going to upload.  The pass that sizes the
 * context's staging buffers (the first one, or one that outgrew them) then sizes them for a batch of that many fragments -- per-fragment
 * buffers directly, count-dependent ones (candidates, L2 streams, mappings) in proportion -- so that a caller whose batches grow (skch::Map
 * ramps its device passes up from one reader batch to four) pays for sizing and allocation once.
 * MM_OPT_L1_GROUP_STREAM (default 0): with 1, under MM_FLAG_SKIP_PREFIX the queued fragments go to the grouped form of the wave-per-fragment
 * kernel (k_l1_stream: one body per reference-group extent of the sorted points) and the literal kernel takes what it leaves -- a position
 * group across two contigs of one extent, minimumHits <= 0; mm_pass_l1_literal then reports that list's length.  Same candidates, same
 * order.  MM_L1_LITERAL still forces the literal kernel; batches with a read longer than segLength are untouched.  Without
 * MM_FLAG_SKIP_PREFIX the option does nothing.  Purely additive: MM_ABI_VERSION stays 2.
 * MM_OPT_L1_GROUP_FUSED (default 0): with 1, under MM_FLAG_SKIP_PREFIX the fragments the lookup kernel queued go through k_lookup_groups
 * first: one wave per fragment lists the interval points of its seeds in LDS, takes them one reference group at a time (the groups
 * number runs of consecutive contigs, so a group's points are one extent of the sorted list: one computeL1CandidateRegions call of
 * computeMap.hpp:1146-1165), sorts each group's points in registers and runs the fused L1 on them -- no gather, no sort through HBM.  It
 * hands a fragment over to the HBM point path (MM_OPT_L1_GROUP_STREAM chooses that path's L1 kernel as before, MM_L1_LITERAL still
 * forces the literal one) when it has more than 8 192 interval points, more than 64 groups, more than 1 024 kept points in one group or
 * more than 128 candidates, a position group across two contigs inside one extent, more than 64 candidate runs in one extent, or
 * minimumHits <= 0; mm_pass_l1_group_fused counts both.  Same candidates, same order.  The kernel is not launched for sketchSize above
 * 512, a batch with a read longer than segLength, under MM_OPT_KEEP_POINTS, or when refGroup is not non-decreasing.  With the option
 * set and without MM_OPT_KEEP_POINTS mm_points_download answers MM_ERR_STATE: the points of a fused fragment never reach HBM.  Without
 * MM_FLAG_SKIP_PREFIX the option does nothing.  Purely additive: MM_ABI_VERSION stays 2.
 * MM_OPT_L2_WINDOW_WAVE (default 0): with 1, the L2 stage of a batch with a read longer than segLength (MM_FLAG_NO_SPLIT) runs on
 * k_l2_window_wave -- one wave per L1 candidate, its query sketch, SlideMapper cells and heap of open records in LDS, 64 events of the contig's
 * stream (inserts and evictions; the inserts are the index records) per step, their records located and gated in parallel -- and the literal k_l2_window sweeps the candidates that kernel hands over (mm_pass_l2_window).  Same loci,
 * same order.  Sketch sizes above 2046 and batches without such a read are untouched.  Purely additive: MM_ABI_VERSION stays 2.
 * MM_OPT_L2_LARGE_WAVE (default 0), two bits.  Bit 0 (value 1, what a caller sets): a split batch on the literal L2 route -- sketchSize
 * above 8190 -- goes to k_l2_large_wave first when sketchSize <= 20460: one wave per L1 candidate, its SlideMapper cells (32-bit counts,
 * boolean `active`, accumulated vote) in LDS, 64 events of the candidate's slice of the index stream per step located in the query sketch in
 * parallel and then applied in event order; the literal k_l2_window sweeps the candidates that kernel hands over (mm_pass_l2_large).  Same
 * loci, same order.  Bit 1 (value 2; 3 with bit 0): split batches take the literal L2 route at ANY sketch size, so that both kernels can be
 * checked at small sketches; such a context runs sized passes only.  Batches with a read longer than segLength are untouched at every
 * value.  Purely additive: MM_ABI_VERSION stays 2.
 * MM_OPT_CHAIN_LONG (default 0): with 1, mm_chain_reads no longer hands over a read of 17 .. MM_CHAIN_LONG_MAX_RECORDS records: the count
 * pass lists such reads, and k_chain_reads_long (one wave per read, working set in LDS) chains and filters them; their rows stand in
 * read order among the others'.  Reads above 512 records are handed over as before -- the single hand-over cause left.  Rows of every
 * other read, the refusals and the one host wait of the stage are unchanged; mm_chain_long_counts reports what the kernel took.  Purely
 * additive: MM_ABI_VERSION stays 2.
 * MM_OPT_SKETCH_LARGE (default 0): with 1, mm_sketch_fragments / mm_map_fragments of a context with sketchSize above 8190 sketch on
 * k_sketch_large instead of the global-memory sketch kernel: one workgroup per fragment, the hashes from the strip hashers of the LDS
 * sketch kernels, the survivors of the same cut sorted in LDS tiles of 4096 entries with sweeps through HBM only between tiles, the same
 * emission.  Same sketch bytes; mm_sketch_large_counts reports what the kernel took.  At sketchSize <= 8190 the option does nothing.
 * Purely additive: MM_ABI_VERSION stays 2.
 * MM_OPT_CHAIN_MODES (default 0): with 1, mm_chain_reads takes a context created with MM_FLAG_SKIP_PREFIX, MM_FLAG_NO_SPLIT or both.
 * Under MM_FLAG_SKIP_PREFIX the stage reads the index's refGroup array (an index that came through mm_index_replicate included) and
 * filters every read run by run (mm_chain_group_counts above says what a run is), as the host's filterByGroup does under -Y; a record
 * whose refSeqId is outside the index's contigs is a "corrupt record" (MM_ERR_STATE), never read past.  Under MM_FLAG_NO_SPLIT a read
 * longer than segLength is one fragment: its row keeps the fragment's coordinates, queryLen is the read's length and n_merged is 0.
 * Every other refusal keeps its place and its
 * text -- sketchSize above 2048, no chain tables, nothing mapped, no replay tables --, and with the option off the two refusals by
 * flag are those of before.  In a context with neither flag the option does nothing.  Purely additive: MM_ABI_VERSION stays 2.
 */
enum { MM_OPT_KEEP_POINTS = 1, MM_OPT_KEEP_FULL_INDEX = 2, MM_OPT_RESERVE_FRAGMENTS = 3, MM_OPT_L1_GROUP_STREAM = 4, MM_OPT_L2_WINDOW_WAVE = 5, MM_OPT_L1_GROUP_FUSED = 6, MM_OPT_L2_LARGE_WAVE = 7, MM_OPT_CHAIN_LONG = 8, MM_OPT_SKETCH_LARGE = 9, MM_OPT_CHAIN_MODES = 10 };
int mm_set_option(mm_ctx* ctx, int option, int value);
/* sorted interval points of fragment f after the seqId filters of computeMap.hpp:891-896 (needs MM_OPT_KEEP_POINTS; (seqId,pos,side) only, hash = 0).
 * Under MM_FLAG_SKIP_PREFIX the points are in HBM without that option too -- unless MM_OPT_L1_GROUP_FUSED is set: then MM_ERR_STATE. */
int mm_points_download(mm_ctx* ctx, size_t frag, mm_interval_point* out, size_t cap, size_t* n);
/* copies the L2 loci (fragment-major device order, not re-sorted) into caller-owned DEVICE memory, e.g. a torch tensor
 * that is then exchanged with RCCL; *n receives the count, cap is the capacity of dst in records */
int mm_results_copy_device(mm_ctx* ctx, mm_l2_locus* dDst, size_t cap, size_t* n);
/* device addresses of the result arrays (for RCCL all-gatherv by the caller); valid until the next map call */
int mm_results_device(const mm_ctx* ctx, const mm_l2_locus** dL2, size_t* nL2);

/*
 * a5-a7 on the device: CommonFunc::addMinmers per contig (commonFunc.hpp:302), Sketch::index
 * (winSketch.hpp:379) and the frequent-seed filter (:410-504), leaving the index resident.
 * contigOffsets has nContigs+1 entries into `bases` (ASCII).  kmerPctThreshold as Parameters::kmer_pct_threshold.
 */
int mm_index_build(mm_ctx* ctx, const char* bases, const int64_t* contigOffsets, size_t nContigs,
                   const int32_t* refGroup, float kmerPctThreshold);
/* the resident index back on the host in reference layout (sizes first, then fill) */
int mm_index_sizes(const mm_ctx* ctx, size_t* nMinmers, size_t* nKeys, size_t* nPoints, size_t* nFreq, int32_t* freqThreshold);
int mm_index_download(mm_ctx* ctx, mm_minmer* minmers, uint64_t* keys, uint64_t* offsets, mm_interval_point* points,
                      uint64_t* freqSeeds);
/* how the resident index lies in HBM: what stands in for minmerPosLookupIndex (winSketch.hpp:101) -- the
 * open-addressing seed table, whether it is the tagged layout the library picks for tables above 1 GiB (one tag byte per slot, keys
 * placed bucket-wise), the presence filter in front of it -- and for minmerIndex (:102): the merged insert / eviction event stream and
 * the per-block lists of open records.  Lets a caller (and the human-scale parity tests) see which lookup kernel variant a map call
 * will run. */
typedef struct {
  uint64_t seedTableSlots, seedTableBytes;   /* slots of 16 bytes */
  uint64_t tagBytes;                         /* 0 unless tagged */
  uint64_t filterBytes;                      /* 0: no presence filter */
  uint64_t events, openRecords;              /* entries of the event stream / of the open-record lists */
  int32_t  tagged, pad_;
} mm_index_layout;
int mm_index_layout_get(const mm_ctx* ctx, mm_index_layout* out);

/*
 * Index persistence (winSketch.hpp:284-374).  mm_index_download_full: the pre-drop minmerIndex (PREFIX.index); the lookup map of
 * mm_index_download is already the full one (PREFIX.map).  mm_index_upload_full: what --loadIndex reads -- the pre-drop
 * minmerIndex and the map, flattened as for mm_index_upload, keys in any order -- followed inside the library by
 * computeFreqHist / computeFreqSeedSet / dropFreqSeedSet (:410-504), exactly the steps the reference runs after loading.
 */
int mm_index_download_full(mm_ctx* ctx, mm_minmer* out, size_t* n);
int mm_index_upload_full(mm_ctx* ctx, const mm_minmer* minmersAll, size_t nMinmers, const uint64_t* keys, const uint64_t* offsets,
                         size_t nKeys, const mm_interval_point* points, size_t nPoints, const int32_t* contigLen,
                         const int32_t* refGroup, size_t nContigs, float kmerPctThreshold);

/*
 * Multi-GPU: reads are sharded over GPUs in contiguous blocks, the index is replicated, and the one exchange
 * step is an all-gatherv of the candidate mappings over RCCL / xGMI -- what a multi-GPU skch::Map needs before the one-to-one
 * filter (computeMap.hpp:358-405) and to write one output stream in input order.  One mm_ctx per GPU.
 *   one process per GPU:  rank 0 calls mm_comm_unique_id and ships the MM_COMM_ID_BYTES to the others (MPI, a file, torch.distributed's
 *                         store ...); every rank calls mm_comm_init_rank; after each mm_map_fragments every rank calls mm_allgatherv_mappings.
 *   one process, n GPUs:  mm_comm_init_local(ctxs, n), then mm_allgatherv_mappings_local(ctxs, n) after all n contexts have mapped their
 *                         batch (contexts that share a device exchange by device copies: RCCL wants distinct GPUs).
 * Afterwards every context holds all ranks' records, rank-major (= input order with contiguous read blocks): mm_gathered_*.
 * mm_index_replicate copies a resident index GPU to GPU (xGMI) instead of building it once per GPU; the replica serves
 * mm_map_fragments but not the mm_index_download calls (the host mirrors stay with the source context).
 */
#define MM_COMM_ID_BYTES 128
int mm_comm_unique_id(void* id);
int mm_comm_init_rank(mm_ctx* ctx, const void* id, int rank, int world);
int mm_comm_init_local(mm_ctx** ctxs, int n);
int mm_comm_world(const mm_ctx* ctx, int* rank, int* world);
/* what the communicator itself says: the number of ranks RCCL sees in it (ncclCommCount; -1 if the bound library does not export it) and
 * the file its entry points were bound from -- for a record of a multi-GPU run to show that RCCL, and which one, carried the exchange */
int mm_comm_info(const mm_ctx* ctx, int* worldSeen, char* libraryPath, size_t cap);
int mm_allgatherv_mappings(mm_ctx* ctx);
/* The same exchange overlapped with the next batch: _begin snapshots the resident candidate mappings and returns at once (the exchange
 * runs on a stream and a host thread of its own); the caller may upload and map the next batch; _end waits for the exchange, after
 * which mm_gathered_* serve the records of the batch _begin was called on.  One exchange in flight per context; every rank must call
 * _begin / _end in the same order as the other ranks' (they are collectives). */
int mm_allgatherv_mappings_begin(mm_ctx* ctx);
int mm_allgatherv_mappings_end(mm_ctx* ctx);
int mm_allgatherv_mappings_local(mm_ctx** ctxs, int n);
int mm_gathered_counts(const mm_ctx* ctx, size_t* perRank, size_t* total);
int mm_gathered_download(mm_ctx* ctx, mm_mapping* out, size_t cap);
/* device address of the gathered records.  Lifetime: valid until the next exchange of this context STARTS (mm_allgatherv_mappings,
 * mm_allgatherv_mappings_local or mm_allgatherv_mappings_begin): the exchange may reallocate the buffer and rewrites the counts, from
 * its own thread in the overlapped form -- consume (or copy) the records of batch i before calling _begin for batch i+1. */
int mm_gathered_device(const mm_ctx* ctx, const mm_mapping** dMappings, size_t* total);
int mm_index_replicate(mm_ctx* dst, mm_ctx* src);

/* per-kernel device timing, measured with hipEvents on the ctx stream (bench.py roofline leg) */
enum { MM_K_PACK = 0, MM_K_SKETCH, MM_K_SKETCH_HARD, MM_K_LOOKUP, MM_K_SORT, MM_K_L1, MM_K_L2, MM_K_REFHASH, MM_K_L2_LOCATE, MM_K_WINNOW, MM_K_SELECT, MM_K_COUNT };
int mm_profile_enable(mm_ctx* ctx, int on);
/* ms[i] = accumulated milliseconds, launches[i] = launch count since the last reset */
int mm_profile_read(mm_ctx* ctx, double* ms, uint64_t* launches, int reset);
const char* mm_kernel_name(int which);
/* integer-roofline yardstick: a kernel that does nothing but the 2 x MurmurHash3_x64_128 per position of
 * every resident fragment (both strands, same tables and staging as the sketch kernel); *msAvg = average of `reps` launches */
int mm_bench_hash_only(mm_ctx* ctx, int reps, double* msAvg);
/*
 * BGZF blocks inflated on the device (k_inflate_blocks, mashmap_amd/csrc/mm_inflate.hip; the decoder is mashmap_amd/csrc/mm_inflate_core.h,
 * which tests/hostlogic/inflate_check.cpp runs against zlib on the host).  A BGZF block (SAM specification, section 4.1) is an independent
 * raw-deflate stream of at most 64 KiB, compressed and inflated, followed by the CRC-32 and the length of its payload: one
 * mm_inflate_block names the stream (comp + cOff, cLen bytes), where its payload goes (dst + uOff, uLen bytes) and the CRC-32 the payload
 * must have.  mm_inflate_blocks copies the compressed bytes the descriptors span to the device, inflates every block on a wave of its
 * own (any number of stored, fixed and dynamic deflate blocks up to BFINAL), checks length and CRC-32, copies every payload to its place
 * in dst and writes every descriptor's status: MM_INFLATE_OK, or why the block was refused -- BAD_STREAM (block type 3, a stored length
 * that is not its complement's, more than 286 literal/length or 30 distance codes, a repeat code with nothing to repeat or past the end,
 * an over-subscribed or -- other than zlib allows -- incomplete code, no end-of-block code, a code that is not assigned, symbols 286 / 287
 * / 30 / 31), TRUNCATED (the cLen bytes end inside the stream), OVERRUN (more than uLen bytes), SHORT (BFINAL's block ends before uLen),
 * BAD_DISTANCE (a match that starts before the block's first byte), BAD_CRC.  The bytes of a refused block's own range in dst are
 * unspecified; nothing outside the descriptors' ranges is written.  A block with uLen == 0 is decoded and checked like any other (the
 * BGZF end-of-file block is one).  *nBad (may be NULL) receives the number of refused blocks.
 * comp and dst are host pointers; page-locked memory (mm_host_alloc) makes both copies DMA transfers at PCIe rate, any host pointer
 * works.  The call needs a context only -- no index, no reads --, touches neither the resident batch nor its results, and runs on a
 * stream of its own: it joins the exception mm_reads_prefetch makes to "a ctx is thread-compatible" -- a reader thread may call it while
 * the context's own thread is inside any other call; against itself it is serialised inside the library.  It returns when dst is filled.
 * The text of a failed call is kept per calling thread: mm_last_error gives it when called next on that thread for that context.
 * MM_ERR_ARG, before anything is launched: a descriptor whose ranges leave nComp or nDst, uLen or cLen above MM_INFLATE_MAX_BLOCK, output
 * ranges that overlap.  MM_OK whenever the kernel ran (and for nBlocks == 0, which launches nothing): the status fields say the rest.
 * The staging buffers belong to the context: they count in mm_device_bytes and go with mm_destroy.
 * mm_inflate_counts: the context's calls that returned MM_OK so far, the blocks they named and the payload
 * bytes of the blocks that were MM_INFLATE_OK -- the last two are kept by the kernel on the device, beside its count of refused blocks.
 * mm_inflate_kernel_ms: device time of the last call's kernel alone (hipEvents on the inflate stream), 0 before the first call.
 * Purely additive: MM_ABI_VERSION stays 2.
 */
#define MM_INFLATE_MAX_BLOCK 65536           /* BGZF's bound, both ways */
enum { MM_INFLATE_OK = 0, MM_INFLATE_BAD_STREAM, MM_INFLATE_TRUNCATED, MM_INFLATE_OVERRUN,
       MM_INFLATE_SHORT, MM_INFLATE_BAD_DISTANCE, MM_INFLATE_BAD_CRC };
typedef struct { uint64_t cOff; uint32_t cLen, uLen; uint64_t uOff; uint32_t crc32, status; } mm_inflate_block;  /* 32 bytes */
int mm_inflate_blocks(mm_ctx* ctx, const void* comp, size_t nComp, mm_inflate_block* blocks, size_t nBlocks,
                      void* dst, size_t nDst, size_t* nBad);
int mm_inflate_counts(const mm_ctx* ctx, uint64_t* calls, uint64_t* blocks, uint64_t* bytesOut);
int mm_inflate_kernel_ms(const mm_ctx* ctx, double* ms);
/*
 * FASTA / FASTQ text parsed on the device into the packed read batch (mashmap_amd/csrc/mm_text.hip; the record rules are
 * mashmap_amd/csrc/mm_text_core.h, which tests/hostlogic/text_check.cpp runs against the host reader's serial functions).  A context owns
 * one TEXT BUFFER on the device (at most 2^32 - 1 bytes; it counts in mm_device_bytes and goes with mm_destroy):
 *   mm_text_reset            empties it (a new file).
 *   mm_text_append           copies n bytes (a host pointer, or a device pointer with onDevice != 0) behind what it holds.
 *   mm_text_append_inflated  is mm_inflate_blocks whose payloads stay on the device: the same checks of the descriptors, the same kernel,
 *                            the same statuses.  uOff only orders the payloads: they are laid end to end, in ascending uOff, behind what
 *                            the buffer holds.  If a block is refused nothing is appended; *nBad says how many were.
 *   mm_text_scan             finds the records of the buffer.  final == 0: FASTA -- every record but the last header line's is complete and
 *                            *consumed is that line's offset (one header line: 0 records, 0 bytes); FASTQ -- newlines / 4 records, and
 *                            *consumed lies behind the last of their newlines.  final != 0: everything to the end belongs to records (a last
 *                            FASTQ group of fewer than four lines is one) and *consumed is the buffer's length.  *nNameBytes: the names' total.
 *   mm_text_records          the last scan's table: one mm_text_record per record (hdrOff: offset of its header line in the buffer; seqLen:
 *                            its bases; hasN: one of them is not A C G T a c g t), and the names end to end, nameLen bytes each (the header
 *                            line without its first byte, cut at the first ' ' only).  Either pointer may be NULL.
 *   mm_text_pack             packs the bases of the records with keep[r] != 0 (keep == NULL: all) the way mm_reads_upload_packed lays a
 *                            batch out -- record after record, each on a 32-base boundary, no gaps; a record that is not kept is a read of
 *                            length 0 -- and hands the piece over as mm_reads_prefetch_packed_append would: if it fits the staging area (the
 *                            same growth rule, the same reservePackedBases) the words are written THERE, as a staged piece with the key
 *                            (bases2, nmask, *nPackedBases), the two host buffers are never touched and *staged = 1; otherwise they are
 *                            copied to the two host buffers, which hold capPackedBases, and *staged = 0.  Either way the caller's
 *                            mm_reads_upload_packed[_parts] with that key and the kept lengths carries the piece.  Then the consumed bytes
 *                            leave the buffer and its tail becomes its front.  MM_ERR_ARG, with the buffer as it was: a kept record of 2^31
 *                            bases or more, a total above capPackedBases.
 *   mm_text_counts           scans that returned MM_OK, the records they found and the bytes they consumed, so far.
 *   mm_text_kernel_ms        device time of the last scan's kernels and of the last pack's (hipEvents), 0 before the first.
 * mm_text_records and mm_text_pack answer MM_ERR_STATE without a scan since the buffer last changed.  All of these join the thread exception
 * of mm_reads_prefetch / mm_inflate_blocks: a reader thread may make them while the context's own thread is inside another call; they run
 * on the inflate stream and are serialised among themselves and against mm_inflate_blocks inside the library; the text of a failed call
 * is kept per calling thread like mm_inflate_blocks's.  Purely additive: MM_ABI_VERSION stays 2.
 */
#define MM_TEXT_TILE 4096                    /* bytes a wave summarises and resolves */
enum { MM_TEXT_FASTA = 0, MM_TEXT_FASTQ = 1 };
typedef struct { uint64_t hdrOff; int64_t seqLen; uint32_t nameLen, hasN; } mm_text_record;   /* 24 bytes */
int mm_text_reset(mm_ctx* ctx);
int mm_text_append(mm_ctx* ctx, const void* bytes, size_t n, int onDevice);
int mm_text_append_inflated(mm_ctx* ctx, const void* comp, size_t nComp, mm_inflate_block* blocks, size_t nBlocks, size_t* nBad);
int mm_text_scan(mm_ctx* ctx, int format, int final, size_t* nRecords, size_t* nNameBytes, size_t* consumed);
int mm_text_records(mm_ctx* ctx, mm_text_record* recs, char* names);
int mm_text_pack(mm_ctx* ctx, const uint8_t* keep, uint32_t* bases2, uint32_t* nmask, size_t capPackedBases,
                 size_t reservePackedBases, size_t* nPackedBases, int* staged);
int mm_text_counts(const mm_ctx* ctx, uint64_t* scans, uint64_t* records, uint64_t* bytes);
int mm_text_kernel_ms(const mm_ctx* ctx, double* scanMs, double* packMs);
/* diagnostic: bytes of device memory the library holds at this moment, over every context of the process (their indexes, batches of
 * reads -- the parked ones included --, staging buffers) and the scratch of a call in progress.  Counted where the library allocates and
 * frees, not asked of the device: memory other libraries or processes hold is not in it.  After the last mm_destroy it is 0.  May be
 * called from any thread.  Purely additive: MM_ABI_VERSION stays 2. */
size_t mm_device_bytes(void);
int mm_synchronize(mm_ctx* ctx);
/* the HIP stream all work of this ctx is ordered on (a hipStream_t) */
void* mm_stream(const mm_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
