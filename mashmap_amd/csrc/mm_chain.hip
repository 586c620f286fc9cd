// mashmap_amd/csrc/mm_chain.hip -- the tail of Map::mapModule on the device (gfx950): chaining and filtering of every read's candidate
// mappings, behind mm_map_fragments and started by the caller (mm_chain_reads).
//
//   Map::mapModule tail   mergeMappingsInRange, filterWeakMappings, filterByGroup     src/map/include/computeMap.hpp:679-714, :1580-1702
//   plane sweep           query axis                                                  src/map/include/filter.hpp:36-160
//
// The restatement is mm_chain_core.h (one function per read; the header says why its rows are the host's bit for bit); this file
// finds every read's records, runs the function, and lays rows and left-over records out compactly the way k_l2_select does: count,
// exclusive scan, write.
//
// Shape.  One thread per read, 128 threads per block.  A read of the headline workload has about two records (2 M records for 1 M
// reads of a 10 Gbp batch); every loop of the tail runs over the read's own records and every step depends on the one before (the
// pair loop feeds the union-find in order, the sweep's status array changes event by event), so a read's work is a few hundred
// dependent integer operations behind 48 n bytes of records -- the stage is bound by reading the records (96 MB) and writing the rows, and
// one lane per read keeps every lane of a wave on a read of its own instead of leaving 14 of 16 lanes of a sub-wave without a record.
// The read's working set (mm_chain_work, ~1 KB) is indexed dynamically and lives in scratch; with two records per read only its first
// lines are touched.  A sub-wave per read with the working set in LDS is what a workload of long chains (n near 16) would want; the
// hand-over limit and the core function do not depend on the choice.
//
// MM_OPT_CHAIN_LONG.  A read of 17 .. 512 records is then not handed over: the count pass of k_chain_reads appends its index to a device
// list (one atomic counter, no host wait), and k_chain_reads_long takes the list's entries, one wave per read, until it is empty.  That
// kernel runs ONCE -- not once to count and once to write --: it leaves a read's rows at the read's record offset in a staging array (a
// read leaves at most as many rows as it has records) and the count in cntRows[r] before the scan; k_chain_copy_long moves the rows to
// their compact place behind the scan.  The stage keeps its single host wait.
//
// MM_OPT_CHAIN_MODES.  A context created with MM_FLAG_SKIP_PREFIX (-Y) or MM_FLAG_NO_SPLIT is then taken: the environment carries the
// index's refGroup array and the noSplit flag, and filterByGroup walks the runs of one reference group (mm_chain_core.h, "runs").  Both
// kernels get that from the core function; in k_chain_reads_long the runs are lane 0's, one after the other, like the rest of the
// filter phase (a run per lane was built and measured: profiles/NOTES.md, "Chaining -Y and --noSplit reads").  Two more words of
// dChainTotals count the runs (mm_chain_group_counts) and come back with the others.
#include "mm_internal.h"
#include "mm_chain_core.h"
#include "../host/mm_stats.hpp"

enum : int { MM_CT_ROWS = 0, MM_CT_LEFT = 1, MM_CT_OFFERED = 2, MM_CT_FINISHED = 3, MM_CT_BAD = 4,
             MM_CT_LONG_OFFERED = 5, MM_CT_LONG_FINISHED = 6, MM_CT_LONG_LIST = 7, MM_CT_LONG_TICKET = 8,
             MM_CT_GROUP_READS = 9, MM_CT_GROUP_RUNS = 10, MM_CT_WORDS = 11 };   // dChainTotals
#define MM_CHAIN_LONG_WG_PER_CU 4

// the records are read-major: a read's are one run of equal querySeqId
__global__ void __launch_bounds__(256)
k_chain_ranges(long long nM, const mm_mapping* __restrict__ recs, int seqCounterBase, int nReads, int32_t* __restrict__ begin, int32_t* __restrict__ end) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nM) return;
  const int q = recs[i].querySeqId;
  const unsigned r = (unsigned)(q - seqCounterBase);
  if (r >= (unsigned)nReads) return;
  if (i == 0 || recs[i - 1].querySeqId != q) begin[r] = (int32_t)i;
  if (i == nM - 1 || recs[i + 1].querySeqId != q) end[r] = (int32_t)(i + 1);
}

// longOn (MM_OPT_CHAIN_LONG): a read of 17 .. 512 records is neither finished nor handed over here -- the count pass lists it in longList
// (in any order: every read's rows have their own place) and leaves cntRows[r] to k_chain_reads_long
template <bool WRITE>
__global__ void __launch_bounds__(128)
k_chain_reads(mm_chain_env E, int nReads, const mm_mapping* __restrict__ recs, const int32_t* __restrict__ begin, const int32_t* __restrict__ end,
              const int32_t* __restrict__ readLen, int32_t* __restrict__ cntRows, int32_t* __restrict__ cntLeft,
              const int64_t* __restrict__ offRows, const int64_t* __restrict__ offLeft, mm_chain_row* __restrict__ rows, mm_mapping* __restrict__ left,
              unsigned long long* __restrict__ totals, int longOn, int32_t* __restrict__ longList) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  int n = 0, b = 0;
  if (r < nReads) { b = begin[r]; n = end[r] - b; if (n < 0) n = 0; }
  int nRows = 0, nLeft = 0, nRuns = 0;
  const bool isLong = longOn && n > MM_CHAIN_MAX_RECORDS && n <= MM_CHAIN_LONG_MAX_RECORDS;
  if (isLong) {
    if (!WRITE) longList[atomicAdd(&totals[MM_CT_LONG_LIST], 1ull)] = r;             // fewer entries than reads
  } else if (n > MM_CHAIN_MAX_RECORDS) {
    nLeft = n;
    if (WRITE) { mm_mapping* dst = left + offLeft[r]; for (int i = 0; i < n; i++) dst[i] = recs[b + i]; }
  } else if (n > 0) {
    nRows = mm_chain_read(E, recs + b, n, readLen[r], WRITE ? rows + offRows[r] : (mm_chain_row*)nullptr, WRITE ? (int*)nullptr : &nRuns);
    if (nRows < 0) { nRows = 0; if (!WRITE) atomicAdd(&totals[MM_CT_BAD], 1ull); }     // MM_CHAIN_BAD_RECORD: the launcher reports it, nothing of the read is written
  }
  if (!WRITE) {
    if (r < nReads) { cntRows[r] = nRows; cntLeft[r] = nLeft; }
    const int offered = __syncthreads_count(n > 0), finished = __syncthreads_count(n > 0 && nLeft == 0);
    const int longOffered = __syncthreads_count(n > MM_CHAIN_MAX_RECORDS);
    // the runs of the block's reads (at most 16 each): reads with more than t runs, summed over t
    const int groupReads = __syncthreads_count(nRuns > 1);
    int groupRuns = 0;
    const int mostRuns = E.refGroup ? MM_CHAIN_MAX_RECORDS : 1;
    for (int t = 0; t < mostRuns; t++) {
      const int above = __syncthreads_count(nRuns > t);
      if (!above) break;
      groupRuns += above;
    }
    if (threadIdx.x == 0) {
      if (offered) atomicAdd(&totals[MM_CT_OFFERED], (unsigned long long)offered);
      if (finished) atomicAdd(&totals[MM_CT_FINISHED], (unsigned long long)finished);
      if (longOffered) atomicAdd(&totals[MM_CT_LONG_OFFERED], (unsigned long long)longOffered);
      if (groupReads) atomicAdd(&totals[MM_CT_GROUP_READS], (unsigned long long)groupReads);
      if (groupRuns) atomicAdd(&totals[MM_CT_GROUP_RUNS], (unsigned long long)groupRuns);
    }
  }
}

// MM_OPT_CHAIN_LONG: one wave (a workgroup of 64) per read of 17 .. 512 records, on a fixed grid of MM_CHAIN_LONG_WG_PER_CU workgroups
// per compute unit; a workgroup takes the next entry of the list (a ticket counter) until none is left.
//
// LDS.  The read's working set (mm_chain_work_long) is in LDS as arrays over the member index: 11 int32 + 1 float + 1 double + 2 int8 =
// 58 B a record of mapping fields, 2 B of order, and 18 B the two phases' scratch shares (union-find parent / partner / rank, 5 B, then
// the sweep's two event words and status id) -- 78 B a record, 39 936 B for 512: four workgroups per compute unit (160 KB), i.e. one wave
// per SIMD.  Lane i reads element i of an array in the parallel steps: consecutive words, no bank conflict.
//
// Who does what.  The order-dependent steps run on lane 0 through the steps of mm_chain_core.h: the five std::sort restatements (a
// parallel sort cannot reproduce introsort's order among ties), the unions in member order, the compaction of the chains, the sweep with
// its status set.  While lane 0 works the other 63 lanes are masked off: the wave issues one lane's LDS accesses, each dependent on the one
// before (an LDS round trip a step), which is what bounds a read -- some n lg n comparisons of two or three loads for each of the five
// sorts of n records; with one such wave per SIMD nothing hides that latency but the other three waves of the unit.  Across the wave run the steps
// whose items are independent: record load, complexity gate and identity lookup (a ballot numbers the records that pass); the partner
// search of the pair loop, member i on lane i mod 64 (the quadratic part; unions follow on lane 0 in i order); the extents and sums of
// the chains, a chain per lane, each in member order; the rows.
__global__ void __launch_bounds__(64)
k_chain_reads_long(mm_chain_env E, const mm_mapping* __restrict__ recs, const int32_t* __restrict__ begin, const int32_t* __restrict__ end,
                   const int32_t* __restrict__ readLen, const int32_t* __restrict__ longList, int32_t* __restrict__ cntRows,
                   mm_chain_row* __restrict__ stage, unsigned long long* __restrict__ totals) {
  __shared__ mm_chain_work_long W;
  __shared__ int sM;
  __shared__ unsigned long long sTicket;
  const int lane = threadIdx.x;
  const unsigned long long nList = totals[MM_CT_LONG_LIST];       // final: the count pass is behind us on the stream
  for (;;) {
    __syncthreads();                                               // the previous read's working set is no longer in use
    if (lane == 0) sTicket = atomicAdd(&totals[MM_CT_LONG_TICKET], 1ull);
    __syncthreads();
    const unsigned long long t = sTicket;
    if (t >= nList) break;
    const int r = longList[t];
    const int b = begin[r], n = end[r] - b;
    if (n <= MM_CHAIN_MAX_RECORDS || n > MM_CHAIN_LONG_MAX_RECORDS) continue;          // (the count pass lists no such read)
    const int32_t len = readLen[r];
    const bool split = !E.noSplit && len > E.segLength;
    const int32_t querySeqId = recs[b].querySeqId;
    const int32_t queryLen = split ? len : recs[b].fragLen;

    // ---- prepare: gate and identity of record p on lane p mod 64; the records that pass become members 0 .. m-1 in record order.
    // Every record of a fragment carries the fragment's maxHash, rawSketchSize and length: its own complexity is the fragment's.
    int m = 0;
    bool bad = false;
    for (int base = 0; base < n; base += 64) {
      const int p = base + lane;
      bool keep = false, ok = true;
      mm_mapping rec;
      float kc = 0.0f;
      if (p < n) {
        rec = recs[b + p];
        kc = mm_chain_kmer_complexity(rec.maxHash, rec.rawSketchSize, rec.fragLen, E.kmerSize);
        keep = !(kc < E.p.kmerComplexityThreshold);
      }
      const unsigned long long mask = __ballot(keep);
      if (keep) {
        const int x = m + __popcll(mask & ((1ull << lane) - 1ull));
        ok = mm_chain_prepare(E, W, x, rec, split, kc);
        if (ok) W.smid[x] = rec.fragStart;                         // for the fragment sorts below; cleared behind them
      }
      bad = bad || __any(!ok);
      m += __popcll(mask);
    }
    if (bad) {                                                     // MM_CHAIN_BAD_RECORD: the launcher reports it, the read leaves nothing
      if (lane == 0) { cntRows[r] = 0; atomicAdd(&totals[MM_CT_BAD], 1ull); }
      continue;
    }
    __syncthreads();
    if (lane == 0)                                                 // mapSingleQueryFrag's sort, fragment by fragment
      for (int x = 0; x < m;) {
        int y = x;
        while (y < m && W.smid[y] == W.smid[x]) y++;               // (members are still in place: v[x] == x)
        mm_chain_sort_ref(W, x, y);
        x = y;
      }
    __syncthreads();
    for (int x = lane; x < m; x += 64) W.smid[x] = 0;
    __syncthreads();

    // ---- mergeMappingsInRange + filterWeakMappings
    if (split && E.p.merge) {
      const bool merged = m >= 2;
      if (merged) {
        if (lane == 0) mm_chain_sort_merge(W, m);
        __syncthreads();
        for (int i = lane; i < m; i += 64) {
          W.uf.parent[i] = (int16_t)i; W.uf.rnk[i] = 0; W.smid[W.v[i]] = i;
          W.uf.best[i] = (int16_t)mm_chain_partner(W, m, i, E.p.chainGap);
        }
        __syncthreads();
        if (lane == 0) {
          for (int i = 0; i < m; i++) if (W.uf.best[i] >= 0) mm_chain_unite(W, i, W.uf.best[i]);
          for (int i = 0; i < m; i++) W.smid[W.v[i]] = mm_chain_find(W, W.smid[W.v[i]]);
          mm_chain_sort_smid(W, m);
        }
        __syncthreads();
        for (int it = lane; it < m; it += 64)                      // a chain per lane: the one that starts at position `it`
          if (it == 0 || W.smid[W.v[it]] != W.smid[W.v[it - 1]]) {
            int e = it + 1;
            while (e < m && W.smid[W.v[e]] == W.smid[W.v[it]]) e++;
            mm_chain_finish_chain(W, it, e);
          }
        __syncthreads();
      }
      if (lane == 0) sM = mm_chain_keep(E, W, m, queryLen, merged);
      __syncthreads();
      m = sM;
      __syncthreads();
    }

    // ---- filterByGroup: its sorts and the sweep of every run (nRuns: lane 0's alone)
    int nRuns = 0;
    if (lane == 0) sM = mm_chain_filter(E, W, m, len, &nRuns);
    __syncthreads();
    m = sM;
    for (int i = lane; i < m; i += 64) stage[(size_t)b + i] = mm_chain_emit(W, W.v[i], querySeqId, queryLen);
    if (lane == 0) {
      cntRows[r] = m; atomicAdd(&totals[MM_CT_LONG_FINISHED], 1ull);
      if (nRuns) atomicAdd(&totals[MM_CT_GROUP_RUNS], (unsigned long long)nRuns);
      if (nRuns > 1) atomicAdd(&totals[MM_CT_GROUP_READS], 1ull);
    }
  }
}

// behind the scan: the rows of listed read t from the staging array to their compact place
__global__ void __launch_bounds__(64)
k_chain_copy_long(const int32_t* __restrict__ longList, const int32_t* __restrict__ begin, const int32_t* __restrict__ cntRows, const int64_t* __restrict__ offRows,
                  const mm_chain_row* __restrict__ stage, mm_chain_row* __restrict__ rows, const unsigned long long* __restrict__ totals) {
  const unsigned long long nList = totals[MM_CT_LONG_LIST];
  for (unsigned long long t = blockIdx.x; t < nList; t += gridDim.x) {
    const int r = longList[t];
    const int n = cntRows[r];
    const mm_chain_row* src = stage + begin[r];
    mm_chain_row* dst = rows + offRows[r];
    for (int i = threadIdx.x; i < n; i += 64) dst[i] = src[i];
  }
}

extern "C" {

int mm_stat_identity_table(int sketchSize, int k, float* identity) {
  if (sketchSize < 1 || !identity) return MM_ERR_ARG;
  const size_t stride = (size_t)sketchSize + 1;
  for (size_t Qs = 0; Qs < stride; Qs++)
    for (size_t shared = 0; shared < stride; shared++) {
      const float mash_dist = Qs == 0 ? 1.0f : mmhost::Stat::j2md(1.0 * (int)shared / (int)Qs, k);     // computeMap.hpp:1211-1213, as MapPost::identityOf
      identity[Qs * stride + shared] = 1 - mash_dist;
    }
  return MM_OK;
}

int mm_set_chain_tables(mm_ctx* c, const mm_chain_params* params, const float* identity, size_t stride) {
  if (!params || !identity || stride != (size_t)c->P.sketchSize + 1) { c->err = "mm_set_chain_tables: need the parameter block and (sketchSize+1)^2 identities"; return MM_ERR_ARG; }
  if (c->P.sketchSize > MM_CHAIN_MAX_SKETCH) { c->err = "mm_set_chain_tables: sketchSize above 2048 (the identity table would be larger than 16 MB)"; return MM_ERR_ARG; }
  if (!mm_chain_params_ok(*params)) { c->err = "mm_set_chain_tables: chainGap must be in 0 .. 1 << 25 (beyond, the chain distances are not exact in a double), filter MM_CHAIN_FILTER_NONE or _QUERY, minMerged >= 0 and the two secondary counts >= -1"; return MM_ERR_ARG; }
  MM_HIP(c, hipSetDevice(c->device));
  MM_HIP(c, c->dChainIdent.ensure(stride * stride * 4));
  MM_HIP(c, hipMemcpyAsync(c->dChainIdent.p, identity, stride * stride * 4, hipMemcpyHostToDevice, c->stream));
  MM_HIP(c, hipStreamSynchronize(c->stream));
  c->chainP = *params; c->haveChainTables = true; c->chainPass = 0;
  return MM_OK;
}

int mm_chain_reads(mm_ctx* c) {
  c->chainPass = 0;
  // what the context was created with first, then what the caller has done with it
  // (both taken with MM_OPT_CHAIN_MODES)
  const bool grouped = (c->P.flags & MM_FLAG_SKIP_PREFIX) != 0, noSplit = (c->P.flags & MM_FLAG_NO_SPLIT) != 0;
  if (grouped && !c->opt.chainModes) { c->err = "mm_chain_reads: MM_FLAG_SKIP_PREFIX is set (filterByGroup then runs reference group by reference group)"; return MM_ERR_STATE; }
  if (noSplit && !c->opt.chainModes) { c->err = "mm_chain_reads: MM_FLAG_NO_SPLIT is set"; return MM_ERR_STATE; }
  if (c->P.sketchSize > MM_CHAIN_MAX_SKETCH) { c->err = "mm_chain_reads: sketchSize above 2048 (the identity table would be larger than 16 MB)"; return MM_ERR_STATE; }
  if (!c->haveChainTables) { c->err = "mm_chain_reads: mm_set_chain_tables was not called"; return MM_ERR_STATE; }
  if (!c->mapped || !c->haveReplayTables) { c->err = "mm_chain_reads: nothing mapped, or mm_set_replay_tables / mm_set_tables_default was not called"; return MM_ERR_STATE; }
  c->chOffered = c->chFinished = c->chRows = c->chLeft = 0; c->chLongOffered = c->chLongFinished = 0; c->chGroupReads = c->chGroupRuns = 0;
  const size_t nR = c->nReads, nM = c->rep.nMappings;
  if (nM > (size_t)0x7fffffff || nR > (size_t)0x7fffffff) { c->err = "mm_chain_reads: more than 2^31 - 1 records in one batch"; return MM_ERR_CAPACITY; }
  if (grouped && nR && nM && (!c->idx.ready || !c->idx.nContigs || c->idx.refGroup.bytes < c->idx.nContigs * 4)) { c->err = "mm_chain_reads: internal error: records without an index's reference groups"; return MM_ERR_STATE; }
  if (nR && nM) {
    MM_HIP(c, hipSetDevice(c->device));
    MM_HIP(c, c->dChainBegin.ensure(nR * 4 + 64)); MM_HIP(c, c->dChainEnd.ensure(nR * 4 + 64));
    MM_HIP(c, c->dChainCntR.ensure(nR * 4 + 64)); MM_HIP(c, c->dChainCntL.ensure(nR * 4 + 64));
    MM_HIP(c, c->dChainOffR.ensure(nR * 8 + 64)); MM_HIP(c, c->dChainOffL.ensure(nR * 8 + 64));
    MM_HIP(c, c->dChainRows.ensure(nM * sizeof(mm_chain_row) + 64)); MM_HIP(c, c->dChainLeft.ensure(nM * sizeof(mm_mapping) + 64));   // a read leaves at most as many rows as it has records
    MM_HIP(c, c->dChainTotals.ensure(MM_CT_WORDS * 8));
    const int longOn = c->opt.chainLong ? 1 : 0;
    if (longOn) {
      MM_HIP(c, c->dChainLongList.ensure(nR * 4 + 64)); MM_HIP(c, c->dChainStage.ensure(nM * sizeof(mm_chain_row) + 64));
      if (!c->chainCUs) { int cus = 0; MM_HIP(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device)); c->chainCUs = cus > 0 ? cus : 1; }
    }
    MM_HIP(c, hipMemsetAsync(c->dChainBegin.p, 0, nR * 4, c->stream)); MM_HIP(c, hipMemsetAsync(c->dChainEnd.p, 0, nR * 4, c->stream));
    MM_HIP(c, hipMemsetAsync(c->dChainTotals.p, 0, MM_CT_WORDS * 8, c->stream));
    const mm_mapping* recs = c->dMappings.as<mm_mapping>();
    hipLaunchKernelGGL(k_chain_ranges, dim3((unsigned)((nM + 255) / 256)), dim3(256), 0, c->stream, (long long)nM, recs, (int)c->seqCounterBase, (int)nR,
                       c->dChainBegin.as<int32_t>(), c->dChainEnd.as<int32_t>());
    mm_chain_env E;
    E.p = c->chainP; E.kmerSize = c->P.kmerSize; E.segLength = c->P.segLength; E.stride = c->P.sketchSize + 1; E.identity = c->dChainIdent.as<float>();
    E.refGroup = grouped ? c->idx.refGroup.as<int32_t>() : nullptr; E.nContigs = (int32_t)c->idx.nContigs; E.noSplit = noSplit ? 1 : 0;
    unsigned long long* totals = c->dChainTotals.as<unsigned long long>();
    const dim3 grid((unsigned)((nR + 127) / 128)), block(128);
    hipLaunchKernelGGL((k_chain_reads<false>), grid, block, 0, c->stream, E, (int)nR, recs, c->dChainBegin.as<int32_t>(), c->dChainEnd.as<int32_t>(),
                       c->dReadLen.as<int32_t>(), c->dChainCntR.as<int32_t>(), c->dChainCntL.as<int32_t>(), (const int64_t*)nullptr, (const int64_t*)nullptr,
                       (mm_chain_row*)nullptr, (mm_mapping*)nullptr, totals, longOn, c->dChainLongList.as<int32_t>());
    MM_HIP(c, hipGetLastError());
    const dim3 longGrid((unsigned)(longOn ? c->chainCUs * MM_CHAIN_LONG_WG_PER_CU : 1));
    if (longOn) {                                                  // once: rows to the staging array, counts into cntRows before the scan
      hipLaunchKernelGGL(k_chain_reads_long, longGrid, dim3(64), 0, c->stream, E, recs, c->dChainBegin.as<int32_t>(), c->dChainEnd.as<int32_t>(),
                         c->dReadLen.as<int32_t>(), c->dChainLongList.as<int32_t>(), c->dChainCntR.as<int32_t>(), c->dChainStage.as<mm_chain_row>(), totals);
      MM_HIP(c, hipGetLastError());
    }
    const int64_t* dTotal = nullptr;                               // (the two scans share dScanTmp: each total is copied out behind its scan)
    int rc = mm_scan_i32_to_i64_dev(c, (int64_t)nR, c->dChainCntR.as<int32_t>(), c->dChainOffR.as<int64_t>(), &dTotal); if (rc != MM_OK) return rc;
    MM_HIP(c, hipMemcpyAsync(totals + MM_CT_ROWS, dTotal, 8, hipMemcpyDeviceToDevice, c->stream));
    rc = mm_scan_i32_to_i64_dev(c, (int64_t)nR, c->dChainCntL.as<int32_t>(), c->dChainOffL.as<int64_t>(), &dTotal); if (rc != MM_OK) return rc;
    MM_HIP(c, hipMemcpyAsync(totals + MM_CT_LEFT, dTotal, 8, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL((k_chain_reads<true>), grid, block, 0, c->stream, E, (int)nR, recs, c->dChainBegin.as<int32_t>(), c->dChainEnd.as<int32_t>(),
                       c->dReadLen.as<int32_t>(), (int32_t*)nullptr, (int32_t*)nullptr, c->dChainOffR.as<int64_t>(), c->dChainOffL.as<int64_t>(),
                       c->dChainRows.as<mm_chain_row>(), c->dChainLeft.as<mm_mapping>(), totals, longOn, (int32_t*)nullptr);
    MM_HIP(c, hipGetLastError());
    if (longOn) {
      hipLaunchKernelGGL(k_chain_copy_long, longGrid, dim3(64), 0, c->stream, c->dChainLongList.as<int32_t>(), c->dChainBegin.as<int32_t>(), c->dChainCntR.as<int32_t>(),
                         c->dChainOffR.as<int64_t>(), c->dChainStage.as<mm_chain_row>(), c->dChainRows.as<mm_chain_row>(), totals);
      MM_HIP(c, hipGetLastError());
    }
    unsigned long long h[MM_CT_WORDS];
    MM_HIP(c, hipMemcpyAsync(h, totals, sizeof h, hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipStreamSynchronize(c->stream));                    // the stage's one host wait
    c->chRows = (size_t)h[MM_CT_ROWS]; c->chLeft = (size_t)h[MM_CT_LEFT]; c->chOffered = (size_t)h[MM_CT_OFFERED]; c->chFinished = (size_t)h[MM_CT_FINISHED];
    c->chLongOffered = h[MM_CT_LONG_OFFERED]; c->chLongFinished = h[MM_CT_LONG_FINISHED];
    c->chGroupReads = h[MM_CT_GROUP_READS]; c->chGroupRuns = h[MM_CT_GROUP_RUNS];
    if (h[MM_CT_BAD]) {
      c->err = grouped ? "mm_chain_reads: corrupt record: a candidate mapping names a sketch size or shared count outside the identity table, or a contig outside the index"
                       : "mm_chain_reads: corrupt record: a candidate mapping names a sketch size or shared count outside the identity table";
      return MM_ERR_STATE;
    }
    if (c->chRows > nM || c->chLeft > nM) { c->err = "mm_chain_reads: internal error: more rows or left-over records than records"; return MM_ERR_CAPACITY; }
  }
  c->chainPass = c->tot.nPasses;
  return MM_OK;
}

static bool chain_valid(const mm_ctx* c) { return c->mapped && c->chainPass != 0 && c->chainPass == c->tot.nPasses; }

int mm_chain_counts(const mm_ctx* c, size_t* offered, size_t* finished, size_t* rows, size_t* leftover) {
  if (!chain_valid(c)) { const_cast<mm_ctx*>(c)->err = "mm_chain_counts: mm_chain_reads has not run on the mapped batch"; return MM_ERR_STATE; }
  if (offered) *offered = c->chOffered;
  if (finished) *finished = c->chFinished;
  if (rows) *rows = c->chRows;
  if (leftover) *leftover = c->chLeft;
  return MM_OK;
}

int mm_chain_long_counts(const mm_ctx* c, uint64_t* offered, uint64_t* finished) {
  if (!chain_valid(c)) { const_cast<mm_ctx*>(c)->err = "mm_chain_long_counts: mm_chain_reads has not run on the mapped batch"; return MM_ERR_STATE; }
  if (offered) *offered = c->chLongOffered;
  if (finished) *finished = c->chLongFinished;
  return MM_OK;
}

int mm_chain_group_counts(const mm_ctx* c, uint64_t* reads, uint64_t* runs) {
  if (!chain_valid(c)) { const_cast<mm_ctx*>(c)->err = "mm_chain_group_counts: mm_chain_reads has not run on the mapped batch"; return MM_ERR_STATE; }
  if (reads) *reads = c->chGroupReads;
  if (runs) *runs = c->chGroupRuns;
  return MM_OK;
}

int mm_chain_download(mm_ctx* c, mm_chain_row* out, size_t cap, size_t* n) {
  if (!chain_valid(c)) { c->err = "mm_chain_download: mm_chain_reads has not run on the mapped batch"; return MM_ERR_STATE; }
  if (n) *n = c->chRows;
  if (c->chRows > cap) { c->err = "mm_chain_download: destination too small"; return MM_ERR_ARG; }
  if (c->chRows) {
    MM_HIP(c, hipSetDevice(c->device));
    MM_HIP(c, hipMemcpyAsync(out, c->dChainRows.p, c->chRows * sizeof(mm_chain_row), hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipStreamSynchronize(c->stream));
  }
  return MM_OK;
}

int mm_chain_leftover_download(mm_ctx* c, mm_mapping* out, size_t cap, size_t* n) {
  if (!chain_valid(c)) { c->err = "mm_chain_leftover_download: mm_chain_reads has not run on the mapped batch"; return MM_ERR_STATE; }
  if (n) *n = c->chLeft;
  if (c->chLeft > cap) { c->err = "mm_chain_leftover_download: destination too small"; return MM_ERR_ARG; }
  if (c->chLeft) {
    MM_HIP(c, hipSetDevice(c->device));
    MM_HIP(c, hipMemcpyAsync(out, c->dChainLeft.p, c->chLeft * sizeof(mm_mapping), hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipStreamSynchronize(c->stream));
  }
  return MM_OK;
}

int mm_chain_device(const mm_ctx* c, const mm_chain_row** dRows, size_t* nRows, const mm_mapping** dLeftover, size_t* nLeftover) {
  if (!chain_valid(c)) { const_cast<mm_ctx*>(c)->err = "mm_chain_device: mm_chain_reads has not run on the mapped batch"; return MM_ERR_STATE; }
  if (dRows) *dRows = c->dChainRows.as<mm_chain_row>();
  if (nRows) *nRows = c->chRows;
  if (dLeftover) *dLeftover = c->dChainLeft.as<mm_mapping>();
  if (nLeftover) *nLeftover = c->chLeft;
  return MM_OK;
}

}  // extern "C"
