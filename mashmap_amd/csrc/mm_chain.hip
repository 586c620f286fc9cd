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
#include "mm_internal.h"
#include "mm_chain_core.h"
#include "../host/mm_stats.hpp"

enum : int { MM_CT_ROWS = 0, MM_CT_LEFT = 1, MM_CT_OFFERED = 2, MM_CT_FINISHED = 3, MM_CT_BAD = 4, MM_CT_WORDS = 5 };   // dChainTotals

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

template <bool WRITE>
__global__ void __launch_bounds__(128)
k_chain_reads(mm_chain_env E, int nReads, const mm_mapping* __restrict__ recs, const int32_t* __restrict__ begin, const int32_t* __restrict__ end,
              const int32_t* __restrict__ readLen, int32_t* __restrict__ cntRows, int32_t* __restrict__ cntLeft,
              const int64_t* __restrict__ offRows, const int64_t* __restrict__ offLeft, mm_chain_row* __restrict__ rows, mm_mapping* __restrict__ left,
              unsigned long long* __restrict__ totals) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  int n = 0, b = 0;
  if (r < nReads) { b = begin[r]; n = end[r] - b; if (n < 0) n = 0; }
  int nRows = 0, nLeft = 0;
  if (n > MM_CHAIN_MAX_RECORDS) {
    nLeft = n;
    if (WRITE) { mm_mapping* dst = left + offLeft[r]; for (int i = 0; i < n; i++) dst[i] = recs[b + i]; }
  } else if (n > 0) {
    nRows = mm_chain_read(E, recs + b, n, readLen[r], WRITE ? rows + offRows[r] : (mm_chain_row*)nullptr);
    if (nRows < 0) { nRows = 0; if (!WRITE) atomicAdd(&totals[MM_CT_BAD], 1ull); }     // MM_CHAIN_BAD_RECORD: the launcher reports it, nothing of the read is written
  }
  if (!WRITE) {
    if (r < nReads) { cntRows[r] = nRows; cntLeft[r] = nLeft; }
    const int offered = __syncthreads_count(n > 0), finished = __syncthreads_count(n > 0 && nLeft == 0);
    if (threadIdx.x == 0) {
      if (offered) atomicAdd(&totals[MM_CT_OFFERED], (unsigned long long)offered);
      if (finished) atomicAdd(&totals[MM_CT_FINISHED], (unsigned long long)finished);
    }
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
  if (c->P.flags & MM_FLAG_SKIP_PREFIX) { c->err = "mm_chain_reads: MM_FLAG_SKIP_PREFIX is set (filterByGroup then runs reference group by reference group)"; return MM_ERR_STATE; }
  if (c->P.flags & MM_FLAG_NO_SPLIT) { c->err = "mm_chain_reads: MM_FLAG_NO_SPLIT is set"; return MM_ERR_STATE; }
  if (c->P.sketchSize > MM_CHAIN_MAX_SKETCH) { c->err = "mm_chain_reads: sketchSize above 2048 (the identity table would be larger than 16 MB)"; return MM_ERR_STATE; }
  if (!c->haveChainTables) { c->err = "mm_chain_reads: mm_set_chain_tables was not called"; return MM_ERR_STATE; }
  if (!c->mapped || !c->haveReplayTables) { c->err = "mm_chain_reads: nothing mapped, or mm_set_replay_tables / mm_set_tables_default was not called"; return MM_ERR_STATE; }
  c->chOffered = c->chFinished = c->chRows = c->chLeft = 0;
  const size_t nR = c->nReads, nM = c->nMappings;
  if (nM > (size_t)0x7fffffff || nR > (size_t)0x7fffffff) { c->err = "mm_chain_reads: more than 2^31 - 1 records in one batch"; return MM_ERR_CAPACITY; }
  if (nR && nM) {
    MM_HIP(c, hipSetDevice(c->device));
    MM_HIP(c, c->dChainBegin.ensure(nR * 4 + 64)); MM_HIP(c, c->dChainEnd.ensure(nR * 4 + 64));
    MM_HIP(c, c->dChainCntR.ensure(nR * 4 + 64)); MM_HIP(c, c->dChainCntL.ensure(nR * 4 + 64));
    MM_HIP(c, c->dChainOffR.ensure(nR * 8 + 64)); MM_HIP(c, c->dChainOffL.ensure(nR * 8 + 64));
    MM_HIP(c, c->dChainRows.ensure(nM * sizeof(mm_chain_row) + 64)); MM_HIP(c, c->dChainLeft.ensure(nM * sizeof(mm_mapping) + 64));   // a read leaves at most as many rows as it has records
    MM_HIP(c, c->dChainTotals.ensure(MM_CT_WORDS * 8));
    MM_HIP(c, hipMemsetAsync(c->dChainBegin.p, 0, nR * 4, c->stream)); MM_HIP(c, hipMemsetAsync(c->dChainEnd.p, 0, nR * 4, c->stream));
    MM_HIP(c, hipMemsetAsync(c->dChainTotals.p, 0, MM_CT_WORDS * 8, c->stream));
    const mm_mapping* recs = c->dMappings.as<mm_mapping>();
    hipLaunchKernelGGL(k_chain_ranges, dim3((unsigned)((nM + 255) / 256)), dim3(256), 0, c->stream, (long long)nM, recs, (int)c->seqCounterBase, (int)nR,
                       c->dChainBegin.as<int32_t>(), c->dChainEnd.as<int32_t>());
    mm_chain_env E;
    E.p = c->chainP; E.kmerSize = c->P.kmerSize; E.segLength = c->P.segLength; E.stride = c->P.sketchSize + 1; E.identity = c->dChainIdent.as<float>();
    unsigned long long* totals = c->dChainTotals.as<unsigned long long>();
    const dim3 grid((unsigned)((nR + 127) / 128)), block(128);
    hipLaunchKernelGGL((k_chain_reads<false>), grid, block, 0, c->stream, E, (int)nR, recs, c->dChainBegin.as<int32_t>(), c->dChainEnd.as<int32_t>(),
                       c->dReadLen.as<int32_t>(), c->dChainCntR.as<int32_t>(), c->dChainCntL.as<int32_t>(), (const int64_t*)nullptr, (const int64_t*)nullptr,
                       (mm_chain_row*)nullptr, (mm_mapping*)nullptr, totals);
    MM_HIP(c, hipGetLastError());
    const int64_t* dTotal = nullptr;                               // (the two scans share dScanTmp: each total is copied out behind its scan)
    int rc = mm_scan_i32_to_i64_dev(c, (int64_t)nR, c->dChainCntR.as<int32_t>(), c->dChainOffR.as<int64_t>(), &dTotal); if (rc != MM_OK) return rc;
    MM_HIP(c, hipMemcpyAsync(totals + MM_CT_ROWS, dTotal, 8, hipMemcpyDeviceToDevice, c->stream));
    rc = mm_scan_i32_to_i64_dev(c, (int64_t)nR, c->dChainCntL.as<int32_t>(), c->dChainOffL.as<int64_t>(), &dTotal); if (rc != MM_OK) return rc;
    MM_HIP(c, hipMemcpyAsync(totals + MM_CT_LEFT, dTotal, 8, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL((k_chain_reads<true>), grid, block, 0, c->stream, E, (int)nR, recs, c->dChainBegin.as<int32_t>(), c->dChainEnd.as<int32_t>(),
                       c->dReadLen.as<int32_t>(), (int32_t*)nullptr, (int32_t*)nullptr, c->dChainOffR.as<int64_t>(), c->dChainOffL.as<int64_t>(),
                       c->dChainRows.as<mm_chain_row>(), c->dChainLeft.as<mm_mapping>(), totals);
    MM_HIP(c, hipGetLastError());
    unsigned long long h[MM_CT_WORDS];
    MM_HIP(c, hipMemcpyAsync(h, totals, sizeof h, hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipStreamSynchronize(c->stream));                    // the stage's one host wait
    c->chRows = (size_t)h[MM_CT_ROWS]; c->chLeft = (size_t)h[MM_CT_LEFT]; c->chOffered = (size_t)h[MM_CT_OFFERED]; c->chFinished = (size_t)h[MM_CT_FINISHED];
    if (h[MM_CT_BAD]) { c->err = "mm_chain_reads: corrupt record: a candidate mapping names a sketch size or shared count outside the identity table"; return MM_ERR_STATE; }
    if (c->chRows > nM || c->chLeft > nM) { c->err = "mm_chain_reads: internal error: more rows or left-over records than records"; return MM_ERR_CAPACITY; }
  }
  c->chainPass = c->nPasses;
  return MM_OK;
}

static bool chain_valid(const mm_ctx* c) { return c->mapped && c->chainPass != 0 && c->chainPass == c->nPasses; }

int mm_chain_counts(const mm_ctx* c, size_t* offered, size_t* finished, size_t* rows, size_t* leftover) {
  if (!chain_valid(c)) { const_cast<mm_ctx*>(c)->err = "mm_chain_counts: mm_chain_reads has not run on the mapped batch"; return MM_ERR_STATE; }
  if (offered) *offered = c->chOffered;
  if (finished) *finished = c->chFinished;
  if (rows) *rows = c->chRows;
  if (leftover) *leftover = c->chLeft;
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
