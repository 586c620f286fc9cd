// mashmap_amd/csrc/mm_paf.hip -- the PAF lines of a pass on the device (gfx950): behind mm_chain_reads, or for rows the caller brings,
// what MapPost::finishRows + appendReadMappings make of every row (mm_paf_rows, mm_paf_format).
//
//   MapPost::reportSteps          filterFalseHighIdentity :441, mappingBoundarySanityCheck :1714     mashmap_amd/host/skch_map_post.hpp
//   MapPost::appendReadMappings   the text of a line                                                  computeMap.hpp:1758-1806
//
// The restatement is mm_paf_core.h (one function per row; the header says why its bytes are the host's); this file measures every
// row, places the lines with the scan the other stages use, and writes them.  No workgroup waits for another.
//
//   k_paf_measure    a lane per row: the two report steps, the length of the numeric part (mm_paf_numeric into a buffer of the lane's own, of
//                    which no character is read: the compiler removes the buffer, the kernel has no scratch memory), plus the two names' lengths -> len[row], 0 for a
//                    dropped row.  A row with a field that is not formattable sets its read's flag.  A corrupt row -- refSeqId outside
//                    the contigs, querySeqId outside the reads or below the row's before it -- is counted and reads no table.
//   k_paf_unflag     a lane per row: the rows of a flagged read get length 0 (the read is handed over as a whole); counts the lines.
//   mm_scan_i32_to_i64_dev   rowOff[row], and the total behind the last.
//   k_paf_offsets    a lane per read r (and one for nReads): off[r] = rowOff[first row of a read >= r], found by bisection over the rows'
//                    querySeqId (they are read-major) -- a read without rows has no first row of its own to look at, and this way no
//                    read waits for its neighbour.  Counts the reads with text and the reads handed over.
//   -- the one host wait: the counts, among them the text's size; the text buffer is sized from it --
//   k_paf_write      a wave (a workgroup of 64) per 64 consecutive rows.  Lane l formats the numeric part of row first + l into its own LDS
//                    slot (MM_PAF_SLOT bytes, 41 words: an odd stride, the lanes' byte stores fall on different banks) and leaves the
//                    places and lengths of its two names beside it; the 65 row offsets are in LDS.  Then the wave writes the span
//                    [rowOff[first], rowOff[first + 64]) together: lane l takes the aligned 4-byte words l, l + 64, ... of the span, finds
//                    the row of a word's first byte by bisection over the offsets (rows of length 0 fall out of it), and fetches every byte
//                    from the part of the line it lies in -- query name (HBM), slot up to the reference name (LDS), reference name (HBM),
//                    rest of the slot (LDS) -- stepping to the next row where a line ends inside the word.  A whole word is one 4-byte
//                    store, 256 consecutive bytes a wave and instruction; the partial words at the two ends of the span are byte
//                    stores, so two waves never store to the same byte.  Names of any length go through the same loop.
//   Bounds before speed: a store is made only below the text's size, a name byte is read only inside its table, a slot byte inside the slot.
#include "mm_internal.h"
#include "mm_paf_core.h"

enum : int { MM_PT_BYTES = 0, MM_PT_LINES = 1, MM_PT_DROPPED = 2, MM_PT_BAD = 3, MM_PT_READS_TEXT = 4, MM_PT_HANDED = 5, MM_PT_WORDS = 8 };   // dPafTotals
#define MM_PAF_SLOT 164                      // MM_PAF_NUMERIC_MAX rounded up to whole words
#define MM_PAF_NAME_MAX ((uint64_t)1 << 30)  // a name is shorter than this: a line's length fits an int32
static_assert(MM_PAF_SLOT >= MM_PAF_NUMERIC_MAX && MM_PAF_SLOT % 4 == 0 && (MM_PAF_SLOT / 4) % 2 == 1, "k_paf_write's slot holds the longest numeric part, on an odd word stride");

// what the kernels need beside the rows
struct mm_paf_env {
  mm_paf_params p;
  mm_paf_mapq mapq;
  const int32_t* refLens; const char* refNames; const uint64_t* refNameOff; uint64_t refNameBytes; int32_t nContigs;
  const char* qNames; const uint64_t* qNameOff; uint64_t qNameBytes;
  const int32_t* readLens; int32_t firstSeqId, nReads;
};

// read index and contig of a row, or false: a corrupt row
__device__ __forceinline__ bool paf_row_ok(const mm_paf_env& E, const mm_chain_row* __restrict__ rows, long long i, const mm_chain_row& r, unsigned* rd) {
  *rd = (unsigned)(r.querySeqId - E.firstSeqId);
  if (*rd >= (unsigned)E.nReads || (unsigned)r.refSeqId >= (unsigned)E.nContigs) return false;
  return i == 0 || rows[i - 1].querySeqId <= r.querySeqId;
}

__global__ void __launch_bounds__(256)
k_paf_measure(mm_paf_env E, long long nRows, const mm_chain_row* __restrict__ rows, int32_t* __restrict__ len, uint8_t* __restrict__ flag,
              unsigned long long* __restrict__ totals) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool dropped = false, bad = false;
  if (i < nRows) {
    mm_chain_row r = rows[i];
    unsigned rd;
    int32_t L = 0;
    if (!paf_row_ok(E, rows, i, r, &rd)) bad = true;
    else {
      const int32_t clen = E.refLens[r.refSeqId];
      if (!mm_paf_report_row(E.p, r, clen, E.readLens[rd])) dropped = true;
      else {
        char buf[MM_PAF_NUMERIC_MAX];
        int beforeRef;
        const int n = mm_paf_numeric(E.p, r, clen, E.mapq, buf, &beforeRef);
        if (n < 0) flag[rd] = 1;             // (several lanes may store the same 1)
        else L = n + (int32_t)(E.qNameOff[rd + 1] - E.qNameOff[rd]) + (int32_t)(E.refNameOff[r.refSeqId + 1] - E.refNameOff[r.refSeqId]);
      }
    }
    len[i] = L;
  }
  const int nDropped = __syncthreads_count(dropped), nBad = __syncthreads_count(bad);
  if (threadIdx.x == 0) {
    if (nDropped) atomicAdd(&totals[MM_PT_DROPPED], (unsigned long long)nDropped);
    if (nBad) atomicAdd(&totals[MM_PT_BAD], (unsigned long long)nBad);
  }
}

__global__ void __launch_bounds__(256)
k_paf_unflag(long long nRows, const mm_chain_row* __restrict__ rows, int32_t firstSeqId, int32_t nReads, const uint8_t* __restrict__ flag,
             int32_t* __restrict__ len, unsigned long long* __restrict__ totals) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool line = false;
  if (i < nRows) {
    const unsigned rd = (unsigned)(rows[i].querySeqId - firstSeqId);
    if (rd < (unsigned)nReads && flag[rd]) len[i] = 0;
    else line = len[i] > 0;
  }
  const int nLines = __syncthreads_count(line);
  if (threadIdx.x == 0 && nLines) atomicAdd(&totals[MM_PT_LINES], (unsigned long long)nLines);
}

// the first row of a read >= r (nRows when there is none)
__device__ __forceinline__ long long paf_first_row(long long nRows, const mm_chain_row* __restrict__ rows, int32_t firstSeqId, long long r) {
  long long lo = 0, hi = nRows;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if ((long long)rows[mid].querySeqId - (long long)firstSeqId < r) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// rowOff has nRows + 1 entries (the total behind the last row); off gets nReads + 1
__global__ void __launch_bounds__(256)
k_paf_offsets(long long nRows, const mm_chain_row* __restrict__ rows, int32_t firstSeqId, int32_t nReads, const int64_t* __restrict__ rowOff,
              const uint8_t* __restrict__ flag, int64_t* __restrict__ off, unsigned long long* __restrict__ totals) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool text = false, handed = false;
  if (r <= nReads) {
    const int64_t a = rowOff[paf_first_row(nRows, rows, firstSeqId, r)];
    off[r] = a;
    if (r < nReads) {
      text = rowOff[paf_first_row(nRows, rows, firstSeqId, r + 1)] > a;
      handed = flag[r] != 0;
    }
  }
  const int nText = __syncthreads_count(text), nHanded = __syncthreads_count(handed);
  if (threadIdx.x == 0) {
    if (nText) atomicAdd(&totals[MM_PT_READS_TEXT], (unsigned long long)nText);
    if (nHanded) atomicAdd(&totals[MM_PT_HANDED], (unsigned long long)nHanded);
  }
}

__global__ void __launch_bounds__(64)
k_paf_write(mm_paf_env E, long long nRows, const mm_chain_row* __restrict__ rows, const int64_t* __restrict__ rowOff, char* __restrict__ text, long long textBytes) {
  __shared__ long long sOff[65];
  __shared__ __attribute__((aligned(4))) char sSlot[64][MM_PAF_SLOT];
  __shared__ unsigned long long sQAt[64], sRAt[64];                // where the row's two names start in their tables
  __shared__ int sQLen[64], sRLen[64], sBefore[64];
  const int lane = threadIdx.x;
  const long long first = (long long)blockIdx.x * 64, i = first + lane;
  sOff[lane] = rowOff[i < nRows ? i : nRows];                      // behind the last row: the total, i.e. rows of length 0
  if (lane == 0) sOff[64] = rowOff[first + 64 < nRows ? first + 64 : nRows];
  sQAt[lane] = 0; sRAt[lane] = 0; sQLen[lane] = 0; sRLen[lane] = 0; sBefore[lane] = 0;
  __syncthreads();
  const long long myLen = sOff[lane + 1] - sOff[lane];
  if (i < nRows && myLen > 0) {                                    // what k_paf_measure measured, once more, this time kept
    mm_chain_row r = rows[i];
    unsigned rd;
    if (paf_row_ok(E, rows, i, r, &rd)) {
      const int32_t clen = E.refLens[r.refSeqId];
      if (mm_paf_report_row(E.p, r, clen, E.readLens[rd])) {
        int beforeRef = 0;
        const int n = mm_paf_numeric(E.p, r, clen, E.mapq, sSlot[lane], &beforeRef);
        const unsigned long long qAt = E.qNameOff[rd], rAt = E.refNameOff[r.refSeqId];
        const int qLen = (int)(E.qNameOff[rd + 1] - qAt), rLen = (int)(E.refNameOff[r.refSeqId + 1] - rAt);
        if (n > 0 && (long long)n + qLen + rLen == myLen) { sQAt[lane] = qAt; sRAt[lane] = rAt; sQLen[lane] = qLen; sRLen[lane] = rLen; sBefore[lane] = beforeRef; }
      }
    }
  }
  __syncthreads();
  const long long start = sOff[0];
  long long end = sOff[64];
  if (end > textBytes) end = textBytes;
  // byte `rel` of row j's line
  auto byteOf = [&](int j, long long rel) -> unsigned {
    const long long qLen = sQLen[j], before = sBefore[j], rLen = sRLen[j];
    if (rel < qLen) { const unsigned long long at = sQAt[j] + (unsigned long long)rel; return at < E.qNameBytes ? (unsigned char)E.qNames[at] : (unsigned)'?'; }
    rel -= qLen;
    if (rel < before) return (unsigned char)sSlot[j][rel];
    rel -= before;
    if (rel < rLen) { const unsigned long long at = sRAt[j] + (unsigned long long)rel; return at < E.refNameBytes ? (unsigned char)E.refNames[at] : (unsigned)'?'; }
    rel += before - rLen;
    return rel < MM_PAF_SLOT ? (unsigned char)sSlot[j][rel] : (unsigned)'?';
  };
  for (long long w = (start & ~3ll) + 4 * lane; w < end; w += 256) {
    const long long p0 = w > start ? w : start;
    if (p0 >= end) continue;
    int lo = 0, hi = 64;                                           // the last row j with sOff[j] <= p0: p0 < end = sOff[64], so sOff[j + 1] > p0
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sOff[mid] <= p0) lo = mid; else hi = mid;
    }
    int j = lo;
    unsigned word = 0, have = 0;
    for (int b = 0; b < 4; b++) {
      const long long p = w + b;
      if (p < start || p >= end) continue;
      while (j < 63 && p >= sOff[j + 1]) j++;
      word |= byteOf(j, p - sOff[j]) << (8 * b);
      have |= 1u << b;
    }
    if (have == 15u) *reinterpret_cast<unsigned*>(text + w) = word;             // text is 256-byte aligned (hipMalloc), w a multiple of 4
    else
      for (int b = 0; b < 4; b++)
        if (have & (1u << b)) text[w + b] = (char)(word >> (8 * b));
  }
}

static bool paf_offsets_ok(const uint64_t* off, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i] || off[i + 1] - off[i] >= MM_PAF_NAME_MAX) return false;
  return true;
}
static bool paf_valid(const mm_ctx* c) { return c->pafDone && c->pafGen == c->batchGen && c->pafPass == c->tot.nPasses; }

// the stage on rows that are on the device: dRows[nRows], dReadLens[nReads]
static int paf_run(mm_ctx* c, const char* who, const mm_chain_row* dRows, size_t nRows, const int32_t* dReadLens, int32_t firstSeqId, const char* queryNames,
                   const uint64_t* queryNameOff, size_t nReads) {
  const uint64_t qBytes = nReads ? queryNameOff[nReads] : 0;
  MM_HIP(c, c->dPafQNames.ensure(qBytes + 64)); MM_HIP(c, c->dPafQOff.ensure((nReads + 1) * 8 + 64));
  MM_HIP(c, c->dPafOff.ensure((nReads + 1) * 8 + 64)); MM_HIP(c, c->dPafFlag.ensure(nReads + 64));
  MM_HIP(c, c->dPafTotals.ensure(MM_PT_WORDS * 8)); MM_HIP(c, c->dPafText.ensure(64));
  MM_HIP(c, hipMemsetAsync(c->dPafOff.p, 0, (nReads + 1) * 8, c->stream));
  MM_HIP(c, hipMemsetAsync(c->dPafFlag.p, 0, nReads + 64, c->stream));
  MM_HIP(c, hipMemsetAsync(c->dPafTotals.p, 0, MM_PT_WORDS * 8, c->stream));
  mm_paf_env E;
  E.p = c->pafP;
  E.mapq.thresholds = c->dPafMapqT.as<float>(); E.mapq.text = c->dPafMapqText.as<char>(); E.mapq.n = c->pafNMapq;
  E.refLens = c->dPafRefLens.as<int32_t>(); E.refNames = c->dPafRefNames.as<char>(); E.refNameOff = c->dPafRefOff.as<uint64_t>();
  E.refNameBytes = c->pafRefNameBytes; E.nContigs = (int32_t)c->pafNContigs;
  E.qNames = c->dPafQNames.as<char>(); E.qNameOff = c->dPafQOff.as<uint64_t>(); E.qNameBytes = qBytes;
  E.readLens = dReadLens; E.firstSeqId = firstSeqId; E.nReads = (int32_t)nReads;
  unsigned long long h[MM_PT_WORDS] = {0};
  if (nRows && nReads) {
    if (qBytes) MM_HIP(c, hipMemcpyAsync(c->dPafQNames.p, queryNames, qBytes, hipMemcpyHostToDevice, c->stream));
    MM_HIP(c, hipMemcpyAsync(c->dPafQOff.p, queryNameOff, (nReads + 1) * 8, hipMemcpyHostToDevice, c->stream));
    MM_HIP(c, c->dPafLen.ensure(nRows * 4 + 64)); MM_HIP(c, c->dPafRowOff.ensure((nRows + 1) * 8 + 64));
    unsigned long long* totals = c->dPafTotals.as<unsigned long long>();
    const dim3 rowGrid((unsigned)((nRows + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_paf_measure, rowGrid, block, 0, c->stream, E, (long long)nRows, dRows, c->dPafLen.as<int32_t>(), c->dPafFlag.as<uint8_t>(), totals);
    MM_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_paf_unflag, rowGrid, block, 0, c->stream, (long long)nRows, dRows, firstSeqId, (int32_t)nReads, c->dPafFlag.as<uint8_t>(), c->dPafLen.as<int32_t>(), totals);
    MM_HIP(c, hipGetLastError());
    const int64_t* dTotal = nullptr;
    const int rc = mm_scan_i32_to_i64_dev(c, (int64_t)nRows, c->dPafLen.as<int32_t>(), c->dPafRowOff.as<int64_t>(), &dTotal);
    if (rc != MM_OK) return rc;
    MM_HIP(c, hipMemcpyAsync(c->dPafRowOff.as<int64_t>() + nRows, dTotal, 8, hipMemcpyDeviceToDevice, c->stream));
    MM_HIP(c, hipMemcpyAsync(totals + MM_PT_BYTES, dTotal, 8, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(k_paf_offsets, dim3((unsigned)((nReads + 1 + 255) / 256)), block, 0, c->stream, (long long)nRows, dRows, firstSeqId, (int32_t)nReads,
                       c->dPafRowOff.as<int64_t>(), c->dPafFlag.as<uint8_t>(), c->dPafOff.as<int64_t>(), totals);
    MM_HIP(c, hipGetLastError());
    MM_HIP(c, hipMemcpyAsync(h, totals, sizeof h, hipMemcpyDeviceToHost, c->stream));
  }
  MM_HIP(c, hipStreamSynchronize(c->stream));                      // the stage's one host wait
  if (h[MM_PT_BAD]) {
    c->err = std::string(who) + ": corrupt row: a row names a contig outside the tables of mm_set_paf_tables or a read outside the batch, or the rows are not in read order";
    return MM_ERR_STATE;
  }
  if (h[MM_PT_BYTES]) {
    MM_HIP(c, c->dPafText.ensure((size_t)h[MM_PT_BYTES] + 64));
    hipLaunchKernelGGL(k_paf_write, dim3((unsigned)((nRows + 63) / 64)), dim3(64), 0, c->stream, E, (long long)nRows, dRows, c->dPafRowOff.as<int64_t>(),
                       c->dPafText.as<char>(), (long long)h[MM_PT_BYTES]);
    MM_HIP(c, hipGetLastError());                                  // (not waited for: the downloads are behind it on the stream)
  }
  c->pafBytes = h[MM_PT_BYTES]; c->pafLines = h[MM_PT_LINES]; c->pafDropped = h[MM_PT_DROPPED]; c->pafReadsText = h[MM_PT_READS_TEXT]; c->pafHanded = h[MM_PT_HANDED];
  c->pafReads = nReads; c->pafGen = c->batchGen; c->pafPass = c->tot.nPasses; c->pafDone = true;
  return MM_OK;
}

extern "C" {

int mm_set_paf_tables(mm_ctx* c, const mm_paf_params* params, const float* mapqThresholds, const char* mapqText, size_t nMapq,
                      const char* refNames, const uint64_t* refNameOff, const int32_t* refLens, size_t nContigs) {
  if (!c) return MM_ERR_ARG;
  if (!params || !mapqThresholds || !mapqText || !refNameOff || (nContigs && !refLens)) { c->err = "mm_set_paf_tables: need the parameter block, the mapQ table, the contigs' name offsets and lengths"; return MM_ERR_ARG; }
  if (!mm_paf_params_ok(*params)) { c->err = "mm_set_paf_tables: a sparsity threshold below 2^64 - 1 (sparsifyMappings hashes through std::hash<float> and stays on the host)"; return MM_ERR_ARG; }
  bool ok = nMapq >= 1 && nMapq <= MM_PAF_MAX_MAPQ && mapqThresholds[0] == 0.0f;
  for (size_t i = 0; ok && i < nMapq; i++) {
    ok = mapqThresholds[i] <= 1.0f && (i == 0 || mapqThresholds[i - 1] < mapqThresholds[i]) && mapqText[i * MM_PAF_MAPQ_TEXT + MM_PAF_MAPQ_TEXT - 1] == 0 && mapqText[i * MM_PAF_MAPQ_TEXT] != 0;
  }
  if (!ok) { c->err = "mm_set_paf_tables: the mapQ table needs 1 .. 128 ascending thresholds from 0 to at most 1 and 8 bytes of NUL-padded text an entry"; return MM_ERR_ARG; }
  if (nContigs > (size_t)0x7fffffff || !paf_offsets_ok(refNameOff, nContigs)) { c->err = "mm_set_paf_tables: the contigs' name offsets are not non-decreasing (or a name of 2^30 bytes and more)"; return MM_ERR_ARG; }
  const uint64_t nameBytes = refNameOff[nContigs];
  if (nameBytes && !refNames) { c->err = "mm_set_paf_tables: name offsets without names"; return MM_ERR_ARG; }
  c->havePafTables = false; c->pafDone = false;
  MM_HIP(c, hipSetDevice(c->device));
  MM_HIP(c, c->dPafMapqT.ensure(nMapq * 4 + 64)); MM_HIP(c, c->dPafMapqText.ensure(nMapq * MM_PAF_MAPQ_TEXT + 64));
  MM_HIP(c, c->dPafRefNames.ensure(nameBytes + 64)); MM_HIP(c, c->dPafRefOff.ensure((nContigs + 1) * 8 + 64)); MM_HIP(c, c->dPafRefLens.ensure(nContigs * 4 + 64));
  MM_HIP(c, hipMemcpyAsync(c->dPafMapqT.p, mapqThresholds, nMapq * 4, hipMemcpyHostToDevice, c->stream));
  MM_HIP(c, hipMemcpyAsync(c->dPafMapqText.p, mapqText, nMapq * MM_PAF_MAPQ_TEXT, hipMemcpyHostToDevice, c->stream));
  if (nameBytes) MM_HIP(c, hipMemcpyAsync(c->dPafRefNames.p, refNames, nameBytes, hipMemcpyHostToDevice, c->stream));
  MM_HIP(c, hipMemcpyAsync(c->dPafRefOff.p, refNameOff, (nContigs + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (nContigs) MM_HIP(c, hipMemcpyAsync(c->dPafRefLens.p, refLens, nContigs * 4, hipMemcpyHostToDevice, c->stream));
  MM_HIP(c, hipStreamSynchronize(c->stream));
  c->pafP = *params; c->pafNMapq = (int32_t)nMapq; c->pafNContigs = nContigs; c->pafRefNameBytes = nameBytes; c->havePafTables = true;
  return MM_OK;
}

int mm_paf_rows(mm_ctx* c, const char* queryNames, const uint64_t* queryNameOff, size_t nReads) {
  if (!c) return MM_ERR_ARG;
  c->pafDone = false;
  if (!c->havePafTables) { c->err = "mm_paf_rows: mm_set_paf_tables was not called"; return MM_ERR_STATE; }
  if (!(c->mapped && c->chainPass != 0 && c->chainPass == c->tot.nPasses)) { c->err = "mm_paf_rows: mm_chain_reads has not run on the mapped batch"; return MM_ERR_STATE; }
  if (nReads != c->nReads) { c->err = "mm_paf_rows: nReads is not the mapped batch's read count"; return MM_ERR_ARG; }
  if (!queryNameOff || !paf_offsets_ok(queryNameOff, nReads) || (nReads && queryNameOff[nReads] && !queryNames)) {
    c->err = "mm_paf_rows: the reads' name offsets are missing or not non-decreasing (or a name of 2^30 bytes and more)"; return MM_ERR_ARG;
  }
  if (c->chRows > (size_t)0x7fffffff) { c->err = "mm_paf_rows: more than 2^31 - 1 rows"; return MM_ERR_ARG; }
  MM_HIP(c, hipSetDevice(c->device));
  return paf_run(c, "mm_paf_rows", c->dChainRows.as<mm_chain_row>(), c->chRows, c->dReadLen.as<int32_t>(), c->seqCounterBase, queryNames, queryNameOff, nReads);
}

int mm_paf_format(mm_ctx* c, const mm_chain_row* rows, size_t nRows, const int32_t* readLens, int32_t firstSeqId, const char* queryNames,
                  const uint64_t* queryNameOff, size_t nReads) {
  if (!c) return MM_ERR_ARG;
  c->pafDone = false;
  if (!c->havePafTables) { c->err = "mm_paf_format: mm_set_paf_tables was not called"; return MM_ERR_STATE; }
  if (nRows > (size_t)0x7fffffff) { c->err = "mm_paf_format: more than 2^31 - 1 rows"; return MM_ERR_ARG; }
  if (nReads > (size_t)0x7fffffff || (nRows && !rows) || (nReads && !readLens)) { c->err = "mm_paf_format: need the rows and the reads' lengths"; return MM_ERR_ARG; }
  if (!queryNameOff || !paf_offsets_ok(queryNameOff, nReads) || (nReads && queryNameOff[nReads] && !queryNames)) {
    c->err = "mm_paf_format: the reads' name offsets are missing or not non-decreasing (or a name of 2^30 bytes and more)"; return MM_ERR_ARG;
  }
  for (size_t i = 0; i < nRows; i++) {
    const uint32_t rd = (uint32_t)(rows[i].querySeqId - firstSeqId);
    if (rd >= (uint32_t)nReads || (uint32_t)rows[i].refSeqId >= (uint32_t)c->pafNContigs || (i && rows[i - 1].querySeqId > rows[i].querySeqId)) {
      c->err = "mm_paf_format: corrupt row " + std::to_string(i) + ": it names a contig outside the tables of mm_set_paf_tables or a read outside [firstSeqId, firstSeqId + nReads), or breaks read order";
      return MM_ERR_ARG;
    }
  }
  MM_HIP(c, hipSetDevice(c->device));
  MM_HIP(c, c->dPafRows.ensure(nRows * sizeof(mm_chain_row) + 64)); MM_HIP(c, c->dPafReadLens.ensure(nReads * 4 + 64));
  if (nRows) MM_HIP(c, hipMemcpyAsync(c->dPafRows.p, rows, nRows * sizeof(mm_chain_row), hipMemcpyHostToDevice, c->stream));
  if (nReads) MM_HIP(c, hipMemcpyAsync(c->dPafReadLens.p, readLens, nReads * 4, hipMemcpyHostToDevice, c->stream));
  return paf_run(c, "mm_paf_format", c->dPafRows.as<mm_chain_row>(), nRows, c->dPafReadLens.as<int32_t>(), firstSeqId, queryNames, queryNameOff, nReads);
}

int mm_paf_counts(const mm_ctx* c, uint64_t* readsWithText, uint64_t* lines, uint64_t* bytes, uint64_t* dropped, uint64_t* handedReads) {
  if (!c) return MM_ERR_ARG;
  if (!paf_valid(c)) { const_cast<mm_ctx*>(c)->err = "mm_paf_counts: mm_paf_rows / mm_paf_format has not run on the current batch"; return MM_ERR_STATE; }
  if (readsWithText) *readsWithText = c->pafReadsText;
  if (lines) *lines = c->pafLines;
  if (bytes) *bytes = c->pafBytes;
  if (dropped) *dropped = c->pafDropped;
  if (handedReads) *handedReads = c->pafHanded;
  return MM_OK;
}

int mm_paf_download(mm_ctx* c, char* text, size_t cap, size_t* n) {
  if (!c) return MM_ERR_ARG;
  if (!paf_valid(c)) { c->err = "mm_paf_download: mm_paf_rows / mm_paf_format has not run on the current batch"; return MM_ERR_STATE; }
  if (n) *n = (size_t)c->pafBytes;
  if (c->pafBytes > cap || (c->pafBytes && !text)) { c->err = "mm_paf_download: destination too small"; return MM_ERR_ARG; }
  if (c->pafBytes) {
    MM_HIP(c, hipSetDevice(c->device));
    MM_HIP(c, hipMemcpyAsync(text, c->dPafText.p, (size_t)c->pafBytes, hipMemcpyDeviceToHost, c->stream));
    MM_HIP(c, hipStreamSynchronize(c->stream));
  }
  return MM_OK;
}

int mm_paf_offsets_download(mm_ctx* c, int64_t* off, uint8_t* handed) {
  if (!c) return MM_ERR_ARG;
  if (!paf_valid(c)) { c->err = "mm_paf_offsets_download: mm_paf_rows / mm_paf_format has not run on the current batch"; return MM_ERR_STATE; }
  if (!off) { c->err = "mm_paf_offsets_download: need room for nReads + 1 offsets"; return MM_ERR_ARG; }
  MM_HIP(c, hipSetDevice(c->device));
  MM_HIP(c, hipMemcpyAsync(off, c->dPafOff.p, (c->pafReads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  if (handed && c->pafReads) MM_HIP(c, hipMemcpyAsync(handed, c->dPafFlag.p, c->pafReads, hipMemcpyDeviceToHost, c->stream));
  MM_HIP(c, hipStreamSynchronize(c->stream));
  return MM_OK;
}

int mm_paf_device(const mm_ctx* c, const char** dText, size_t* n, const int64_t** dOff) {
  if (!c) return MM_ERR_ARG;
  if (!paf_valid(c)) { const_cast<mm_ctx*>(c)->err = "mm_paf_device: mm_paf_rows / mm_paf_format has not run on the current batch"; return MM_ERR_STATE; }
  if (dText) *dText = c->dPafText.as<char>();
  if (n) *n = (size_t)c->pafBytes;
  if (dOff) *dOff = c->dPafOff.as<int64_t>();
  return MM_OK;
}

}  // extern "C"
