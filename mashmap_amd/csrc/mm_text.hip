// mashmap_amd/csrc/mm_text.hip -- mm_text_*: FASTA / FASTQ text in device memory parsed there into the record table and the packed read
// batch.  The record rules and their decomposition over tiles are mm_text_core.h, the text tests/hostlogic/text_check.cpp runs against
// the host reader's serial functions; this file spreads a tile over a wave and supplies the kernels and the entry points.
//
// No workgroup waits for another one: the parse is separate launches on the inflate stream --
//   k_text_summarise   a wave per tile of MM_TEXT_TILE bytes: one MmTextSum per tile
//   k_text_scan        one workgroup: the carry into every tile (mm_text_combine / mm_text_apply), the totals
//   k_text_records     a wave per tile, resolved from its carry: hdrOff, the sequence-byte index at every record start, hasN, FASTQ's consumed
//   k_text_finish      a wave per record: seqLen, nameLen, the names' total, FASTA's consumed
//   k_text_plan        one workgroup: P(r), the packed start of every record, from the keep flags (mm_text_pack)
//   k_text_pack        a wave per tile, resolved again: every kept base to packed base P(rec) + index in record
// A wave holds its tile in LDS, 64 bytes to a lane (rows of MMT_ROW bytes: the lanes' bytes i lie in different banks); a lane summarises
// or resolves its own 64 bytes with the header's functions, and the lanes' summaries are scanned across the wave with its combine.
//
// Bounds.  A tile is loaded with 16-byte loads where they lie inside [0, nBytes) and byte by byte at the buffer's end; nothing else reads
// the text but k_text_finish's name search, every step of which is checked against nBytes.  Every table write is checked against the
// table's rows, every packed base against the piece's length.  The host sizes every buffer from the totals before the launch that
// writes it.  Every loop runs over a count fixed before it starts, or advances through the text.
#include "mm_internal.h"
#include <algorithm>
#include "mm_text_core.h"

static_assert(MM_TEXT_FASTA == MMT_FASTA && MM_TEXT_FASTQ == MMT_FASTQ, "mm_text_core.h restates the format values");
static_assert(sizeof(mm_text_record) == 24, "mm_text_record is 24 bytes");
static_assert(MM_TEXT_TILE == 64 * 64, "a lane owns 64 bytes of its wave's tile");

#define MMT_WAVES 4                          // waves (tiles) per workgroup
#define MMT_ROW 68                           // bytes between two lanes' rows in LDS: 17 words
#define MMT_SCAN_THREADS 1024
enum : int {                                 // the totals block, 64-bit words
  MMT_T_RECORDS = 0, MMT_T_HEADERS, MMT_T_CONSUMED_NL, MMT_T_LAST_HEADER, MMT_T_SEQ, MMT_T_ROWS, MMT_T_CONSUMED, MMT_T_NAME_BYTES,
  MMT_T_PACKED, MMT_T_TOO_LONG, MMT_T_WORDS = 16
};

__device__ inline MmTextSum mmt_shfl_up(const MmTextSum& s, unsigned d) {
  MmTextSum r;
  r.nl = (uint32_t)__shfl_up((int)s.nl, d); r.out = (uint32_t)__shfl_up((int)s.out, d);
  for (int k = 0; k < MMT_STATES; k++) { r.hdr[k] = (uint32_t)__shfl_up((int)s.hdr[k], d); r.seq[k] = (uint32_t)__shfl_up((int)s.seq[k], d); }
  return r;
}
// inclusive scan of the lanes' summaries, lane 0 first
__device__ inline MmTextSum mmt_wave_scan(MmTextSum s, uint32_t ln) {
  for (unsigned d = 1; d < 64; d <<= 1) {
    const MmTextSum o = mmt_shfl_up(s, d);
    if (ln >= d) s = mm_text_combine(o, s);
  }
  return s;
}

// The wave's tile into its LDS rows: load j of lane ln is the 16 bytes at tile offset 1024 j + 16 ln (the wave's loads are contiguous),
// which belong to lane (16 j + ln / 4)'s row.  Returns whether the lane saw a '\n' (or, with gt, a '>') in what it loaded.  Bytes at or
// beyond nBytes are not read; their places in LDS are not read either (every lane walks its own count of bytes only).
__device__ inline bool mmt_load_tile(const uint8_t* __restrict__ text, uint64_t nBytes, uint64_t tileOff, uint8_t* rows, uint32_t ln, bool gt) {
  bool seen = false;
  for (uint32_t j = 0; j < 4; j++) {
    const uint32_t q = j * 1024 + ln * 16;
    const uint64_t at = tileOff + q;
    uint8_t* dst = rows + (q >> 6) * MMT_ROW + (q & 63);
    if (at + 16 <= nBytes) {
      const uint4 v = *reinterpret_cast<const uint4*>(text + at);
      uint32_t* d = reinterpret_cast<uint32_t*>(dst);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      for (int k = 0; k < 4; k++) {
        const uint32_t a = w[k] ^ 0x0a0a0a0au, b = w[k] ^ 0x3e3e3e3eu;           // a zero byte where the word holds '\n' / '>'
        seen |= ((a - 0x01010101u) & ~a & 0x80808080u) != 0;
        if (gt) seen |= ((b - 0x01010101u) & ~b & 0x80808080u) != 0;
      }
    } else {
      for (uint32_t i = 0; i < 16 && at + i < nBytes; i++) { const uint8_t b = text[at + i]; dst[i] = b; seen |= b == '\n' || (gt && b == '>'); }
    }
  }
  return seen;
}
__device__ inline uint32_t mmt_lane_bytes(uint64_t nBytes, uint64_t laneOff) { return laneOff >= nBytes ? 0u : (uint32_t)(nBytes - laneOff < 64 ? nBytes - laneOff : 64); }

__global__ __launch_bounds__(64 * MMT_WAVES) void k_text_summarise(const uint8_t* __restrict__ text, uint64_t nBytes, int fmt, uint32_t nTiles, MmTextSum* __restrict__ sums) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[MMT_WAVES][64 * MMT_ROW];
  const uint32_t wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const uint32_t tile = blockIdx.x * MMT_WAVES + wave;
  const bool active = tile < nTiles;
  const uint64_t tileOff = (uint64_t)tile * MM_TEXT_TILE;
  bool seen = false;
  if (active) seen = mmt_load_tile(text, nBytes, tileOff, lds[wave], ln, fmt == MMT_FASTA);
  __syncthreads();
  if (!active) return;
  const uint64_t marks = __ballot(seen);                          // lanes that loaded a line break or a '>'
  if (!marks) {                                                     // a tile inside one line: nothing to walk
    if (ln == 0) sums[tile] = mm_text_summarise_plain(fmt, (uint32_t)(nBytes - tileOff < MM_TEXT_TILE ? nBytes - tileOff : MM_TEXT_TILE));
    return;
  }
  const MmTextSum mine = mm_text_summarise(fmt, lds[wave] + ln * MMT_ROW, mmt_lane_bytes(nBytes, tileOff + ln * 64));
  const MmTextSum inc = mmt_wave_scan(mine, ln);
  if (ln == 63) sums[tile] = inc;
}

// One workgroup.  Thread t combines its run of tiles, thread 0 walks the 1024 runs from mm_text_carry0, every thread then walks its run
// again from its carry and writes the tiles' carries; carry[nTiles] is the one behind the buffer.  Then the totals.
__global__ __launch_bounds__(MMT_SCAN_THREADS) void k_text_scan(const uint8_t* __restrict__ text, uint64_t nBytes, int fmt, int final, uint32_t nTiles,
                                                                const MmTextSum* __restrict__ sums, MmTextCarry* __restrict__ carry, unsigned long long* totals) {
  __shared__ MmTextSum part[MMT_SCAN_THREADS];
  __shared__ MmTextCarry start[MMT_SCAN_THREADS];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (nTiles + MMT_SCAN_THREADS - 1) / MMT_SCAN_THREADS;
  const uint32_t lo = min(nTiles, t * per), hi = min(nTiles, lo + per);
  MmTextSum acc = mm_text_identity();
  for (uint32_t k = lo; k < hi; k++) acc = mm_text_combine(acc, sums[k]);
  part[t] = acc;
  __syncthreads();
  if (t == 0) {
    MmTextCarry c = mm_text_carry0(fmt);
    for (uint32_t i = 0; i < MMT_SCAN_THREADS; i++) { start[i] = c; c = mm_text_apply(c, part[i]); }
    carry[nTiles] = c;
    const uint8_t last = nBytes ? text[nBytes - 1] : 0;
    uint32_t consumedNl; int lastHeader;
    const uint32_t nRec = mm_text_complete(fmt, final, nBytes, last, c, &consumedNl, &lastHeader);
    totals[MMT_T_RECORDS] = nRec; totals[MMT_T_HEADERS] = mm_text_headers(fmt, nBytes, last, c);
    totals[MMT_T_CONSUMED_NL] = consumedNl; totals[MMT_T_LAST_HEADER] = (unsigned long long)lastHeader;
    totals[MMT_T_SEQ] = c.seq; totals[MMT_T_ROWS] = (unsigned long long)c.rec + 1;
    totals[MMT_T_CONSUMED] = final ? nBytes : 0; totals[MMT_T_NAME_BYTES] = 0;
  }
  __syncthreads();
  MmTextCarry c = start[t];
  for (uint32_t k = lo; k < hi; k++) { carry[k] = c; c = mm_text_apply(c, sums[k]); }
}

// the lane's carry: the tile's, moved across the summaries of the lanes before it
__device__ inline MmTextCarry mmt_lane_carry(int fmt, const uint8_t* row, uint32_t n, const MmTextCarry& tileCarry, uint32_t ln) {
  const MmTextSum inc = mmt_wave_scan(mm_text_summarise(fmt, row, n), ln);
  MmTextSum before = mmt_shfl_up(inc, 1);
  if (ln == 0) before = mm_text_identity();
  return mm_text_apply(tileCarry, before);
}

struct MmtRecordVisitor {
  uint64_t laneOff, nBytes; mm_text_record* recs; uint32_t* seqStart; uint32_t rows; unsigned long long* totals; uint32_t consumedNl;
  uint32_t nRec = 0xffffffffu; uint32_t anyN = 0;                   // the record whose N flag the lane is gathering
  __device__ void flush() { if (anyN && nRec < rows) atomicOr(&recs[nRec].hasN, 1u); anyN = 0; }
  __device__ void header(uint32_t ordinal, uint32_t i, uint32_t seq) {
    if (laneOff + i >= nBytes || ordinal >= rows) return;
    recs[ordinal].hdrOff = laneOff + i; seqStart[ordinal] = seq;
  }
  __device__ void byte(uint32_t i, uint8_t b, uint32_t cls, const MmTextCarry& c) {
    if (cls == MMT_BREAK) { if (consumedNl && c.nl + 1 == consumedNl) totals[MMT_T_CONSUMED] = laneOff + i + 1; return; }
    if (cls != MMT_BASE) return;
    if (c.rec - 1 != nRec) { flush(); nRec = c.rec - 1; }
    uint32_t isN; (void)mm_text_code(b, isN);
    anyN |= isN;
  }
};

__global__ __launch_bounds__(64 * MMT_WAVES) void k_text_records(const uint8_t* __restrict__ text, uint64_t nBytes, int fmt, uint32_t nTiles, const MmTextCarry* __restrict__ carry,
                                                                   mm_text_record* recs, uint32_t* seqStart, uint32_t rows, unsigned long long* totals) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[MMT_WAVES][64 * MMT_ROW];
  const uint32_t wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const uint32_t tile = blockIdx.x * MMT_WAVES + wave;
  const bool active = tile < nTiles;
  const uint64_t tileOff = (uint64_t)tile * MM_TEXT_TILE;
  if (active) (void)mmt_load_tile(text, nBytes, tileOff, lds[wave], ln, false);
  __syncthreads();
  if (!active) return;
  const uint8_t* row = lds[wave] + ln * MMT_ROW;
  const uint32_t n = mmt_lane_bytes(nBytes, tileOff + ln * 64);
  const MmTextCarry c = mmt_lane_carry(fmt, row, n, carry[tile], ln);
  MmtRecordVisitor v{tileOff + ln * 64, nBytes, recs, seqStart, rows, totals, (uint32_t)totals[MMT_T_CONSUMED_NL]};
  if (tile == 0 && ln == 0) v.header(0, 0, 0);                     // the header line at offset 0 is given
  (void)mm_text_resolve(fmt, row, n, c, v);
  v.flush();
}

// A wave per table row r <= nRecords: seqLen from the sequence-byte indexes at consecutive record starts (behind the last header line: the
// total), nameLen by a search from hdrOff + 1 to the first ' ' or '\n', 64 bytes a step.  Row nRecords, where the buffer holds that header
// line, is the incomplete FASTA record: its offset is `consumed`.
__global__ __launch_bounds__(64 * MMT_WAVES) void k_text_finish(const uint8_t* __restrict__ text, uint64_t nBytes, mm_text_record* recs, const uint32_t* __restrict__ seqStart,
                                                                  uint32_t rows, unsigned long long* totals) {
  const uint32_t r = blockIdx.x * MMT_WAVES + (threadIdx.x >> 6), ln = threadIdx.x & 63;
  const uint32_t nRec = (uint32_t)totals[MMT_T_RECORDS], nHdr = (uint32_t)totals[MMT_T_HEADERS];
  if (r >= rows || r >= nHdr) return;
  if (r >= nRec) {
    if (r == nRec && totals[MMT_T_LAST_HEADER] && ln == 0) totals[MMT_T_CONSUMED] = recs[r].hdrOff;
    return;
  }
  const uint64_t hdr = recs[r].hdrOff;
  uint32_t nameLen = 0;
  if (hdr < nBytes && text[hdr] != '\n') {
    uint64_t pos = hdr + 1;
    for (;;) {                                                      // every step moves pos on by 64 or ends the search
      const bool stop = pos + ln >= nBytes || text[pos + ln] == ' ' || text[pos + ln] == '\n';
      const uint64_t m = __ballot(stop);
      if (m) { pos += (uint64_t)__builtin_ctzll(m); break; }
      pos += 64;
    }
    nameLen = (uint32_t)(pos - hdr - 1);
  }
  if (ln == 0) {
    const uint32_t next = r + 1 < nHdr ? seqStart[r + 1] : (uint32_t)totals[MMT_T_SEQ];
    recs[r].seqLen = (int64_t)(next - seqStart[r]);
    recs[r].nameLen = nameLen;
    if (nameLen) atomicAdd(&totals[MMT_T_NAME_BYTES], (unsigned long long)nameLen);
  }
}

// names end to end: a wave per record copies nameLen bytes from hdrOff + 1 to nameOff[r]
__global__ __launch_bounds__(64 * MMT_WAVES) void k_text_names(const uint8_t* __restrict__ text, uint64_t nBytes, const mm_text_record* __restrict__ recs, uint32_t nRec,
                                                                 const uint64_t* __restrict__ nameOff, uint8_t* out, uint64_t nOut) {
  const uint32_t r = blockIdx.x * MMT_WAVES + (threadIdx.x >> 6), ln = threadIdx.x & 63;
  if (r >= nRec) return;
  const uint64_t src = recs[r].hdrOff + 1, dst = nameOff[r];
  const uint32_t len = recs[r].nameLen;
  for (uint32_t i = ln; i < len; i += 64) if (src + i < nBytes && dst + i < nOut) out[dst + i] = text[src + i];
}

// One workgroup: P(r) = the 32-rounded lengths of the kept records before r, summed; the total; a kept record of 2^31 bases or more
__global__ __launch_bounds__(MMT_SCAN_THREADS) void k_text_plan(const mm_text_record* __restrict__ recs, uint32_t nRec, const uint8_t* __restrict__ keep, int64_t* packOff, unsigned long long* totals) {
  __shared__ unsigned long long part[MMT_SCAN_THREADS];
  __shared__ unsigned int tooLong;
  const uint32_t t = threadIdx.x;
  if (t == 0) tooLong = 0;
  __syncthreads();
  const uint32_t per = (nRec + MMT_SCAN_THREADS - 1) / MMT_SCAN_THREADS;
  const uint32_t lo = min(nRec, t * per), hi = min(nRec, lo + per);
  unsigned long long sum = 0;
  for (uint32_t r = lo; r < hi; r++) {
    const uint64_t len = (!keep || keep[r]) ? (uint64_t)recs[r].seqLen : 0;
    if (len > 0x7fffffffull) atomicOr(&tooLong, 1u);
    sum += (len + 31) / 32 * 32;
  }
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    unsigned long long at = 0;
    for (uint32_t i = 0; i < MMT_SCAN_THREADS; i++) { const unsigned long long v = part[i]; part[i] = at; at += v; }
    totals[MMT_T_PACKED] = at; totals[MMT_T_TOO_LONG] = tooLong;
  }
  __syncthreads();
  unsigned long long at = part[t];
  for (uint32_t r = lo; r < hi; r++) {
    packOff[r] = (int64_t)at;
    const uint64_t len = (!keep || keep[r]) ? (uint64_t)recs[r].seqLen : 0;
    at += (len + 31) / 32 * 32;
  }
}

// A lane's bases are consecutive in the text, so within a record they are consecutive packed bases: the lane gathers the codes of one
// code word (16 bases) and the N bits of one mask word (32 bases) in registers.  A word the lane filled alone is stored; a word it shares
// -- with the lane before or behind it, across a record's end -- is ORed into the zeroed destination.
struct MmtPackVisitor {
  const uint8_t* keep; const int64_t* packOff; const uint32_t* seqStart; uint32_t nRec;
  uint32_t* b2; uint32_t* nm; uint64_t nPacked;
  uint32_t rec = 0xffffffffu; bool kept = false; int64_t shift = 0;   // packed base = shift + global sequence-byte index
  int64_t cw = -1, mw = -1; uint32_t cbits = 0, ccnt = 0, mbits = 0, mcnt = 0;
  __device__ void flushCodes() { if (ccnt == 16) b2[cw] = cbits; else if (cbits) atomicOr(&b2[cw], cbits); cbits = 0; ccnt = 0; }
  __device__ void flushMask() { if (mcnt == 32) nm[mw] = mbits; else if (mbits) atomicOr(&nm[mw], mbits); mbits = 0; mcnt = 0; }
  __device__ void header(uint32_t, uint32_t, uint32_t) {}
  __device__ void byte(uint32_t, uint8_t b, uint32_t cls, const MmTextCarry& c) {
    if (cls != MMT_BASE) return;
    if (c.rec - 1 != rec) {
      rec = c.rec - 1;
      kept = rec < nRec && (!keep || keep[rec]);
      if (kept) shift = packOff[rec] - (int64_t)seqStart[rec];
    }
    if (!kept) return;
    const int64_t d = shift + (int64_t)c.seq;
    if (d < 0 || (uint64_t)d >= nPacked) return;
    uint32_t isN; const uint32_t code = mm_text_code(b, isN);
    if ((d >> 4) != cw) { flushCodes(); cw = d >> 4; }
    if ((d >> 5) != mw) { flushMask(); mw = d >> 5; }
    cbits |= code << ((uint32_t)(d & 15) * 2); ccnt++;
    mbits |= isN << (uint32_t)(d & 31); mcnt++;
  }
};

__global__ __launch_bounds__(64 * MMT_WAVES) void k_text_pack(const uint8_t* __restrict__ text, uint64_t nBytes, int fmt, uint32_t nTiles, const MmTextCarry* __restrict__ carry,
                                                                uint32_t nRec, const uint8_t* __restrict__ keep, const int64_t* __restrict__ packOff, const uint32_t* __restrict__ seqStart,
                                                                uint32_t* b2, uint32_t* nm, uint64_t nPacked) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[MMT_WAVES][64 * MMT_ROW];
  const uint32_t wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const uint32_t tile = blockIdx.x * MMT_WAVES + wave;
  const bool active = tile < nTiles;
  const uint64_t tileOff = (uint64_t)tile * MM_TEXT_TILE;
  if (active) (void)mmt_load_tile(text, nBytes, tileOff, lds[wave], ln, false);
  __syncthreads();
  if (!active) return;
  const uint8_t* row = lds[wave] + ln * MMT_ROW;
  const uint32_t n = mmt_lane_bytes(nBytes, tileOff + ln * 64);
  const MmTextCarry c = mmt_lane_carry(fmt, row, n, carry[tile], ln);
  MmtPackVisitor v{keep, packOff, seqStart, nRec, b2, nm, nPacked};
  (void)mm_text_resolve(fmt, row, n, c, v);
  v.flushCodes(); v.flushMask();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// entry points.  Every one runs under DeviceInput::inflateMu and leaves its error text to the calling thread (mm_input_call).
// ---------------------------------------------------------------------------------------------------------------------------------
static int text_stream(mm_ctx* c, InflateErr* e) {
  DeviceInput::Text& T = c->input.text;
  { const int rc = c->input.ready(c->device, e); if (rc != MM_OK) return rc; }
  MM_HIP(e, T.textEvA.ensure());
  MM_HIP(e, T.textEvB.ensure());
  MM_HIP(e, T.textDone.ensure(hipEventDisableTiming));
  return MM_OK;
}

// room for `more` bytes behind the textLen the buffer holds, which stay
static int text_room(mm_ctx* c, InflateErr* e, size_t more, const char* who) {
  DeviceInput::Text& T = c->input.text;
  if (more > 0xffffffffull - T.textLen) { e->err = std::string(who) + ": the text buffer holds at most 2^32 - 1 bytes"; return MM_ERR_ARG; }
  const size_t need = T.textLen + more + 64;
  if (need <= T.dText.bytes) return MM_OK;
  MM_HIP(e, T.dTextAlt.ensure(need));
  if (T.textLen) MM_HIP(e, hipMemcpyAsync(T.dTextAlt.p, T.dText.p, T.textLen, hipMemcpyDeviceToDevice, c->input.inflateStream));
  MM_HIP(e, hipStreamSynchronize(c->input.inflateStream));
  std::swap(T.dText, T.dTextAlt);
  return MM_OK;
}

static float text_elapsed(const DeviceInput::Text& T) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, T.textEvA, T.textEvB) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return ms;
}

static int text_scan(mm_ctx* c, InflateErr* e, int format, int final, size_t* nRecords, size_t* nNameBytes, size_t* consumed) {
  DeviceInput::Text& T = c->input.text;
  if (format != MM_TEXT_FASTA && format != MM_TEXT_FASTQ) { e->err = "mm_text_scan: unknown format"; return MM_ERR_ARG; }
  { const int rc = text_stream(c, e); if (rc != MM_OK) return rc; }
  final = final != 0;
  T.textScanned = false;
  T.textFormat = format; T.textFinal = final; T.textRecords = 0; T.textNameBytes = 0; T.textConsumed = 0; T.textScanMs = 0;
  if (T.textLen) {
    hipStream_t st = c->input.inflateStream;
    const uint64_t nBytes = T.textLen;
    const uint32_t nTiles = (uint32_t)((nBytes + MM_TEXT_TILE - 1) / MM_TEXT_TILE);
    const unsigned grid = (nTiles + MMT_WAVES - 1) / MMT_WAVES;
    MM_HIP(e, T.dTextSum.ensure((size_t)nTiles * sizeof(MmTextSum)));
    MM_HIP(e, T.dTextCarry.ensure(((size_t)nTiles + 1) * sizeof(MmTextCarry)));
    MM_HIP(e, T.dTextTotals.ensure(MMT_T_WORDS * 8));
    unsigned long long* totals = T.dTextTotals.as<unsigned long long>();
    unsigned long long h[MMT_T_WORDS] = {0};
    MM_HIP(e, hipMemsetAsync(totals, 0, MMT_T_WORDS * 8, st));
    MM_HIP(e, hipEventRecord(T.textEvA, st));
    hipLaunchKernelGGL(k_text_summarise, dim3(grid), dim3(64 * MMT_WAVES), 0, st, T.dText.as<uint8_t>(), nBytes, format, nTiles, T.dTextSum.as<MmTextSum>());
    MM_HIP(e, hipGetLastError());
    hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(MMT_SCAN_THREADS), 0, st, T.dText.as<uint8_t>(), nBytes, format, final, nTiles, T.dTextSum.as<MmTextSum>(),
                       T.dTextCarry.as<MmTextCarry>(), totals);
    MM_HIP(e, hipGetLastError());
    MM_HIP(e, hipEventRecord(T.textEvB, st));
    MM_HIP(e, hipMemcpyAsync(h, totals, sizeof h, hipMemcpyDeviceToHost, st));
    MM_HIP(e, hipStreamSynchronize(st));
    double ms = text_elapsed(T);
    // the table: a row for every header line the carry counted and one more (the kernels check every row against it)
    const uint64_t rows = h[MMT_T_ROWS];
    if (h[MMT_T_RECORDS] >= rows || h[MMT_T_HEADERS] >= rows || rows > 0xffffffffull) { e->err = "mm_text_scan: inconsistent totals"; return MM_ERR_DEVICE; }
    MM_HIP(e, T.dTextRecs.ensure((size_t)rows * sizeof(mm_text_record)));
    MM_HIP(e, T.dTextSeqStart.ensure((size_t)rows * sizeof(uint32_t)));
    MM_HIP(e, hipMemsetAsync(T.dTextRecs.p, 0, (size_t)rows * sizeof(mm_text_record), st));
    MM_HIP(e, hipMemsetAsync(T.dTextSeqStart.p, 0, (size_t)rows * sizeof(uint32_t), st));
    MM_HIP(e, hipEventRecord(T.textEvA, st));
    hipLaunchKernelGGL(k_text_records, dim3(grid), dim3(64 * MMT_WAVES), 0, st, T.dText.as<uint8_t>(), nBytes, format, nTiles, T.dTextCarry.as<MmTextCarry>(),
                       T.dTextRecs.as<mm_text_record>(), T.dTextSeqStart.as<uint32_t>(), (uint32_t)rows, totals);
    MM_HIP(e, hipGetLastError());
    hipLaunchKernelGGL(k_text_finish, dim3((unsigned)((rows + MMT_WAVES - 1) / MMT_WAVES)), dim3(64 * MMT_WAVES), 0, st, T.dText.as<uint8_t>(), nBytes,
                       T.dTextRecs.as<mm_text_record>(), T.dTextSeqStart.as<uint32_t>(), (uint32_t)rows, totals);
    MM_HIP(e, hipGetLastError());
    MM_HIP(e, hipEventRecord(T.textEvB, st));
    MM_HIP(e, hipMemcpyAsync(h, totals, sizeof h, hipMemcpyDeviceToHost, st));
    MM_HIP(e, hipStreamSynchronize(st));
    ms += text_elapsed(T);
    if (h[MMT_T_CONSUMED] > nBytes) { e->err = "mm_text_scan: inconsistent totals"; return MM_ERR_DEVICE; }
    T.textRecords = (size_t)h[MMT_T_RECORDS]; T.textNameBytes = (size_t)h[MMT_T_NAME_BYTES]; T.textConsumed = (size_t)h[MMT_T_CONSUMED];
    T.textScanMs = ms;
  }
  T.textScanned = true;
  T.textScans++; T.textRecordsTotal += T.textRecords; T.textBytesTotal += T.textConsumed;
  if (nRecords) *nRecords = T.textRecords;
  if (nNameBytes) *nNameBytes = T.textNameBytes;
  if (consumed) *consumed = T.textConsumed;
  return MM_OK;
}

static int text_records(mm_ctx* c, InflateErr* e, mm_text_record* recs, char* names) {
  DeviceInput::Text& T = c->input.text;
  if (!T.textScanned) { e->err = "mm_text_records: no mm_text_scan since the text buffer last changed"; return MM_ERR_STATE; }
  const size_t n = T.textRecords;
  if (!n || (!recs && !names)) return MM_OK;
  { const int rc = text_stream(c, e); if (rc != MM_OK) return rc; }
  hipStream_t st = c->input.inflateStream;
  std::vector<mm_text_record> own;
  if (!recs) { own.resize(n); recs = own.data(); }
  MM_HIP(e, hipMemcpyAsync(recs, T.dTextRecs.p, n * sizeof(mm_text_record), hipMemcpyDeviceToHost, st));
  MM_HIP(e, hipStreamSynchronize(st));
  if (!names || !T.textNameBytes) return MM_OK;
  std::vector<uint64_t> off(n);
  uint64_t at = 0;
  for (size_t r = 0; r < n; r++) { off[r] = at; at += recs[r].nameLen; }
  if (at != T.textNameBytes) { e->err = "mm_text_records: inconsistent name lengths"; return MM_ERR_DEVICE; }
  const size_t offBytes = (n * 8 + 63) / 64 * 64;
  MM_HIP(e, T.dTextNames.ensure(offBytes + (size_t)at + 64));
  MM_HIP(e, hipMemcpyAsync(T.dTextNames.p, off.data(), n * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_text_names, dim3((unsigned)((n + MMT_WAVES - 1) / MMT_WAVES)), dim3(64 * MMT_WAVES), 0, st, T.dText.as<uint8_t>(), (uint64_t)T.textLen,
                     T.dTextRecs.as<mm_text_record>(), (uint32_t)n, T.dTextNames.as<uint64_t>(), T.dTextNames.as<uint8_t>() + offBytes, at);
  MM_HIP(e, hipGetLastError());
  MM_HIP(e, hipMemcpyAsync(names, T.dTextNames.as<char>() + offBytes, (size_t)at, hipMemcpyDeviceToHost, st));
  MM_HIP(e, hipStreamSynchronize(st));
  return MM_OK;
}

static int text_pack(mm_ctx* c, InflateErr* e, const uint8_t* keep, uint32_t* bases2, uint32_t* nmask, size_t capPackedBases, size_t reservePackedBases,
                     size_t* nPackedBases, int* staged) {
  DeviceInput::Text& T = c->input.text;
  if (!T.textScanned) { e->err = "mm_text_pack: no mm_text_scan since the text buffer last changed"; return MM_ERR_STATE; }
  { const int rc = text_stream(c, e); if (rc != MM_OK) return rc; }
  hipStream_t st = c->input.inflateStream;
  const size_t nRec = T.textRecords;
  uint64_t nPacked = 0;
  T.textPackMs = 0;
  if (nRec) {
    unsigned long long* totals = T.dTextTotals.as<unsigned long long>();
    MM_HIP(e, T.dTextPackOff.ensure(nRec * sizeof(int64_t)));
    if (keep) { MM_HIP(e, T.dTextKeep.ensure(nRec)); MM_HIP(e, hipMemcpyAsync(T.dTextKeep.p, keep, nRec, hipMemcpyHostToDevice, st)); }
    const uint8_t* dKeep = keep ? T.dTextKeep.as<uint8_t>() : nullptr;
    hipLaunchKernelGGL(k_text_plan, dim3(1), dim3(MMT_SCAN_THREADS), 0, st, T.dTextRecs.as<mm_text_record>(), (uint32_t)nRec, dKeep, T.dTextPackOff.as<int64_t>(), totals);
    MM_HIP(e, hipGetLastError());
    unsigned long long h[2] = {0, 0};
    MM_HIP(e, hipMemcpyAsync(h, totals + MMT_T_PACKED, sizeof h, hipMemcpyDeviceToHost, st));
    MM_HIP(e, hipStreamSynchronize(st));
    if (h[1]) { e->err = "mm_text_pack: a kept record of 2^31 bases or more"; return MM_ERR_ARG; }
    nPacked = h[0];
  }
  if (nPacked > capPackedBases) { e->err = "mm_text_pack: the kept records need more than capPackedBases"; return MM_ERR_ARG; }
  if (nPacked && (!bases2 || !nmask)) { e->err = "mm_text_pack: null argument"; return MM_ERR_ARG; }
  int isStaged = 0;
  if (nPacked) {
    // under prefetchMu until the words are where they go: the staging area is shared with the uploads of the context's own thread
    Staging& S = c->stage;
    std::lock_guard<std::mutex> prefetchLock(S.prefetchMu);
    bool fits = false;
    { const int rc = mm_stage_place(c, (size_t)nPacked, reservePackedBases, &fits); if (rc != MM_OK) { e->err = c->err; return rc; } }
    char* dst;
    if (fits) dst = S.dAsciiNext.as<char>() + S.ring.next;
    else { MM_HIP(e, T.dTextWords.ensure(StageRing::bytes((size_t)nPacked) + 64)); dst = T.dTextWords.as<char>(); }
    uint32_t* dB = (uint32_t*)dst; uint32_t* dM = (uint32_t*)(dst + nPacked / 4);
    const uint64_t nBytes = T.textConsumed;                       // the complete records lie in front of `consumed`
    const uint32_t nTiles = (uint32_t)((nBytes + MM_TEXT_TILE - 1) / MM_TEXT_TILE);
    MM_HIP(e, hipMemsetAsync(dst, 0, StageRing::bytes((size_t)nPacked), st));
    MM_HIP(e, hipEventRecord(T.textEvA, st));
    hipLaunchKernelGGL(k_text_pack, dim3((nTiles + MMT_WAVES - 1) / MMT_WAVES), dim3(64 * MMT_WAVES), 0, st, T.dText.as<uint8_t>(), nBytes, T.textFormat, nTiles,
                       T.dTextCarry.as<MmTextCarry>(), (uint32_t)nRec, keep ? T.dTextKeep.as<uint8_t>() : nullptr, T.dTextPackOff.as<int64_t>(),
                       T.dTextSeqStart.as<uint32_t>(), dB, dM, nPacked);
    MM_HIP(e, hipGetLastError());
    MM_HIP(e, hipEventRecord(T.textEvB, st));
    if (fits) {
      // the upload waits for copyDone: recorded on the copy stream behind this kernel
      MM_HIP(e, hipEventRecord(T.textDone, st));
      MM_HIP(e, hipStreamWaitEvent(S.copyStream, T.textDone, 0));
      MM_HIP(e, hipEventRecord(S.copyDone, S.copyStream));
    } else {
      MM_HIP(e, hipMemcpyAsync(bases2, dB, (size_t)nPacked / 4, hipMemcpyDeviceToHost, st));
      MM_HIP(e, hipMemcpyAsync(nmask, dM, (size_t)nPacked / 8, hipMemcpyDeviceToHost, st));
    }
    MM_HIP(e, hipStreamSynchronize(st));
    if (fits) { mm_stage_commit(c, bases2, nmask, (size_t)nPacked); isStaged = 1; }
    T.textPackMs = text_elapsed(T);
  }
  // the consumed bytes leave: the tail goes to the other buffer, which becomes the text buffer
  const size_t tail = T.textLen - T.textConsumed;
  if (T.textConsumed) {
    if (tail) {
      MM_HIP(e, T.dTextAlt.ensure(tail + 64));
      MM_HIP(e, hipMemcpyAsync(T.dTextAlt.p, T.dText.as<char>() + T.textConsumed, tail, hipMemcpyDeviceToDevice, st));
      MM_HIP(e, hipStreamSynchronize(st));
      std::swap(T.dText, T.dTextAlt);
    }
    T.textLen = tail;
  }
  T.textScanned = false;
  if (nPackedBases) *nPackedBases = (size_t)nPacked;
  if (staged) *staged = isStaged;
  return MM_OK;
}

extern "C" {

int mm_text_reset(mm_ctx* c) {
  return mm_input_call(c, [&](InflateErr*) -> int { c->input.text.textLen = 0; c->input.text.textScanned = false; return MM_OK; });
}

int mm_text_append(mm_ctx* c, const void* bytes, size_t n, int onDevice) {
  return mm_input_call(c, [&](InflateErr* e) -> int {
    DeviceInput::Text& T = c->input.text;
    if (n && !bytes) { e->err = "mm_text_append: null argument"; return MM_ERR_ARG; }
    if (!n) return MM_OK;
    { const int rc = text_stream(c, e); if (rc != MM_OK) return rc; }
    { const int rc = text_room(c, e, n, "mm_text_append"); if (rc != MM_OK) return rc; }
    MM_HIP(e, hipMemcpyAsync(T.dText.as<char>() + T.textLen, bytes, n, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->input.inflateStream));
    MM_HIP(e, hipStreamSynchronize(c->input.inflateStream));
    T.textLen += n; T.textScanned = false;
    return MM_OK;
  });
}

int mm_text_append_inflated(mm_ctx* c, const void* comp, size_t nComp, mm_inflate_block* blocks, size_t nBlocks, size_t* nBad) {
  if (nBad) *nBad = 0;
  return mm_input_call(c, [&](InflateErr* e) -> int {
    DeviceInput::Text& T = c->input.text;
    if (nBlocks && !blocks) { e->err = "mm_text_append_inflated: null argument"; return MM_ERR_ARG; }
    uint64_t total = 0;
    for (size_t i = 0; i < nBlocks; i++) {
      if (blocks[i].uLen > MM_INFLATE_MAX_BLOCK) { e->err = "mm_inflate_blocks: a block above MM_INFLATE_MAX_BLOCK"; return MM_ERR_ARG; }
      total += blocks[i].uLen;
    }
    { const int rc = text_stream(c, e); if (rc != MM_OK) return rc; }
    { const int rc = text_room(c, e, (size_t)total, "mm_text_append_inflated"); if (rc != MM_OK) return rc; }
    size_t bad = 0;
    const int rc = mm_inflate_run(c, e, comp, nComp, blocks, nBlocks, nullptr, ~(size_t)0, &bad, T.dText.as<uint8_t>() + T.textLen);
    if (nBad) *nBad = bad;
    if (rc != MM_OK) return rc;
    if (!bad && total) { T.textLen += (size_t)total; T.textScanned = false; }   // a refused block: the bytes behind textLen are nobody's
    return MM_OK;
  });
}

int mm_text_scan(mm_ctx* c, int format, int final, size_t* nRecords, size_t* nNameBytes, size_t* consumed) {
  return mm_input_call(c, [&](InflateErr* e) -> int { return text_scan(c, e, format, final, nRecords, nNameBytes, consumed); });
}

int mm_text_records(mm_ctx* c, mm_text_record* recs, char* names) {
  return mm_input_call(c, [&](InflateErr* e) -> int { return text_records(c, e, recs, names); });
}

int mm_text_pack(mm_ctx* c, const uint8_t* keep, uint32_t* bases2, uint32_t* nmask, size_t capPackedBases, size_t reservePackedBases, size_t* nPackedBases, int* staged) {
  if (nPackedBases) *nPackedBases = 0;
  if (staged) *staged = 0;
  return mm_input_call(c, [&](InflateErr* e) -> int { return text_pack(c, e, keep, bases2, nmask, capPackedBases, reservePackedBases, nPackedBases, staged); });
}

int mm_text_counts(const mm_ctx* c, uint64_t* scans, uint64_t* records, uint64_t* bytes) {
  if (!c) return MM_ERR_ARG;
  std::lock_guard<std::mutex> lock(c->input.inflateMu);
  if (scans) *scans = c->input.text.textScans;
  if (records) *records = c->input.text.textRecordsTotal;
  if (bytes) *bytes = c->input.text.textBytesTotal;
  return MM_OK;
}

int mm_text_kernel_ms(const mm_ctx* c, double* scanMs, double* packMs) {
  if (!c) return MM_ERR_ARG;
  std::lock_guard<std::mutex> lock(c->input.inflateMu);
  if (scanMs) *scanMs = c->input.text.textScanMs;
  if (packMs) *packMs = c->input.text.textPackMs;
  return MM_OK;
}

}  // extern "C"
