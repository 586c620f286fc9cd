// mashmap_amd/csrc/mm_text_core.h -- the record rules of FASTA / FASTQ text, stated once for the host and the device (the kernels of
// mm_text.hip; tests/hostlogic/text_check.cpp runs the same text against the serial functions of mashmap_amd/host/seq_parse.hpp).
//
// The rules (seq_parse.hpp's detail::record_name / record_lines driven by one thread, which restate seqiter::for_each_seq_in_file):
//   * lines end at '\n', the last one may be unterminated; line 0 of the buffer is a header line whatever its first byte; a '\r' is an
//     ordinary byte (it stays in a name, and is a base -- an N -- in a sequence line);
//   * FASTA: a header line is line 0 or a line whose first byte is '>'; every byte of the other lines is a base of the record of the
//     last header line (empty lines give nothing, a record may have no base);
//   * FASTQ: line 4i is a header line, line 4i+1 the sequence line, lines 4i+2 and 4i+3 are skipped whatever they hold;
//   * the name is the header line without its first byte and its '\n', cut at the first ' ' (mm_text_name_len).
//
// The parse as a decomposition over tiles.  A byte's class depends on the bytes before it only through a small STATE, the kind of the
// line it lies in:
//   FASTA  MMT_H in a header line, MMT_S in a sequence line, MMT_F at a line start whose first byte has not been seen (the byte decides)
//   FASTQ  the line's index mod 4
// so a tile is summarised, without knowing what precedes it, as a function of the state it is entered in (MmTextSum: for each entering
// state the state it is left in, the header lines that start and the sequence bytes that lie in it; the newline count does not depend
// on the state).  Before the tile's first '\n' the answer depends on the entering state, behind it the tile resolves itself; the table
// holds both parts added up.  mm_text_combine composes two such functions -- composition is associative, so any scan order gives the
// same carries --, mm_text_apply moves a concrete carry (MmTextCarry) across a summary, and mm_text_resolve walks a tile from its carry
// and hands every byte's class, record ordinal and global sequence-byte index to a visitor.
//
// Where a header line is counted.  FASTA: at its first byte (state MMT_F and the byte is '>').  FASTQ: at the '\n' that ends line 4i+3;
// the header then starts one byte on, and a caller drops the one that would start at the buffer's end.  The header line at offset 0 is
// given: mm_text_carry0 starts the count at 1, and the caller notes record 0 at offset 0 itself.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MM_TXT_HD __host__ __device__ inline
#else
#define MM_TXT_HD inline
#endif

// the values of include/mashmap_hip.h's MM_TEXT_* (this header stays free of the C ABI; mm_text.hip asserts that they agree)
enum { MMT_FASTA = 0, MMT_FASTQ = 1 };
enum { MMT_H = 0, MMT_S = 1, MMT_F = 2 };                          // FASTA states (FASTQ: 0 .. 3, the line index mod 4)
enum { MMT_HEADER = 0, MMT_BASE = 1, MMT_BREAK = 2, MMT_SKIP = 3 };  // a byte's class
#define MMT_STATES 4
#define MMT_OUT_IDENTITY 0x03020100u

struct MmTextSum {             // a tile as a function of the entering state s: out byte s of `out`, hdr[s], seq[s]; nl for every s
  uint32_t nl, out;
  uint32_t hdr[MMT_STATES], seq[MMT_STATES];
};
struct MmTextCarry {           // what precedes a byte: the state it is met in, header lines started, sequence bytes and newlines so far
  uint32_t state, rec, seq, nl;
};

MM_TXT_HD MmTextCarry mm_text_carry0(int fmt) { (void)fmt; return MmTextCarry{0u, 1u, 0u, 0u}; }   // MMT_H == 0 == FASTQ line 0
MM_TXT_HD MmTextSum mm_text_identity() { return MmTextSum{0u, MMT_OUT_IDENTITY, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}; }

// One byte met in state s: its class, the state behind it, and whether a header line starts AT it (FASTA) or BEHIND it (FASTQ).
MM_TXT_HD uint32_t mm_text_step(int fmt, uint32_t s, uint8_t b, uint32_t& cls, uint32_t& hdrHere, uint32_t& hdrNext) {
  hdrHere = 0; hdrNext = 0;
  if (fmt == MMT_FASTA) {
    if (s >= MMT_F) { hdrHere = b == '>'; s = hdrHere ? MMT_H : MMT_S; }
    if (b == '\n') { cls = MMT_BREAK; return MMT_F; }
    cls = s == MMT_H ? MMT_HEADER : MMT_BASE;
    return s;
  }
  if (b == '\n') { cls = MMT_BREAK; hdrNext = s == 3; return (s + 1) & 3; }
  cls = s == 0 ? MMT_HEADER : s == 1 ? MMT_BASE : MMT_SKIP;
  return s;
}

// k_pack2bit's code: A0 C1 G2 T3 after & 0xDF, anything else code 0 and an N
MM_TXT_HD uint32_t mm_text_code(uint8_t b, uint32_t& isN) {
  const uint32_t ch = b & 0xDFu;
  const bool ok = (ch == 'A') | (ch == 'C') | (ch == 'G') | (ch == 'T');
  isN = ok ? 0u : 1u;
  return ok ? (((ch >> 1) ^ (ch >> 2)) & 3u) : 0u;
}

// the summary of n bytes
MM_TXT_HD MmTextSum mm_text_summarise(int fmt, const uint8_t* p, uint32_t n) {
  MmTextSum r = mm_text_identity();
  uint32_t st[MMT_STATES] = {0, 1, 2, 3};
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t b = p[i];
    r.nl += b == '\n';
    for (int s = 0; s < MMT_STATES; s++) {
      uint32_t cls, here, next;
      st[s] = mm_text_step(fmt, st[s], b, cls, here, next);
      r.hdr[s] += here + next; r.seq[s] += cls == MMT_BASE;
    }
  }
  r.out = st[0] | st[1] << 8 | st[2] << 16 | st[3] << 24;
  return r;
}

// the summary of n bytes that hold no '\n' and (FASTA) no '>': every state is left as it was entered -- MMT_F as MMT_S -- and the n bytes
// are sequence bytes where that state says so.  What mm_text_summarise gives for such bytes, without looking at them.
MM_TXT_HD MmTextSum mm_text_summarise_plain(int fmt, uint32_t n) {
  MmTextSum r = mm_text_identity();
  if (!n) return r;
  if (fmt == MMT_FASTA) { r.out = MMT_H | MMT_S << 8 | MMT_S << 16 | MMT_S << 24; r.seq[1] = r.seq[2] = r.seq[3] = n; }
  else r.seq[1] = n;
  return r;
}

// a, then b
MM_TXT_HD MmTextSum mm_text_combine(const MmTextSum& a, const MmTextSum& b) {
  MmTextSum r;
  r.nl = a.nl + b.nl; r.out = 0;
  for (int s = 0; s < MMT_STATES; s++) {
    const uint32_t m = (a.out >> (8 * s)) & 3u;
    r.out |= ((b.out >> (8 * m)) & 3u) << (8 * s);
    r.hdr[s] = a.hdr[s] + b.hdr[m]; r.seq[s] = a.seq[s] + b.seq[m];
  }
  return r;
}

MM_TXT_HD MmTextCarry mm_text_apply(const MmTextCarry& c, const MmTextSum& t) {
  const uint32_t s = c.state & 3u;
  return MmTextCarry{(t.out >> (8 * s)) & 3u, c.rec + t.hdr[s], c.seq + t.seq[s], c.nl + t.nl};
}

// Walks n bytes from carry c and returns the carry behind them.  The visitor sees
//   v.byte(i, b, cls, before)   every byte: its class and the carry it was met with -- its record's ordinal is before.rec - 1 (a FASTA
//                               header's first byte: before.rec, the header() call precedes it), a base's global index before.seq;
//   v.header(ordinal, i, seq)   a header line that starts at byte i of these n (i == n: behind them), with the sequence bytes before it.
template <class V>
MM_TXT_HD MmTextCarry mm_text_resolve(int fmt, const uint8_t* p, uint32_t n, MmTextCarry c, V& v) {
  for (uint32_t i = 0; i < n; i++) {
    uint32_t cls, here, next;
    const uint32_t s = mm_text_step(fmt, c.state, p[i], cls, here, next);
    if (here) { v.header(c.rec, i, c.seq); c.rec++; }
    v.byte(i, p[i], cls, c);
    c.state = s; c.seq += cls == MMT_BASE; c.nl += cls == MMT_BREAK;
    if (next) { v.header(c.rec, i + 1, c.seq); c.rec++; }
  }
  return c;
}

// Records and bytes that are complete, from the carry behind the whole buffer (mm_text_carry0 applied to every tile's summary):
//   final       everything belongs to records, consumed = nBytes
//   FASTA       all records but the last header line's; consumed is that line's offset (the caller has it from the record table:
//               *consumedIsLastHeader)
//   FASTQ       newlines / 4 records; consumed lies behind the newline with the 1-based index *consumedNl (0: consumed = 0)
MM_TXT_HD uint32_t mm_text_complete(int fmt, int final, uint64_t nBytes, uint8_t lastByte, const MmTextCarry& end, uint32_t* consumedNl, int* consumedIsLastHeader) {
  *consumedNl = 0; *consumedIsLastHeader = 0;
  if (!nBytes) return 0;
  if (fmt == MMT_FASTA) {
    if (final) return end.rec;
    *consumedIsLastHeader = 1;
    return end.rec - 1;
  }
  if (final) return (uint32_t)(((uint64_t)end.nl + (lastByte != '\n') + 3) / 4);
  *consumedNl = end.nl / 4 * 4;
  return end.nl / 4;
}

// header lines that start inside the buffer: the count of the carry behind it, without the FASTQ header that would start at the buffer's end
MM_TXT_HD uint32_t mm_text_headers(int fmt, uint64_t nBytes, uint8_t lastByte, const MmTextCarry& end) {
  if (!nBytes) return 0;
  return end.rec - (fmt == MMT_FASTQ && lastByte == '\n' && end.nl % 4 == 0 ? 1u : 0u);
}

// the name's length: from the byte behind hdrOff to the first ' ' or '\n' or the buffer's end; an empty header line ("\n") has none
MM_TXT_HD uint32_t mm_text_name_len(const uint8_t* p, uint64_t nBytes, uint64_t hdrOff) {
  if (hdrOff >= nBytes || p[hdrOff] == '\n') return 0;
  uint64_t i = hdrOff + 1;
  while (i < nBytes && p[i] != ' ' && p[i] != '\n') i++;
  return (uint32_t)(i - hdrOff - 1);
}
