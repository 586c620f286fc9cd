// mashmap_amd/csrc/mm_inflate_core.h -- a raw-deflate (RFC 1951) decoder for ONE BGZF block, and CRC-32 with its combine step, stated
// once for the host and the device (k_inflate_blocks, mm_inflate.hip; tests/hostlogic/inflate_check.cpp runs the same text against zlib).
//
// The caller supplies an emission policy E:
//   e.literal(byte)            one byte of output
//   e.match(length, distance)  `length` (3..258) bytes, byte i of them equal to output[pos - distance + i mod distance]
//   e.stored(src, n)           the n (1..65535) bytes of a stored block, src inside the block's input
//   e.lane(), E::kLanes, e.sync(), e.count(p)
//                              how the table build is spread: lane() of kLanes workers run the decoder in lockstep on the same input (the
//                              host: one worker; the kernel: the 64 lanes of a wave, every lane reading the same bits and taking the same
//                              branches); sync() makes the workers' table writes visible to one another; count(p) adds one to *p atomically.
// The decoder itself keeps the output position and checks every emission BEFORE it hands it to the policy: literal() is called only with
// pos < uLen, stored() only with n bytes left in the input and pos + n <= uLen, match() only with distance <= pos and pos + length <= uLen.  The policy never sees an emission that leaves the block.
//
// Bounds.  Input is read through BitReader only, which holds the block's base and cLen and never touches a byte at or beyond cLen (a stored
// block's bytes are checked against the bytes left before they are read).  Output goes through the policy only, under the checks above.
//
// Termination.  Every iteration of every loop below either consumes at least one input bit or emits at least one output byte, or
// leaves the decoder with an error (an iteration is counted once it has consumed or emitted):
//   * the block loop reads the 3 header bits of a deflate block per iteration;
//   * a stored block of LEN bytes is handed over whole and counted as LEN iterations;
//   * the code-length loop consumes a code (>= 1 bit) per iteration;
//   * the symbol loop consumes a literal/length code (>= 1 bit) per iteration.
// (decodeSym's walk over code lengths and the table fills are bounded by 15, 19, 320 and the table sizes.)  So a block of cLen bytes
// that may emit uLen bytes ends within 8 * cLen + uLen iterations in all.  The decoder counts its iterations against
// 8 * cLen + uLen + 64 all the same and answers MM_INFLATE_BAD_STREAM beyond: a mistake in the argument cannot make a wave spin.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MM_INF_HD __host__ __device__ inline
#else
#define MM_INF_HD inline
#endif

// the values of include/mashmap_hip.h's MM_INFLATE_* (this header stays free of the C ABI; mm_inflate.hip asserts that they agree)
enum { MMI_OK = 0, MMI_BAD_STREAM = 1, MMI_TRUNCATED = 2, MMI_OVERRUN = 3, MMI_SHORT = 4, MMI_BAD_DISTANCE = 5, MMI_BAD_CRC = 6 };

#define MMI_FAST_LIT 10      // width of the literal/length fast table
#define MMI_FAST_DIST 8      // width of the distance fast table
#define MMI_MAX_BITS 15

// ---------------------------------------------------------------------------------------------------------------------------------
// CRC-32, zlib's: reflected polynomial 0xEDB88320, register preset to and result inverted with 0xFFFFFFFF.
// ---------------------------------------------------------------------------------------------------------------------------------
#define MMI_CRC_POLY 0xEDB88320u
MM_INF_HD uint32_t mm_crc32_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ MMI_CRC_POLY : c >> 1;
  return c;
}
// crc32 of `prev`'s data followed by p[0..n): the bytewise table form (tab: 256 entries of mm_crc32_table_entry)
MM_INF_HD uint32_t mm_crc32_update(const uint32_t* tab, uint32_t prev, const uint8_t* p, uint32_t n) {
  uint32_t c = ~prev;
  for (uint32_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xff] ^ (c >> 8);
  return ~c;
}
// a(x) * b(x) mod P(x) on reflected 32-bit polynomials (bit 31 is x^0)
MM_INF_HD uint32_t mm_crc32_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; k++) {
    if (a & (0x80000000u >> k)) p ^= b;
    b = (b & 1) ? (b >> 1) ^ MMI_CRC_POLY : b >> 1;
  }
  return p;
}
// x^(8 * nBytes) mod P(x): square and multiply over the bits of 8 * nBytes
MM_INF_HD uint32_t mm_crc32_xpow8(uint64_t nBytes) {
  uint32_t r = 0x80000000u;            // x^0
  uint32_t sq = 0x00800000u;           // x^8
  for (; nBytes; nBytes >>= 1) {
    if (nBytes & 1) r = mm_crc32_mulmod(sq, r);
    sq = mm_crc32_mulmod(sq, sq);
  }
  return r;
}
// crc(A || B) from crc(A), crc(B) and x^(8 * len(B)): the presets and inversions of the two cancel
MM_INF_HD uint32_t mm_crc32_combine_op(uint32_t crcA, uint32_t crcB, uint32_t xpowLenB) { return mm_crc32_mulmod(xpowLenB, crcA) ^ crcB; }
MM_INF_HD uint32_t mm_crc32_combine(uint32_t crcA, uint32_t crcB, uint64_t lenB) { return mm_crc32_combine_op(crcA, crcB, mm_crc32_xpow8(lenB)); }

// The block's bytes in 64 slices for 64 workers to checksum: slice 0 takes the odd bytes, every other slice is exactly uLen / 64 long,
// so that the right-hand side of every combine step of a pairwise tree over the slices (1, 2, 4 ... 32 slices) has a length that
// depends on the step alone: its x^(8 len) is the square of the step before.
MM_INF_HD void mm_crc32_slice(uint32_t uLen, uint32_t slice, uint32_t& off, uint32_t& len) {
  const uint32_t each = uLen / 64, odd = uLen % 64;
  off = slice ? odd + slice * each : 0;
  len = slice ? each : each + odd;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The bit reader: LSB first (RFC 1951 3.1.1), bounded by cLen.
// ---------------------------------------------------------------------------------------------------------------------------------
struct MmBitReader {
  const uint8_t* in; uint32_t cLen, pos; uint64_t hold; uint32_t nbits;
  MM_INF_HD void init(const uint8_t* p, uint32_t n) { in = p; cLen = n; pos = 0; hold = 0; nbits = 0; }
  MM_INF_HD void refill() { while (nbits <= 56 && pos < cLen) { hold |= (uint64_t)in[pos++] << nbits; nbits += 8; } }
  // n <= 32 bits; false: the input holds fewer
  MM_INF_HD bool take(uint32_t n, uint32_t& v) {
    if (nbits < n) { refill(); if (nbits < n) return false; }
    v = (uint32_t)(hold & (((uint64_t)1 << n) - 1)); hold >>= n; nbits -= n;
    return true;
  }
  MM_INF_HD void drop(uint32_t n) { hold >>= n; nbits -= n; }
  // to the next byte boundary, and the bytes held ahead given back: pos is then the next unread byte
  MM_INF_HD void alignToByte() { drop(nbits & 7); pos -= nbits >> 3; hold = 0; nbits = 0; }
};

// One canonical code (RFC 1951 3.2.2): cnt[l] codes of length l, the symbols sorted by (length, symbol).  Lives where the caller puts
// it: the kernel keeps one MmInflateTables per wave in LDS (4.1 KB).
struct MmCanon { uint32_t cnt[16]; uint16_t sorted[288]; };
struct MmInflateTables {
  MmCanon lit, dist;                        // dist doubles as the code-length code (19 symbols) while a dynamic header is read
  uint16_t fastLit[1 << MMI_FAST_LIT];      // (length << 9 | symbol) of the code that prefixes the index, 0: longer than the table is wide (or unused)
  uint16_t fastDist[1 << MMI_FAST_DIST];
  uint32_t offs[16];
  uint8_t lens[320];                        // code lengths of a dynamic header: HLIT + HDIST of them in one run (a repeat may cross the boundary)
};

// Builds the code of lens[0..n).  kind: 0 the code-length code (an incomplete set is refused, as zlib refuses it), 1 literal/length or
// distance (an incomplete set passes when it is a single code of one bit, or no code at all: zlib's rule; using a code that is not
// there is an error where it is met).  Over-subscribed sets are refused.  fast may be null.
template <class E>
MM_INF_HD int mm_inflate_build(E& e, MmCanon& C, uint32_t* offs, const uint8_t* lens, uint32_t n, int kind, uint16_t* fast, uint32_t fastBits) {
  const uint32_t lane = e.lane();
  for (uint32_t l = lane; l < 16; l += E::kLanes) C.cnt[l] = 0;
  e.sync();
  for (uint32_t s = lane; s < n; s += E::kLanes) e.count(&C.cnt[lens[s]]);     // the counts, across the workers
  e.sync();
  int32_t left = 1; uint32_t maxLen = 0;
  for (uint32_t l = 1; l <= MMI_MAX_BITS; l++) {
    left <<= 1; left -= (int32_t)C.cnt[l];
    if (left < 0) return MMI_BAD_STREAM;                                        // over-subscribed
    if (C.cnt[l]) maxLen = l;
  }
  if (left > 0 && maxLen != 0 && (kind == 0 || maxLen != 1)) return MMI_BAD_STREAM;   // incomplete
  if (lane == 0) {
    uint32_t at = 0;
    for (uint32_t l = 1; l <= MMI_MAX_BITS; l++) { offs[l] = at; at += C.cnt[l]; }
    for (uint32_t s = 0; s < n; s++) if (lens[s]) C.sorted[offs[lens[s]]++] = (uint16_t)s;
  }
  e.sync();
  if (fast) {
    // entry i: the code that prefixes the bits of i (first bit of the stream in bit 0), found by the walk decodeSym makes on the stream
    for (uint32_t i = lane; i < (1u << fastBits); i += E::kLanes) {
      uint32_t code = 0, first = 0, index = 0; uint16_t ent = 0;
      for (uint32_t l = 1; l <= fastBits; l++) {
        code |= (i >> (l - 1)) & 1;
        const uint32_t c = C.cnt[l];
        if (code - first < c) { ent = (uint16_t)(l << 9 | C.sorted[index + (code - first)]); break; }
        index += c; first = (first + c) << 1; code <<= 1;
      }
      fast[i] = ent;
    }
    e.sync();
  }
  return MMI_OK;
}

// one symbol of code C off the stream: MMI_OK, MMI_TRUNCATED (the input ends inside the code) or MMI_BAD_STREAM (no such code)
MM_INF_HD int mm_inflate_sym(MmBitReader& br, const MmCanon& C, const uint16_t* fast, uint32_t fastBits, uint32_t& sym) {
  br.refill();                                   // 57 bits or more, or all that is left
  if (fast) {
    const uint16_t ent = fast[br.hold & ((1u << fastBits) - 1)];
    if (ent) {
      const uint32_t l = ent >> 9;
      if (l > br.nbits) return MMI_TRUNCATED;
      br.drop(l); sym = ent & 511;
      return MMI_OK;
    }
  }
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l <= MMI_MAX_BITS; l++) {
    if (l > br.nbits) return MMI_TRUNCATED;
    code |= (uint32_t)(br.hold >> (l - 1)) & 1;
    const uint32_t c = C.cnt[l];
    if (code - first < c) { sym = C.sorted[index + (code - first)]; br.drop(l); return MMI_OK; }
    index += c; first = (first + c) << 1; code <<= 1;
  }
  return MMI_BAD_STREAM;
}

// Decodes the raw-deflate stream in[0..cLen) that should yield uLen bytes.  MMI_OK: BFINAL's block ended with exactly uLen bytes
// emitted (bytes behind it in the input are not looked at, as zlib does not).  *steps (may be null) receives the iteration count.
template <class E>
MM_INF_HD int mm_inflate_decode(E& e, MmInflateTables& T, const uint8_t* in, uint32_t cLen, uint32_t uLen, uint64_t* stepsOut = nullptr) {
  MmBitReader br; br.init(in, cLen);
  const uint64_t bound = (uint64_t)8 * cLen + uLen + 64;
  uint64_t steps = 0;
  uint32_t pos = 0;                               // bytes emitted
  int rc = MMI_OK;
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
#define MMI_STEP() do { if (++steps > bound) { rc = MMI_BAD_STREAM; goto done; } } while (0)
#define MMI_FAIL(x) do { rc = (x); goto done; } while (0)
  for (;;) {
    uint32_t hdr;
    if (!br.take(3, hdr)) MMI_FAIL(MMI_TRUNCATED);
    MMI_STEP();
    const uint32_t bfinal = hdr & 1, btype = hdr >> 1;
    if (btype == 3) MMI_FAIL(MMI_BAD_STREAM);
    if (btype == 0) {
      br.alignToByte();
      if (cLen - br.pos < 4) MMI_FAIL(MMI_TRUNCATED);
      const uint32_t len = in[br.pos] | (uint32_t)in[br.pos + 1] << 8, nlen = in[br.pos + 2] | (uint32_t)in[br.pos + 3] << 8;
      br.pos += 4;
      if ((len ^ nlen) != 0xffff) MMI_FAIL(MMI_BAD_STREAM);
      if (cLen - br.pos < len) MMI_FAIL(MMI_TRUNCATED);
      if (uLen - pos < len) MMI_FAIL(MMI_OVERRUN);
      steps += len;                                                     // len bytes emitted: len iterations' worth
      if (steps > bound) MMI_FAIL(MMI_BAD_STREAM);
      if (len) e.stored(in + br.pos, len);
      br.pos += len; pos += len;
    } else {
      if (btype == 1) {
        // the fixed code (3.2.6), built like any other
        if (e.lane() == 0) {
          for (uint32_t s = 0; s < 288; s++) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
          for (uint32_t s = 288; s < 320; s++) T.lens[s] = 5;
        }
        e.sync();
        if ((rc = mm_inflate_build(e, T.lit, T.offs, T.lens, 288, 1, T.fastLit, MMI_FAST_LIT)) != MMI_OK) goto done;
        if ((rc = mm_inflate_build(e, T.dist, T.offs, T.lens + 288, 32, 1, T.fastDist, MMI_FAST_DIST)) != MMI_OK) goto done;
      } else {
        uint32_t v;
        if (!br.take(14, v)) MMI_FAIL(MMI_TRUNCATED);
        const uint32_t nlen = (v & 31) + 257, ndist = ((v >> 5) & 31) + 1, ncode = (v >> 10) + 4;
        if (nlen > 286 || ndist > 30) MMI_FAIL(MMI_BAD_STREAM);
        e.sync();                                                        // (the previous block's readers of T.lens are done)
        for (uint32_t i = 0; i < 19; i++) {
          uint32_t l = 0;
          if (i < ncode && !br.take(3, l)) MMI_FAIL(MMI_TRUNCATED);
          if (e.lane() == 0) T.lens[order[i]] = (uint8_t)l;
        }
        e.sync();
        if ((rc = mm_inflate_build(e, T.dist, T.offs, T.lens, 19, 0, (uint16_t*)nullptr, 0)) != MMI_OK) goto done;
        // the code lengths, with the repeat codes: one run over HLIT + HDIST entries
        uint32_t n = 0, prev = 0;
        while (n < nlen + ndist) {
          uint32_t sym;
          if ((rc = mm_inflate_sym(br, T.dist, nullptr, 0, sym)) != MMI_OK) goto done;
          MMI_STEP();
          uint32_t rep = 1, val = sym;
          if (sym == 16) { if (n == 0) MMI_FAIL(MMI_BAD_STREAM); uint32_t x; if (!br.take(2, x)) MMI_FAIL(MMI_TRUNCATED); rep = 3 + x; val = prev; }
          else if (sym == 17) { uint32_t x; if (!br.take(3, x)) MMI_FAIL(MMI_TRUNCATED); rep = 3 + x; val = 0; }
          else if (sym == 18) { uint32_t x; if (!br.take(7, x)) MMI_FAIL(MMI_TRUNCATED); rep = 11 + x; val = 0; }
          if (n + rep > nlen + ndist) MMI_FAIL(MMI_BAD_STREAM);         // a repeat running past the end
          if (e.lane() == 0) for (uint32_t i = 0; i < rep; i++) T.lens[n + i] = (uint8_t)val;
          n += rep; prev = val;
        }
        e.sync();
        if (T.lens[256] == 0) MMI_FAIL(MMI_BAD_STREAM);                  // no end-of-block code
        if ((rc = mm_inflate_build(e, T.lit, T.offs, T.lens, nlen, 1, T.fastLit, MMI_FAST_LIT)) != MMI_OK) goto done;
        if ((rc = mm_inflate_build(e, T.dist, T.offs, T.lens + nlen, ndist, 1, T.fastDist, MMI_FAST_DIST)) != MMI_OK) goto done;
      }
      for (;;) {
        uint32_t sym;
        if ((rc = mm_inflate_sym(br, T.lit, T.fastLit, MMI_FAST_LIT, sym)) != MMI_OK) goto done;
        MMI_STEP();
        if (sym < 256) {
          if (pos >= uLen) MMI_FAIL(MMI_OVERRUN);
          e.literal((uint8_t)sym); pos++;
          continue;
        }
        if (sym == 256) break;
        if (sym > 285) MMI_FAIL(MMI_BAD_STREAM);
        // length 3..258 (3.2.5): codes 257..264 no extra bits, then four codes per extra bit, 285 is 258
        const uint32_t lc = sym - 257;
        uint32_t len, x;
        if (lc < 8) len = 3 + lc;
        else if (lc == 28) len = 258;
        else { const uint32_t eb = (lc >> 2) - 1; if (!br.take(eb, x)) MMI_FAIL(MMI_TRUNCATED); len = 3 + ((4 + (lc & 3)) << eb) + x; }
        uint32_t dc;
        if ((rc = mm_inflate_sym(br, T.dist, T.fastDist, MMI_FAST_DIST, dc)) != MMI_OK) goto done;
        if (dc > 29) MMI_FAIL(MMI_BAD_STREAM);
        uint32_t dist;
        if (dc < 4) dist = 1 + dc;
        else { const uint32_t eb = (dc >> 1) - 1; if (!br.take(eb, x)) MMI_FAIL(MMI_TRUNCATED); dist = 1 + ((2 + (dc & 1)) << eb) + x; }
        if (dist > pos) MMI_FAIL(MMI_BAD_DISTANCE);
        if (uLen - pos < len) MMI_FAIL(MMI_OVERRUN);
        e.match(len, dist); pos += len;
      }
    }
    if (bfinal) break;
  }
  if (pos < uLen) rc = MMI_SHORT;
done:
#undef MMI_STEP
#undef MMI_FAIL
  if (stepsOut) *stepsOut = steps;
  return rc;
}

// the host's policy: bytes copied one by one into out[0..uLen)
struct MmInflateHostEmit {
  static constexpr uint32_t kLanes = 1;
  uint8_t* out; uint32_t pos = 0;
  explicit MmInflateHostEmit(uint8_t* o) : out(o) {}
  uint32_t lane() const { return 0; }
  void sync() {}
  void count(uint32_t* p) { ++*p; }
  void literal(uint8_t b) { out[pos++] = b; }
  void stored(const uint8_t* src, uint32_t n) { for (uint32_t i = 0; i < n; i++) out[pos++] = src[i]; }
  void match(uint32_t len, uint32_t dist) { for (uint32_t i = 0; i < len; i++, pos++) out[pos] = out[pos - dist]; }
};
// one block on the host: decoded into out[0..uLen) and checked against the descriptor's CRC-32 (tab: 256 entries of mm_crc32_table_entry)
inline int mm_inflate_block_host(MmInflateTables& T, const uint32_t* tab, const uint8_t* in, uint32_t cLen, uint8_t* out, uint32_t uLen, uint32_t crc, uint64_t* steps = nullptr) {
  MmInflateHostEmit e(out);
  const int rc = mm_inflate_decode(e, T, in, cLen, uLen, steps);
  if (rc != MMI_OK) return rc;
  return mm_crc32_update(tab, 0, out, uLen) == crc ? MMI_OK : MMI_BAD_CRC;
}
