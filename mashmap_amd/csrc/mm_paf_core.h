// mashmap_amd/csrc/mm_paf_core.h -- the second half of MapPost::finishRead for ONE row of mm_chain_reads, and the bytes of its PAF line.
//
//   MapPost::reportSteps             filterFalseHighIdentity (:441-454), mappingBoundarySanityCheck (:1714-1750)    mashmap_amd/host/skch_map_post.hpp
//   MapPost::appendReadMappings      the line, field by field through std::to_chars                                  (computeMap.hpp:1758-1806)
//
// Shared by the kernels (k_paf_measure, k_paf_write, mm_paf.hip) and by the CPU check (tests/hostlogic/paf_check.cpp), which runs it
// beside MapPost::finishRows + appendReadMappings on generated reads and compares every byte.  Compiles for the host (g++) and for the
// device (hipcc).
//
// Why the bytes are the host's:
//   length filter   (float)delta / (float)q_l is a float division on the host.  Here the two floats are divided in double and the quotient
//                   narrowed: a double holds 53 >= 2 * 24 + 2 bits, so the narrowed quotient is the correctly rounded float quotient, and
//                   x / 0 and 0 / 0 give the same +-inf and NaN.  Then 1.0 - quotient in double, narrowed to float, compared in double with
//                   the threshold the host computed (std::min(0.7, pow(pi, 3)), passed in): -inf drops the row, NaN keeps it.
//   clamps          integer comparisons in the host's order.
//   sparsify        NOT restated (std::hash<float> of nucIdentityUpperBound): mm_paf_params_ok refuses a block that asks for it.
//   integers        mm_paf_i64: the digits of std::to_chars.
//   floats          mm_paf_g6: std::to_chars(v, chars_format::general, 6), i.e. printf's %g, from the exact binary value in integer
//                   arithmetic -- a few 64-bit words of big integer --: the six digits are round-half-even(|v| / 10^(X - 5)) with X the
//                   decimal exponent, taken again when rounding carries into a seventh digit; X of the ROUNDED value picks the form
//                   (scientific for X < -4 or X >= 6).  Exact for +-0 and 2^-64 <= |v| < 2^64; anything else is "not formattable" (-1) and
//                   the read goes back to the host.  What is formatted: (100.0 or 1.0) * (double)nucIdentity -- a 24-bit by 5-bit product,
//                   exact in a double, so the one IEEE multiply rounds nothing --; kmerComplexity, the host's long double holding the row's
//                   double exactly; float(conservedSketches) / sketchSize, a float division taken through double as above, widened.
//   fakeMapQ        std::round(-10.0 * std::log10(1 - identity)) goes through log10f, which the device does not share bit for bit.  The
//                   host tabulates it instead (mmh_paf_mapq_table): ascending float thresholds t0 = 0 < t1 < ... <= 1 and, per interval
//                   [t_i, t_i+1), the text of the value (`-0` at 0, `255` at exactly 1).  An identity outside [0, 1] is not formattable.
#pragma once
#include <stdint.h>
#include "mm_heap.h"
#include "../../include/mashmap_hip.h"

// ---- the longest numeric part, field by field (mm_paf_numeric writes no more; k_paf_write's LDS slot is this long)
#define MM_PAF_I32_MAX 11                    // "-2147483648"; an end minus 1 of legacy output is computed in 64 bits: "-2147483649", as long
#define MM_PAF_G6_MAX 12                     // "-1.23457e-05", "-0.000123457": sign, 6 digits, point, and 4 of exponent or of "0.000"
#define MM_PAF_G6_POS_MAX (MM_PAF_G6_MAX - 1)        // of a value that is not negative (the identity, inside [0, 1])
#define MM_PAF_MAPQ_TEXT_MAX (MM_PAF_MAPQ_TEXT - 1)  // an entry of the mapQ table: 8 bytes, NUL-padded
// separator, queryLen, queryStartPos, queryEndPos, strand, each with its separator in front, and the one in front of the reference name
#define MM_PAF_BEFORE_REF_MAX (1 + MM_PAF_I32_MAX + 1 + MM_PAF_I32_MAX + 1 + MM_PAF_I32_MAX + 1 + 1 + 1)
// behind the reference name: its length, refStartPos, refEndPos, conservedSketches, blockLength, mapQ, id:f:, kc:f:, jc:f:, the newline
#define MM_PAF_AFTER_REF_MAX (5 * (1 + MM_PAF_I32_MAX) + (1 + MM_PAF_MAPQ_TEXT_MAX) + (1 + 5 + MM_PAF_G6_POS_MAX) + 2 * (1 + 5 + MM_PAF_G6_MAX) + 1)
// legacy: the length, the two positions, the identity in per cent, the newline
#define MM_PAF_AFTER_REF_LEGACY_MAX (3 * (1 + MM_PAF_I32_MAX) + (1 + MM_PAF_G6_POS_MAX) + 1)
#define MM_PAF_NUMERIC_MAX (MM_PAF_BEFORE_REF_MAX + MM_PAF_AFTER_REF_MAX)
static_assert(MM_PAF_BEFORE_REF_MAX == 39 && MM_PAF_AFTER_REF_MAX == 122 && MM_PAF_AFTER_REF_LEGACY_MAX == 49, "the fields of a PAF line, summed");
static_assert(MM_PAF_AFTER_REF_LEGACY_MAX <= MM_PAF_AFTER_REF_MAX && MM_PAF_NUMERIC_MAX == 161, "the longest numeric part of a line");
#define MM_PAF_NOT_FORMATTABLE (-1)

// the mapQ table as mm_paf_numeric reads it
struct mm_paf_mapq {
  const float* thresholds;                   // n of them, ascending, thresholds[0] == 0, the last <= 1
  const char* text;                          // MM_PAF_MAPQ_TEXT bytes an entry, NUL-padded
  int32_t n;
};

MM_HD bool mm_paf_params_ok(const mm_paf_params& p) { return p.sparsityThreshold == ~0ull; }

MM_HD uint64_t mm_paf_bits(double v) { uint64_t b; __builtin_memcpy(&b, &v, 8); return b; }
// a / b as the float division rounds it (see "length filter" above)
MM_HD float mm_paf_fdiv(float a, float b) { return (float)((double)a / (double)b); }

// ---- decimal integers; -> characters written (at most 20).  The digits are counted first and written from the last one back, so that
// no array of a lane's own is indexed by a variable (on the device that would be scratch memory)
MM_HD int mm_paf_u64(uint64_t v, char* out) {
  int n = 1;
  for (uint64_t t = v; t >= 10u; t /= 10u) n++;
  for (int i = n - 1; i >= 0; i--) { out[i] = (char)('0' + (int)(v % 10u)); v /= 10u; }
  return n;
}
MM_HD int mm_paf_u32(uint32_t v, char* out) {
  int n = 1;
  for (uint32_t t = v; t >= 10u; t /= 10u) n++;
  for (int i = n - 1; i >= 0; i--) { out[i] = (char)('0' + (int)(v % 10u)); v /= 10u; }
  return n;
}
MM_HD int mm_paf_i64(int64_t v, char* out) {
  if (v >= 0) return (uint64_t)v <= 0xffffffffull ? mm_paf_u32((uint32_t)v, out) : mm_paf_u64((uint64_t)v, out);
  out[0] = '-';
  const uint64_t m = 0ull - (uint64_t)v;
  return 1 + (m <= 0xffffffffull ? mm_paf_u32((uint32_t)m, out + 1) : mm_paf_u64(m, out + 1));
}

// ---- three 64-bit words of unsigned integer, least significant first: m * 10^25 < 2^53 * 2^84
struct mm_paf_u192 { uint64_t w[3]; };
MM_HD uint64_t mm_paf_mulhi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
MM_HD void mm_paf_mul(mm_paf_u192& x, uint64_t f) {
  uint64_t carry = 0;
  for (int i = 0; i < 3; i++) {
    const uint64_t lo = x.w[i] * f, hi = mm_paf_mulhi(x.w[i], f);
    const uint64_t s = lo + carry;
    carry = hi + (s < lo ? 1u : 0u);         // hi <= 2^64 - 2: no wrap
    x.w[i] = s;
  }
}
MM_HD uint64_t mm_paf_pow10(int n) {         // 0 <= n <= 19
  uint64_t p = 1;
  for (int i = 0; i < n; i++) p *= 10u;
  return p;
}
// word k of x by selection (x.w[k] with a variable k would put the three words into scratch memory on the device); 0 beyond them
MM_HD uint64_t mm_paf_word(const mm_paf_u192& x, int k) { return k == 0 ? x.w[0] : k == 1 ? x.w[1] : k == 2 ? x.w[2] : 0ull; }
// bit i of x, and whether any bit below i is set (0 <= i < 192)
MM_HD bool mm_paf_bit(const mm_paf_u192& x, int i) { return (mm_paf_word(x, i >> 6) >> (i & 63)) & 1u; }
MM_HD bool mm_paf_any_below(const mm_paf_u192& x, int i) {
  bool any = false;
  for (int k = 0; k < 3; k++) {
    if (i >= 64 * (k + 1)) any = any || x.w[k] != 0;
    else if (i > 64 * k) any = any || (x.w[k] & ((1ull << (i - 64 * k)) - 1ull)) != 0;
  }
  return any;
}
// the low 64 bits of x >> s (0 <= s < 192)
MM_HD uint64_t mm_paf_shr(const mm_paf_u192& x, int s) {
  const int k = s >> 6, b = s & 63;
  uint64_t v = mm_paf_word(x, k) >> b;
  if (b) v |= mm_paf_word(x, k + 1) << (64 - b);
  return v;
}

// round-half-even(m * 2^e / 10^s), for a quotient below 10^7: m < 2^53, -116 <= e <= 11, -25 <= s <= 14
MM_HD uint64_t mm_paf_scaled(uint64_t m, int e, int s) {
  if (s <= 0) {                              // m * 10^-s, times or over a power of two
    mm_paf_u192 N;
    N.w[0] = m; N.w[1] = 0; N.w[2] = 0;
    int p = -s;
    if (p > 19) { mm_paf_mul(N, mm_paf_pow10(19)); p -= 19; }
    mm_paf_mul(N, mm_paf_pow10(p));
    if (e >= 0) return N.w[0] << e;          // an integer below 10^7: nothing to round
    const int k = -e;                        // 1 .. 116
    uint64_t q = mm_paf_shr(N, k);
    if (mm_paf_bit(N, k - 1) && (mm_paf_any_below(N, k - 1) || (q & 1u))) q++;
    return q;
  }
  // |v| >= 10^6: over 10^s, and a power of two on whichever side it belongs.  The divisor stays below 2^64: the quotient is at least
  // 10^5, so 10^s * 2^-e <= m / 10^5 < 2^37, and for e >= 0 the dividend m << e is |v| < 2^64 itself
  uint64_t num = m, den = mm_paf_pow10(s);
  if (e >= 0) num <<= e; else den <<= -e;
  uint64_t q = num / den;
  const uint64_t r = num - q * den;          // r < den < 2^63: 2 * r does not wrap
  if (2 * r > den || (2 * r == den && (q & 1u))) q++;
  return q;
}

// The characters std::to_chars(v, std::chars_format::general, 6) writes -> their number (at most MM_PAF_G6_MAX), or
// MM_PAF_NOT_FORMATTABLE for inf, NaN and every finite v other than +-0 outside 2^-64 <= |v| < 2^64
MM_HD int mm_paf_g6(double v, char* out) {
  const uint64_t bits = mm_paf_bits(v);
  const int E = (int)((bits >> 52) & 0x7ffu);
  const uint64_t frac = bits & 0xfffffffffffffull;
  int n = 0;
  if (E == 0 && frac == 0) {
    if (bits >> 63) out[n++] = '-';
    out[n++] = '0';
    return n;
  }
  const int b2 = E - 1023;                   // floor(log2 |v|)
  if (E == 0 || E == 0x7ff || b2 < -64 || b2 >= 64) return MM_PAF_NOT_FORMATTABLE;
  const uint64_t m = frac | (1ull << 52);
  const int e = b2 - 52;
  // X = floor(log10 |v|) is floor(b2 * log10 2) or one more (|v| is in [2^b2, 2^(b2 + 1))); 1233 / 4096 = 0.30103 gives that floor for every
  // |b2| <= 64 (paf_check.cpp walks them all)
  int X = (b2 * 1233) >> 12;
  uint64_t D = mm_paf_scaled(m, e, X - 5);
  if (D >= 1000000u) { X++; D = mm_paf_scaled(m, e, X - 5); }   // the estimate was one short: 7 digits in front of the rounding
  if (D >= 1000000u) { X++; D = 100000u; }                     // 999999.5 and above: the rounding carried (D == 10^6 exactly)
  uint32_t packed = 0;                       // digit i (0: the leading one) in bits 4i .. 4i + 3: no array of the lane's own
  int nd = 6;
  bool tail = true;
  for (int i = 5; i >= 0; i--) {
    const uint32_t digit = (uint32_t)(D % 10u);
    D /= 10u;
    if (tail && digit == 0 && i > 0) nd = i; else tail = false;     // %g strips trailing zeros
    packed |= digit << (4 * i);
  }
#define MM_PAF_DIGIT(i) ((char)('0' + (int)((packed >> (4 * (i))) & 15u)))
  if (bits >> 63) out[n++] = '-';
  if (X < -4 || X >= 6) {
    out[n++] = MM_PAF_DIGIT(0);
    if (nd > 1) { out[n++] = '.'; for (int i = 1; i < nd; i++) out[n++] = MM_PAF_DIGIT(i); }
    out[n++] = 'e';
    int a = X;
    if (a < 0) { out[n++] = '-'; a = -a; } else out[n++] = '+';
    out[n++] = (char)('0' + a / 10); out[n++] = (char)('0' + a % 10);           // |X| <= 20: two digits, as %g pads them
  } else if (X >= 0) {
    for (int i = 0; i <= X; i++) out[n++] = MM_PAF_DIGIT(i);                              // (zeros behind nd belong to the integer part)
    if (nd > X + 1) { out[n++] = '.'; for (int i = X + 1; i < nd; i++) out[n++] = MM_PAF_DIGIT(i); }
  } else {
    out[n++] = '0'; out[n++] = '.';
    for (int i = 0; i < -X - 1; i++) out[n++] = '0';
    for (int i = 0; i < nd; i++) out[n++] = MM_PAF_DIGIT(i);
  }
#undef MM_PAF_DIGIT
  return n;
}

// ---- filterFalseHighIdentity (when asked for), then mappingBoundarySanityCheck, of one row; false: the row is dropped
MM_HD bool mm_paf_report_row(const mm_paf_params& P, mm_chain_row& e, int32_t contigLen, int32_t readLen) {
  if (P.filterLengthMismatches) {
    const int64_t q_l = (int64_t)e.queryEndPos - (int64_t)e.queryStartPos;
    const int64_t r_l = (int64_t)e.refEndPos + 1 - (int64_t)e.refStartPos;
    const int64_t d = r_l - q_l;
    const uint64_t delta = (uint64_t)(d < 0 ? -d : d);
    const float len_id_bound = (float)(1.0 - (double)mm_paf_fdiv((float)delta, (float)q_l));
    if ((double)len_id_bound < P.lenIdThreshold) return false;
  }
  const int32_t rlen = contigLen, inputLen = readLen;
  if (e.refStartPos < 0) e.refStartPos = 0;
  if (e.refStartPos >= rlen) e.refStartPos = rlen - 1;
  if (e.refEndPos < e.refStartPos) e.refEndPos = e.refStartPos;
  if (e.refEndPos >= rlen) e.refEndPos = rlen - 1;
  if (e.queryStartPos < 0) e.queryStartPos = 0;
  if (e.queryStartPos >= inputLen) e.queryStartPos = inputLen;
  if (e.queryEndPos < e.queryStartPos) e.queryEndPos = e.queryStartPos;
  if (e.queryEndPos >= inputLen) e.queryEndPos = inputLen;
  return true;
}

// the text of fakeMapQ for an identity -> its length into out, or MM_PAF_NOT_FORMATTABLE outside [0, 1] (NaN included)
MM_HD int mm_paf_mapq_text(const mm_paf_mapq& T, float identity, char* out) {
  if (!(identity >= 0.0f && identity <= 1.0f) || T.n < 1) return MM_PAF_NOT_FORMATTABLE;
  int lo = 0, hi = T.n;                      // the last entry with thresholds[i] <= identity (thresholds[0] == 0: there is one)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (T.thresholds[mid] <= identity) lo = mid; else hi = mid;
  }
  const char* t = T.text + (size_t)lo * MM_PAF_MAPQ_TEXT;
  int n = 0;
  while (n < MM_PAF_MAPQ_TEXT_MAX && t[n]) { out[n] = t[n]; n++; }
  return n;
}

// Everything of a line except the two names, in appendReadMappings' field order, of a row mm_paf_report_row kept: out[0, *beforeRef)
// stands between the query name and the reference name, out[*beforeRef, length) behind the reference name, newline included.
// -> length (at most MM_PAF_NUMERIC_MAX), or MM_PAF_NOT_FORMATTABLE when a field is not formattable (out is then undefined)
MM_HD int mm_paf_numeric(const mm_paf_params& P, const mm_chain_row& e, int32_t contigLen, const mm_paf_mapq& T, char* out, int* beforeRef) {
  const char sep = P.legacy ? ' ' : '\t';
  const int64_t back = P.legacy ? 1 : 0;
  int n = 0, k;
  out[n++] = sep; n += mm_paf_i64(e.queryLen, out + n);
  out[n++] = sep; n += mm_paf_i64(e.queryStartPos, out + n);
  out[n++] = sep; n += mm_paf_i64((int64_t)e.queryEndPos - back, out + n);
  out[n++] = sep; out[n++] = (int16_t)e.strand == 1 ? '+' : '-';   // MappingResult::strand is 16 bits wide (MapPost::finishRows casts)
  out[n++] = sep;
  *beforeRef = n;
  out[n++] = sep; n += mm_paf_i64(contigLen, out + n);
  out[n++] = sep; n += mm_paf_i64(e.refStartPos, out + n);
  out[n++] = sep; n += mm_paf_i64((int64_t)e.refEndPos - back, out + n);
  if (!P.legacy) {
    out[n++] = sep; n += mm_paf_i64(e.conservedSketches, out + n);
    out[n++] = sep; n += mm_paf_i64(e.blockLength, out + n);
    out[n++] = sep; k = mm_paf_mapq_text(T, e.nucIdentity, out + n); if (k < 0) return MM_PAF_NOT_FORMATTABLE; n += k;
    out[n++] = sep; out[n++] = 'i'; out[n++] = 'd'; out[n++] = ':'; out[n++] = 'f'; out[n++] = ':';
    k = mm_paf_g6((P.aniPercentage ? 100.0 : 1.0) * (double)e.nucIdentity, out + n); if (k < 0) return MM_PAF_NOT_FORMATTABLE; n += k;
    out[n++] = sep; out[n++] = 'k'; out[n++] = 'c'; out[n++] = ':'; out[n++] = 'f'; out[n++] = ':';
    k = mm_paf_g6(e.kmerComplexity, out + n); if (k < 0) return MM_PAF_NOT_FORMATTABLE; n += k;
    if (!P.merge) {
      out[n++] = sep; out[n++] = 'j'; out[n++] = 'c'; out[n++] = ':'; out[n++] = 'f'; out[n++] = ':';
      k = mm_paf_g6((double)mm_paf_fdiv((float)e.conservedSketches, (float)e.sketchSize), out + n); if (k < 0) return MM_PAF_NOT_FORMATTABLE; n += k;
    }
  } else {
    // the identity of legacy output is not range-checked by a mapQ field: the same bound, so that a length above the slot cannot occur
    if (!(e.nucIdentity >= 0.0f && e.nucIdentity <= 1.0f)) return MM_PAF_NOT_FORMATTABLE;
    out[n++] = sep; k = mm_paf_g6((double)e.nucIdentity * 100.0, out + n); if (k < 0) return MM_PAF_NOT_FORMATTABLE; n += k;
  }
  out[n++] = '\n';
  return n;
}
