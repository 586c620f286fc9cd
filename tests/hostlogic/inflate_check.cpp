// tests/hostlogic/inflate_check.cpp -- mashmap_amd/csrc/mm_inflate_core.h (the raw-deflate decoder and CRC-32 the kernel
// k_inflate_blocks runs) against zlib.  Stand-alone; built with -fsanitize=address,undefined by tests/test_inflate_core.py, links -lz.
//   inflate_check              runs everything, prints one line per section and "differences N"
//   inflate_check --dump FILE  writes the zoo (generated blocks at the GPU test's lengths, every hand-built stream, every named
//                              malformed block) for tests/test_gpu_inflate.py: the bytes this program has run under the sanitizers
// Every input and output buffer is a heap block of exactly cLen / uLen bytes: a read or write one byte outside is a sanitizer report.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../mashmap_amd/csrc/mm_inflate_core.h"

typedef std::vector<uint8_t> Bytes;
static uint32_t g_tab[256];
static long g_diff = 0;
static void fail(const std::string& what) { if (g_diff++ < 40) printf("DIFF %s\n", what.c_str()); }

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 11); }

// ---- the bit writer the hand-built streams come from ----------------------------------------------------------------------------
struct BitWriter {
  Bytes out; uint64_t hold = 0; int n = 0;
  void bits(uint32_t v, int k) { hold |= (uint64_t)v << n; n += k; while (n >= 8) { out.push_back((uint8_t)hold); hold >>= 8; n -= 8; } }   // LSB first
  void code(uint32_t c, int len) { for (int i = len - 1; i >= 0; i--) bits((c >> i) & 1, 1); }                                                // a Huffman code: MSB first
  void align() { if (n) bits(0, 8 - n); }
  void byte(uint8_t b) { bits(b, 8); }
  Bytes done() { align(); return out; }
};
// canonical codes of a length array (RFC 1951 3.2.2)
static std::vector<uint32_t> canon(const std::vector<int>& lens) {
  std::vector<uint32_t> codes(lens.size(), 0); int cnt[17] = {0}; uint32_t next[17] = {0};
  for (int l : lens) cnt[l]++;
  cnt[0] = 0;
  uint32_t c = 0;
  for (int b = 1; b <= 16; b++) { c = (c + cnt[b - 1]) << 1; next[b] = c; }
  for (size_t s = 0; s < lens.size(); s++) if (lens[s]) codes[s] = next[lens[s]]++;
  return codes;
}
struct Code { std::vector<int> lens; std::vector<uint32_t> codes; void set(const std::vector<int>& l) { lens = l; codes = canon(l); }
              void put(BitWriter& w, int sym) const { w.code(codes[sym], lens[sym]); } };
static Code fixedLit() { std::vector<int> l(288); for (int s = 0; s < 288; s++) l[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; Code c; c.set(l); return c; }
static Code fixedDist() { Code c; c.set(std::vector<int>(32, 5)); return c; }
// a complete code over the given symbols: lengths of a balanced tree
static std::vector<int> completeLens(int n, const std::vector<int>& syms) {
  std::vector<int> l(n, 0); const int m = (int)syms.size(); int L = 1; while ((1 << L) < m) L++;
  const int shortOnes = (1 << L) - m;
  for (int i = 0; i < m; i++) l[syms[i]] = i < shortOnes ? L - 1 : L;
  return l;
}
static void putMatch(BitWriter& w, const Code& lit, const Code& dist, int len, int d) {
  int lc; if (len == 258) lc = 28; else if (len < 11) lc = len - 3; else { int eb = 1; while (len - 3 >= (8 << eb)) eb++; lc = 4 * (eb + 1) + ((len - 3) >> eb) - 4; }
  lit.put(w, 257 + lc);
  if (lc >= 8 && lc != 28) { const int eb = (lc >> 2) - 1; w.bits((uint32_t)(len - 3 - ((4 + (lc & 3)) << eb)), eb); }
  int dc; if (d <= 4) dc = d - 1; else { int eb = 1; while (d - 1 >= (4 << eb)) eb++; dc = 2 * (eb + 1) + ((d - 1) >> eb) - 2; }
  dist.put(w, dc);
  if (dc >= 4) { const int eb = (dc >> 1) - 1; w.bits((uint32_t)(d - 1 - ((2 + (dc & 1)) << eb)), eb); }
}
// the code-length code every hand-built dynamic header uses: 13 symbols of 4 bits, 6 of 5 (complete)
static Code clCode() { std::vector<int> l(19, 4); for (int s = 10; s <= 15; s++) l[s] = 5; Code c; c.set(l); return c; }
typedef std::vector<std::pair<int, int>> ClSyms;   // (symbol, value of its extra bits)
static ClSyms rle(const std::vector<int>& all) {
  ClSyms o;
  for (size_t i = 0; i < all.size();) {
    size_t j = i; while (j < all.size() && all[j] == all[i]) j++;
    size_t run = j - i;
    if (all[i] == 0) { while (run >= 11) { const size_t r = std::min<size_t>(run, 138); o.push_back({18, (int)r - 11}); run -= r; }
                       if (run >= 3) { o.push_back({17, (int)run - 3}); run = 0; } while (run--) o.push_back({0, 0}); }
    else { o.push_back({all[i], 0}); run--; while (run >= 3) { const size_t r = std::min<size_t>(run, 6); o.push_back({16, (int)r - 3}); run -= r; } while (run--) o.push_back({all[i], 0}); }
    i = j;
  }
  return o;
}
static void dynHeaderRaw(BitWriter& w, int bfinal, int hlit, int hdist, int hclen, const std::vector<int>& clLens, const ClSyms& syms) {
  static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  w.bits(bfinal, 1); w.bits(2, 2); w.bits(hlit, 5); w.bits(hdist, 5); w.bits(hclen - 4, 4);
  for (int i = 0; i < hclen; i++) w.bits(clLens[order[i]], 3);
  Code cl; cl.set(clLens);
  for (auto& s : syms) { cl.put(w, s.first); if (s.first == 16) w.bits(s.second, 2); else if (s.first == 17) w.bits(s.second, 3); else if (s.first == 18) w.bits(s.second, 7); }
}
static void dynHeader(BitWriter& w, int bfinal, const std::vector<int>& lit, const std::vector<int>& dist) {
  std::vector<int> all(lit); all.insert(all.end(), dist.begin(), dist.end());
  dynHeaderRaw(w, bfinal, (int)lit.size() - 257, (int)dist.size() - 1, 19, clCode().lens, rle(all));
}

// ---- zlib as the oracle -----------------------------------------------------------------------------------------------------------
// true: inflate(..., -15) accepts the stream with total_out == uLen; out receives the bytes
static bool zlibInflate(const uint8_t* in, uint32_t cLen, uint32_t uLen, Bytes& out) {
  out.assign(uLen, 0);
  z_stream zs; memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, -15) != Z_OK) { printf("inflateInit2 failed\n"); exit(2); }
  uint8_t dummyIn = 0, dummyOut = 0;
  zs.next_in = cLen ? (Bytef*)in : &dummyIn; zs.avail_in = cLen; zs.next_out = uLen ? out.data() : &dummyOut; zs.avail_out = uLen;
  const int rc = inflate(&zs, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && zs.total_out == uLen;
  inflateEnd(&zs);
  return ok;
}
static Bytes zlibDeflate(const Bytes& in, int level, int strategy) {
  z_stream zs; memset(&zs, 0, sizeof zs);
  if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) { printf("deflateInit2 failed\n"); exit(2); }
  Bytes out(deflateBound(&zs, in.size()) + 64);
  uint8_t dummy = 0;
  zs.next_in = in.empty() ? &dummy : (Bytef*)in.data(); zs.avail_in = (uInt)in.size(); zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
  if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { printf("deflate failed\n"); exit(2); }
  out.resize(zs.total_out); deflateEnd(&zs);
  return out;
}

// ---- one comparison ---------------------------------------------------------------------------------------------------------------
static long g_runs = 0, g_accepted = 0, g_onlyOurs = 0, g_overBound = 0; static long g_status[8] = {0};
// runs the core on exact-size heap copies; returns its status.  The acceptance rules against zlib:
//  (i) zlib accepts and the CRC is the payload's  =>  status OK and the same bytes;  (ii) status OK  =>  uLen bytes whose CRC-32 is crc
static int runOne(const std::string& name, const uint8_t* in, uint32_t cLen, uint32_t uLen, uint32_t crc, Bytes* outBytes = nullptr) {
  uint8_t* cin = (uint8_t*)malloc(cLen ? cLen : 1); if (cLen) memcpy(cin, in, cLen);
  uint8_t* cout = (uint8_t*)malloc(uLen ? uLen : 1);
  if (uLen) memset(cout, 0xA5, uLen);
  static MmInflateTables T;
  uint64_t steps = 0;
  const int rc = mm_inflate_block_host(T, g_tab, cLen ? cin : cin, cLen, cout, uLen, crc, &steps);
  g_runs++; g_status[rc & 7]++;
  if (steps > (uint64_t)8 * cLen + uLen) { g_overBound++; fail(name + ": more iterations than 8 cLen + uLen"); }
  Bytes z;
  const bool zok = zlibInflate(cin, cLen, uLen, z);
  const bool zcrc = zok && (uint32_t)crc32(crc32(0L, Z_NULL, 0), z.data(), uLen) == crc;
  if (zcrc) { g_accepted++; if (rc != MMI_OK) fail(name + ": zlib accepts, status " + std::to_string(rc)); else if (uLen && memcmp(z.data(), cout, uLen)) fail(name + ": bytes differ from zlib's"); }
  if (rc == MMI_OK) {
    if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), cout, uLen) != crc) fail(name + ": status OK with another CRC");
    if (!zcrc) g_onlyOurs++;
  }
  if (zok && !zcrc && rc != MMI_BAD_CRC) fail(name + ": zlib's bytes have another CRC, status " + std::to_string(rc));
  if (outBytes) outBytes->assign(cout, cout + uLen);
  free(cin); free(cout);
  return rc;
}
static uint32_t crcOf(const Bytes& b) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), b.data(), (uInt)b.size()); }

// ---- corpora ------------------------------------------------------------------------------------------------------------------------
static Bytes corpus(int kind, size_t n) {
  Bytes b; b.reserve(n + 256);
  if (kind == 0) { size_t col = 0; b.insert(b.end(), {'>', 'c', 'h', 'r', '1', '\n'}); while (b.size() < n) { if (col == 60) { b.push_back('\n'); col = 0; } else { b.push_back("ACGT"[rnd() & 3]); col++; } } }
  else if (kind == 1) { int r = 0; while (b.size() < n) { char h[64]; const int hl = snprintf(h, sizeof h, "@read%d/1\n", r++); b.insert(b.end(), h, h + hl); const int L = 50 + rnd() % 100;
                         for (int i = 0; i < L; i++) b.push_back("ACGT"[rnd() & 3]); b.push_back('\n'); b.push_back('+'); b.push_back('\n'); for (int i = 0; i < L; i++) b.push_back((uint8_t)(33 + rnd() % 41)); b.push_back('\n'); } }
  else while (b.size() < n) b.push_back((uint8_t)rnd());
  b.resize(n);
  return b;
}
struct Config { int level, strategy; const char* name; };
static const Config kConfigs[7] = {{0, Z_DEFAULT_STRATEGY, "l0"}, {1, Z_DEFAULT_STRATEGY, "l1"}, {6, Z_DEFAULT_STRATEGY, "l6"}, {9, Z_DEFAULT_STRATEGY, "l9"},
                                   {6, Z_FIXED, "fixed"}, {6, Z_RLE, "rle"}, {6, Z_HUFFMAN_ONLY, "huff"}};
static const char* kCorpus[3] = {"fasta", "fastq", "random"};

// ---- the hand-built streams and the named malformed blocks ----------------------------------------------------------------------
struct Item { std::string name; Bytes comp; uint32_t uLen; uint32_t crc; int expect; Bytes payload; };   // expect: the status (payload: what OK yields)
static Item good(const std::string& name, const Bytes& comp, const Bytes& payload) { return Item{name, comp, (uint32_t)payload.size(), crcOf(payload), MMI_OK, payload}; }
static Item bad(const std::string& name, const Bytes& comp, uint32_t uLen, int expect, uint32_t crc = 0) { return Item{name, comp, uLen, crc, expect, Bytes()}; }
static Bytes str(const char* s) { return Bytes(s, s + strlen(s)); }
static void lits(BitWriter& w, const Code& c, const Bytes& b) { for (uint8_t x : b) c.put(w, x); }

static std::vector<Item> handBuilt() {
  std::vector<Item> v;
  g_rng = 0x243F6A8885A308D3ull;           // the same bytes in every run and in the dump
  const Code FL = fixedLit(), FD = fixedDist();
  { // a single 1-bit distance code (an incomplete set zlib accepts)
    Code L; L.set(completeLens(265, {'A', 'C', 256, 257 + 7})); Code D; D.set({1});
    BitWriter w; dynHeader(w, 1, L.lens, D.lens); lits(w, L, str("AC")); putMatch(w, L, D, 10, 1); L.put(w, 256);
    v.push_back(good("one_bit_distance_code", w.done(), str("ACCCCCCCCCCC")));
  }
  { // no distance code at all
    Code L; L.set(completeLens(257, {'A', 'C', 'G', 'T', 256})); Code D; D.set({0});
    BitWriter w; dynHeader(w, 1, L.lens, D.lens); lits(w, L, str("GATTACA")); L.put(w, 256);
    v.push_back(good("no_distance_code", w.done(), str("GATTACA")));
  }
  { // 15-bit codes: lengths 1, 2 ... 14, 15, 15
    std::vector<int> l(257, 0); const int syms[16] = {'A', 'C', 'G', 'T', 'N', '\n', '>', 'a', 'c', 'g', 't', 'n', '0', '1', 256, 'x'};
    for (int i = 0; i < 16; i++) l[syms[i]] = i < 15 ? i + 1 : 15;
    Code L; L.set(l); Code D; D.set({0});
    BitWriter w; dynHeader(w, 1, L.lens, D.lens); const Bytes p = str("xACGTNx01\n>acgtnxxA"); lits(w, L, p); L.put(w, 256);
    v.push_back(good("fifteen_bit_codes", w.done(), p));
  }
  { // HCLEN 5, the least a stream zlib accepts can have (HCLEN 4 names the lengths of 16, 17, 18 and 0 only: no code can be longer than 0
    // bits and the end-of-block code is missing -- that stream is among the malformed ones): symbols 1..256 at 8 bits
    std::vector<int> cl(19, 0); cl[0] = 1; cl[8] = 1;
    ClSyms s; s.push_back({0, 0}); for (int i = 0; i < 256; i++) s.push_back({8, 0}); s.push_back({0, 0});
    BitWriter w; dynHeaderRaw(w, 1, 0, 0, 5, cl, s);
    std::vector<int> l(257, 8); l[0] = 0; Code L; L.set(l); const Bytes p = str("ACGTACGTNN\n"); lits(w, L, p); L.put(w, 256);
    v.push_back(good("hclen_5", w.done(), p));
  }
  { // repeat codes that cross from the literal/length lengths into the distance lengths: zeros (18) and a copied length (16)
    std::vector<int> l = completeLens(270, {'A', 'C', 'G', 'T', 256}); std::vector<int> d(10, 0); d[8] = 1; d[9] = 1;
    Code L; L.set(l); BitWriter w; dynHeader(w, 1, l, d); const Bytes p = str("TTGACA"); lits(w, L, p); L.put(w, 256);
    v.push_back(good("zero_repeat_across_the_boundary", w.done(), p));
    std::vector<int> l2(257, 0); l2['A'] = 2; l2['C'] = 2; l2['G'] = 3; l2['T'] = 3; l2[256] = 2; std::vector<int> d2(4, 2);
    Code L2; L2.set(l2); BitWriter w2; dynHeader(w2, 1, l2, d2); lits(w2, L2, p); L2.put(w2, 256);
    v.push_back(good("copied_length_across_the_boundary", w2.done(), p));
  }
  { // a match of 258 at distances 1 to 8; the last one ends exactly at uLen
    BitWriter w; w.bits(1, 1); w.bits(1, 2); Bytes p = str("ACGTTGCA"); lits(w, FL, p);
    for (int d = 1; d <= 8; d++) { putMatch(w, FL, FD, 258, d); for (int i = 0; i < 258; i++) p.push_back(p[p.size() - d]); }
    FL.put(w, 256);
    v.push_back(good("length_258_at_distances_1_to_8", w.done(), p));
  }
  { // a match at distance 32768, behind a stored block
    Bytes p = corpus(2, 32768); BitWriter w; w.bits(0, 1); w.bits(0, 2); w.align(); w.bits(32768, 16); w.bits(32768 ^ 0xffff, 16); for (uint8_t x : p) w.byte(x);
    w.bits(1, 1); w.bits(1, 2); putMatch(w, FL, FD, 100, 32768); FL.put(w, 256);
    for (int i = 0; i < 100; i++) p.push_back(p[p.size() - 32768]);
    v.push_back(good("distance_32768", w.done(), p));
  }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, str("AC")); putMatch(w, FL, FD, 5, 2); FL.put(w, 256); v.push_back(good("match_ends_at_ulen", w.done(), str("ACACACA"))); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, str("ACG")); putMatch(w, FL, FD, 3, 3); FL.put(w, 256); v.push_back(good("match_reaches_byte_0", w.done(), str("ACGACG"))); }
  { BitWriter w; w.bits(1, 1); w.bits(0, 2); w.align(); w.bits(0, 16); w.bits(0xffff, 16); v.push_back(good("stored_len_0", w.done(), Bytes())); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); FL.put(w, 256); v.push_back(good("bgzf_eof_block", w.done(), Bytes())); }
  { // a stored block of 65535 bytes whose header starts in mid-byte
    Bytes p = str("A"); BitWriter w; w.bits(0, 1); w.bits(1, 2); lits(w, FL, p); FL.put(w, 256);
    w.bits(1, 1); w.bits(0, 2); w.align(); w.bits(65535, 16); w.bits(0, 16); const Bytes q = corpus(0, 65535); for (uint8_t x : q) w.byte(x);
    p.insert(p.end(), q.begin(), q.end());
    v.push_back(good("stored_65535_behind_a_header_in_mid_byte", w.done(), p));
  }
  { // the same with 65520 bytes: the longest such stream that still fits a BGZF block (65527 bytes compressed; the one above is 65542)
    Bytes p = str("A"); BitWriter w; w.bits(0, 1); w.bits(1, 2); lits(w, FL, p); FL.put(w, 256);
    w.bits(1, 1); w.bits(0, 2); w.align(); w.bits(65520, 16); w.bits(65520 ^ 0xffff, 16); const Bytes q = corpus(1, 65520); for (uint8_t x : q) w.byte(x);
    p.insert(p.end(), q.begin(), q.end());
    v.push_back(good("stored_65520_behind_a_header_in_mid_byte", w.done(), p));
  }
  { // the end-of-block code's last bit is the input's last bit: 3 + 6 * 9 + 7 = 64 bits
    Bytes p; for (int i = 0; i < 6; i++) p.push_back((uint8_t)(200 + i)); BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, p); FL.put(w, 256);
    if (w.n != 0 || w.out.size() != 8) { printf("hand-built stream is not 64 bits\n"); exit(2); }
    v.push_back(good("end_of_block_on_the_last_bit", w.done(), p));
  }
  { // an empty stored block in mid-stream, as Z_SYNC_FLUSH leaves one
    BitWriter w; w.bits(0, 1); w.bits(1, 2); lits(w, FL, str("ACGT")); FL.put(w, 256); w.bits(0, 1); w.bits(0, 2); w.align(); w.bits(0, 16); w.bits(0xffff, 16);
    w.bits(1, 1); w.bits(1, 2); lits(w, FL, str("TGCA")); putMatch(w, FL, FD, 4, 8); FL.put(w, 256);
    v.push_back(good("empty_stored_block_in_mid_stream", w.done(), str("ACGTTGCAACGT")));
  }
  return v;
}

static std::vector<Item> malformed() {
  std::vector<Item> v;
  const Code FL = fixedLit(), FD = fixedDist();
  const Bytes acgt = str("ACGTACGT");
  { BitWriter w; w.bits(1, 1); w.bits(3, 2); w.bits(0, 13); v.push_back(bad("block_type_3", w.done(), 8, MMI_BAD_STREAM)); }
  { BitWriter w; w.bits(1, 1); w.bits(0, 2); w.align(); w.bits(8, 16); w.bits(8, 16); for (uint8_t x : acgt) w.byte(x); v.push_back(bad("stored_len_is_not_the_complement", w.done(), 8, MMI_BAD_STREAM)); }
  { ClSyms s; for (int i = 0; i < 288; i++) s.push_back({8, 0}); BitWriter w; dynHeaderRaw(w, 1, 30, 0, 19, clCode().lens, s); w.bits(0, 32); v.push_back(bad("hlit_above_286", w.done(), 8, MMI_BAD_STREAM)); }
  { ClSyms s; for (int i = 0; i < 288; i++) s.push_back({8, 0}); BitWriter w; dynHeaderRaw(w, 1, 0, 30, 19, clCode().lens, s); w.bits(0, 32); v.push_back(bad("hdist_above_30", w.done(), 8, MMI_BAD_STREAM)); }
  { ClSyms s; s.push_back({16, 0}); for (int i = 0; i < 258; i++) s.push_back({8, 0}); BitWriter w; dynHeaderRaw(w, 1, 0, 0, 19, clCode().lens, s); w.bits(0, 32); v.push_back(bad("repeat_with_nothing_to_repeat", w.done(), 8, MMI_BAD_STREAM)); }
  { ClSyms s; for (int i = 0; i < 256; i++) s.push_back({8, 0}); s.push_back({18, 127}); BitWriter w; dynHeaderRaw(w, 1, 0, 0, 19, clCode().lens, s); w.bits(0, 32); v.push_back(bad("repeat_past_the_end", w.done(), 8, MMI_BAD_STREAM)); }
  { ClSyms s; for (int i = 0; i < 257; i++) s.push_back({7, 0}); s.push_back({0, 0}); BitWriter w; dynHeaderRaw(w, 1, 0, 0, 19, clCode().lens, s); w.bits(0, 32); v.push_back(bad("over_subscribed_set", w.done(), 8, MMI_BAD_STREAM)); }
  { ClSyms s; s.push_back({0, 0}); for (int i = 0; i < 255; i++) s.push_back({8, 0}); s.push_back({0, 0}); s.push_back({0, 0}); BitWriter w; dynHeaderRaw(w, 1, 0, 0, 19, clCode().lens, s); w.bits(0, 32);
    v.push_back(bad("missing_end_of_block_code", w.done(), 8, MMI_BAD_STREAM)); }
  { std::vector<int> cl(19, 0); cl[16] = 2; cl[17] = 2; cl[18] = 2; cl[0] = 2; ClSyms s; s.push_back({18, 127}); s.push_back({18, 109}); BitWriter w; dynHeaderRaw(w, 1, 0, 0, 4, cl, s); w.bits(0, 32);
    v.push_back(bad("hclen_4", w.done(), 8, MMI_BAD_STREAM)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, acgt); FL.put(w, 286); FD.put(w, 0); FL.put(w, 256); v.push_back(bad("length_symbol_286", w.done(), 16, MMI_BAD_STREAM)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, acgt); FL.put(w, 287); FD.put(w, 0); FL.put(w, 256); v.push_back(bad("length_symbol_287", w.done(), 16, MMI_BAD_STREAM)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, acgt); FL.put(w, 257); FD.put(w, 30); FL.put(w, 256); v.push_back(bad("distance_symbol_30", w.done(), 11, MMI_BAD_STREAM)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, acgt); FL.put(w, 257); FD.put(w, 31); FL.put(w, 256); v.push_back(bad("distance_symbol_31", w.done(), 11, MMI_BAD_STREAM)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, str("ACG")); putMatch(w, FL, FD, 3, 4); FL.put(w, 256); v.push_back(bad("distance_one_before_byte_0", w.done(), 6, MMI_BAD_DISTANCE)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, acgt); FL.put(w, 256); Bytes c = w.done(); c.resize(c.size() - 2); v.push_back(bad("input_exhausted", c, 8, MMI_TRUNCATED)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, acgt); FL.put(w, 256); v.push_back(bad("output_past_ulen", w.done(), 7, MMI_OVERRUN)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, str("AC")); putMatch(w, FL, FD, 6, 2); FL.put(w, 256); v.push_back(bad("match_past_ulen", w.done(), 7, MMI_OVERRUN)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, acgt); FL.put(w, 256); v.push_back(bad("stream_ends_before_ulen", w.done(), 9, MMI_SHORT)); }
  { BitWriter w; w.bits(1, 1); w.bits(1, 2); lits(w, FL, acgt); FL.put(w, 256); v.push_back(bad("crc_mismatch", w.done(), 8, MMI_BAD_CRC, crcOf(acgt) ^ 0x10)); }
  return v;
}

static const uint32_t kBigLens[6] = {32767, 32768, 32769, 65280, 65535, 65536};
static const uint32_t kGpuLens[12] = {0, 1, 63, 64, 65, 257, 258, 259, 32768, 32769, 65535, 65536};

static int dump(const char* path) {
  FILE* f = fopen(path, "wb"); if (!f) return 2;
  auto put = [&](const Item& it) {
    Bytes o;                                // nothing is written that has not been through the core here
    const int rc = runOne(it.name, it.comp.data(), (uint32_t)it.comp.size(), it.uLen, it.crc, &o);
    if (rc != it.expect || (rc == MMI_OK && o != it.payload)) fail(it.name + ": status " + std::to_string(rc));
    fprintf(f, "%s %d %u %u %zu %zu\n", it.name.c_str(), it.expect, it.uLen, it.crc, it.comp.size(), it.payload.size());
    if (!it.comp.empty()) fwrite(it.comp.data(), 1, it.comp.size(), f);
    if (!it.payload.empty()) fwrite(it.payload.data(), 1, it.payload.size(), f);
  };
  for (auto& it : handBuilt()) put(it);
  for (auto& it : malformed()) put(it);
  for (int c = 0; c < 3; c++) for (auto& cf : kConfigs) for (uint32_t n : kGpuLens) { const Bytes p = corpus(c, n); put(good(std::string(kCorpus[c]) + "_" + cf.name + "_" + std::to_string(n), zlibDeflate(p, cf.level, cf.strategy), p)); }
  fclose(f);
  return g_diff ? 1 : 0;
}

int main(int argc, char** argv) {
  for (uint32_t i = 0; i < 256; i++) g_tab[i] = mm_crc32_table_entry(i);
  if (argc == 3 && !strcmp(argv[1], "--dump")) return dump(argv[2]);

  // CRC-32 and the combine step against zlib
  { long n = 0; const Bytes b = corpus(2, 300);
    for (uint32_t len = 0; len <= 300; len++) for (uint32_t k = 0; k <= len; k++) {
      const uint32_t a = mm_crc32_update(g_tab, 0, b.data(), k), bb = mm_crc32_update(g_tab, 0, b.data() + k, len - k);
      const uint32_t want = (uint32_t)crc32(crc32(0L, Z_NULL, 0), b.data(), len);
      if (a != (uint32_t)crc32(crc32(0L, Z_NULL, 0), b.data(), k)) fail("crc32 of " + std::to_string(k) + " bytes");
      if (mm_crc32_combine(a, bb, len - k) != want) fail("combine at " + std::to_string(k) + " of " + std::to_string(len));
      if (mm_crc32_update(g_tab, a, b.data() + k, len - k) != want) fail("crc32 continued at " + std::to_string(k));
      n++;
    }
    // 64 slices and the pairwise tree, as the kernel's lanes run it
    for (uint32_t len : {0u, 1u, 63u, 64u, 65u, 4097u, 65280u, 65535u, 65536u}) {
      const Bytes d = corpus(len & 1 ? 0 : 2, len); uint32_t c[64]; uint32_t off, l, sum = 0;
      for (uint32_t s = 0; s < 64; s++) { mm_crc32_slice(len, s, off, l); if (off != sum) fail("slices are not consecutive"); sum += l; c[s] = mm_crc32_update(g_tab, 0, d.data() + off, l); }
      if (sum != len) fail("slices do not cover the block");
      if (len == 65536) { mm_crc32_slice(len, 5, off, l); if (l != 1024 || off != 5 * 1024) fail("65536 is not 64 equal slices"); }
      uint32_t op = mm_crc32_xpow8(len / 64);
      for (uint32_t step = 1; step < 64; step <<= 1) { for (uint32_t s = 0; s < 64; s += 2 * step) c[s] = mm_crc32_combine_op(c[s], c[s + step], op); op = mm_crc32_mulmod(op, op); }
      if (c[0] != crcOf(d)) fail("64-slice tree at " + std::to_string(len));
      n++;
    }
    printf("crc checks %ld\n", n);
  }

  // the corpora: every length 0..600 and the six large ones, three kinds, seven ways to compress
  std::vector<Item> bases;     // what the mutations start from
  { long n = 0;
    for (int c = 0; c < 3; c++) for (auto& cf : kConfigs) {
      std::vector<uint32_t> lens; for (uint32_t i = 0; i <= 600; i++) lens.push_back(i); for (uint32_t b : kBigLens) lens.push_back(b);
      for (uint32_t len : lens) {
        const Bytes p = corpus(c, len); const Bytes z = zlibDeflate(p, cf.level, cf.strategy);
        const std::string name = std::string(kCorpus[c]) + "_" + cf.name + "_" + std::to_string(len);
        if (runOne(name, z.data(), (uint32_t)z.size(), len, crcOf(p)) != MMI_OK) fail(name + ": not OK");
        if (len % 97 == 5 || len == 600) bases.push_back(good(name, z, p));
        n++;
      }
    }
    printf("corpus streams %ld\n", n);
  }
  // hand-built streams and the named malformed blocks
  { long n = 0;
    for (auto& it : handBuilt()) { Bytes o; const int rc = runOne(it.name, it.comp.data(), (uint32_t)it.comp.size(), it.uLen, it.crc, &o); if (rc != MMI_OK || o != it.payload) fail(it.name + ": status " + std::to_string(rc)); Bytes z;
                                    if (!zlibInflate(it.comp.data(), (uint32_t)it.comp.size(), it.uLen, z) || z != it.payload) fail(it.name + ": zlib does not accept the hand-built stream"); bases.push_back(it); n++; }
    printf("hand-built streams %ld\n", n);
    n = 0;
    for (auto& it : malformed()) { const int rc = runOne(it.name, it.comp.data(), (uint32_t)it.comp.size(), it.uLen, it.crc); if (rc != it.expect) fail(it.name + ": status " + std::to_string(rc) + ", expected " + std::to_string(it.expect)); Bytes z;
                                    if (zlibInflate(it.comp.data(), (uint32_t)it.comp.size(), it.uLen, z) && crcOf(z) == it.crc) fail(it.name + ": zlib accepts the malformed block"); n++; }
    printf("malformed blocks %ld\n", n);
  }
  // mutations: bit flips, truncations, descriptors that lie about cLen, uLen or the CRC
  { long n = 0;
    while (n < 210000) for (auto& b : bases) {
      if (b.comp.size() > 2000) { if (rnd() % 16) continue; }         // the long ones now and then
      Bytes c = b.comp; uint32_t uLen = b.uLen, crc = b.crc;
      const uint32_t kind = rnd() % 8;
      if (kind <= 2 && !c.empty()) { const uint32_t flips = 1 + (kind == 2 ? rnd() % 4 : 0); for (uint32_t i = 0; i < flips; i++) { const uint32_t bit = rnd() % (uint32_t)(c.size() * 8); c[bit >> 3] ^= (uint8_t)(1u << (bit & 7)); } }
      else if (kind == 3 && !c.empty()) c.resize(rnd() % c.size());                                   // truncated, cLen says so
      else if (kind == 4) { const uint32_t extra = 1 + rnd() % 8; for (uint32_t i = 0; i < extra; i++) c.push_back((uint8_t)rnd()); }   // cLen reaches into what follows
      else if (kind == 5) uLen = rnd() % 3 ? uLen + 1 + rnd() % 3 : (uLen ? uLen - 1 - rnd() % std::min(uLen, 3u) : 1);
      else if (kind == 6) crc ^= 1u << (rnd() % 32);
      else if (!c.empty()) c[rnd() % c.size()] = (uint8_t)rnd();
      runOne(b.name + " mutated", c.data(), (uint32_t)c.size(), uLen, crc);
      n++;
    }
    printf("mutated streams %ld\n", n);
  }
  printf("runs %ld accepted by zlib %ld accepted here only %ld over the step bound %ld\n", g_runs, g_accepted, g_onlyOurs, g_overBound);
  printf("status counts ok %ld bad_stream %ld truncated %ld overrun %ld short %ld bad_distance %ld bad_crc %ld\n", g_status[0], g_status[1], g_status[2], g_status[3], g_status[4], g_status[5], g_status[6]);
  printf("differences %ld\n", g_diff);
  return g_diff ? 1 : 0;
}
