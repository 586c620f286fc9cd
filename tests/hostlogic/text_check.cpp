// tests/hostlogic/text_check.cpp -- mashmap_amd/csrc/mm_text_core.h (the record rules the kernels of mm_text.hip run: summarise ->
// scan -> resolve over tiles) against the serial functions of mashmap_amd/host/seq_parse.hpp (detail::record_name, detail::record_lines,
// driven the way parseWindow drives them with one thread).  A stand-alone program: tests/test_text_core.py builds it with
// -fsanitize=address,undefined and plain.  Compared for TILE 1, 7, 64 and 4096, FASTA and FASTQ, final 0 and 1: the record count, every
// hdrOff, name, length, hasN flag, the packed words (mmhost::pack2bit) and `consumed`.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../mashmap_amd/csrc/mm_text_core.h"
#include "../../mashmap_amd/host/pack2bit.hpp"
#include "../../mashmap_amd/host/seq_parse.hpp"

static long g_diff = 0, g_runs = 0, g_texts = 0, g_records = 0, g_assoc = 0, g_plain = 0;
static void fail(const char* what, const std::string& text, int fmt, int fin, unsigned tile) {
  if (g_diff++ < 20) {
    std::string shown;
    for (unsigned char ch : text.substr(0, 200)) { char t[8]; if (ch >= 32 && ch < 127) shown += (char)ch; else { snprintf(t, sizeof t, "\\x%02x", ch); shown += t; } }
    printf("DIFF %s fmt %d final %d tile %u text[%zu] \"%s\"\n", what, fmt, fin, tile, text.size(), shown.c_str());
  }
}

struct Rec { uint64_t hdrOff; std::string name, seq; };

// the specification: one thread of parseWindow
static std::vector<Rec> serial(const char* b, size_t n, bool fasta) {
  std::vector<Rec> out;
  const char* q = b; const char* e = b + n;
  while (q < e) {
    const char* body = mmhost::detail::next_line(q, e);
    const char* nb; const char* ne;
    mmhost::detail::record_name(q, body, nb, ne);
    Rec r; r.hdrOff = (uint64_t)(q - b); r.name.assign(nb, ne);
    q = mmhost::detail::record_lines(body, e, fasta, [&](const char* l, size_t m) { r.seq.append(l, m); });
    out.push_back(std::move(r));
  }
  return out;
}

struct Expect { std::vector<Rec> recs; uint64_t consumed; };
static Expect expect(const std::string& t, bool fasta, int fin) {
  Expect x;
  if (fin) { x.recs = serial(t.data(), t.size(), fasta); x.consumed = t.size(); return x; }
  if (fasta) {
    std::vector<Rec> all = serial(t.data(), t.size(), true);
    x.consumed = all.empty() ? 0 : all.back().hdrOff;
  } else {
    size_t nl = 0; for (char ch : t) nl += ch == '\n';
    size_t want = nl / 4 * 4, seen = 0; x.consumed = 0;
    for (size_t i = 0; i < t.size() && seen < want; i++) if (t[i] == '\n' && ++seen == want) x.consumed = i + 1;
  }
  x.recs = serial(t.data(), (size_t)x.consumed, fasta);
  return x;
}

struct Builder {                   // the visitor: what k_text_records and k_text_pack do with a resolved tile
  uint64_t base = 0, nBytes = 0;   // the tile's offset
  std::vector<uint64_t> hdrOff; std::vector<uint32_t> seqStart; std::vector<std::string> seq;
  bool bad = false;
  void need(uint32_t r) { if (hdrOff.size() <= r) { hdrOff.resize(r + 1, ~0ull); seqStart.resize(r + 1, 0); seq.resize(r + 1); } }
  void header(uint32_t ordinal, uint32_t i, uint32_t s) { if (base + i >= nBytes) return; need(ordinal); hdrOff[ordinal] = base + i; seqStart[ordinal] = s; }
  void byte(uint32_t, uint8_t b, uint32_t cls, const MmTextCarry& c) {
    if (cls != MMT_BASE) return;
    if (!c.rec) { bad = true; return; }
    need(c.rec - 1);
    if (c.seq - seqStart[c.rec - 1] != seq[c.rec - 1].size()) bad = true;      // the base's index inside its record
    seq[c.rec - 1] += (char)b;
  }
};

static void check(const std::string& t, int fmt, int fin, unsigned TILE) {
  g_runs++;
  const uint8_t* p = (const uint8_t*)t.data(); const uint64_t n = t.size();
  const size_t nTiles = (size_t)((n + TILE - 1) / TILE);
  std::vector<MmTextSum> sum(nTiles);
  for (size_t k = 0; k < nTiles; k++) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(TILE, n - k * TILE);
    sum[k] = mm_text_summarise(fmt, p + k * TILE, m);
    // a tile without '\n' (FASTA: and without '>'): the summary the kernel writes without the walk
    if (!memchr(p + k * TILE, '\n', m) && !(fmt == MMT_FASTA && memchr(p + k * TILE, '>', m))) {
      const MmTextSum plain = mm_text_summarise_plain(fmt, m);
      g_plain++;
      if (memcmp(&plain, &sum[k], sizeof plain)) { fail("plain summary", t, fmt, fin, TILE); return; }
    }
  }
  // the scan: the carries by apply() tile after tile, and by a tree of combines (pairs, then pairs of pairs) -- any order agrees
  std::vector<MmTextCarry> carry(nTiles + 1);
  carry[0] = mm_text_carry0(fmt);
  for (size_t k = 0; k < nTiles; k++) carry[k + 1] = mm_text_apply(carry[k], sum[k]);
  {
    std::vector<MmTextSum> lvl = sum;
    while (lvl.size() > 1) {
      std::vector<MmTextSum> up;
      for (size_t k = 0; k < lvl.size(); k += 2) up.push_back(k + 1 < lvl.size() ? mm_text_combine(lvl[k], lvl[k + 1]) : lvl[k]);
      lvl.swap(up);
    }
    const MmTextCarry viaTree = mm_text_apply(carry[0], lvl.empty() ? mm_text_identity() : lvl[0]);
    g_assoc++;
    if (memcmp(&viaTree, &carry[nTiles], sizeof viaTree)) fail("tree of combines", t, fmt, fin, TILE);
  }
  Builder B; B.nBytes = n;
  if (n) B.header(0, 0, 0);
  for (size_t k = 0; k < nTiles; k++) {
    B.base = k * TILE;
    const MmTextCarry end = mm_text_resolve(fmt, p + k * TILE, (uint32_t)std::min<uint64_t>(TILE, n - k * TILE), carry[k], B);
    if (memcmp(&end, &carry[k + 1], sizeof end)) { fail("resolve's carry against the summary's", t, fmt, fin, TILE); return; }
  }
  if (B.bad) { fail("base index inside the record", t, fmt, fin, TILE); return; }
  { size_t seen = 0; for (uint64_t h : B.hdrOff) seen += h != ~0ull;
    if (seen != mm_text_headers(fmt, n, n ? p[n - 1] : 0, carry[nTiles])) { fail("header lines inside the buffer", t, fmt, fin, TILE); return; } }
  uint32_t consumedNl; int lastHdr;
  const uint32_t nRec = mm_text_complete(fmt, fin, n, n ? p[n - 1] : 0, carry[nTiles], &consumedNl, &lastHdr);
  uint64_t consumed = fin ? n : 0;
  if (!fin && lastHdr) { if (nRec >= B.hdrOff.size()) { fail("table holds the last header", t, fmt, fin, TILE); return; } consumed = B.hdrOff[nRec]; }
  if (!fin && consumedNl) { uint32_t seen = 0; for (uint64_t i = 0; i < n; i++) if (p[i] == '\n' && ++seen == consumedNl) { consumed = i + 1; break; } }
  const Expect x = expect(t, fmt == MMT_FASTA, fin);
  if (consumed != x.consumed) { fail("consumed", t, fmt, fin, TILE); return; }
  if (nRec != x.recs.size()) { fail("record count", t, fmt, fin, TILE); return; }
  B.need(nRec);
  for (uint32_t r = 0; r < nRec; r++) {
    g_records++;
    const Rec& w = x.recs[r];
    if (B.hdrOff[r] != w.hdrOff) { fail("hdrOff", t, fmt, fin, TILE); return; }
    const uint32_t nameLen = mm_text_name_len(p, n, B.hdrOff[r]);
    if (std::string((const char*)p + B.hdrOff[r] + (nameLen ? 1 : 0), nameLen) != w.name) { fail("name", t, fmt, fin, TILE); return; }
    if (B.seq[r] != w.seq) { fail("sequence bytes", t, fmt, fin, TILE); return; }
    // packed words and the hasN flag, base by base with mm_text_code, against mmhost::pack2bit
    const size_t L = w.seq.size(), W = (L + 31) / 32;
    std::vector<uint32_t> b2(2 * W + 2, 0), nm(W + 1, 0), wb2(2 * W + 2, 0), wnm(W + 1, 0);
    uint32_t anyN = 0;
    for (size_t i = 0; i < L; i++) { uint32_t isN; const uint32_t code = mm_text_code((uint8_t)B.seq[r][i], isN); b2[i / 16] |= code << (i % 16 * 2); nm[i / 32] |= isN << (i % 32); anyN |= isN; }
    const size_t nN = mmhost::pack2bit(w.seq.data(), L, wb2.data(), wnm.data());
    if (b2 != wb2 || nm != wnm || (anyN != 0) != (nN != 0)) { fail("packed words", t, fmt, fin, TILE); return; }
  }
}

static void check_all(const std::string& t) {
  g_texts++;
  static const unsigned tiles[] = {1, 7, 64, 4096};
  for (int fmt = 0; fmt < 2; fmt++) for (int fin = 0; fin < 2; fin++) for (unsigned T : tiles) check(t, fmt, fin, T);
}

static std::mt19937_64 rng(20240607);
static std::string bases(size_t n, const char* alpha = "ACGT") { std::string s(n, 'A'); const size_t k = strlen(alpha); for (auto& ch : s) ch = alpha[rng() % k]; return s; }

// the edge texts at tile size T (the list tests/test_gpu_text.py runs at MM_TEXT_TILE), FASTA and FASTQ forms
static std::vector<std::string> edge_texts(size_t T) {
  std::vector<std::string> v;
  auto fa = [](const std::string& name, const std::string& seq, size_t width = 0) {
    std::string s = ">" + name + "\n";
    if (!width) return s + seq + "\n";
    for (size_t i = 0; i < seq.size(); i += width) s += seq.substr(i, width) + "\n";
    return s;
  };
  auto fq = [](const std::string& name, const std::string& seq, const std::string& qual) { return "@" + name + "\n" + seq + "\n+\n" + qual + "\n"; };
  for (int d = -1; d <= 1; d++) {
    { std::string s = fa("a", bases(T - 4 + d)); v.push_back(s + fa("b", bases(9))); }                      // '\n' last in a tile, '>' first in the next
    { std::string s = fa("a", bases(T - 5 + d)); v.push_back(s + ">" + fa("", bases(5))); v.push_back(s + ">"); }   // '>' as the last byte of a tile
    v.push_back(fa("r1", bases(T - 20 + d)) + fa("name_that_crosses_the_tile_boundary", bases(40)));
    v.push_back(fa(std::string(T + 10 + d, 'h') + " " + std::string(T + 9, 'k'), bases(33)) + fa("z", bases(3)));
    v.push_back(fa(std::string(2 * T + 9 + d, 'h'), bases(33)) + fa("z", bases(3)));
    v.push_back(">long\n" + bases(3 * T + 5 + d));
    v.push_back(fa("x", bases(3 * T + 5 + d)) + fa("y", bases(2)));
    v.push_back(fq("q1", bases(3 * T + 5 + d), std::string(3 * T + 5 + d, 'I')) + fq("q2", bases(5), "IIIII"));
    v.push_back(fa("w", bases(16 * T + d), 60) + fa("v", bases(7)));
    v.push_back(fq("w", bases(16 * T + d), bases(16 * T + d, "@+>I")));
  }
  { std::string s; for (int i = 0; i < 40; i++) s += fa("r" + std::to_string(i), bases(i % 4)); v.push_back(s); }
  { std::string s; for (int i = 0; i < 40; i++) s += fq("r" + std::to_string(i), bases(i % 4), std::string(i % 4, 'I')); v.push_back(s); }
  v.push_back(">a\n>b\n>c\nAC\n>d\n");
  v.push_back(">a\n\nAC\n\n\nGT\n\n>b\n\n");
  v.push_back(">a x\r\nACGT\r\nAC\r\n>b\r\n");
  v.push_back("@a x\r\nACGT\r\n+\r\nIIII\r\n");
  v.push_back(">a>b @c\nAC>GT@A\n>b\nA");
  v.push_back("@a>b @c\nAC>GT@A\n+\n@@@@@@@\n");
  v.push_back(">iupac\nacgtnRYKMSWBDHVNacgu\n");
  for (size_t L : {31, 32, 33, 63, 64, 65}) { v.push_back(fa("l", bases(L, "ACGTNacgt")) + fa("m", bases(L), 7)); v.push_back(fq("l", bases(L, "ACGTNacgt"), std::string(L, '5'))); }
  v.push_back(">nolf\nACGT");
  v.push_back("@q\nACGT\n+\n@III\n@r\nAC\n+\n+I\n@s\nGG\n+\n>I\n");
  v.push_back("@q\nACGT\n+\nIIII\n@r"); v.push_back("@q\nACGT\n+\nIIII\n@r\nAC"); v.push_back("@q\nACGT\n+\nIIII\n@r\nAC\n+"); v.push_back("@q\nACGT\n+\nIIII\n@r\nAC\n+\n");
  v.push_back(""); v.push_back("\n"); v.push_back(">"); v.push_back("ACGT\nAC\n>x\tY z\nGG\n"); v.push_back("\n\n\n\n\n"); v.push_back("> \n \n");
  return v;
}

// --parse FILE fasta|fastq FINAL: what the specification gives for the file's bytes, one record per line (hdrOff, name in hex, bases,
// hasN), then `consumed N` -- tests/test_text_core.py holds the Python reference of the GPU tests (tests/textzoo.py) against it
static int parse_file(const char* path, bool fasta, int fin) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  std::string t; char buf[65536]; size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) t.append(buf, k);
  fclose(f);
  const Expect x = expect(t, fasta, fin);
  for (const Rec& r : x.recs) {
    std::string hex; for (unsigned char ch : r.name) { char h[4]; snprintf(h, sizeof h, "%02x", ch); hex += h; }
    bool anyN = false; for (char ch : r.seq) { uint32_t isN; (void)mm_text_code((uint8_t)ch, isN); anyN |= isN != 0; }
    printf("%llu %s. %zu %d\n", (unsigned long long)r.hdrOff, hex.c_str(), r.seq.size(), anyN ? 1 : 0);
  }
  printf("consumed %llu\n", (unsigned long long)x.consumed);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "--parse")) return parse_file(argv[2], !strcmp(argv[3], "fasta"), atoi(argv[4]));
  for (size_t T : {64, 97}) {
    for (const std::string& t : edge_texts(T)) {
      check_all(t);
      for (int m = 0; m < 6; m++) {                       // mutated: a few bytes replaced, one cut
        std::string u = t;
        static const char alpha[] = {'>', '@', '+', '\n', '\r', ' ', 'A', 'c', 'N', 'x'};
        for (int k = 0; k < 3 && !u.empty(); k++) u[rng() % u.size()] = alpha[rng() % sizeof alpha];
        if (m & 1 && !u.empty()) u.resize(rng() % u.size());
        check_all(u);
      }
    }
  }
  { const std::string big = edge_texts(4096)[9]; check_all(big); }   // several tiles of 4096
  long randoms = 0;
  for (int i = 0; i < 6000; i++) {
    static const char alpha[] = {'>', '@', '+', '\n', '\r', ' ', 'A', 'c', 'N', 'x'};
    std::string u(rng() % 90, 'A');
    const int nlBias = (int)(rng() % 3);
    for (auto& ch : u) ch = (nlBias && rng() % 4 == 0) ? '\n' : alpha[rng() % sizeof alpha];
    check_all(u); randoms++;
  }
  // associativity on summaries of random pieces
  long assoc = 0;
  for (int i = 0; i < 20000; i++) {
    static const char alpha[] = {'>', '\n', 'A', '\n', '>', 'x'};
    std::string a(rng() % 6, 'A'), b(rng() % 6, 'A'), c(rng() % 6, 'A');
    for (std::string* s : {&a, &b, &c}) for (auto& ch : *s) ch = alpha[rng() % sizeof alpha];
    for (int fmt = 0; fmt < 2; fmt++) {
      const MmTextSum A = mm_text_summarise(fmt, (const uint8_t*)a.data(), (uint32_t)a.size()), Bs = mm_text_summarise(fmt, (const uint8_t*)b.data(), (uint32_t)b.size()),
                      C = mm_text_summarise(fmt, (const uint8_t*)c.data(), (uint32_t)c.size());
      const MmTextSum l = mm_text_combine(mm_text_combine(A, Bs), C), r = mm_text_combine(A, mm_text_combine(Bs, C));
      const std::string abc = a + b + c;
      const MmTextSum whole = mm_text_summarise(fmt, (const uint8_t*)abc.data(), (uint32_t)abc.size());
      assoc++;
      if (memcmp(&l, &r, sizeof l) || memcmp(&l, &whole, sizeof l)) fail("associativity", abc, fmt, 0, 0);
    }
  }
  printf("texts %ld\nrandom texts %ld\nruns %ld\nrecords %ld\nplain tiles %ld\nscan orders %ld\nassociativity checks %ld\ndifferences %ld\n", g_texts, randoms, g_runs, g_records, g_plain, g_assoc, assoc, g_diff);
  return g_diff ? 1 : 0;
}
