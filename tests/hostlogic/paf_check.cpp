// tests/hostlogic/paf_check.cpp -- mashmap_amd/csrc/mm_paf_core.h (what k_paf_measure and k_paf_write run per row) compiled for the host,
// beside the host's own code: mm_paf_g6 against std::to_chars(general, 6); the mapQ table of MapPost::mapqTable against
// MapPost::fakeMapQOf (which also shows that the table's bisection was legitimate); mm_paf_report_row + mm_paf_numeric + the two names
// against MapPost::finishRows + appendReadMappings on generated reads, byte for byte, in every output mode.  Stand-alone, built by
// tests/test_paf_core.py under -fsanitize=address,undefined.  k 16, segLength 1000, sketch 80, three contigs.
//
// Prints one line per check (the figures test_paf_core.py asserts); exit status 1 with the first differences on stderr when anything differs.
#include <charconv>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../mashmap_amd/host/skch_map_post.hpp"
#include "../../mashmap_amd/csrc/mm_paf_core.h"

static const int K = 16, SEG = 1000, SK = 80;
static long g_bad = 0;

static bool formattable(double v) { return v == 0 || (std::isfinite(v) && std::fabs(v) >= std::ldexp(1.0, -64) && std::fabs(v) < std::ldexp(1.0, 64)); }

// one value: the header's characters against to_chars', or -1 outside the range; -> the exponent form was used
static long g_checked = 0, g_scientific = 0, g_longest = 0;
static void g6(double v) {
  char a[64], b[64];
  std::memset(a, '#', sizeof a);
  const int n = mm_paf_g6(v, a);
  g_checked++;
  if (!formattable(v)) {
    if (n != MM_PAF_NOT_FORMATTABLE && g_bad++ < 10) std::fprintf(stderr, "g6(%.17g): %d characters for a value outside the range\n", v, n);
    return;
  }
  const auto r = std::to_chars(b, b + sizeof b, v, std::chars_format::general, 6);
  const int m = (int)(r.ptr - b);
  if (n > g_longest) g_longest = n;
  if (n > 0 && std::memchr(a, 'e', (size_t)n)) g_scientific++;
  if (n != m || std::memcmp(a, b, (size_t)m) != 0 || a[n < 0 ? 0 : n] != '#') {
    if (g_bad++ < 10) std::fprintf(stderr, "g6(%.17g): '%.*s' (%d), to_chars '%.*s'\n", v, n < 0 ? 0 : n, a, n, m, b);
  }
}
static void g6_around(double v, int ulps) {
  double lo = v, hi = v;
  g6(v);
  for (int i = 0; i < ulps; i++) { lo = std::nextafter(lo, -INFINITY); hi = std::nextafter(hi, INFINITY); g6(lo); g6(hi); }
}

static std::vector<float> identity_table(int s, int k) {   // mm_stat_identity_table's expression (mm_chain.hip)
  const size_t stride = (size_t)s + 1;
  std::vector<float> t(stride * stride);
  for (size_t q = 0; q < stride; q++)
    for (size_t sh = 0; sh < stride; sh++) {
      const float mash_dist = q == 0 ? 1.0f : mmhost::Stat::j2md(1.0 * (int)sh / (int)q, k);
      t[q * stride + sh] = 1 - mash_dist;
    }
  return t;
}

static void check_g6() {
  long before = g_bad, n0 = g_checked;
  for (int s : {1, 80, 130, 2048})
    for (int k : {16, 19})
      for (float f : identity_table(s, k)) { g6((double)f); g6(100.0 * (double)f); }
  std::printf("g6 identity table values %ld bad %ld\n", g_checked - n0, g_bad - before);

  // every representable 6-digit tie D.5 * 10^(X - 5), the double below it and the one above
  before = g_bad; n0 = g_checked;
  long ties = 0;
  for (int X = -20; X <= 19; X++) {
    for (uint64_t D = 100000; D <= 999999; D++) {
      const uint64_t odd = 2 * D + 1;          // the tie is odd * 10^(X - 5) / 2
      double t;
      if (X >= 6) {
        unsigned __int128 T = (unsigned __int128)odd * 5u;
        for (int i = 0; i < X - 6; i++) T *= 10u;
        if (T >> 64) continue;
        t = (double)(uint64_t)T;
        if ((unsigned __int128)t != T) continue;
      } else {
        uint64_t p5 = 1;
        for (int i = 0; i < 5 - X; i++) p5 *= 5u;          // 5^25 < 2^64
        if (p5 > odd || odd % p5) continue;
        t = std::ldexp((double)(odd / p5), -(6 - X));
      }
      if (!formattable(t)) continue;
      ties++;
      g6_around(t, 1);
      g6(-t);
    }
  }
  std::printf("g6 representable ties %ld values %ld bad %ld\n", ties, g_checked - n0, g_bad - before);

  before = g_bad; n0 = g_checked;
  for (int n = -19; n <= 19; n++) {
    double p = 1;
    for (int i = 0; i < (n < 0 ? -n : n); i++) p *= 10.0;  // exact up to 10^22
    g6_around(n < 0 ? 1.0 / p : p, 4);
    g6_around(n < 0 ? -1.0 / p : -p, 4);
  }
  g6_around(999999.5, 4); g6_around(0.000099999951, 4); g6_around(99999.95, 4); g6_around(0.00001, 4); g6_around(0.0001, 4);
  std::printf("g6 powers of ten values %ld bad %ld\n", g_checked - n0, g_bad - before);

  before = g_bad; n0 = g_checked;
  for (int p = -64; p < 64; p++) { g6_around(std::ldexp(1.0, p), 1); g6_around(-std::ldexp(1.0, p), 1); }
  g6(0.0); g6(-0.0);
  std::printf("g6 powers of two and zeros values %ld bad %ld\n", g_checked - n0, g_bad - before);

  before = g_bad; n0 = g_checked;
  std::mt19937_64 rng(20241);
  for (int i = 0; i < 2000000; i++) {
    const uint64_t r = rng();
    const uint64_t bits = (r & 0x800fffffffffffffull) | ((uint64_t)(1023 - 64 + (rng() % 128)) << 52);
    double v; std::memcpy(&v, &bits, 8);
    g6(v);
  }
  std::printf("g6 random doubles values %ld bad %ld\n", g_checked - n0, g_bad - before);
  before = g_bad; n0 = g_checked;
  for (int i = 0; i < 1000000; i++) {
    const uint32_t r = (uint32_t)rng();
    const uint32_t bits = (r & 0x807fffffu) | ((uint32_t)(127 - 64 + (rng() % 128)) << 23);
    float f; std::memcpy(&f, &bits, 4);
    g6((double)f);
  }
  std::printf("g6 random floats values %ld bad %ld\n", g_checked - n0, g_bad - before);

  before = g_bad; n0 = g_checked;
  for (double v : {std::ldexp(1.0, 64), -std::ldexp(1.0, 64), std::nextafter(std::ldexp(1.0, -64), 0.0), -std::nextafter(std::ldexp(1.0, -64), 0.0), 1e300, -1e300,
                   1e-300, std::numeric_limits<double>::denorm_min(), std::numeric_limits<double>::min(), std::numeric_limits<double>::max(),
                   (double)INFINITY, -(double)INFINITY, (double)NAN, -(double)NAN, std::ldexp(1.0, -70)})
    g6(v);
  std::printf("g6 out of range values %ld bad %ld\n", g_checked - n0, g_bad - before);
  std::printf("g6 longest %ld scientific %ld\n", g_longest, g_scientific);
}

// ---- the mapQ table
static std::vector<float> g_thr;
static std::vector<char> g_txt;
static long g_mapqChecked = 0;
static void mapq(float x) {
  const mm_paf_mapq T{g_thr.data(), g_txt.data(), (int32_t)g_thr.size()};
  char a[16], b[64];
  const int n = mm_paf_mapq_text(T, x, a);
  const auto r = std::to_chars(b, b + sizeof b, skch::MapPost::fakeMapQOf(x), std::chars_format::general, 6);
  const int m = (int)(r.ptr - b);
  g_mapqChecked++;
  if (n != m || std::memcmp(a, b, (size_t)m) != 0) {
    if (g_bad++ < 10) std::fprintf(stderr, "mapq(%.9g): table '%.*s', host '%.*s'\n", x, n < 0 ? 0 : n, a, m, b);
  }
}
static void check_mapq() {
  skch::MapPost::mapqTable(g_thr, g_txt);
  long before = g_bad;
  bool ascending = g_thr.size() >= 2 && g_thr[0] == 0.0f && g_thr.back() == 1.0f && g_thr.size() <= MM_PAF_MAX_MAPQ && g_txt.size() == g_thr.size() * MM_PAF_MAPQ_TEXT;
  for (size_t i = 1; i < g_thr.size(); i++) ascending = ascending && g_thr[i - 1] < g_thr[i];
  for (size_t i = 0; i < g_thr.size(); i++) ascending = ascending && g_txt[i * MM_PAF_MAPQ_TEXT + MM_PAF_MAPQ_TEXT - 1] == 0;
  if (!ascending) { g_bad++; std::fprintf(stderr, "mapq table: not ascending from 0 to 1, or too long\n"); }
  std::printf("mapq table entries %zu first '%s' second '%s' last '%s' last_below_one '%s'\n", g_thr.size(), g_txt.data(), g_txt.data() + MM_PAF_MAPQ_TEXT,
              g_txt.data() + (g_thr.size() - 1) * MM_PAF_MAPQ_TEXT, g_txt.data() + (g_thr.size() - 2) * MM_PAF_MAPQ_TEXT);
  for (float t : g_thr) {
    float lo = t, hi = t;
    mapq(t);
    for (int i = 0; i < 64; i++) {
      lo = std::nextafter(lo, -1.0f); hi = std::nextafter(hi, 2.0f);
      if (lo >= 0.0f) mapq(lo);
      if (hi <= 1.0f) mapq(hi);
    }
  }
  std::printf("mapq around thresholds values %ld bad %ld\n", g_mapqChecked, g_bad - before);
  before = g_bad; long n0 = g_mapqChecked;
  for (int s : {1, 80, 130, 2048})
    for (int k : {16, 19})
      for (float f : identity_table(s, k)) if (f >= 0.0f && f <= 1.0f) mapq(f);
  std::printf("mapq identity table values %ld bad %ld\n", g_mapqChecked - n0, g_bad - before);
  before = g_bad; n0 = g_mapqChecked;
  std::mt19937_64 rng(20242);
  uint32_t one; { const float f = 1.0f; std::memcpy(&one, &f, 4); }
  for (int i = 0; i < 500000; i++) {            // half by bit pattern (every binade alike), half uniform (mostly near 1, where the values change)
    const uint32_t bits = (uint32_t)(rng() % ((uint64_t)one + 1));
    float f; std::memcpy(&f, &bits, 4);
    mapq(f);
    mapq((float)((double)(rng() >> 11) / 9007199254740992.0));
  }
  mapq(0.0f); mapq(-0.0f); mapq(1.0f);
  std::printf("mapq random values %ld bad %ld\n", g_mapqChecked - n0, g_bad - before);
  const mm_paf_mapq T{g_thr.data(), g_txt.data(), (int32_t)g_thr.size()};
  char a[16];
  const int outside = (mm_paf_mapq_text(T, std::nextafter(1.0f, 2.0f), a) == -1) + (mm_paf_mapq_text(T, -std::numeric_limits<float>::denorm_min(), a) == -1) +
                      (mm_paf_mapq_text(T, NAN, a) == -1) + (mm_paf_mapq_text(T, INFINITY, a) == -1);
  std::printf("mapq outside refused %d of 4\n", outside);
  if (outside != 4) g_bad++;
}

// ---- rows
struct Mode { const char* name; bool legacy, ani, merge, lengthFilter; };
static const Mode MODES[] = {{"default", false, false, true, false}, {"legacy", true, false, true, false}, {"ani_percentage", false, true, true, false},
                             {"merge_off", false, false, false, false}, {"length_filter", false, false, true, true}, {"legacy_length_filter", true, false, true, true}};

struct Setup {
  skch::Parameters p;
  std::vector<skch::ContigInfo> meta;
  std::vector<int> grp;
  mutable std::unique_ptr<skch::MapPost> made;          // one per setup: its cache of identity bounds is filled once
  const skch::MapPost& post() const { if (!made) made.reset(new skch::MapPost(p, meta, grp)); return *made; }
  Setup(const Setup&) = delete;
  explicit Setup(const Mode& m) {
    p.kmerSize = K; p.segLength = SEG; p.block_length = SEG; p.chain_gap = SEG; p.sketchSize = SK; p.percentageIdentity = 0.85f;
    p.filterMode = skch::filter::MAP; p.legacy_output = m.legacy; p.report_ANI_percentage = m.ani; p.mergeMappings = m.merge; p.filterLengthMismatches = m.lengthFilter;
    meta = {skch::ContigInfo{"chr1", 60000}, skch::ContigInfo{std::string(300, 'N') + "_a_long_contig_name", 40000}, skch::ContigInfo{"", 1}};
    grp = {0, 0, 0};
  }
};

struct Tally {
  long reads = 0, rows = 0, lines = 0, dropped = 0, readsEmptied = 0, handed = 0, longestNumeric = 0, zeroLenKept = 0, zeroLenDropped = 0;
  long clamp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

static mm_chain_row row(int qid, int qlen, int qs, int qe, int ref, int rs, int re, int strand, int cons, int sk, float ident, double kc) {
  mm_chain_row r{};
  r.querySeqId = qid; r.queryLen = qlen; r.queryStartPos = qs; r.queryEndPos = qe; r.refSeqId = ref; r.refStartPos = rs; r.refEndPos = re; r.strand = strand;
  r.conservedSketches = cons; r.sketchSize = sk; r.blockLength = std::max(re - rs, qe - qs); r.approxMatches = 0; r.n_merged = 1; r.nucIdentity = ident; r.kmerComplexity = kc;
  return r;
}

// one read both ways; -> the header's text ("" with *handed when a row is not formattable).  The host's text is compared inside.
static std::string both(const Setup& S, const std::vector<mm_chain_row>& rows, int len, const std::string& qname, Tally& T, bool* handedOut = nullptr, const char* what = "generated") {
  const skch::MapPost& post = S.post();
  skch::MappingResultsVector_t host;
  post.finishRows(rows.data(), rows.data() + rows.size(), len, host);
  std::string want, got;
  post.appendReadMappings(host, qname, want);
  const mm_paf_params P = post.pafParams();
  const mm_paf_mapq M{g_thr.data(), g_txt.data(), (int32_t)g_thr.size()};
  bool handed = false;
  long kept = 0;
  for (const mm_chain_row& in : rows) {
    mm_chain_row r = in;
    const int32_t clen = (int32_t)S.meta[(size_t)r.refSeqId].len;
    if (S.p.filterLengthMismatches && r.queryEndPos == r.queryStartPos) {
      mm_chain_row t = r;
      if (mm_paf_report_row(P, t, clen, len)) T.zeroLenKept++; else T.zeroLenDropped++;
    }
    if (!mm_paf_report_row(P, r, clen, len)) { T.dropped++; continue; }
    T.clamp[0] += in.refStartPos < 0; T.clamp[1] += in.refStartPos >= clen; T.clamp[2] += in.refEndPos < r.refStartPos; T.clamp[3] += std::max(in.refEndPos, r.refStartPos) >= clen;
    T.clamp[4] += in.queryStartPos < 0; T.clamp[5] += in.queryStartPos >= len; T.clamp[6] += in.queryEndPos < r.queryStartPos; T.clamp[7] += std::max(in.queryEndPos, r.queryStartPos) >= len;
    char buf[MM_PAF_NUMERIC_MAX + 8];
    std::memset(buf, '#', sizeof buf);
    int beforeRef = 0;
    const int n = mm_paf_numeric(P, r, clen, M, buf, &beforeRef);
    if (n < 0) { handed = true; continue; }
    if (n > MM_PAF_NUMERIC_MAX || buf[MM_PAF_NUMERIC_MAX] != '#') { if (g_bad++ < 10) std::fprintf(stderr, "%s: numeric part of %d characters\n", what, n); }
    if (n > T.longestNumeric) T.longestNumeric = n;
    got += qname; got.append(buf, (size_t)beforeRef); got += S.meta[(size_t)r.refSeqId].name; got.append(buf + beforeRef, (size_t)(n - beforeRef));
    kept++;
  }
  T.reads++; T.rows += (long)rows.size();
  if (handedOut) *handedOut = handed;
  if (handed) { T.handed++; return std::string(); }
  T.lines += kept;
  if (kept == 0 && !rows.empty()) T.readsEmptied++;
  if (got != want || kept != (long)host.size()) {
    if (g_bad++ < 10) std::fprintf(stderr, "%s: %zu rows, len %d:\n header '%s'\n host   '%s'\n", what, rows.size(), len, got.c_str(), want.c_str());
  }
  return got;
}

static void named_scenarios() {
  Tally T;
  {  // the length filter on both sides of its threshold: pi 0.85, min(0.7, 0.85^3) = 0.614125; q_l 1000, r_l 1000 + delta: 1 - delta / 1000
    Setup S(MODES[4]);
    const std::string a = both(S, {row(3, 5000, 0, 1000, 0, 2000, 2999 + 385, 1, 70, SK, 0.93f, 0.5)}, 5000, "read", T, nullptr, "filter_above");
    const std::string b = both(S, {row(3, 5000, 0, 1000, 0, 2000, 2999 + 386, 1, 70, SK, 0.93f, 0.5)}, 5000, "read", T, nullptr, "filter_below");
    const std::string c = both(S, {row(3, 5000, 1000, 1000, 0, 2000, 1999, 1, 70, SK, 0.93f, 0.5)}, 5000, "read", T, nullptr, "q_l_0_delta_0");   // 0 / 0: NaN keeps the row
    const std::string d = both(S, {row(3, 5000, 1000, 1000, 0, 2000, 2000, 1, 70, SK, 0.93f, 0.5)}, 5000, "read", T, nullptr, "q_l_0_delta_1");   // 1 / 0: -inf drops it
    std::printf("scenario length_filter delta_385_lines %d delta_386_lines %d zero_length_delta_0_lines %d zero_length_delta_1_lines %d\n",
                (int)std::count(a.begin(), a.end(), '\n'), (int)std::count(b.begin(), b.end(), '\n'), (int)std::count(c.begin(), c.end(), '\n'), (int)std::count(d.begin(), d.end(), '\n'));
  }
  {  // every clamp of the boundary check on both axes, in one read (contig 0 is 60000 long, the read 5000)
    Setup S(MODES[0]);
    const std::string t = both(S, {row(3, 5000, -5, 900, 0, -7, 800, 1, 70, SK, 0.9f, 0.5), row(3, 5000, 5000, 5100, 0, 60000, 60100, -1, 71, SK, 0.9f, 0.5),
                                   row(3, 5000, 300, 200, 0, 500, 400, 1, 72, SK, 0.9f, 0.5), row(3, 5000, 4000, 5000, 0, 59000, 60000, 1, 73, SK, 0.9f, 0.5)},
                               5000, "read", T, nullptr, "clamps");
    std::printf("scenario clamps text %s", t.c_str());
  }
  {  // identity exactly 0 and exactly 1, a complexity in exponent form, complexity 0
    Setup S(MODES[0]);
    const std::string t = both(S, {row(3, 5000, 0, 1000, 0, 0, 1000, 1, 0, SK, 0.0f, 1e-7), row(3, 5000, 1000, 2000, 0, 1000, 2000, 1, SK, SK, 1.0f, 0.0)}, 5000, "read", T, nullptr, "identity_0_and_1");
    std::printf("scenario identity_0_and_1 text %s", t.c_str());
  }
  {  // a row that is not formattable: complexity 2^-70
    Setup S(MODES[0]);
    bool handed = false, fine = true;
    both(S, {row(3, 5000, 0, 1000, 0, 0, 1000, 1, 70, SK, 0.9f, 0.5), row(3, 5000, 1000, 2000, 0, 1000, 2000, 1, 70, SK, 0.9f, std::ldexp(1.0, -70)),
             row(3, 5000, 2000, 3000, 0, 2000, 3000, 1, 70, SK, 0.9f, 0.5)}, 5000, "read", T, &handed, "not_formattable");
    both(S, {row(3, 5000, 0, 1000, 0, 0, 1000, 1, 70, SK, 0.9f, 0.0)}, 5000, "read", T, &fine, "complexity_0");
    std::printf("scenario not_formattable handed %d complexity_0_handed %d\n", handed ? 1 : 0, fine ? 1 : 0);
  }
  {  // the longest numeric part: every integer at its longest, a mapQ text of 7 characters, floats of 11 and 12 characters
    const float thr[1] = {0.0f};
    const char txt[MM_PAF_MAPQ_TEXT] = {'1', '2', '3', '4', '5', '6', '7', 0};
    const mm_paf_mapq M{thr, txt, 1};
    mm_paf_params P{};
    P.merge = 0; P.sparsityThreshold = ~0ull;
    const int32_t lo = std::numeric_limits<int32_t>::min();
    mm_chain_row r = row(lo, lo, lo, lo, 0, lo, lo, 1, lo, 1, 1.23457e-5f, -1.23457e-5);
    r.blockLength = lo;
    char buf[MM_PAF_NUMERIC_MAX + 8];
    std::memset(buf, '#', sizeof buf);
    int beforeRef = 0;
    const int n = mm_paf_numeric(P, r, lo, M, buf, &beforeRef);
    std::printf("scenario longest_numeric length %d of %d before_ref %d of %d untouched_behind %d\n", n, MM_PAF_NUMERIC_MAX, beforeRef, MM_PAF_BEFORE_REF_MAX, buf[MM_PAF_NUMERIC_MAX] == '#' ? 1 : 0);
    P.legacy = 1;
    const int nl = mm_paf_numeric(P, r, lo, M, buf, &beforeRef);
    std::printf("scenario longest_numeric_legacy length %d of %d\n", nl, MM_PAF_BEFORE_REF_MAX + MM_PAF_AFTER_REF_LEGACY_MAX);
  }
}

static void generated(int nReads) {
  std::mt19937_64 rng(20243);
  auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
  const size_t nModes = sizeof MODES / sizeof MODES[0];
  std::vector<Tally> tallies(nModes);
  std::vector<std::unique_ptr<Setup>> setups;
  for (const Mode& m : MODES) setups.emplace_back(new Setup(m));
  for (int i = 0; i < nReads; i++) {
    const size_t mode = (size_t)i % nModes;
    const Setup& S = *setups[mode];
    const int len = uni(0, 9) == 0 ? uni(16, 999) : uni(1000, 20000);
    const int nRows = i % 97 == 0 ? 16 : uni(1, uni(1, 16));
    std::vector<mm_chain_row> rows;
    const int flavour = uni(0, 9);                                   // 0: every row of the read fails the length filter
    for (int j = 0; j < nRows; j++) {
      const int ref = uni(0, 9) == 0 ? 2 : uni(0, 1);
      const int clen = (int)S.meta[(size_t)ref].len;
      int qs = uni(0, len), qe = qs + uni(0, 3000), rs = uni(0, clen), re = rs + (qe - qs) + uni(-40, 40);
      switch (uni(0, 24)) {                                           // the clamps, one at a time and together
        case 0: qs = -uni(1, 50); break;
        case 1: qs = len + uni(0, 50); qe = qs + uni(0, 10); break;
        case 2: qe = qs - uni(1, 50); break;
        case 3: qe = len + uni(0, 50); break;
        case 4: rs = -uni(1, 50); break;
        case 5: rs = clen + uni(0, 50); re = rs + uni(0, 10); break;
        case 6: re = rs - uni(1, 50); break;
        case 7: re = clen + uni(0, 50); break;
        case 8: qe = qs; re = rs - 1; break;                          // q_l == 0, delta == 0
        case 9: qe = qs; re = rs + uni(0, 5); break;                  // q_l == 0, delta > 0
        case 10: re = rs + (qe - qs) * 2; break;                      // the length filter drops it
        case 11: re = rs - 1 + (int)((qe - qs) * 1.385); break;       // ... near its threshold
        case 12: re = rs - 1 + (int)((qe - qs) * 1.386) + 1; break;
        default: break;
      }
      if (flavour == 0) re = rs + (qe - qs) * 3 + 10;
      const int sk = uni(1, SK), cons = uni(0, sk);
      float ident;
      switch (uni(0, 9)) {
        case 0: ident = 0.0f; break;
        case 1: ident = 1.0f; break;
        case 2: ident = (float)((double)(rng() >> 11) / 9007199254740992.0); break;
        default: ident = 1 - mmhost::Stat::j2md(1.0 * cons / sk, K); break;
      }
      double kc;
      switch (uni(0, 19)) {
        case 0: kc = 0.0; break;
        case 1: kc = 1e-7 * (1 + uni(0, 1000)); break;
        case 2: kc = uni(0, 200) == 0 ? std::ldexp(1.0, -70) : 123456.5 + uni(0, 9000000); break;
        case 3: kc = (double)(float)((double)(rng() >> 11) / 9007199254740992.0 * 1000.0); break;
        default: kc = (double)(rng() >> 11) / 9007199254740992.0 * 4.0; break;
      }
      rows.push_back(row(i, len, qs, qe, ref, rs, re, uni(0, 1) ? 1 : -1, cons, sk, ident, kc));
      rows.back().blockLength = uni(0, 30000);
    }
    const std::string qname = i % 11 == 0 ? std::string() : "read" + std::to_string(i) + std::string((size_t)(i % 7 == 0 ? 70 : 0), 'x');
    both(S, rows, len, qname, tallies[mode]);
  }
  for (size_t m = 0; m < nModes; m++) {
    const Tally& T = tallies[m];
    long everyClamp = 1;
    for (int c = 0; c < 8; c++) everyClamp = everyClamp && T.clamp[c] > 0;
    std::printf("generated mode %s reads %ld rows %ld lines %ld dropped %ld reads_emptied %ld handed %ld every_clamp %ld zero_length_kept %ld zero_length_dropped %ld longest_numeric %ld\n",
                MODES[m].name, T.reads, T.rows, T.lines, T.dropped, T.readsEmptied, T.handed, everyClamp, T.zeroLenKept, T.zeroLenDropped, T.longestNumeric);
  }
}

int main(int argc, char** argv) {
  const int nReads = argc > 1 ? std::atoi(argv[1]) : 20000;
  check_g6();
  check_mapq();
  named_scenarios();
  generated(nReads);
  std::printf("differences %ld\n", g_bad);
  return g_bad ? 1 : 0;
}
