// tests/hostlogic/chain_check.cpp -- mashmap_amd/csrc/mm_chain_core.h (what k_chain_reads runs per read) compiled for the host, beside
// MapPost::chainedFromRecords (mapModuleFromRecords stopped behind filterByGroup) on generated reads of 1 to 16 records: every field of
// every row bit for bit, floats included.  kmerComplexity's integer derivation of the long double ratio is checked apart.  Stand-alone,
// built by tests/test_chain_core.py under -fsanitize=address,undefined.  k 16, segLength 1000, sketch 80, two contigs.
//
// Prints one line per named scenario ("scenario NAME rows R ...": the figures test_chain_core.py asserts the scenario really shows), one
// line for the generated reads and one per kmerComplexity check; exit status 1 with the first differences on stderr when anything differs.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../mashmap_amd/host/skch_map_post.hpp"
#include "../../mashmap_amd/csrc/mm_chain_core.h"

static const int K = 16, SEG = 1000, SK = 80;
static int g_bad = 0;

struct Setup {
  skch::Parameters p;
  std::vector<skch::ContigInfo> meta;
  std::vector<int> grp;
  std::vector<float> identity;
  Setup() {
    p.kmerSize = K; p.segLength = SEG; p.block_length = SEG; p.chain_gap = SEG; p.sketchSize = SK; p.percentageIdentity = 0.85f;
    p.filterMode = skch::filter::MAP; p.split = true; p.mergeMappings = true;
    meta = {skch::ContigInfo{"c0", 60000}, skch::ContigInfo{"c1", 40000}};
    grp = {0, 0};
    identity.assign((size_t)(SK + 1) * (SK + 1), 0.0f);
    for (int q = 1; q <= SK; q++)
      for (int s = 0; s <= SK; s++) identity[(size_t)q * (SK + 1) + s] = 1 - mmhost::Stat::j2md(1.0 * s / q, K);
  }
};

static mm_mapping rec(int fragStart, int fragLen, int refId, int refStart, int cons, int strand, uint64_t maxHash = 0x9000000000000000ull, int raw = SK, int sketch = SK) {
  mm_mapping m{};
  m.querySeqId = 7; m.fragStart = fragStart; m.fragLen = fragLen; m.refSeqId = refId; m.refStartPos = refStart;
  m.conservedSketches = cons; m.sketchSize = sketch; m.strand = strand; m.rawSketchSize = raw; m.maxHash = maxHash;
  return m;
}

// runs both forms on one read; returns the rows of the header's form (the host's when they differ: reported)
static std::vector<mm_chain_row> both(const Setup& S, const std::vector<mm_mapping>& recs, int len, const char* what) {
  skch::MapPost post(S.p, S.meta, S.grp);
  skch::MappingResultsVector_t host;
  post.chainedFromRecords(recs.data(), recs.data() + recs.size(), len, host);
  mm_chain_env E;
  E.p = post.chainParams(); E.kmerSize = K; E.segLength = SEG; E.stride = SK + 1; E.identity = S.identity.data();
  std::vector<mm_chain_row> rows(recs.size() + 1);
  const int counted = mm_chain_read(E, recs.data(), (int)recs.size(), len, nullptr);
  const int n = mm_chain_read(E, recs.data(), (int)recs.size(), len, rows.data());
  rows.resize(n < 0 ? 0 : n);
  bool same = counted == n && n == (int)host.size();
  for (int i = 0; same && i < n; i++) {
    const mm_chain_row& r = rows[i]; const skch::MappingResult& h = host[i];
    uint32_t a, b; std::memcpy(&a, &r.nucIdentity, 4); std::memcpy(&b, &h.nucIdentity, 4);
    same = r.querySeqId == h.querySeqId && r.queryLen == h.queryLen && r.queryStartPos == h.queryStartPos && r.queryEndPos == h.queryEndPos &&
           r.refSeqId == h.refSeqId && r.refStartPos == h.refStartPos && r.refEndPos == h.refEndPos && r.strand == (int)h.strand &&
           r.conservedSketches == h.conservedSketches && r.sketchSize == h.sketchSize && r.blockLength == h.blockLength &&
           r.approxMatches == h.approxMatches && r.n_merged == h.n_merged && r.splitMappingId == h.splitMappingId && a == b &&
           (long double)r.kmerComplexity == h.kmerComplexity && r.pad_ == 0;
    if (!same) std::fprintf(stderr, "%s: row %d differs: q %d-%d / %d-%d ref %d:%d-%d / %d:%d-%d cons %d / %d n_merged %d / %d id %d / %d identity %.9g / %.9g kc %.17g / %.17Lg approx %d / %d\n",
                            what, i, r.queryStartPos, r.queryEndPos, (int)h.queryStartPos, (int)h.queryEndPos, r.refSeqId, r.refStartPos, r.refEndPos,
                            (int)h.refSeqId, (int)h.refStartPos, (int)h.refEndPos, r.conservedSketches, h.conservedSketches, r.n_merged, h.n_merged,
                            r.splitMappingId, (int)h.splitMappingId, r.nucIdentity, h.nucIdentity, r.kmerComplexity, h.kmerComplexity, r.approxMatches, h.approxMatches);
  }
  if (!same) {
    if (g_bad++ < 10) std::fprintf(stderr, "%s: %zu records, len %d: header %d (counted %d) rows, host %zu\n", what, recs.size(), len, n, counted, host.size());
  }
  return rows;
}

static void say(const char* name, const std::vector<mm_chain_row>& rows, const std::string& more = "") {
  std::printf("scenario %s rows %zu", name, rows.size());
  for (const auto& r : rows) std::printf(" [%d-%d %d:%d-%d %c cons %d merged %d]", r.queryStartPos, r.queryEndPos, r.refSeqId, r.refStartPos, r.refEndPos, r.strand == 1 ? '+' : '-', r.conservedSketches, r.n_merged);
  std::printf("%s\n", more.c_str());
}

static void named_scenarios() {
  Setup S;
  {  // colinear chains, both strands
    std::vector<mm_mapping> v;
    for (int i = 0; i < 5; i++) v.push_back(rec(i * SEG, SEG, 0, 10000 + i * SEG + (i % 2) * 3, 70 + i, 1));
    say("colinear_fwd", both(S, v, 5 * SEG, "colinear_fwd"));
    v.clear();
    for (int i = 0; i < 5; i++) v.push_back(rec(i * SEG, SEG, 1, 20000 - i * SEG - (i % 2) * 3, 70 + i, -1));
    say("colinear_rev", both(S, v, 5 * SEG, "colinear_rev"));
  }
  {  // a gap just below and just at chain_gap: dist = sqrt(0 + ref_dist^2) = ref_dist, the test is dist < max_dist
    std::vector<mm_mapping> v = {rec(0, SEG, 0, 5000, 75, 1), rec(SEG, SEG, 0, 5000 + SEG + (SEG - 1), 75, 1), rec(2 * SEG, SEG, 0, 5000 + 2 * SEG + (SEG - 1), 75, 1)};
    say("gap_below", both(S, v, 3 * SEG, "gap_below"));
    v[1].refStartPos += 1; v[2].refStartPos += 1;
    say("gap_at", both(S, v, 3 * SEG, "gap_at"));
  }
  {  // two chains for one read
    std::vector<mm_mapping> v;
    for (int i = 0; i < 3; i++) v.push_back(rec(i * SEG, SEG, 0, 3000 + i * SEG, 72, 1));
    for (int i = 3; i < 6; i++) v.push_back(rec(i * SEG, SEG, 1, 9000 + i * SEG, 64, 1));
    Setup N = S; N.p.filterMode = skch::filter::NONE;
    say("two_chains_filter_none", both(N, v, 6 * SEG, "two_chains_filter_none"));
    say("two_chains", both(S, v, 6 * SEG, "two_chains"));
  }
  {  // several records with equal (refSeqId, refStartPos, queryStartPos) and different conservedSketches: the representative of the chain is the
     // first of them in the (stable) order, and its conservedSketches is what the row carries
    std::vector<mm_mapping> v = {rec(0, SEG, 0, 8000, 61, 1), rec(0, SEG, 0, 8000, 77, 1), rec(0, SEG, 0, 8000, 69, 1),
                                 rec(SEG, SEG, 0, 9000, 70, 1), rec(SEG, SEG, 0, 9000, 58, 1), rec(2 * SEG, SEG, 0, 10000, 66, 1), rec(2 * SEG, SEG, 0, 10000, 80, 1)};
    say("equal_keys", both(S, v, 3 * SEG, "equal_keys"));
    std::vector<mm_mapping> w(v.rbegin(), v.rend());
    for (size_t i = 0; i + 1 < w.size(); i++) for (size_t j = i + 1; j < w.size(); j++) if (w[j].fragStart < w[i].fragStart) std::swap(w[i], w[j]);
    say("equal_keys_other_order", both(S, w, 3 * SEG, "equal_keys_other_order"));
  }
  {  // mappings equivalent under the sweep's comparator: same identity, queryStartPos and refSeqId at different reference positions
     // (two chains on one contig that start with the same fragment and have equal average identity), with secondaryToKeep 0 and 2
    std::vector<mm_mapping> v;
    for (int i = 0; i < 3; i++) { v.push_back(rec(i * SEG, SEG, 0, 4000 + i * SEG, 70, 1)); v.push_back(rec(i * SEG, SEG, 0, 30000 + i * SEG, 70, 1)); v.push_back(rec(i * SEG, SEG, 0, 50000 + i * SEG, 70, 1)); }
    say("sweep_equivalent_keep0", both(S, v, 3 * SEG, "sweep_equivalent_keep0"));
    Setup T = S; T.p.numMappingsForSegment = 3; T.p.numMappingsForShortSequence = 3;
    say("sweep_equivalent_keep2", both(T, v, 3 * SEG, "sweep_equivalent_keep2"));
    Setup N = S; N.p.filterMode = skch::filter::NONE;
    say("sweep_equivalent_filter_none", both(N, v, 3 * SEG, "sweep_equivalent_filter_none"));
  }
  {  // a lone record of a longer read: dropped by filterWeakMappings (n_merged 0 < 1)
    std::vector<mm_mapping> v = {rec(2 * SEG, SEG, 0, 7000, 75, 1)};
    say("lone_record", both(S, v, 4 * SEG, "lone_record"));
  }
  {  // a read shorter than segLength (numMappingsForShortSequence applies), and one of exactly segLength
    Setup T = S; T.p.numMappingsForShortSequence = 3;
    std::vector<mm_mapping> v = {rec(0, 600, 0, 7000, 75, 1), rec(0, 600, 1, 9000, 75, -1), rec(0, 600, 0, 100, 60, 1), rec(0, 600, 1, 15000, 62, 1)};
    say("short_read_keep0", both(S, v, 600, "short_read_keep0"));
    say("short_read_keep2", both(T, v, 600, "short_read_keep2"));
    for (auto& m : v) m.fragLen = SEG;
    say("read_of_one_segment", both(T, v, SEG, "read_of_one_segment"));
  }
  {  // minMerged 1 and 3: a chain of two
    std::vector<mm_mapping> v = {rec(0, SEG, 0, 7000, 75, 1), rec(SEG, SEG, 0, 8000, 75, 1), rec(3 * SEG, SEG, 1, 500, 75, -1)};
    say("min_merged_1", both(S, v, 5 * SEG, "min_merged_1"));
    Setup T = S; T.p.block_length = 3 * SEG;
    say("min_merged_3", both(T, v, 5 * SEG, "min_merged_3"));
    for (int i = 2; i < 5; i++) v.push_back(rec(i * SEG, SEG, 0, 7000 + i * SEG, 70, 1));
    say("min_merged_3_chain_of_5", both(T, v, 5 * SEG, "min_merged_3_chain_of_5"));
  }
  {  // merge off
    Setup T = S; T.p.mergeMappings = false;
    std::vector<mm_mapping> v;
    for (int i = 0; i < 4; i++) v.push_back(rec(i * SEG, SEG, 0, 10000 + i * SEG, 60 + 5 * i, 1));
    v.push_back(rec(SEG, SEG, 1, 300, 80, -1));
    say("merge_off", both(T, v, 4 * SEG, "merge_off"));
    T.p.filterMode = skch::filter::NONE;
    say("merge_off_filter_none", both(T, v, 4 * SEG, "merge_off_filter_none"));
  }
  {  // the complexity gate: the middle fragment's sketch reaches the top of the hash range (complexity 80 / 1 / 1970 = 0.0406 < 0.05)
    Setup T = S; T.p.kmerComplexityThreshold = 0.05f;
    std::vector<mm_mapping> v = {rec(0, SEG, 0, 7000, 75, 1), rec(SEG, SEG, 0, 8000, 75, 1, ~0ull), rec(2 * SEG, SEG, 0, 9000, 75, 1), rec(3 * SEG, SEG, 0, 10000, 75, 1, 1ull << 62)};
    say("complexity_gate", both(T, v, 4 * SEG, "complexity_gate"));
  }
  {  // numMappings 0: secondaryToKeep is (uint16_t)-1 = 65535 in MapPost::filterByGroup and in the header alike -- every mapping of the status set is kept
    Setup T = S; T.p.numMappingsForSegment = 0; T.p.numMappingsForShortSequence = 0;
    std::vector<mm_mapping> v;
    for (int i = 0; i < 3; i++) { v.push_back(rec(i * SEG, SEG, 0, 4000 + i * SEG, 76, 1)); v.push_back(rec(i * SEG, SEG, 1, 30000 + i * SEG, 70, 1)); v.push_back(rec(i * SEG, SEG, 0, 50000 + i * SEG, 64, 1)); }
    say("num_mappings_0", both(T, v, 3 * SEG, "num_mappings_0"));
    say("num_mappings_1", both(S, v, 3 * SEG, "num_mappings_1"));
  }
  {  // a chain whose members' complexities lie 2^23 apart (maxHash 2^63 and 2^40): inside the assumed range, the average is the host's
    std::vector<mm_mapping> v = {rec(0, SEG, 0, 7000, 75, 1, 1ull << 63, 77), rec(SEG, SEG, 0, 8000, 75, 1, (1ull << 40) + 12345, 61), rec(2 * SEG, SEG, 0, 9000, 75, 1, 0xF123456789ABCDEFull, 80)};
    const std::vector<mm_chain_row> rows = both(S, v, 3 * SEG, "complexities_far_apart");
    std::printf("scenario complexities_far_apart rows %zu merged %d kc %.17g\n", rows.size(), rows.empty() ? 0 : rows[0].n_merged, rows.empty() ? 0.0 : rows[0].kmerComplexity);
  }
  {  // 17 records: refused
    std::vector<mm_mapping> v;
    for (int i = 0; i < 17; i++) v.push_back(rec(i * SEG, SEG, 0, 1000 + i * SEG, 70, 1));
    Setup T = S; skch::MapPost post(T.p, T.meta, T.grp);
    mm_chain_env E; E.p = post.chainParams(); E.kmerSize = K; E.segLength = SEG; E.stride = SK + 1; E.identity = T.identity.data();
    std::vector<mm_chain_row> rows(17);
    const int a = mm_chain_read(E, v.data(), 17, 17 * SEG, rows.data()), b = mm_chain_read(E, v.data(), 16, 17 * SEG, rows.data());
    v[3].conservedSketches = SK + 1;                                  // a record outside the identity table: an error, not a hand-over
    const int c = mm_chain_read(E, v.data(), 5, 17 * SEG, rows.data());
    std::printf("scenario seventeen_records returns %d sixteen %d bad_record %d\n", a, b, c);
  }
}

// generated reads: fragments as mapModule cuts them, 0 to 3 records per fragment around a colinear placement with the jitters that
// matter -- none, a few bases, just below / at / above chain_gap --, tandem copies, both strands, two contigs, few identity values
static void generated(int nReads, uint64_t seed) {
  std::mt19937_64 rng(seed);
  auto pick = [&rng](int n) { return (int)(rng() % (uint64_t)n); };
  long reads = 0, rows = 0, merged = 0, dropped = 0, maxN = 0, histo16 = 0;
  for (int it = 0; it < nReads; it++) {
    Setup S;
    S.p.block_length = pick(3) == 0 ? 3 * SEG : SEG;
    const int keep = pick(2) ? 3 : 1; S.p.numMappingsForSegment = keep; S.p.numMappingsForShortSequence = pick(4) ? keep : 4 - keep;
    S.p.mergeMappings = pick(6) != 0;
    S.p.filterMode = pick(5) == 0 ? skch::filter::NONE : (pick(2) ? skch::filter::MAP : skch::filter::ONETOONE);
    S.p.chain_gap = pick(4) == 0 ? 2 * SEG : SEG;
    S.p.kmerComplexityThreshold = pick(4) == 0 ? 0.05f : 0.0f;
    int len = pick(8) == 0 ? 300 + pick(701) : (1 + pick(8)) * SEG + (pick(2) ? pick(SEG) : 0);
    std::vector<int> starts;
    if (len <= SEG) starts.push_back(0);
    else { for (int i = 0; i < len / SEG; i++) starts.push_back(i * SEG); if (len % SEG) starts.push_back(len - SEG); }
    const int fl = len <= SEG ? len : SEG;
    const int strand = pick(2) ? 1 : -1, refId = pick(2), base = 5000 + pick(20000), period = pick(3) ? 0 : 700 + pick(2000);
    std::vector<mm_mapping> v;
    const int want = 1 + pick(16);
    for (size_t f = 0; f < starts.size() && (int)v.size() < want; f++) {
      const int nrec = pick(8) == 0 ? 0 : 1 + pick(3);
      // maxHash over the whole range the header's note on the averages assumes: 2^40 .. 2^64, so the complexities of a chain's members lie up to 2^24 apart
      const uint64_t mh = pick(10) == 0 ? ~0ull - (uint64_t)pick(1000) : (rng() | (1ull << 63)) >> pick(24);
      const int raw = 60 + pick(21);
      for (int r = 0; r < nrec && (int)v.size() < want; r++) {
        static const int jit[] = {0, 0, 0, 1, -3, 17, SEG - 1, SEG, SEG + 1, -SEG + 1, 2 * SEG - 1, 2 * SEG, 3 * SEG, -250};
        int pos = strand == 1 ? base + starts[f] : base + 9000 - starts[f];
        pos += jit[pick((int)(sizeof jit / sizeof jit[0]))] + r * period;
        if (pick(6) == 0 && !v.empty()) pos = v.back().refStartPos;                         // an equal reference position
        v.push_back(rec(starts[f], fl, pick(8) ? refId : 1 - refId, pos, 56 + 4 * pick(7), pick(10) ? strand : -strand, mh, raw, 64 + 4 * pick(5)));
      }
    }
    if (v.empty()) v.push_back(rec(starts[0], fl, refId, base, 70, strand));
    for (auto& m : v) if (m.conservedSketches > m.sketchSize) m.conservedSketches = m.sketchSize;
    const std::vector<mm_chain_row> out = both(S, v, len, "generated");
    reads++; rows += (long)out.size(); if ((long)v.size() > maxN) maxN = (long)v.size(); if (v.size() == 16) histo16++;
    for (const auto& r : out) if (r.n_merged > 1) merged++;
    if (out.empty()) dropped++;
  }
  std::printf("generated reads %ld rows %ld chains_of_two_or_more %ld reads_without_rows %ld largest_read %ld reads_of_16 %ld\n", reads, rows, merged, dropped, maxN, histo16);
}

static void complexity() {
  long n = 0, bad = 0;
  auto one = [&](uint64_t m) {
    const double want = (double)((long double)m / std::numeric_limits<uint64_t>::max());
    const double got = mm_chain_hash01(m);
    n++;
    if (std::memcmp(&want, &got, 8) != 0) { if (bad++ < 5) std::fprintf(stderr, "hash01(%" PRIu64 "): %.17g, long double gives %.17g\n", m, got, want); }
  };
  one(1); one(~0ull);
  for (int p = 1; p <= 63; p++) { one(1ull << p); one((1ull << p) + 1); one((1ull << p) - 1); }
  std::printf("hash01 edge values %ld bad %ld\n", n, bad);
  g_bad += (int)bad; n = 0; bad = 0;
  std::mt19937_64 rng(20240611);
  for (int i = 0; i < 1000000; i++) one(rng() >> (i % 7 == 0 ? (int)(rng() % 60) : 0));
  std::printf("hash01 random values %ld bad %ld\n", n, bad);
  g_bad += (int)bad;
  long fb = 0;
  for (int i = 0; i < 200000; i++) {                                 // the whole expression of getSeedHits (:830-831), against the long double form
    const uint64_t m = (rng() >> (int)(rng() % 40)) | 1; const int raw = 1 + (int)(rng() % 2048), Qlen = K + (int)(rng() % 5000);
    const double max_hash_01 = (long double)(m) / std::numeric_limits<uint64_t>::max();
    const float want = (double(raw) / max_hash_01) / ((Qlen - K + 1) * 2);
    const float got = mm_chain_kmer_complexity(m, raw, Qlen, K);
    if (std::memcmp(&want, &got, 4) != 0) fb++;
  }
  std::printf("kmerComplexity random values 200000 bad %ld\n", fb);
  g_bad += (int)fb;
}

int main(int argc, char** argv) {
  const int nReads = argc > 1 ? std::atoi(argv[1]) : 20000;
  named_scenarios();
  generated(nReads, 99);
  complexity();
  std::printf("differences %d\n", g_bad);
  return g_bad ? 1 : 0;
}
