// tests/hostlogic/chain_long_check.cpp -- mm_chain_read_long (mashmap_amd/csrc/mm_chain_core.h: the tail of Map::mapModule for a read of
// up to 512 records, what k_chain_reads_long runs step by step) compiled for the host, beside MapPost::chainedFromRecords on generated
// reads of 17 to 512 records: every field of every row bit for bit, floats included.  Above 16 elements the host's five std::sort calls
// are introsort; the header's go through mm_stdsort.h.  Stand-alone, built by tests/test_chain_long_core.py under
// -fsanitize=address,undefined.  k 16, segLength 1000, sketch 80, two contigs.
//
// Prints one line per named scenario, one for the generated long reads ("generated ..."), one for reads of 1 to 16 records through
// both entry points ("short ..."); exit status 1 with the first differences on stderr when anything differs.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../mashmap_amd/host/skch_map_post.hpp"
#include "../../mashmap_amd/csrc/mm_chain_core.h"

static const int K = 16, SEG = 1000, SK = 80;
static int g_bad = 0;
static mm_chain_work_long g_work;             // 39 KB: the caller's working set

struct Setup {
  skch::Parameters p;
  std::vector<skch::ContigInfo> meta;
  std::vector<int> grp;
  std::vector<float> identity;
  Setup() {
    p.kmerSize = K; p.segLength = SEG; p.block_length = SEG; p.chain_gap = SEG; p.sketchSize = SK; p.percentageIdentity = 0.85f;
    p.filterMode = skch::filter::MAP; p.split = true; p.mergeMappings = true;
    meta = {skch::ContigInfo{"c0", 6000000}, skch::ContigInfo{"c1", 4000000}};
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

static mm_chain_env env_of(const Setup& S, const skch::MapPost& post) {
  mm_chain_env E;
  E.p = post.chainParams(); E.kmerSize = K; E.segLength = SEG; E.stride = SK + 1; E.identity = S.identity.data();
  return E;
}

// runs both forms on one read; returns the rows of the header's form (differences are reported and counted)
static std::vector<mm_chain_row> both(const Setup& S, const std::vector<mm_mapping>& recs, int len, const char* what) {
  skch::MapPost post(S.p, S.meta, S.grp);
  skch::MappingResultsVector_t host;
  post.chainedFromRecords(recs.data(), recs.data() + recs.size(), len, host);
  const mm_chain_env E = env_of(S, post);
  std::vector<mm_chain_row> rows(recs.size() + 1);
  const int counted = mm_chain_read_long(E, g_work, recs.data(), (int)recs.size(), len, nullptr);
  const int n = mm_chain_read_long(E, g_work, recs.data(), (int)recs.size(), len, rows.data());
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

static void say(const char* name, const std::vector<mm_chain_row>& rows) {
  std::printf("scenario %s rows %zu", name, rows.size());
  for (const auto& r : rows) std::printf(" [%d-%d %d:%d-%d %c cons %d merged %d]", r.queryStartPos, r.queryEndPos, r.refSeqId, r.refStartPos, r.refEndPos, r.strand == 1 ? '+' : '-', r.conservedSketches, r.n_merged);
  std::printf("\n");
}

static void named_scenarios() {
  Setup S;
  {  // one chain of 17, pairwise different conservedSketches (50 + segment): every member ties in the sort by splitMappingId, and the
     // one introsort leaves in front -- not member 0 -- is the representative
    std::vector<mm_mapping> v;
    for (int i = 0; i < 17; i++) v.push_back(rec(i * SEG, SEG, 0, 10000 + i * SEG, 50 + i, 1));
    say("chain_of_17", both(S, v, 17 * SEG, "chain_of_17"));
    v.clear();                                                     // 20 on the reverse strand: key order is the reverse of segment order
    for (int i = 0; i < 20; i++) v.push_back(rec(i * SEG, SEG, 1, 40000 - i * SEG, 50 + i, -1));
    say("chain_of_20_rev", both(S, v, 20 * SEG, "chain_of_20_rev"));
  }
  {  // 513 records are refused, 512 are taken, a bad record is an error
    std::vector<mm_mapping> v;
    for (int i = 0; i < 513; i++) v.push_back(rec(i * SEG, SEG, 0, 1000 + i * SEG, 70, 1));
    skch::MapPost post(S.p, S.meta, S.grp);
    const mm_chain_env E = env_of(S, post);
    std::vector<mm_chain_row> rows(513);
    const int a = mm_chain_read_long(E, g_work, v.data(), 513, 513 * SEG, rows.data());
    v.pop_back();
    const std::vector<mm_chain_row> r512 = both(S, v, 512 * SEG, "records_512");
    v[300].sketchSize = SK + 1;
    const int c = mm_chain_read_long(E, g_work, v.data(), 512, 512 * SEG, rows.data());
    std::printf("scenario limits records_513 %d records_512 rows %zu merged %d bad_record %d\n", a, r512.size(), r512.empty() ? 0 : r512[0].n_merged, c);
  }
}

struct Tally { long reads = 0, rows = 0, merged = 0, longChains = 0, maxN = 0, at512 = 0, fragOver16 = 0, notSplit = 0, mergeOff = 0, tied = 0, multiChain = 0, rev = 0;
               long keep[3] = {0, 0, 0}, filt[3] = {0, 0, 0}; std::map<int, long> sizes; };

// One read of exactly `want` records.  Shapes: c interleaved colinear chains over many fragments; few fragments out of a tandem array
// (more than 16 records each); a read of one fragment; a mix with the jitters that matter around chain_gap.
static void one_read(std::mt19937_64& rng, int want, bool small, Tally& T) {
  auto pick = [&rng](int n) { return (int)(rng() % (uint64_t)n); };
  Setup S;
  S.p.block_length = pick(3) == 0 ? 3 * SEG : SEG;
  const int keepSel = pick(3), keep = keepSel == 0 ? 1 : keepSel == 1 ? 3 : 0;      // secondaryToKeep 0, 2, 65535
  S.p.numMappingsForSegment = keep; S.p.numMappingsForShortSequence = keep;
  S.p.mergeMappings = pick(8) != 0;
  const int filtSel = pick(5) == 0 ? 0 : 1 + pick(2);
  S.p.filterMode = filtSel == 0 ? skch::filter::NONE : filtSel == 1 ? skch::filter::MAP : skch::filter::ONETOONE;
  S.p.chain_gap = pick(4) == 0 ? 2 * SEG : SEG;
  S.p.kmerComplexityThreshold = pick(5) == 0 ? 0.05f : 0.0f;
  const int shape = pick(10);                                      // 0-4 chains, 5-6 tandem, 7 one fragment, 8-9 mix
  const int strand = pick(2) ? 1 : -1, refId = pick(2);
  static const int jit[] = {0, 0, 0, 0, 1, -3, 17, SEG - 1, SEG, SEG + 1, -SEG + 1, 2 * SEG - 1, 2 * SEG, 3 * SEG, -250};
  const int nJit = (int)(sizeof jit / sizeof jit[0]);
  std::vector<mm_mapping> v;
  int len, maxFrag = 0; bool tied = false;
  auto hashOf = [&]() { return pick(10) == 0 ? ~0ull - (uint64_t)pick(1000) : (rng() | (1ull << 63)) >> pick(24); };
  auto push = [&](int fs, int fl, int rid, int pos, int st, uint64_t mh, int raw) {
    if (pick(7) == 0 && !v.empty() && v.back().fragStart == fs) { pos = v.back().refStartPos; rid = v.back().refSeqId; tied = true; }   // ties in (refSeqId, refStartPos, queryStartPos)
    mm_mapping m = rec(fs, fl, rid, pos, 56 + 4 * pick(7) + pick(4), st, mh, raw, 64 + 4 * pick(5));
    if (m.conservedSketches > m.sketchSize) m.conservedSketches = m.sketchSize;
    v.push_back(m);
  };
  if (shape == 7) {                                                // not split
    len = 300 + pick(701);
    const uint64_t mh = hashOf(); const int raw = 60 + pick(21);
    for (int r = 0; r < want; r++) push(0, len, pick(6) ? refId : 1 - refId, 5000 + pick(40) * 1100 + pick(3), pick(5) ? strand : -strand, mh, raw);
    T.notSplit++;
  } else {
    const int c = shape <= 4 ? 1 + pick(4) : shape <= 6 ? 17 + pick(30) : 1 + pick(3);       // records per fragment, about
    int nseg = (want + c - 1) / c + (shape >= 8 ? pick(4) : 0);
    if (nseg < 2) nseg = 2;
    len = nseg * SEG + (pick(2) ? 1 + pick(SEG - 1) : 0);
    std::vector<int> starts;
    for (int i = 0; i < len / SEG; i++) starts.push_back(i * SEG);
    if (len % SEG) starts.push_back(len - SEG);
    const int base = 5000 + pick(20000), period = shape <= 4 ? 200000 + pick(1000) : 700 + pick(900);
    for (size_t f = 0; f < starts.size() && (int)v.size() < want; f++) {
      const bool lastFrag = f + 1 == starts.size();
      int nrec = shape >= 8 ? (pick(8) == 0 ? 0 : 1 + pick(2 * c)) : pick(12) == 0 ? c - 1 : c;
      if (lastFrag) nrec = want - (int)v.size();
      const uint64_t mh = hashOf(); const int raw = 60 + pick(21);
      const int before = (int)v.size();
      for (int r = 0; r < nrec && (int)v.size() < want; r++) {
        int pos = strand == 1 ? base + starts[f] : base + (int)starts.size() * SEG - starts[f];
        pos += (shape >= 8 || pick(6) == 0 ? jit[pick(nJit)] : pick(5) - 2) + r * period;
        push(starts[f], SEG, pick(20) ? refId : 1 - refId, pos, pick(25) ? strand : -strand, mh, raw);
      }
      if ((int)v.size() - before > maxFrag) maxFrag = (int)v.size() - before;
    }
    while ((int)v.size() < want) push(starts.back(), SEG, refId, base + pick(100000), strand, v.empty() ? hashOf() : v.back().maxHash, v.empty() ? 70 : v.back().rawSketchSize);
    if (shape <= 4 && c > 1) T.multiChain++;
  }
  if (small) {                                                     // 1 .. 16 records: both entry points, byte for byte
    skch::MapPost post(S.p, S.meta, S.grp);
    const mm_chain_env E = env_of(S, post);
    std::vector<mm_chain_row> a(want + 1), b(want + 1);
    std::memset(a.data(), 0, a.size() * sizeof(mm_chain_row)); std::memset(b.data(), 0, b.size() * sizeof(mm_chain_row));
    const int na = mm_chain_read(E, v.data(), want, len, a.data()), nb = mm_chain_read_long(E, g_work, v.data(), want, len, b.data());
    if (na != nb || std::memcmp(a.data(), b.data(), a.size() * sizeof(mm_chain_row)) != 0) { if (g_bad++ < 10) std::fprintf(stderr, "short read of %d records: mm_chain_read %d rows, mm_chain_read_long %d, or rows differ\n", want, na, nb); }
    T.reads++; T.rows += na; T.sizes[want]++;
    return;
  }
  const std::vector<mm_chain_row> out = both(S, v, len, "generated");
  T.reads++; T.rows += (long)out.size(); T.sizes[want]++; T.keep[keepSel]++; T.filt[filtSel]++;
  if (want > T.maxN) T.maxN = want;
  if (want == 512) T.at512++;
  if (maxFrag > 16) T.fragOver16++;
  if (!S.p.mergeMappings) T.mergeOff++;
  if (tied) T.tied++;
  if (strand == -1) T.rev++;
  for (const auto& r : out) { if (r.n_merged > 1) T.merged++; if (r.n_merged > 16) T.longChains++; }
}

static void generated(int nReads, uint64_t seed) {
  std::mt19937_64 rng(seed);
  Tally T;
  for (int it = 0; it < nReads; it++) {
    int want;
    if (it < 240) want = 17 + it % 24;                             // every size from 17 to 40, ten times
    else if (it % 50 == 0) want = 512;
    else if (it % 3 == 0) want = 17 + (int)(rng() % 48);
    else if (it % 3 == 1) want = 17 + (int)(rng() % 200);
    else want = 17 + (int)(rng() % 496);
    one_read(rng, want, false, T);
  }
  int from17to40 = 0;
  for (int n = 17; n <= 40; n++) if (T.sizes.count(n)) from17to40++;
  std::printf("generated reads %ld rows %ld chains_of_two_or_more %ld chains_over_16 %ld largest_read %ld reads_of_512 %ld sizes_17_to_40 %d "
              "fragment_over_16 %ld not_split %ld merge_off %ld tied %ld several_chains %ld reverse %ld keep0 %ld keep2 %ld keep65535 %ld filter_none %ld filter_map %ld filter_one2one %ld\n",
              T.reads, T.rows, T.merged, T.longChains, T.maxN, T.at512, from17to40, T.fragOver16, T.notSplit, T.mergeOff, T.tied, T.multiChain, T.rev,
              T.keep[0], T.keep[1], T.keep[2], T.filt[0], T.filt[1], T.filt[2]);
  Tally Sm;
  for (int it = 0; it < 2000; it++) one_read(rng, 1 + it % 16, true, Sm);
  std::printf("short reads %ld rows %ld sizes %zu\n", Sm.reads, Sm.rows, Sm.sizes.size());
}

int main(int argc, char** argv) {
  const int nReads = argc > 1 ? std::atoi(argv[1]) : 5000;
  named_scenarios();
  generated(nReads, 4242);
  std::printf("differences %d\n", g_bad);
  return g_bad ? 1 : 0;
}
