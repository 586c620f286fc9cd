// tests/hostlogic/chain_modes_check.cpp -- mm_chain_read and mm_chain_read_long (mashmap_amd/csrc/mm_chain_core.h) with the reference
// groups of -Y (mm_chain_env::refGroup) and with --noSplit (mm_chain_env::noSplit), compiled for the host, beside
// MapPost::chainedFromRecords with skip_prefix / split set accordingly, on generated reads of 1 to 512 records: every field of every row
// bit for bit, floats included, and the run count of every read against the runs counted in MapPost's own input to filterByGroup.
// Stand-alone, built by tests/test_chain_modes_core.py under -fsanitize=address,undefined.  k 16, segLength 1000, sketch 80, ten contigs
// in eight groups, either numbered as Map::setRefGroups numbers them (0 0 1 1 2 3 4 5 6 7) or not non-decreasing (0 1 0 2 1 3 4 5 6 7:
// the C ABI takes such an array, and groups 0 and 1 then form two runs each).
//
// Prints one line per named scenario, one for the generated reads ("generated ..."), one for the ungrouped reads that go through the
// same filter code as before ("ungrouped ..."); exit status 1 with the first differences on stderr when anything differs.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../mashmap_amd/host/skch_map_post.hpp"
#include "../../mashmap_amd/csrc/mm_chain_core.h"

static const int K = 16, SEG = 1000, SK = 80, NC = 10;
static const int GRP_MONO[NC] = {0, 0, 1, 1, 2, 3, 4, 5, 6, 7};
static const int GRP_MIX[NC] = {0, 1, 0, 2, 1, 3, 4, 5, 6, 7};
static int g_bad = 0;
static mm_chain_work_long g_work;             // 39 KB: the caller's working set

struct Setup {
  skch::Parameters p;
  std::vector<skch::ContigInfo> meta;
  std::vector<int> grp;                       // MapPost's refIdGroup
  std::vector<int32_t> grp32;                 // the same as the environment's array
  bool grouped = false;
  std::vector<float> identity;
  Setup() {
    p.kmerSize = K; p.segLength = SEG; p.block_length = SEG; p.chain_gap = SEG; p.sketchSize = SK; p.percentageIdentity = 0.85f;
    p.filterMode = skch::filter::MAP; p.split = true; p.mergeMappings = true;
    for (int i = 0; i < NC; i++) meta.push_back(skch::ContigInfo{"c" + std::to_string(i), 6000000});
    grp.assign(NC, 0); grp32.assign(NC, 0);
    identity.assign((size_t)(SK + 1) * (SK + 1), 0.0f);
    for (int q = 1; q <= SK; q++)
      for (int s = 0; s <= SK; s++) identity[(size_t)q * (SK + 1) + s] = 1 - mmhost::Stat::j2md(1.0 * s / q, K);
  }
  void groups(const int* g) {                 // nullptr: no -Y
    grouped = g != nullptr; p.skip_prefix = grouped;
    for (int i = 0; i < NC; i++) { grp[i] = g ? g[i] : 0; grp32[i] = grp[i]; }
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
  E.refGroup = S.grouped ? S.grp32.data() : nullptr; E.nContigs = NC; E.noSplit = S.p.split ? 0 : 1;
  return E;
}

// the runs of filterByGroup from MapPost's own input to it: the read's mappings behind chaining and the weak-chain filter, sorted by
// (refSeqId, refStartPos) -- equal keys are one contig, so any sort shows the same runs
struct Runs { int runs = 0, ones = 0, over16 = 0, groups = 0; };
static Runs host_runs(const Setup& S, const skch::MapPost& post, const std::vector<mm_mapping>& recs, int len) {
  Runs R;
  if (!(S.p.filterMode == skch::filter::MAP || S.p.filterMode == skch::filter::ONETOONE)) return R;
  skch::MappingResultsVector_t v;
  const bool split = post.unfilteredFromRecords(recs.data(), recs.data() + recs.size(), len, v);
  if (split && S.p.mergeMappings) {
    post.mergeMappingsInRange(v, S.p.chain_gap);
    post.filterWeakMappings(v, (int64_t)std::floor(S.p.block_length / S.p.segLength));
  }
  std::stable_sort(v.begin(), v.end(), [](const skch::MappingResult& a, const skch::MappingResult& b) {
    return std::tie(a.refSeqId, a.refStartPos) < std::tie(b.refSeqId, b.refStartPos); });
  std::set<int> seen;
  for (size_t b = 0; b < v.size();) {
    size_t e = v.size();
    if (S.grouped) { e = b; while (e < v.size() && S.grp[v[e].refSeqId] == S.grp[v[b].refSeqId]) e++; }
    R.runs++;
    if (e - b == 1) R.ones++;
    if (e - b > 16) R.over16++;
    seen.insert(S.grouped ? S.grp[v[b].refSeqId] : 0);
    b = e;
  }
  R.groups = (int)seen.size();
  return R;
}

// runs both forms on one read; returns the rows of the header's form (differences are reported and counted)
static std::vector<mm_chain_row> both(const Setup& S, const std::vector<mm_mapping>& recs, int len, const char* what, Runs* runsOut = nullptr) {
  skch::MapPost post(S.p, S.meta, S.grp);
  skch::MappingResultsVector_t host;
  post.chainedFromRecords(recs.data(), recs.data() + recs.size(), len, host);
  const Runs R = host_runs(S, post, recs, len);
  if (runsOut) *runsOut = R;
  const mm_chain_env E = env_of(S, post);
  std::vector<mm_chain_row> rows(recs.size() + 1);
  std::memset(rows.data(), 0, rows.size() * sizeof(mm_chain_row));
  int runsCounted = -1, runs = -1;
  const int counted = mm_chain_read_long(E, g_work, recs.data(), (int)recs.size(), len, nullptr, &runsCounted);
  const int n = mm_chain_read_long(E, g_work, recs.data(), (int)recs.size(), len, rows.data(), &runs);
  bool same = counted == n && n == (int)host.size() && runs == R.runs && runsCounted == R.runs;
  if (same && mm_chain_read_long(E, g_work, recs.data(), (int)recs.size(), len, nullptr) != n) same = false;       // the signature of before
  if (same && (int)recs.size() <= MM_CHAIN_MAX_RECORDS) {          // the one-thread form: the same bytes, the same count
    std::vector<mm_chain_row> a(recs.size() + 1);
    std::memset(a.data(), 0, a.size() * sizeof(mm_chain_row));
    int runsShort = -1;
    const int na = mm_chain_read(E, recs.data(), (int)recs.size(), len, a.data(), &runsShort);
    if (na != n || runsShort != R.runs || std::memcmp(a.data(), rows.data(), a.size() * sizeof(mm_chain_row)) != 0 ||
        mm_chain_read(E, recs.data(), (int)recs.size(), len, nullptr) != n) {
      same = false;
      std::fprintf(stderr, "%s: mm_chain_read %d rows %d runs, mm_chain_read_long %d rows %d runs, or rows differ\n", what, na, runsShort, n, runs);
    }
  }
  rows.resize(n < 0 ? 0 : n);
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
    if (g_bad++ < 10) std::fprintf(stderr, "%s: %zu records, len %d, grouped %d split %d: header %d (counted %d) rows %d (counted %d) runs, host %zu rows %d runs\n", what, recs.size(), len,
                                   (int)S.grouped, (int)S.p.split, n, counted, runs, runsCounted, host.size(), R.runs);
  }
  return rows;
}

static void say(const char* name, const std::vector<mm_chain_row>& rows, int runs) {
  std::printf("scenario %s runs %d rows %zu", name, runs, rows.size());
  for (const auto& r : rows) std::printf(" [%d-%d %d:%d-%d %c cons %d merged %d]", r.queryStartPos, r.queryEndPos, r.refSeqId, r.refStartPos, r.refEndPos, r.strand == 1 ? '+' : '-', r.conservedSketches, r.n_merged);
  std::printf("\n");
}

static void named_scenarios() {
  {  // one read of three segments, a colinear chain on contigs 0, 2 and 4 -- groups 0, 1 and 2 --, secondaryToKeep 0: a row per group;
     // the same records without groups compete in one sweep and the best identity alone is left
    Setup S;
    S.p.numMappingsForSegment = 1; S.p.numMappingsForShortSequence = 1;
    std::vector<mm_mapping> v;
    for (int i = 0; i < 3; i++)
      for (int g = 0; g < 3; g++) v.push_back(rec(i * SEG, SEG, 2 * g, 10000 + i * SEG, 70 - 4 * g, 1));
    Runs R;
    S.groups(GRP_MONO);
    const std::vector<mm_chain_row> a = both(S, v, 3 * SEG, "three_groups_three_rows", &R);
    say("three_groups_three_rows", a, R.runs);
    S.groups(nullptr);
    const std::vector<mm_chain_row> b = both(S, v, 3 * SEG, "three_groups_no_groups", &R);
    say("three_groups_no_groups", b, R.runs);
  }
  {  // refGroup 0 1 0 2 1 ...: contigs 0 and 2 are both group 0, but contig 1 (group 1) lies between them in the order sorted by the
     // reference key: three runs, each swept alone, three rows -- where 0 0 1 ... puts contigs 0 and 1 into one run of which one row is left
    Setup S;
    S.p.numMappingsForSegment = 1; S.p.numMappingsForShortSequence = 1;
    std::vector<mm_mapping> v;
    for (int i = 0; i < 2; i++)
      for (int c = 0; c < 3; c++) v.push_back(rec(i * SEG, SEG, c, 20000 + i * SEG, 72 - 3 * c, 1));
    Runs R;
    S.groups(GRP_MIX);
    const std::vector<mm_chain_row> a = both(S, v, 2 * SEG, "group_in_two_runs", &R);
    say("group_in_two_runs", a, R.runs);
    S.groups(GRP_MONO);
    const std::vector<mm_chain_row> b = both(S, v, 2 * SEG, "group_in_one_run", &R);
    say("group_in_one_run", b, R.runs);
  }
  {  // with refGroup set a record outside the contigs is an error from both entry points, and nothing is read outside the array;
     // without refGroup the contig id is not looked up
    Setup S;
    S.groups(GRP_MONO);
    skch::MapPost post(S.p, S.meta, S.grp);
    mm_chain_env E = env_of(S, post);
    std::vector<mm_mapping> v;
    for (int i = 0; i < 3; i++) v.push_back(rec(i * SEG, SEG, 1, 30000 + i * SEG, 70, 1));
    std::vector<mm_chain_row> rows(32);
    int runs = 5;
    v[1].refSeqId = NC;
    const int a = mm_chain_read(E, v.data(), 3, 3 * SEG, rows.data(), &runs), b = mm_chain_read_long(E, g_work, v.data(), 3, 3 * SEG, rows.data());
    v[1].refSeqId = -1;
    const int c = mm_chain_read(E, v.data(), 3, 3 * SEG, rows.data());
    v[1].refSeqId = NC - 1;
    const int d = mm_chain_read(E, v.data(), 3, 3 * SEG, rows.data());
    E.refGroup = nullptr; v[1].refSeqId = NC;
    const int e = mm_chain_read(E, v.data(), 3, 3 * SEG, rows.data());
    std::printf("scenario bad_refseqid past_the_end %d long %d runs %d negative %d last_contig %d no_groups %d\n", a, b, runs, c, d, e);
  }
}

struct Tally { long reads = 0, rows = 0, merged = 0, rev = 0, mergeOff = 0, small = 0, large = 0, maxN = 0;
               long inGroups[9] = {0}, sameInterval = 0, sibling = 0, runsOfOne = 0, runsOver16 = 0, twoRuns = 0, multiRun = 0, runs = 0;
               long noSplitShort[2] = {0, 0}, noSplitLong[2] = {0, 0}, splitShort = 0, mix = 0, mono = 0, none = 0;
               long keep[3] = {0, 0, 0}, filt[3] = {0, 0, 0}; std::set<int> sizes; };

// One read of exactly `want` records on the contigs of 1, 2, 3 or 8 groups: the same chain in every group (and, one time in three, on
// a second contig of a group), over the same query interval; c chains per contig, up to more than 16; reads of one fragment, split or
// not.  mode 0: no groups (-Y off), 1: groups 0 0 1 1 2 ..., 2: groups 0 1 0 2 1 ...
static void one_read(std::mt19937_64& rng, int want, int mode, Tally& T) {
  auto pick = [&rng](int n) { return (int)(rng() % (uint64_t)n); };
  Setup S;
  S.groups(mode == 0 ? nullptr : mode == 1 ? GRP_MONO : GRP_MIX);
  S.p.block_length = pick(3) == 0 ? 3 * SEG : SEG;
  const int keepSel = pick(3), keep = keepSel == 0 ? 1 : keepSel == 1 ? 3 : 0;      // secondaryToKeep 0, 2, 65535
  S.p.numMappingsForSegment = keep; S.p.numMappingsForShortSequence = keep;
  S.p.mergeMappings = pick(6) != 0;
  const int filtSel = pick(6) == 0 ? 0 : 1 + pick(2);
  S.p.filterMode = filtSel == 0 ? skch::filter::NONE : filtSel == 1 ? skch::filter::MAP : skch::filter::ONETOONE;
  S.p.chain_gap = pick(4) == 0 ? 2 * SEG : SEG;
  S.p.kmerComplexityThreshold = pick(6) == 0 ? 0.05f : 0.0f;
  S.p.split = pick(3) != 0;
  static const int nGs[] = {1, 2, 3, 8};
  const int nG = nGs[pick(4)];
  std::vector<int> targets;                                        // the contigs the read maps to
  bool sibling = false;
  if (mode == 2) {
    const int upTo = nG == 1 ? 0 : nG == 2 ? 3 : nG == 3 ? 5 : NC;  // contigs 0 .. upTo-1 hold nG groups; 0 and 2 are group 0, 1 and 4 group 1
    if (nG == 1) { targets = {0, 2}; sibling = true; }
    else { for (int c = 0; c < upTo; c++) targets.push_back(c); sibling = true; }
  } else {
    static const int firstOf[] = {0, 2, 4, 5, 6, 7, 8, 9};
    for (int g = 0; g < nG; g++) targets.push_back(firstOf[g]);
    if (pick(3) == 0) { targets.insert(targets.begin() + 1, 1); sibling = true; if (nG > 1 && pick(2)) targets.push_back(3); }
  }
  const int nT = (int)targets.size();
  const int strand = pick(2) ? 1 : -1;
  const int shape = pick(10);                                      // 0-5 chains, 6-7 many chains per contig, 8-9 one fragment
  const int c = shape <= 5 ? 1 + pick(3) : 17 + pick(12);
  static const int jit[] = {0, 0, 0, 0, 1, -3, 17, SEG - 1, SEG, SEG + 1, -SEG + 1, 2 * SEG - 1, 2 * SEG, 3 * SEG, -250};
  const int nJit = (int)(sizeof jit / sizeof jit[0]);
  auto hashOf = [&]() { return pick(10) == 0 ? ~0ull - (uint64_t)pick(1000) : (rng() | (1ull << 63)) >> pick(24); };
  std::vector<mm_mapping> v;
  auto push = [&](int fs, int fl, int rid, int pos, int st, uint64_t mh, int raw) {
    if (pick(9) == 0 && !v.empty() && v.back().fragStart == fs) { pos = v.back().refStartPos; rid = v.back().refSeqId; }   // ties in (refSeqId, refStartPos, queryStartPos)
    mm_mapping m = rec(fs, fl, rid, pos, 56 + 4 * pick(7) + pick(4), st, mh, raw, 64 + 4 * pick(5));
    if (m.conservedSketches > m.sketchSize) m.conservedSketches = m.sketchSize;
    v.push_back(m);
  };
  int len;
  const int base = 5000 + pick(20000), period = shape <= 5 ? 200000 + pick(1000) : 20000 + pick(900);
  if (shape >= 8 || (!S.p.split && pick(2))) {                     // one fragment: shorter than a segment, or (not split) longer
    len = (!S.p.split && pick(2)) ? SEG + 1 + pick(5000) : 300 + pick(701);
    const uint64_t mh = hashOf(); const int raw = 60 + pick(21);
    for (int r = 0; r < want; r++) push(0, len, targets[r % nT], base + (r / nT) * 1100 + pick(3), pick(5) ? strand : -strand, mh, raw);
  } else {
    int nseg = (want + nT * c - 1) / (nT * c);
    if (nseg < 2) nseg = 2;
    len = nseg * SEG + (pick(2) ? 1 + pick(SEG - 1) : 0);
    if (!S.p.split) {                                              // --noSplit: the whole read is the one fragment
      const uint64_t mh = hashOf(); const int raw = 60 + pick(21);
      for (int r = 0; r < want; r++) push(0, len, targets[r % nT], base + (r / nT) * 1100 + pick(3), pick(5) ? strand : -strand, mh, raw);
    } else {
      std::vector<int> starts;
      for (int i = 0; i < len / SEG; i++) starts.push_back(i * SEG);
      if (len % SEG) starts.push_back(len - SEG);
      for (size_t f = 0; f < starts.size() && (int)v.size() < want; f++) {
        const uint64_t mh = hashOf(); const int raw = 60 + pick(21);
        for (int ch = 0; ch < c && (int)v.size() < want; ch++)
          for (int t = 0; t < nT && (int)v.size() < want; t++) {
            if (pick(15) == 0) continue;                           // a fragment that misses a contig
            int pos = strand == 1 ? base + starts[f] : base + (int)starts.size() * SEG - starts[f];
            pos += (pick(6) == 0 ? jit[pick(nJit)] : pick(5) - 2) + ch * period;
            push(starts[f], SEG, targets[t], pos, pick(25) ? strand : -strand, mh, raw);
          }
      }
      while ((int)v.size() < want) push(starts.back(), SEG, targets[pick(nT)], base + pick(100000), strand, v.empty() ? hashOf() : v.back().maxHash, v.empty() ? 70 : v.back().rawSketchSize);
    }
  }
  Runs R;
  const std::vector<mm_chain_row> out = both(S, v, len, "generated", &R);
  T.reads++; T.rows += (long)out.size(); T.sizes.insert(want); T.keep[keepSel]++; T.filt[filtSel]++;
  if (want <= 16) T.small++; else T.large++;
  if (want > T.maxN) T.maxN = want;
  (mode == 0 ? T.none : mode == 1 ? T.mono : T.mix)++;
  if (!S.p.mergeMappings) T.mergeOff++;
  if (strand == -1) T.rev++;
  for (const auto& r : out) if (r.n_merged > 1) T.merged++;
  if (!S.p.split) (len > SEG ? T.noSplitLong : T.noSplitShort)[mode != 0]++;
  else if (len <= SEG) T.splitShort++;
  if (mode != 0) {
    std::set<int> gs;
    for (const auto& m : v) gs.insert(S.grp[m.refSeqId]);
    T.inGroups[gs.size() <= 8 ? gs.size() : 8]++;
    if (sibling) {                                                 // two contigs of one group hit by the same fragment
      std::map<std::pair<int, int>, std::set<int>> per;
      for (const auto& m : v) per[{m.fragStart, S.grp[m.refSeqId]}].insert(m.refSeqId);
      for (const auto& kv : per) if (kv.second.size() > 1) { T.sibling++; break; }
    }
    bool overlap = false;                                          // rows of several groups over the same query interval
    for (size_t i = 0; i < out.size() && !overlap; i++)
      for (size_t j = i + 1; j < out.size() && !overlap; j++)
        overlap = S.grp[out[i].refSeqId] != S.grp[out[j].refSeqId] && out[i].queryStartPos < out[j].queryEndPos && out[j].queryStartPos < out[i].queryEndPos;
    if (overlap) T.sameInterval++;
    if (R.runs > R.groups) T.twoRuns++;                            // a group in two runs
    if (R.runs > 1) T.multiRun++;
  }
  T.runs += R.runs; T.runsOfOne += R.ones; T.runsOver16 += R.over16;
}

static void generated(int nReads, uint64_t seed) {
  std::mt19937_64 rng(seed);
  Tally T;
  for (int it = 0; it < nReads; it++) {
    int want;
    if (it < 96) want = 1 + it % 48;                               // every size from 1 to 48, twice
    else if (it % 60 == 0) want = 512;
    else if (it % 4 == 0) want = 1 + (int)(rng() % 16);
    else if (it % 4 == 1) want = 17 + (int)(rng() % 48);
    else if (it % 4 == 2) want = 17 + (int)(rng() % 200);
    else want = 17 + (int)(rng() % 496);
    one_read(rng, want, it % 5 == 0 ? 0 : it % 5 <= 2 ? 1 : 2, T);
  }
  int upTo16 = 0;
  for (int n = 1; n <= 16; n++) upTo16 += (int)T.sizes.count(n);
  std::printf("generated reads %ld rows %ld chains_of_two_or_more %ld largest_read %ld sizes_1_to_16 %d reads_up_to_16 %ld reads_over_16 %ld "
              "no_groups %ld groups_in_order %ld groups_out_of_order %ld in_1_group %ld in_2_groups %ld in_3_groups %ld in_8_groups %ld "
              "several_groups_same_interval %ld two_contigs_of_a_group %ld runs %ld runs_of_one %ld runs_over_16 %ld group_in_two_runs %ld reads_with_several_runs %ld "
              "nosplit_short %ld nosplit_short_grouped %ld nosplit_long %ld nosplit_long_grouped %ld split_short %ld "
              "merge_off %ld reverse %ld keep0 %ld keep2 %ld keep65535 %ld filter_none %ld filter_map %ld filter_one2one %ld\n",
              T.reads, T.rows, T.merged, T.maxN, upTo16, T.small, T.large, T.none, T.mono, T.mix, T.inGroups[1], T.inGroups[2], T.inGroups[3], T.inGroups[8],
              T.sameInterval, T.sibling, T.runs, T.runsOfOne, T.runsOver16, T.twoRuns, T.multiRun,
              T.noSplitShort[0], T.noSplitShort[1], T.noSplitLong[0], T.noSplitLong[1], T.splitShort,
              T.mergeOff, T.rev, T.keep[0], T.keep[1], T.keep[2], T.filt[0], T.filt[1], T.filt[2]);
  // the filter of a context without groups is the code of before the runs: 2 000 ungrouped reads against MapPost, as the other checks do
  Tally U;
  for (int it = 0; it < 2000; it++) one_read(rng, it % 3 == 0 ? 1 + it % 16 : 17 + (int)(rng() % 120), 0, U);
  std::printf("ungrouped reads %ld rows %ld runs %ld reads_with_several_runs %ld\n", U.reads, U.rows, U.runs, U.multiRun);
}

int main(int argc, char** argv) {
  const int nReads = argc > 1 ? std::atoi(argv[1]) : 4000;
  named_scenarios();
  generated(nReads, 5151);
  std::printf("differences %d\n", g_bad);
  return g_bad ? 1 : 0;
}
