// tests/hostlogic/pass_state_check.cpp -- mm_pass_state.h (the bookkeeping of a mapping pass: its report, what a sized pass leaves, the
// steady-state decisions of mm_launch_map, the sizing rules, the route predicates) on the host.  Built with -fsanitize=address,undefined
// and run by tests/test_pass_state.py.
//
//   pass_state_check     prints "ok <what>" per group of checks that passed, "FAIL ..." (with a non-zero status) for a check that did not,
//                        and "rule <name> <input> <value>" for every sizing rule at every input: tests/test_pass_state.py compares those
//                        with the restatement the GPU tests use (tests/mmutil.py)
#include <cstdio>
#include <type_traits>
#include "../../include/mashmap_hip.h"
#include "../../mashmap_amd/csrc/mm_pass_state.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
static void done(const char* what, int before) { if (failures == before) printf("ok %s\n", what); }

static_assert(std::is_trivially_copyable<PassReport>::value && std::is_trivially_copyable<SizedPass>::value && std::is_trivially_copyable<PassTotals>::value,
              "the three structs are assigned and reset as wholes");

// ---- the structs ---------------------------------------------------------------------------------------------------------------------
static void structs() {
  const int f0 = failures;
  const PassReport r{};
  CHECK(r.nL1 == 0 && r.nL2 == 0 && r.nMappings == 0 && r.nSyncs == 0 && !r.lastSteady && r.redoCause == 0 && r.lastHard == 0 && r.lastOps == 0 && r.lastBig == 0 && r.lastMid == 0, "PassReport{}");
  const SizedPass s{};
  CHECK(!s.steady.steadyOk && s.steady.steadyFails == 0 && s.steady.sizedFrags == 0 && s.steady.candCap == 0 && s.steady.l2Chunks == 1 && s.steady.prevLocap == 0, "SizedPass{}.steady");
  CHECK(!s.seen.midKnown && s.seen.prevBig + s.seen.prevLit + s.seen.prevMid + s.seen.grpOffered + s.seen.grpFused + s.seen.lwCands + s.seen.lwLit + s.seen.winCands + s.seen.winLit == 0, "SizedPass{}.seen");
  const PassTotals t{};
  CHECK(t.nPasses == 0 && t.nSteadyPasses == 0 && t.nRedone == 0, "PassTotals{}");
  done("structs", f0);
}

// ---- the steady-state decisions: the expected values are mm_launch_map's lines before the header existed, read literally --------------
// a sized pass as mm_launch_map ends it; `chunks` is what l2_plan left in l2Chunks on the way
static void sized(SizedPass& S, const Options& o, size_t nF, bool ok, bool never, size_t nL1, size_t chunks) {
  S.steady.l2Chunks = chunks;
  mm_sized_pass_done(S.steady, mm_frag_cap(o, nF), ok, never, nL1);
}
static bool eligible(const SizedPass& S, size_t nF) { return mm_may_try_steady(S.steady, nF, false); }

static void steady_state() {
  const int f0 = failures;
  const Options plain;
  {
    SizedPass S;
    CHECK(!eligible(S, 0) && !eligible(S, 1) && !eligible(S, 1000), "a fresh state is not eligible");
    sized(S, plain, 1000, true, false, 5, 1);
    CHECK(S.steady.sizedFrags == 1000 && S.steady.steadyOk, "sizedFrags %zu", S.steady.sizedFrags);
    CHECK(eligible(S, 1) && eligible(S, 1000) && eligible(S, 1100) && !eligible(S, 1101), "a tenth more fragments is the limit");
    CHECK(!mm_may_try_steady(S.steady, 1000, true), "never steady");
  }
  {                                                                       // a reservation larger than the batch
    Options o; o.reserveFrags = 1000;
    SizedPass S;
    sized(S, o, 10, true, false, 5, 1);
    CHECK(S.steady.sizedFrags == 1000 && eligible(S, 1100) && !eligible(S, 1101), "sizedFrags %zu", S.steady.sizedFrags);
    CHECK(mm_frag_cap(o, 999) == 1000 && mm_frag_cap(o, 1000) == 1000 && mm_frag_cap(o, 1001) == 1001 && mm_frag_cap(plain, 0) == 0, "mm_frag_cap");
  }
  {                                                                       // what keeps a sized pass from leaving the state eligible
    SizedPass S;
    sized(S, plain, 1000, true, false, 0, 1);  CHECK(!eligible(S, 1000) && S.steady.sizedFrags == 1000, "nL1 == 0");
    sized(S, plain, 1000, true, false, 5, 2);  CHECK(!eligible(S, 1000), "two chunks");
    sized(S, plain, 1000, true, true, 5, 1);   CHECK(!eligible(S, 1000), "never steady");
    sized(S, plain, 1000, false, false, 5, 1); CHECK(!eligible(S, 1000), "a failing rc");
    sized(S, plain, 1000, true, false, 5, 1);  CHECK(eligible(S, 1000), "and a good one behind them");
  }
  {                                                                       // a redone attempt, a pass that stood
    SizedPass S; PassTotals T; PassReport R;
    sized(S, plain, 1000, true, false, 5, 1);
    mm_steady_redone(S.steady, T);
    CHECK(!S.steady.steadyOk && S.steady.steadyFails == 1 && T.nRedone == 1 && T.nPasses == 0 && T.nSteadyPasses == 0 && !eligible(S, 1000), "redone: fails %d, redone %llu", S.steady.steadyFails, (unsigned long long)T.nRedone);
    CHECK(S.steady.sizedFrags == 1000 && S.steady.l2Chunks == 1, "a redone attempt touches nothing else");
    sized(S, plain, 1000, true, false, 5, 1);
    CHECK(eligible(S, 1000) && S.steady.steadyFails == 1, "eligible again behind a good sized pass");
    mm_steady_redone(S.steady, T);
    sized(S, plain, 1000, true, false, 5, 1);
    CHECK(S.steady.steadyFails == 2 && T.nRedone == 2 && eligible(S, 1000), "two in a row");
    mm_steady_stood(S.steady, R);
    CHECK(S.steady.steadyFails == 0 && S.steady.steadyOk && R.lastSteady && eligible(S, 1000), "a pass that stood");
  }
  {                                                                       // three redone attempts end the attempts
    SizedPass S; PassTotals T;
    for (int i = 0; i < 3; i++) {
      sized(S, plain, 1000, true, false, 5, 1);
      CHECK(eligible(S, 1000), "attempt %d", i);
      mm_steady_redone(S.steady, T);
    }
    sized(S, plain, 1000, true, false, 5, 1);
    CHECK(S.steady.steadyOk && S.steady.steadyFails == 3 && T.nRedone == 3 && !eligible(S, 1000) && !eligible(S, 1), "never eligible again");
    sized(S, plain, 2000, true, false, 5, 1);
    CHECK(!eligible(S, 2000), "... a further good sized pass notwithstanding");
  }
  done("steady_state", f0);
}

// ---- the grid guesses ------------------------------------------------------------------------------------------------------------------
static void grid_guesses() {
  const int f0 = failures;
  SizedPass::Seen s;
  CHECK(mm_mid_grid_guess(s, 1) == 1 && mm_mid_grid_guess(s, 5000) == 5000 && mm_mid_grid_guess(s, 0) == 1, "nothing known: every fragment (one block at least)");
  s.midKnown = true;
  CHECK(mm_mid_grid_guess(s, 5000) == 256 && mm_mid_grid_guess(s, 100) == 100 && mm_mid_grid_guess(s, 0) == 1, "prevMid 0");
  s.prevMid = 7;    CHECK(mm_mid_grid_guess(s, 5000) == 7 + 3 + 256 && mm_mid_grid_guess(s, 266) == 266 && mm_mid_grid_guess(s, 265) == 265, "prevMid 7");
  s.prevMid = 1000; CHECK(mm_mid_grid_guess(s, 5000) == 1756 && mm_mid_grid_guess(s, 1756) == 1756 && mm_mid_grid_guess(s, 1755) == 1755 && mm_mid_grid_guess(s, 1000) == 1000, "prevMid 1000");
  CHECK(mm_big_grid_guess(s, 5000) == 1024 && mm_big_grid_guess(s, 1000) == 1000 && mm_big_grid_guess(s, 0) == 0, "prevBig 0");
  s.prevBig = 7;    CHECK(mm_big_grid_guess(s, 5000) == 7 + 3 + 1024 && mm_big_grid_guess(s, 1034) == 1034 && mm_big_grid_guess(s, 1033) == 1033, "prevBig 7");
  s.prevBig = 4000; CHECK(mm_big_grid_guess(s, 10000) == 7024 && mm_big_grid_guess(s, 7023) == 7023 && mm_big_grid_guess(s, 4000) == 4000, "prevBig 4000");
  done("grid_guesses", f0);
}

// ---- the sizing rules: each against the arithmetic its call site carried, and printed for the Python side ----------------------------------
static void sizing_rules() {
  const int f0 = failures;
  const size_t R = 64, CAND = sizeof(mm_l1_candidate), REC = sizeof(mm_mapping);   // MM_L1_REGIONS (mm_map.hip)
  const size_t inputs[] = {0, 1, 7, 8, 63, 64, 1000, 1000000, ((size_t)1 << 31) + 5, 3072, 3073};
  for (const size_t n : inputs) {
    CHECK(mm_pts_cap0(n, false) == n * 8 + 65536 && mm_pts_cap0(n, true) == n * 128 + 4096, "pts_cap0 %zu", n);
    CHECK(mm_pts_cap_grown(n) == n + n / 8 + 4096, "pts_cap_grown %zu", n);
    CHECK(mm_l1_cap0(n) == n * 2 + 1024, "l1_cap0 %zu", n);
    CHECK(mm_region_cap(n, R) == (n + R - 1) / R + 64, "region_cap %zu", n);
    CHECK(mm_l1_cap_grown(n, R) == (n + n / 4 + 256) * R, "l1_cap_grown %zu", n);
    CHECK(mm_l1_bytes(n, R, CAND) == n * R * CAND + 64, "l1_bytes %zu", n);
    CHECK(mm_cand_cap(n) == n + n / 8 + 1024, "cand_cap %zu", n);
    CHECK(mm_loci_cap0(n) == n * 2 + 1024 && mm_loci_cap_grown(n) == n + n / 8 + 1024, "loci caps %zu", n);
    CHECK(mm_mappings_bytes(n, REC) == (n + n / 16) * REC + 4096 && mm_l2_ops_bytes(n) == (n + n / 16) * 4 + 256, "sixteenth %zu", n);
    const size_t regionCap = mm_region_cap(mm_l1_cap0(n), R);
    printf("rule pts_cap %zu %zu\n", n, mm_pts_cap0(n, false));
    printf("rule pts_cap_hbm %zu %zu\n", n, mm_pts_cap0(n, true));
    printf("rule pts_cap_grown %zu %zu\n", n, mm_pts_cap_grown(n));
    printf("rule region_cap %zu %zu\n", n, regionCap);
    printf("rule l1_cap_grown %zu %zu\n", n, mm_l1_cap_grown(n, R));
    printf("rule dense_bytes %zu %zu\n", n, mm_l1_bytes(regionCap, R, CAND));
    printf("rule cand_cap %zu %zu\n", n, mm_cand_cap(n));
    printf("rule loci_cap0 %zu %zu\n", n, mm_loci_cap0(mm_cand_cap(n)));
    printf("rule loci_cap_grown %zu %zu\n", n, mm_loci_cap_grown(n));
    printf("rule map_bytes %zu %zu\n", n, mm_mappings_bytes(n, REC));
    printf("rule ops_bytes %zu %zu\n", n, mm_l2_ops_bytes(n));
  }
  done("sizing_rules", f0);
}

// ---- the route predicates: every combination against the three expressions of the issue that asked for them --------------------------------
static void predicates() {
  const int f0 = failures;
  for (int m = 0; m < 64; m++) {
    const bool keepPoints = m & 1, skipPrefix = m & 2, windowed = m & 4, largeSketch = m & 8, bit1 = m & 16, bit0 = m & 32;
    Options o; o.keepPoints = keepPoints; o.l2LargeWave = (bit1 ? 2 : 0) | (bit0 ? 1 : 0);
    const int sketchSize = largeSketch ? MM_LDS_MAX_SKETCH + 1 : MM_LDS_MAX_SKETCH;
    const bool hbm = keepPoints || skipPrefix || windowed;
    const bool literal = windowed || sketchSize > 8190 || (o.l2LargeWave & 2);
    CHECK(mm_points_in_hbm(o, skipPrefix, windowed) == hbm, "points in HBM, combination %d", m);
    CHECK(mm_l2_literal_route(o, windowed, sketchSize) == literal, "literal L2 route, combination %d", m);
    CHECK(mm_never_steady(o, skipPrefix, windowed, sketchSize) == (hbm || literal), "never steady, combination %d", m);
  }
  Options all; all.keepFiltered = all.keepFullIndex = all.l1GroupStream = all.l1GroupFused = all.l2WindowWave = all.chainLong = true; all.reserveFrags = 1 << 20; all.l2LargeWave = 1;
  CHECK(!mm_never_steady(all, false, false, 1) && !mm_never_steady(all, false, false, MM_LDS_MAX_SKETCH), "no other option decides a route");
  done("predicates", f0);
}

int main() {
  structs();
  steady_state();
  grid_guesses();
  sizing_rules();
  predicates();
  printf("mismatches %d\n", failures);
  return failures ? 1 : 0;
}
