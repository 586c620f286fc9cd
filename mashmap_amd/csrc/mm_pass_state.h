// mashmap_amd/csrc/mm_pass_state.h -- the host bookkeeping of a mapping pass (mm_launch_map): what mm_set_option
// set, what the last pass reports, what the last SIZED pass left for the steady-state passes behind it, the context's totals; the
// steady-state decisions and the sizing rules of a sized pass as functions.  No HIP: tests/hostlogic/pass_state_check.cpp runs all of it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define MM_LDS_MAX_SKETCH 8190             // beyond: the global-memory sketch kernel and the literal L2 kernels (any size up to MM_MAX_SKETCH)

struct Options {                            // written by mm_set_option alone
  bool keepPoints = false;                  // MM_OPT_KEEP_POINTS: route every fragment through the HBM point list
  bool keepFiltered = false;                // MM_OPT_KEEP_POINTS = 2: ... and k_filter_points runs on them as it does on a queued fragment's (mm_points_download returns what it leaves)
  bool keepFullIndex = false;               // MM_OPT_KEEP_FULL_INDEX: hMinmersAll keeps minmerIndex before dropFreqSeedSet (--saveIndex)
  size_t reserveFrags = 0;                  // MM_OPT_RESERVE_FRAGMENTS: fragments of the largest batch the caller will upload; sized passes size for it
  bool l1GroupStream = false;               // MM_OPT_L1_GROUP_STREAM: under MM_FLAG_SKIP_PREFIX the queued fragments go to the grouped k_l1_stream first
  bool l1GroupFused = false;                // MM_OPT_L1_GROUP_FUSED: ... through k_lookup_groups first; the HBM point path takes what it hands over
  bool l2WindowWave = false;                // MM_OPT_L2_WINDOW_WAVE: the windowed L2 stage on k_l2_window_wave first, the literal k_l2_window takes what it hands over
  int l2LargeWave = 0;                      // MM_OPT_L2_LARGE_WAVE: bit 0: split batches on the literal L2 route go to k_l2_large_wave first; bit 1: they take that route at any sketch size
  bool sketchLarge = false;                 // MM_OPT_SKETCH_LARGE: sketches beyond MM_LDS_MAX_SKETCH on k_sketch_large instead of k_sketch_global
  bool chainLong = false;                   // MM_OPT_CHAIN_LONG: reads of 17 .. 512 records are chained on the device as well
  bool chainModes = false;                  // MM_OPT_CHAIN_MODES: mm_chain_reads takes a context created with MM_FLAG_SKIP_PREFIX and / or MM_FLAG_NO_SPLIT
};

// the last mm_map_fragments, and nothing older: PassReport{} at the top of mm_launch_map (mm_pass_stats, mm_pass_redo_cause, mm_result_counts)
struct PassReport {
  size_t nL1 = 0, nL2 = 0, nMappings = 0;   // L1 candidates, L2 loci, candidate mappings
  size_t nSyncs = 0;                        // host synchronisations inside it (MM_SYNC)
  bool lastSteady = false;                  // it went through as a steady-state pass
  uint64_t redoCause = 0;                   // MM_REDO_* of the steady attempt it had redone, 0 when it had none
  size_t lastHard = 0;                      // fragments the fast sketch kernel handed to the hard list
  size_t lastOps = 0;                       // L2 stream entries reserved (split route)
  size_t lastBig = 0;                       // fragments queued for the HBM point path (a steady-state pass cannot count them: the last sized pass's figure)
  size_t lastMid = 0;                       // fragments k_lookup_mid took (sized pass only)
};

// the last SIZED pass.  Never wiped: a sized pass reads what the one before it left (the grid guesses, candCap) while it runs.
struct SizedPass {
  struct Seen {                             // what the getters report "as of the last sized pass"; map_pass assigns it as a whole ...
    size_t prevBig = 0, prevLit = 0;        // fragments queued for the HBM point path; of those, the ones the literal k_l1_sweep took (mm_pass_l1_literal)
    size_t prevMid = 0; bool midKnown = false;   // fragments k_lookup_mid took; whether it ran
    size_t grpOffered = 0, grpFused = 0;    // fragments offered to k_lookup_groups and those it finished (mm_pass_l1_group_fused); 0 / 0 when it was not launched
    size_t lwCands = 0, lwLit = 0;          // ... and mm_launch_l2_window fills these four behind that: candidates of a split batch on the literal L2 route and
    size_t winCands = 0, winLit = 0;        // those k_l2_window swept (mm_pass_l2_large); the same of a windowed batch (mm_pass_l2_window)
  } seen;
  struct Steady {                           // what steady-state passes run against
    bool steadyOk = false;                  // the last sized pass went through and left every buffer sized
    int steadyFails = 0;                    // steady attempts redone since the last one that stood
    size_t sizedFrags = 0;                  // fragments the per-fragment buffers were sized for
    size_t candCap = 0;                     // candidates the candidate-indexed staging holds (l2_extents)
    size_t l2Chunks = 1;                    // chunks its L2 streams went through in (l2_plan)
    int prevLocap = 0;                      // staging slots per candidate its L2 sweeps ended with
  } steady;
};

struct PassTotals { uint64_t nPasses = 0, nSteadyPasses = 0, nRedone = 0; };   // of the context: mm_map_fragments calls, those that went through steady, steady attempts redone

// ---- routes -------------------------------------------------------------------------------------------------------------------------
// every fragment's interval points go to HBM (no fused lookup, no k_lookup_mid)
constexpr bool mm_points_in_hbm(const Options& o, bool skipPrefix, bool windowed) { return o.keepPoints || skipPrefix || windowed; }
// L2 on the literal kernels (mm_launch_l2_window): fragments longer than segLength, a sketch no LDS state holds, or bit 1 of MM_OPT_L2_LARGE_WAVE
constexpr bool mm_l2_literal_route(const Options& o, bool windowed, int sketchSize) { return windowed || sketchSize > MM_LDS_MAX_SKETCH || (o.l2LargeWave & 2) != 0; }
// either: such a context's passes are all sized ones
constexpr bool mm_never_steady(const Options& o, bool skipPrefix, bool windowed, int sketchSize) {
  return mm_points_in_hbm(o, skipPrefix, windowed) || mm_l2_literal_route(o, windowed, sketchSize);
}

// ---- the steady-state decisions of mm_launch_map -----------------------------------------------------------------------------------------
constexpr size_t mm_frag_cap(const Options& o, size_t nF) { return nF > o.reserveFrags ? nF : o.reserveFrags; }   // fragments to size per-fragment buffers for
// (a batch with a tenth more fragments than the buffers were sized for would only fail and be redone: it is sized right away; three
// redone attempts without one that stood: this context's batches keep outgrowing what the one before left, no further attempt)
constexpr bool mm_may_try_steady(const SizedPass::Steady& s, size_t nF, bool neverSteady) {
  return s.steadyOk && s.steadyFails < 3 && !neverSteady && nF <= s.sizedFrags + s.sizedFrags / 10;
}
inline void mm_steady_redone(SizedPass::Steady& s, PassTotals& t) { s.steadyOk = false; s.steadyFails++; t.nRedone++; }
inline void mm_steady_stood(SizedPass::Steady& s, PassReport& r) { r.lastSteady = true; s.steadyFails = 0; }
// the end of a sized pass (a batch whose L2 streams go through in chunks needs the host between them)
inline void mm_sized_pass_done(SizedPass::Steady& s, size_t fragCap, bool ok, bool neverSteady, size_t nL1) {
  s.sizedFrags = fragCap;
  s.steadyOk = ok && !neverSteady && nL1 > 0 && s.l2Chunks == 1;
}
// grids over lists whose lengths stay on the device (the kernels walk them with whatever grid they get): what the last sized pass saw
// plus a half; for k_lookup_mid every fragment while nothing is known
constexpr size_t mm_min(size_t a, size_t b) { return a < b ? a : b; }
constexpr size_t mm_mid_grid_guess(const SizedPass::Seen& s, size_t nF) {
  const size_t g = mm_min(s.midKnown ? s.prevMid + s.prevMid / 2 + 256 : nF, nF);
  return g ? g : 1;
}
constexpr size_t mm_big_grid_guess(const SizedPass::Seen& s, size_t nF) { return mm_min(s.prevBig + s.prevBig / 2 + 1024, nF); }

// ---- the sizing rules of a sized pass (tests/mmutil.py restates them for the GPU tests).  Counts are already mm_scaled where that applies.
constexpr size_t mm_pts_cap0(size_t cF, bool pointsInHbm) { return pointsInHbm ? cF * 128 + 4096 : cF * 8 + 65536; }   // interval points to start with
constexpr size_t mm_pts_cap_grown(size_t need) { return need + need / 8 + 4096; }                                      // ... after an overflow
constexpr size_t mm_l1_cap0(size_t cF) { return cF * 2 + 1024; }                                                       // L1 candidates to start with
constexpr size_t mm_region_cap(size_t l1Cap, size_t regions) { return (l1Cap + regions - 1) / regions + 64; }          // ... per output region of the fused kernels
constexpr size_t mm_l1_cap_grown(size_t fullest, size_t regions) { return (fullest + fullest / 4 + 256) * regions; }   // ... after a region overflowed
constexpr size_t mm_l1_bytes(size_t regionCap, size_t regions, size_t candBytes) { return regionCap * regions * candBytes + 64; }   // dL1, dL1b
constexpr size_t mm_cand_cap(size_t nL1) { return nL1 + nL1 / 8 + 1024; }                        // candidate-indexed staging; the dense L1 buffer after an overflow
constexpr size_t mm_loci_cap0(size_t nCand) { return nCand * 2 + 1024; }                         // L2 loci to start with
constexpr size_t mm_loci_cap_grown(size_t need) { return need + need / 8 + 1024; }               // ... after an overflow
// a sixteenth of head room for the steady-state passes behind this one: candidate mappings (dMappings), L2 stream entries (dL2Ops)
constexpr size_t mm_mappings_bytes(size_t total, size_t recBytes) { return (total + total / 16) * recBytes + 4096; }
constexpr size_t mm_l2_ops_bytes(size_t ops) { return (ops + ops / 16) * 4 + 256; }
