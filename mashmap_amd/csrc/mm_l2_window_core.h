// mashmap_amd/csrc/mm_l2_window_core.h -- computeL2MappedRegions with windowLen != 0 (--noSplit, a read longer than segLength), the pieces
// that must be literal, stated once.
//
//   Map::computeL2MappedRegions   src/map/include/computeMap.hpp:1276-1451
//   SlideMapper                   src/map/include/slidingMap.hpp:125-211      WinSlide
//   hash_to_freq (:1310)          as a presence rule                          mm_win_present
//   evaluation, runs, the join    :1376-1449                                  WinRuns
//   one entering record           :1342-1373                                  mm_win_enter
//   a candidate, record by record                                             mm_win_candidate
//
// Shared by k_l2_window_wave (mm_l2.hip: one wave per candidate, this state in LDS) and by the CPU check (tests/hostlogic/l2_window_check.cpp),
// which runs mm_win_candidate beside the oracle under a host sanitizer.  Compiles for the host (g++) and for the device (hipcc).
//
// The presence rule.  The reference counts the open windows of a hash (hash_to_freq[h]) and lets a record into the heap and the SlideMapper
// only when it finds the count at 0; a later record of the same hash raises the count and is skipped (`continue`: no evaluation).  When the
// record that is in reaches the heap's front with wpos_end <= wpos(it) - windowLen, the loop at :1344-1357 decrements the count until it is
// 0 and pops the record, whatever the count was.  So the count never matters beyond zero / non-zero: per hash the state is "absent" or
// "present with record R", and at a slide record `it` the hash is present iff an entry exists and R.wpos_end > wpos(it) - windowLen (the heap
// is a min-heap on wpos_end and every front at or below that threshold is popped before the insert is looked at).  In the set-up loop
// (:1323-1338) nothing is evicted: there "present" is "an entry exists".  A record that enters stores its own wpos_end as the entry.
//
// Evictions.  The reference evicts at EVERY slide record, also at one the gate then skips.  Here only entering records do any work, so the
// evictions a skipped record would have made are made by the next entering one -- the pops come in the same order, no push lies between --
// but in two parts: up to the previous slide record's threshold first, because the strand of a closing run is taken from the votes before
// the record's OWN evictions (:1342), then up to its own.  mm_win_finish makes those still due behind the last entering record.
#pragma once
#include "mm_heap.h"
#include <stdint.h>

#define MM_WIN_NONE (-2147483647 - 1)                 // "no slide record yet" for prevSlideW

struct WinCell { int32_t cnt; int16_t vote; int16_t active; };     // num_before_inc, accumulated strand_vote, active (slidingMap.hpp:40-50)
struct WinLocus { int32_t start, end, shared, strand; };

// a located record: 1-based lower_bound position j of its hash in the query sketch (0: beyond the last hash, no effect on the SlideMapper),
// whether the hash equals q[j], and the vote of a matching insert (query strand x reference strand) + 1
MM_HD uint32_t mm_win_loc(int j, bool match, int vote) { return (uint32_t)j | (match ? 0x10000u : 0u) | ((uint32_t)(vote + 1) << 17); }
MM_HD int mm_win_loc_j(uint32_t loc) { return (int)(loc & 0xFFFFu); }
MM_HD bool mm_win_loc_match(uint32_t loc) { return (loc & 0x10000u) != 0; }
MM_HD int mm_win_loc_vote(uint32_t loc) { return (int)((loc >> 17) & 3u) - 1; }
// lower_bound of h in the ascending sketch q[0, S), as a located record (slidingMap.hpp:128-131)
MM_HD uint32_t mm_win_locate(const uint64_t* q, const int8_t* qs, int S, uint64_t h, bool revRef) {
  int lo = 0, hi = S;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (q[mid] < h) lo = mid + 1; else hi = mid; }
  if (lo >= S) return 0u;
  return mm_win_loc(lo + 1, q[lo] == h, revRef ? -(int)qs[lo] : (int)qs[lo]);
}

// an open record in the heap: wpos_end in the high word (the heap's order, heap_cmp :1299), its located form in the low one, so that the
// eviction needs no second search of the sketch
MM_HD uint64_t mm_win_open(int wend, uint32_t loc) { return ((uint64_t)(uint32_t)wend << 32) | loc; }
MM_HD int mm_win_open_end(uint64_t e) { return (int)(uint32_t)(e >> 32); }
struct WinLater { MM_HD bool operator()(uint64_t a, uint64_t b) const { return mm_win_open_end(a) > mm_win_open_end(b); } };   // min-heap on wpos_end

// hash h is open at this record: see "the presence rule" above
MM_HD bool mm_win_present(bool exists, int entryEnd, bool setup, int wpos, int W) { return exists && (setup || entryEnd > wpos - W); }

// SlideMapper on located records.  cell[0 .. S]: cell[0] = {0, 0, 0}, cell[1 .. S] = {1, 0, 0} (SlideMapper::init, :103-121), set by the caller
struct WinSlide {
  WinCell* cell; int S, pivot, pivRank, shared, votes;
  MM_HD void start(WinCell* cells, int S_) { cell = cells; S = S_; pivot = S_; pivRank = S_; shared = 0; votes = 0; }
  MM_HD void insert(uint32_t loc) {                                // insert_minmer (:125-165)
    const int j = mm_win_loc_j(loc);
    if (j == 0) return;
    WinCell x = cell[j];
    if (mm_win_loc_match(loc)) {
      x.active = 1; x.vote = (int16_t)(x.vote + mm_win_loc_vote(loc));
      cell[j] = x;
      if (j <= pivot) { shared++; votes += x.vote; }
    } else {
      x.cnt++; cell[j] = x;
      if (j <= pivot) pivRank++;
      if (pivRank > S) { const WinCell pc = cell[pivot]; shared -= pc.active; votes -= pc.vote; pivRank -= pc.cnt; pivot--; }
    }
  }
  MM_HD void remove(uint32_t loc) {                                // delete_minmer (:171-211)
    const int j = mm_win_loc_j(loc);
    if (j == 0) return;
    WinCell x = cell[j];
    if (mm_win_loc_match(loc)) {
      if (j <= pivot) { shared--; votes -= x.vote; }
      x.active = 0; x.vote = 0; cell[j] = x;
    } else {
      x.cnt--; cell[j] = x;
      if (j <= pivot) pivRank--;
      if (pivot + 1 <= S && pivRank + cell[pivot + 1].cnt <= S) { pivot++; const WinCell pc = cell[pivot]; shared += pc.active; votes += pc.vote; pivRank += pc.cnt; }
    }
  }
};

// best-position bookkeeping (:1376-1449): the loci of the best shared count so far, joined when closer than segLength.  `slots` holds
// the closed loci but the last, which stays in `pend` (a later run may extend it): up to locap + 1 loci.  A locus that finds no slot
// sets `overflow`, which a better count clears together with the loci (l2_vec_out.clear()).
struct WinRuns {
  int segLength, W, bestShared, curStart, curEnd, curShared, nFlushed, locap;
  bool inRun, havePend, overflow;
  WinLocus pend; WinLocus* slots;
  MM_HD void start(int segLength_, int W_, WinLocus* slots_, int locap_) {
    segLength = segLength_; W = W_; bestShared = 1; curStart = curEnd = curShared = 0; nFlushed = 0; locap = locap_;
    inRun = havePend = overflow = false; pend = WinLocus{0, 0, 0, 0}; slots = slots_;
  }
  MM_HD void close_run(int strand) {                               // :1417-1426 / :1440-1449
    if (!havePend || pend.end + segLength < curStart) {
      if (havePend) { if (nFlushed < locap) slots[nFlushed] = pend; else overflow = true; nFlushed++; }
      pend.start = curStart; pend.end = curEnd; pend.shared = curShared; pend.strand = strand; havePend = true;
    } else pend.end = curEnd;
  }
  // behind an entering slide record at wpos: `shared` after its insert, nextW = wpos of the index record behind it in the same contig
  // (its own at the contig's end, :1387-1390), prevVotes = strand_votes before the record's own evictions (:1342)
  MM_HD void evaluate(int shared, int wpos, int nextW, int prevVotes) {
    if (shared > bestShared) {
      nFlushed = 0; havePend = false; overflow = false;
      inRun = true; bestShared = shared; curShared = shared;
      curStart = wpos;                                             // (the one place without "- windowLen" in the reference, :1386)
      curEnd = nextW - W;
    } else if (shared == bestShared) {
      if (!inRun) { curShared = shared; curStart = wpos - W; }
      inRun = true;
      curEnd = nextW - W;
    } else {
      if (inRun) { curEnd = nextW - W; close_run(prevVotes >= 0 ? 1 : -1); curStart = curEnd = curShared = 0; }
      inRun = false;
    }
  }
  MM_HD int total() const { return nFlushed + (havePend ? 1 : 0); }
  MM_HD WinLocus locus(int k) const { return k < nFlushed ? slots[k] : pend; }
};

// every open record whose window ended at or before `threshold` leaves the SlideMapper and the heap, front first
MM_HD void mm_win_evict(WinSlide& sm, uint64_t* heap, int& nHeap, int threshold) {
  while (nHeap > 0 && mm_win_open_end(heap[0]) <= threshold) {
    sm.remove((uint32_t)heap[0]);
    mm_pop_heap(heap, nHeap, WinLater()); nHeap--;
  }
}

// One record that the gate lets in.  setup: it lies before rangeStart (:1323-1338: no eviction, no evaluation); prevSlideW: wpos of the
// slide record before it, entering or not (MM_WIN_NONE: there is none).  false: the heap is full (checked before the write) -- the
// candidate cannot be finished with this state.
MM_HD bool mm_win_enter(WinSlide& sm, uint64_t* heap, int& nHeap, int heapCap, WinRuns& rn, bool setup, int wpos, int wend, uint32_t loc, int nextW, int prevSlideW) {
  int prevVotes = 0;
  if (!setup) {
    if (prevSlideW != MM_WIN_NONE) mm_win_evict(sm, heap, nHeap, prevSlideW - rn.W);     // what the skipped records before this one evicted
    prevVotes = sm.votes;
    mm_win_evict(sm, heap, nHeap, wpos - rn.W);
  }
  if (nHeap >= heapCap) return false;
  sm.insert(loc);
  heap[nHeap] = mm_win_open(wend, loc); nHeap++;
  mm_heap_push(heap, nHeap - 1, 0, heap[nHeap - 1], WinLater());
  if (!setup) rn.evaluate(sm.shared, wpos, nextW, prevVotes);
  return true;
}

// the end of a candidate: the evictions of the slide records behind the last entering one, then the open run (:1435-1450)
MM_HD void mm_win_finish(WinSlide& sm, uint64_t* heap, int& nHeap, WinRuns& rn, int lastSlideW) {
  if (lastSlideW != MM_WIN_NONE) mm_win_evict(sm, heap, nHeap, lastSlideW - rn.W);
  if (rn.inRun) rn.close_run(sm.votes >= 0 ? 1 : -1);
}

// The serial driver.  Records: the contig's index records from lower_bound(rangeStart - segLength - 1) on, in index order (n of them;
// the walk ends by itself behind rangeEnd + W).  Presence: find(h, end&) -> an entry exists, set(h, end).  Returns false when the heap
// outgrew heapCap.  counts (may be null): walked, entering, skipped, re-entries after an expiry, largest heap.
struct WinRecord { uint64_t hash; int32_t wpos, wend; int32_t rev; };
template <class Presence>
MM_HD bool mm_win_candidate(const WinRecord* rec, long long n, const uint64_t* q, const int8_t* qs, int S, int rangeStart, int rangeEnd, int segLength, int W,
                            WinCell* cells, uint64_t* heap, int heapCap, Presence& present, WinRuns& rn, WinLocus* slots, int locap, long long* counts) {
  cells[0] = WinCell{0, 0, 0};
  for (int p = 1; p <= S; p++) cells[p] = WinCell{1, 0, 0};
  WinSlide sm; sm.start(cells, S);
  rn.start(segLength, W, slots, locap);
  int nHeap = 0, lastSlideW = MM_WIN_NONE;
  for (long long i = 0; i < n && (long long)rec[i].wpos <= (long long)rangeEnd + W; i++) {
    const WinRecord& r = rec[i];
    const bool setup = r.wpos < rangeStart;
    if (setup && !(r.wend > rangeStart)) continue;
    if (counts) counts[0]++;
    const int prevSlideW = lastSlideW;
    if (!setup) lastSlideW = r.wpos;
    if (W > 0) {
      int end = 0;
      const bool exists = present.find(r.hash, end);
      if (mm_win_present(exists, end, setup, r.wpos, W)) { if (counts) counts[2]++; continue; }
      if (counts && exists) counts[3]++;
      present.set(r.hash, r.wend);
    }
    if (counts) counts[1]++;
    const int nextW = i + 1 < n ? rec[i + 1].wpos : r.wpos;
    if (!mm_win_enter(sm, heap, nHeap, heapCap, rn, setup, r.wpos, r.wend, mm_win_locate(q, qs, S, r.hash, r.rev != 0), nextW, prevSlideW)) return false;
    if (counts && nHeap > counts[4]) counts[4] = nHeap;
  }
  mm_win_finish(sm, heap, nHeap, rn, lastSlideW);
  return true;
}
