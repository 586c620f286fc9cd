// mashmap_amd/csrc/mm_stage_plan.h -- StageRing: where the packed pieces sent ahead of their upload lie in the staging area (mm_ctx::stage).
// Host arithmetic only, no HIP: the callers (mm_api.hip, mm_text.hip) size the area, copy the words and order the streams;
// tests/hostlogic/stage_check.cpp runs these rules against a byte map.
//
// A piece is [codes | mask] of nPacked bases, bytes(nPacked) long, at `off` in the area, and is known by its two host pointers and its
// length.  Three producers place and commit (mm_reads_prefetch_packed, mm_reads_prefetch_packed_append, mm_text_pack -- the last on a
// reader thread), one consumer matches and retires (the packed upload), all under Staging::prefetchMu.  The one invariant: from its commit
// to its retirement (or a clear) a piece is overlapped by no other and does not move.  The area is used as a ring: pieces leave in the
// order they came, so the next one goes behind the newest, or to the front again once the oldest have left.  It may grow only while the
// ring is empty.
#pragma once
#include <stddef.h>
#include <vector>

struct StageRing {
  struct Piece { const void* b2; const void* nm; size_t nPacked; size_t off; };
  static constexpr size_t npos = ~(size_t)0;
  static constexpr size_t kRunOff = 64;         // bytes kept free behind a piece
  std::vector<Piece> pieces;                    // oldest first
  size_t next = 0;                              // after place(): where the piece goes; after commit(): the byte behind the newest piece

  static size_t bytes(size_t nPacked) { return nPacked / 4 + nPacked / 8; }
  // null, or why a piece of this length is not taken
  static const char* refusal(size_t nPacked) { return nPacked % 32 ? "mm_reads_prefetch_packed: the packed length of a batch is a multiple of 32 bases" : nullptr; }
  // what an empty ring asks the area to hold
  static size_t want(size_t nPacked, size_t reserve) { const size_t a = bytes(nPacked), b = bytes(reserve); return (a > b ? a : b) + kRunOff; }

  bool empty() const { return pieces.empty(); }
  // true: `next` is the piece's offset in an area of areaBytes.  false: no room under the live pieces, nothing changed
  bool place(size_t nPacked, size_t areaBytes) {
    const size_t b = bytes(nPacked);
    auto fits = [&](size_t off) {
      if (off + b + kRunOff > areaBytes) return false;
      for (const Piece& q : pieces) if (off < q.off + bytes(q.nPacked) && q.off < off + b) return false;
      return true;
    };
    const size_t behind = pieces.empty() ? 0 : next;
    if (fits(behind)) next = behind; else if (fits(0)) next = 0; else return false;
    return true;
  }
  // the piece placed last is on its way to `next`
  void commit(const void* b2, const void* nm, size_t nPacked) { pieces.push_back(Piece{b2, nm, nPacked, next}); next += bytes(nPacked); }
  // the oldest piece with this key that `used` (a flag per piece) does not name yet, or npos
  size_t match(const void* b2, const void* nm, size_t nPacked, const std::vector<char>& used) const {
    for (size_t q = 0; q < pieces.size(); q++)
      if (!used[q] && pieces[q].b2 == b2 && pieces[q].nm == nm && pieces[q].nPacked == nPacked) return q;
    return npos;
  }
  // the pieces `used` names leave; the others stay where and in the order they are
  void retire(const std::vector<char>& used) {
    size_t n = 0;
    for (size_t q = 0; q < pieces.size(); q++) if (!used[q]) pieces[n++] = pieces[q];
    pieces.resize(n);
  }
  void clear() { pieces.clear(); next = 0; }
};
