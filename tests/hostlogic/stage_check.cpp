// tests/hostlogic/stage_check.cpp -- StageRing (mashmap_amd/csrc/mm_stage_plan.h), the bookkeeping of the staging area of packed pieces,
// on the host: fixed cases for each of its rules, then seeded random sequences of place / commit / match / retire / clear against a
// byte map of the area -- after every step no two live pieces overlap, every piece lies inside [0, areaBytes - 64], no live piece has
// moved, and place() refuses exactly when neither "behind the newest piece" nor offset 0 is free in the map.  Built with
// -fsanitize=address,undefined and run by tests/test_stage_plan.py.
//
//   stage_check [sequences] [seed]   prints "ok <case>" per case that passed, "FAIL ..." for a check that did not, then "cases <n>",
//                                    "mismatches <n>" and "sequences <n> steps <n> placed <n> refused <n> wrapped <n> matched <n> retired <n>
//                                    cleared <n>"; the status is non-zero on any mismatch
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../mashmap_amd/csrc/mm_stage_plan.h"

static int failures = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
static void done(const char* name, int before) { cases++; if (failures == before) printf("ok %s\n", name); }

static uint32_t hostWords[16];                                   // the keys: addresses only, never read
static const void* key(int i) { return &hostWords[i]; }
static bool same(const StageRing& a, const StageRing& b) {
  if (a.next != b.next || a.pieces.size() != b.pieces.size()) return false;
  for (size_t i = 0; i < a.pieces.size(); i++)
    if (a.pieces[i].b2 != b.pieces[i].b2 || a.pieces[i].nm != b.pieces[i].nm || a.pieces[i].nPacked != b.pieces[i].nPacked || a.pieces[i].off != b.pieces[i].off) return false;
  return true;
}
// place and commit, as the producers do; the offset, or npos when the ring refuses
static size_t add(StageRing& r, int k, size_t nPacked, size_t area) {
  if (!r.place(nPacked, area)) return StageRing::npos;
  r.commit(key(k), key(k + 1), nPacked);
  return r.pieces.back().off;
}

// ---- the fixed cases ---------------------------------------------------------------------------------------------------------------
static void empty_ring_wants() {
  const int f0 = failures;
  CHECK(StageRing::bytes(32) == 12 && StageRing::bytes(512) == 192 && StageRing::bytes(0) == 0, "a piece is a quarter of its bases in codes and an eighth in mask bytes");
  CHECK(StageRing::want(512, 0) == 192 + 64 && StageRing::want(512, 256) == 192 + 64, "the piece sets the size: %zu", StageRing::want(512, 256));
  CHECK(StageRing::want(64, 512) == 192 + 64 && StageRing::want(0, 512) == 192 + 64, "the reserve sets the size: %zu", StageRing::want(64, 512));
  StageRing r;
  CHECK(r.empty() && r.next == 0, "a new ring is empty");
  CHECK(add(r, 0, 512, StageRing::want(512, 0)) == 0, "an area of what the empty ring wants takes the piece at 0");
  CHECK(!r.empty() && r.next == 192, "the next piece goes behind it: %zu", r.next);
  done("empty_ring_wants", f0);
}

static void fills_retires_wraps() {
  const int f0 = failures;
  const size_t area = 3 * 96 + 64;                               // three pieces of 256 bases and the run-off
  StageRing r;
  CHECK(add(r, 0, 256, area) == 0 && add(r, 2, 256, area) == 96 && add(r, 4, 256, area) == 192, "three pieces end to end");
  StageRing before = r;
  CHECK(add(r, 6, 256, area) == StageRing::npos && same(r, before), "a fourth does not fit while all three are live");
  std::vector<char> used(3, 0);
  CHECK(r.match(key(0), key(1), 256, used) == 0, "the oldest is matched");
  used[0] = 1;
  r.retire(used);
  CHECK(r.pieces.size() == 2 && r.pieces[0].off == 96 && r.pieces[1].off == 192 && r.next == 288, "the two others stay where they are");
  CHECK(add(r, 6, 256, area) == 0, "the next piece goes to offset 0");
  CHECK(r.next == 96 && add(r, 8, 32, area) == StageRing::npos, "behind it lies the second piece, still live");
  done("fills_retires_wraps", f0);
}

static void refusal_changes_nothing() {
  const int f0 = failures;
  const size_t area = 300;
  StageRing r;
  CHECK(add(r, 0, 512, area) == 0, "setup");                     // [0, 192)
  const StageRing before = r;
  CHECK(!r.place(128, area) && same(r, before), "192 + 48 + 64 > 300 behind, and offset 0 is taken");
  CHECK(r.place(96, area) && r.next == 192, "192 + 36 + 64 <= 300: the run-off counts");
  CHECK(!r.place(512, 192 + 63) && r.place(512, 192 + 64) == false, "a live piece at 0 refuses a second of its size anywhere");
  StageRing none;
  CHECK(!none.place(512, 192 + 63) && none.next == 0 && none.empty(), "an empty ring refuses what the area cannot hold");
  none.next = 40;                                                // (as a retire leaves it)
  CHECK(none.place(512, 192 + 64) && none.next == 0, "an empty ring starts at 0");
  done("refusal_changes_nothing", f0);
}

static void equal_pieces_match_once_each() {
  const int f0 = failures;
  StageRing r;
  CHECK(add(r, 0, 64, 400) == 0 && add(r, 2, 64, 400) == 24 && add(r, 0, 64, 400) == 48, "setup: the first and third carry the same key");
  std::vector<char> used(3, 0);
  size_t q = r.match(key(0), key(1), 64, used);
  CHECK(q == 0, "first match %zu", q);
  used[q] = 1;
  q = r.match(key(0), key(1), 64, used);
  CHECK(q == 2, "second match %zu", q);
  used[q] = 1;
  CHECK(r.match(key(0), key(1), 64, used) == StageRing::npos, "no third");
  CHECK(r.match(key(0), key(1), 96, used) == StageRing::npos && r.match(key(0), key(3), 64, used) == StageRing::npos && r.match(key(2), key(1), 64, used) == StageRing::npos,
        "another length or either pointer another: no match");
  CHECK(r.match(key(2), key(3), 64, used) == 1, "the one in between");
  done("equal_pieces_match_once_each", f0);
}

static void retire_keeps_order() {
  const int f0 = failures;
  StageRing r;
  for (int i = 0; i < 5; i++) CHECK(add(r, 2 * i, 32, 400) == (size_t)i * 12, "setup");
  std::vector<char> used = {0, 1, 0, 1, 0};
  r.retire(used);
  CHECK(r.pieces.size() == 3 && r.pieces[0].b2 == key(0) && r.pieces[1].b2 == key(4) && r.pieces[2].b2 == key(8) && r.pieces[0].off == 0 && r.pieces[1].off == 24 &&
        r.pieces[2].off == 48 && r.next == 60, "pieces 0, 2, 4 stay, in that order, where they were");
  r.retire(std::vector<char>(3, 0));
  CHECK(r.pieces.size() == 3, "retiring none keeps all");
  r.retire(std::vector<char>(3, 1));
  CHECK(r.empty(), "retiring all empties the ring");
  done("retire_keeps_order", f0);
}

static void odd_length_refused() {
  const int f0 = failures;
  CHECK(!StageRing::refusal(0) && !StageRing::refusal(32) && !StageRing::refusal(512) && !StageRing::refusal((size_t)1 << 33), "multiples of 32 are taken");
  for (size_t n : {(size_t)1, (size_t)31, (size_t)33, (size_t)48, (size_t)511})
    CHECK(StageRing::refusal(n) && !strcmp(StageRing::refusal(n), "mm_reads_prefetch_packed: the packed length of a batch is a multiple of 32 bases"), "length %zu", n);
  done("odd_length_refused", f0);
}

static void clear_lets_the_area_grow() {
  const int f0 = failures;
  size_t area = StageRing::want(64, 0);
  StageRing r;
  CHECK(add(r, 0, 64, area) == 0, "setup");
  CHECK(add(r, 2, 512, area) == StageRing::npos, "the area is too small for the larger piece, and must not grow under a live one");
  r.clear();
  CHECK(r.empty() && r.next == 0, "clear");
  area = StageRing::want(512, 0);                                // what the caller does for an empty ring
  CHECK(add(r, 2, 512, area) == 0, "the grown area takes it");
  done("clear_lets_the_area_grow", f0);
}

// ---- the random run ----------------------------------------------------------------------------------------------------------------
static uint64_t rngState;
static uint32_t rnd(uint32_t n) {                                // xorshift64*, [0, n)
  rngState ^= rngState >> 12; rngState ^= rngState << 25; rngState ^= rngState >> 27;
  return (uint32_t)(((rngState * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

struct ModelPiece { const void* b2; const void* nm; size_t nPacked, off; int id; };
struct Tally { size_t steps = 0, placed = 0, refused = 0, wrapped = 0, matched = 0, retired = 0, cleared = 0; };

// the ring against the model: the same pieces in the same order at the offsets they were committed at; in the byte map, drawn anew from
// the ring's own list, no byte belongs to two pieces and every piece ends at or before areaBytes - 64
static void compare(const StageRing& r, const std::vector<ModelPiece>& model, size_t area, size_t seq, const char* step) {
  CHECK(r.pieces.size() == model.size(), "sequence %zu after %s: %zu pieces, the model holds %zu", seq, step, r.pieces.size(), model.size());
  std::vector<int> map(area, -1);
  for (size_t i = 0; i < r.pieces.size() && i < model.size(); i++) {
    const StageRing::Piece& p = r.pieces[i];
    CHECK(p.b2 == model[i].b2 && p.nm == model[i].nm && p.nPacked == model[i].nPacked, "sequence %zu after %s: piece %zu is another one", seq, step, i);
    CHECK(p.off == model[i].off, "sequence %zu after %s: piece %zu moved from %zu to %zu", seq, step, i, model[i].off, p.off);
    const size_t b = StageRing::bytes(p.nPacked);
    CHECK(p.off + b + 64 <= area, "sequence %zu after %s: piece %zu at %zu + %zu leaves [0, %zu - 64]", seq, step, i, p.off, b, area);
    for (size_t x = p.off; x < p.off + b && x < area; x++) {
      CHECK(map[x] < 0, "sequence %zu after %s: byte %zu belongs to pieces %d and %zu", seq, step, x, map[x], i);
      map[x] = (int)i;
    }
  }
}

static void random_sequence(size_t seq, Tally& t) {
  StageRing r;
  std::vector<ModelPiece> model;
  size_t area = 0, behind = 0;                                   // the model's own: the area's size, the byte behind the piece placed last
  int nextId = 0;
  const size_t reserve = rnd(4) ? 32 * (size_t)rnd(24) : 0;      // 0 .. 736 bases
  const int steps = 8 + (int)rnd(40);
  for (int s = 0; s < steps; s++, t.steps++) {
    const uint32_t what = rnd(16);
    if (what < 9) {                                              // a producer: place, and commit unless its copy failed
      const size_t n = 32 * (size_t)(1 + rnd(16));               // 32 .. 512 bases
      const size_t b = StageRing::bytes(n);
      const int k = 2 * (int)rnd(3);                             // few keys: equal pieces are common
      if (r.empty() && StageRing::want(n, reserve) > area) area = StageRing::want(n, reserve);   // only an empty ring lets the area grow
      std::vector<char> map(area, 0);
      for (const ModelPiece& p : model) memset(map.data() + p.off, 1, StageRing::bytes(p.nPacked));
      auto freeAt = [&](size_t off) {
        if (off + b + 64 > area) return false;
        for (size_t x = off; x < off + b; x++) if (map[x]) return false;
        return true;
      };
      const size_t first = model.empty() ? 0 : behind;
      const size_t expect = freeAt(first) ? first : freeAt(0) ? 0 : StageRing::npos;
      const StageRing before = r;
      const bool fits = r.place(n, area);
      CHECK(fits == (expect != StageRing::npos), "sequence %zu step %d: place(%zu) in %zu bytes says %d, the map %d", seq, s, n, area, (int)fits, (int)(expect != StageRing::npos));
      if (!fits) { CHECK(same(r, before), "sequence %zu step %d: a refusal changed the ring", seq, s); t.refused++; }
      else {
        CHECK(r.next == expect, "sequence %zu step %d: placed at %zu, the map says %zu", seq, s, r.next, expect);
        if (r.next != expect) return;                            // (ring and model have parted: nothing behind this step would mean anything)
        if (expect == 0 && first != 0) t.wrapped++;
        behind = r.next;
        if (rnd(16)) {
          r.commit(key(k), key(k + 1), n);
          model.push_back(ModelPiece{key(k), key(k + 1), n, expect, nextId++});
          behind = expect + b;
          t.placed++;
        }
      }
      compare(r, model, area, seq, "place");
    } else if (what < 15) {                                      // the consumer: an upload names some parts, then retires what it took
      std::vector<char> used(model.size(), 0);
      const int parts = (int)rnd(5);
      for (int p = 0; p < parts; p++) {
        const void* b2; const void* nm; size_t n;
        if (!model.empty() && rnd(4)) { const ModelPiece& m = model[rnd((uint32_t)model.size())]; b2 = m.b2; nm = m.nm; n = m.nPacked; }
        else { const int k = 2 * (int)rnd(3); b2 = key(k); nm = key(k + 1); n = 32 * (size_t)(1 + rnd(16)); }
        size_t expect = StageRing::npos;
        for (size_t q = 0; q < model.size() && expect == StageRing::npos; q++)
          if (!used[q] && model[q].b2 == b2 && model[q].nm == nm && model[q].nPacked == n) expect = q;
        const size_t hit = r.match(b2, nm, n, used);
        CHECK(hit == expect, "sequence %zu step %d: match gives %zu, the model %zu", seq, s, hit, expect);
        if (hit != StageRing::npos && hit < used.size()) { used[hit] = 1; t.matched++; }
      }
      compare(r, model, area, seq, "match");
      r.retire(used);
      std::vector<ModelPiece> left;
      for (size_t q = 0; q < model.size(); q++) if (!used[q]) left.push_back(model[q]); else t.retired++;
      model.swap(left);
      compare(r, model, area, seq, "retire");
    } else {
      r.clear(); model.clear(); behind = 0; t.cleared++;
      CHECK(r.empty() && r.next == 0, "sequence %zu step %d: clear", seq, s);
    }
  }
}

int main(int argc, char** argv) {
  const size_t sequences = argc > 1 ? (size_t)strtoull(argv[1], nullptr, 10) : 100000;
  rngState = argc > 2 ? strtoull(argv[2], nullptr, 10) : 0x9E3779B97F4A7C15ull;
  if (!rngState) rngState = 1;
  empty_ring_wants();
  fills_retires_wraps();
  refusal_changes_nothing();
  equal_pieces_match_once_each();
  retire_keeps_order();
  odd_length_refused();
  clear_lets_the_area_grow();
  Tally t;
  const int f0 = failures;
  for (size_t seq = 0; seq < sequences; seq++) random_sequence(seq, t);
  done("random_sequences", f0);
  printf("cases %d\nmismatches %d\n", cases, failures);
  printf("sequences %zu steps %zu placed %zu refused %zu wrapped %zu matched %zu retired %zu cleared %zu\n", sequences, t.steps, t.placed, t.refused, t.wrapped, t.matched,
         t.retired, t.cleared);
  return failures ? 1 : 0;
}
