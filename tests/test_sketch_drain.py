"""k_sketch_fast tests a position on the high words of its two hashes and leaves what only a survivor needs to the drain.  The two decisions
this rests on are plain C++ at the head of mashmap_amd/csrc/mm_sketch_dev.h and are checked here on the CPU: tests/hostlogic/
sketch_drain_check.cpp, a stand-alone program built with -fsanitize=address,undefined.

 * mm_sketch_cut_hiword: for every fragment the planner gives the fast kernel at K in {16, 19, 21, 32}, s in {1, 40, 130, 310, 498, 1998},
   n = 1..25 000 positions, the cut as a multiple of 2^32 is >= the cut it replaces, less than 2^32 above it, and equal to it wherever the
   old low word is zero.  How often it is not equal (the same at each K: the cut depends on s and n alone):

       s        1      40    130   310   498   1998
       moved  20253   3918     0     0     0      0      of 25 000 lengths each

   mm_sketch_fast_cut makes T from a float, 24 significant bits, so the low word is zero from T = 2^55 on: n <= 256 wantFast, i.e. every n up to
   1 536 at s = 1, 17 152 at s = 40 and 45 568 at s = 130.  Where it moves, the cut grows by less than 2^-19 of itself.
 * mm_sk_drain_keep: on fragments of K - 1 .. 200 bases with an N at every base in turn, pairs one k-mer apart, groups across a 32-bit mask
   word and runs, for every queued position up to 64 past the end, keep <=> the position lies inside the fragment and no base of its k-mer is
   an N -- what the strip loop's `ok` bit said per position before.  K = 16 .. 64; the bases behind the fragment are all N in the mask words."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = {1: 20253, 40: 3918, 130: 0, 310: 0, 498: 0, 1998: 0}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sketch_drain_check") / "sketch_drain_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "sketch_drain_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "FAIL" not in p.stdout, "sketch_drain_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    return p.stdout.splitlines()


def test_the_high_word_cut_lets_through_what_the_cut_did(report):
    assert "ok cuts" in report, report[-5:]
    rows = [tuple(int(x) for x in re.match(r"cut (\d+) (\d+): (\d+) plans, (\d+) moved", l).groups()) for l in report if l.startswith("cut ")]
    assert sorted((k, s) for k, s, _, _ in rows) == sorted((k, s) for k in (16, 19, 21, 32) for s in MOVED)
    for k, s, plans, moved in rows:
        assert plans == 25000, (k, s, plans)                 # the fast kernel takes every one of these lengths
        assert moved == MOVED[s], (k, s, moved)              # the flagship's cut (s = 130, n = 4 982) is the value it was


def test_the_drain_keeps_what_the_ok_bit_kept(report):
    for k in (16, 19, 20, 21, 32, 33, 34, 40, 49, 63, 64):
        assert any(l.startswith("ok drain %d: " % k) for l in report), (k, report[-12:])


def test_the_kernel_asks_the_shared_decisions():
    """the fast kernel's cut and drain are the header's functions, and the yardstick kernel next to it still hashes and nothing else"""
    src = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_sketch.hip")).read()
    fast = src[src.index("mm_sketch_fast(unsigned char* smem"):src.index("k_hash_only(const uint4*")]
    assert "mm_sketch_cut_hiword(" in fast and "mm_sketch_cut_last_hi(" in fast and "mm_sk_drain_keep<K>(" in fast
    hash_only = src[src.index("k_hash_only(const uint4*"):src.index("k_sketch_tables(")]
    assert "mm_sk_drain_keep" not in hash_only and "qH" not in hash_only
