"""mashmap_amd/csrc/mm_sketch_large_plan.h -- the cut, the tile and the sort schedule of k_sketch_large (MM_OPT_SKETCH_LARGE) -- on the
CPU: tests/hostlogic/sketch_large_check.cpp, a stand-alone program built with -fsanitize=address,undefined.  It runs the schedule
serially, the way the kernel walks it, for every padded length 2 .. 2^18 at MM_SKL_TILE and at a tile of 8 entries, against std::sort, and
sweeps mm_sketch_cut over sketch sizes and fragment lengths."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sketch_large_check") / "sketch_large_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "sketch_large_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "FAIL" not in p.stdout, "sketch_large_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    return p.stdout.splitlines()


def test_the_schedule_sorts_like_std_sort_at_every_length(report):
    assert any(l.startswith("ok schedule ") for l in report), report[-5:]
    rounds = {(int(a), int(b)): (int(c), int(d), int(e)) for a, b, c, d, e in (l.split()[1:] for l in report if l.startswith("rounds "))}
    # one tile round while everything fits a tile; k2 = 2 tile brings one sweep and a tile round more, every doubling one sweep more than the last
    assert rounds[(4096, 4096)] == (1, 0, 1) and rounds[(8192, 4096)] == (3, 1, 2) and rounds[(64, 8)] == (10, 6, 4)
    assert rounds[(32768, 4096)] == (10, 6, 4) and rounds[(262144, 4096)] == (28, 21, 7)


def test_the_round_count_is_the_one_design_md_states(report):
    """DESIGN.md section 3 states the schedule of an s = 19 998 fragment: 32 768 entries in tiles of 4 096"""
    tile = [int(l.split()[1]) for l in report if l.startswith("tile ")]
    assert tile == [4096]
    got = [l.split()[3:] for l in report if l.startswith("rounds 32768 4096 ")]
    assert len(got) == 1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"32 768 entries in tiles of 4 096: (\d+) rounds, (\d+) sweeps through HBM and (\d+) tile rounds", design)
    assert m, "DESIGN.md does not state the schedule of k_sketch_large"
    assert [int(x) for x in m.groups()] == [int(x) for x in got[0]]
    hdr = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_sketch_large_plan.h")).read()
    assert re.search(r"#define MM_SKL_TILE 4096\b", hdr)


def test_the_cut_is_the_global_kernels(report):
    assert any(l.startswith("ok cut ") for l in report), report[-5:]
    # ... and k_sketch_global calls the function the sweep ran, instead of spelling the expression beside it
    src = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_sketch_global.hip")).read()
    assert "uint64_t T = mm_sketch_cut(s, n);" in src
    assert "sqrt((double)" not in src and "18446744073709551616" not in src and "5.0 *" not in src
    large = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_sketch_large.hip")).read()
    assert "uint64_t T = mm_sketch_cut(s, n);" in large and "sqrt((double)" not in large and "18446744073709551616" not in large
    # one definition of it in the sources
    csrc = os.path.join(ROOT, "mashmap_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip")) and "uint64_t mm_sketch_cut(int s, int n) {" in open(os.path.join(csrc, f)).read()]
    assert defs == ["mm_sketch_plan.h"]
