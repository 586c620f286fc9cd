"""mashmap_amd/csrc/mm_stage_plan.h -- StageRing, the bookkeeping of the staging area that packed pieces travel in ahead of their upload
(mm_reads_prefetch_packed[_append] and mm_text_pack place and commit, the packed upload matches and retires):
tests/hostlogic/stage_check.cpp, a stand-alone program built with -fsanitize=address,undefined, runs the fixed cases -- what an empty ring
asks the area to hold, pieces filling the area and the next one going to offset 0 once the oldest has left, a refusal that changes
nothing, equal pieces matched once each, retire keeping the order of the rest, a length that is no multiple of 32, clear letting the area
grow -- and 100 000 seeded random sequences of place / commit / match / retire / clear against a byte map: after every step no two live
pieces overlap, every piece lies inside [0, areaBytes - 64], no live piece has moved, and place() refuses exactly when neither of its two
offsets is free in the map.  Runs without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["clear_lets_the_area_grow", "empty_ring_wants", "equal_pieces_match_once_each", "fills_retires_wraps", "odd_length_refused", "random_sequences",
         "refusal_changes_nothing", "retire_keeps_order"]


@pytest.fixture(scope="module")
def stage_out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_check") / "stage_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "stage_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "stage_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def test_every_case_ran_without_a_mismatch(stage_out):
    assert re.search(r"^cases 8$", stage_out, re.M)
    assert sorted(re.findall(r"^ok (\w+)$", stage_out, re.M)) == CASES
    assert re.search(r"^mismatches 0$", stage_out, re.M) and "FAIL" not in stage_out


def test_the_random_run_reached_every_rule(stage_out):
    m = re.search(r"^sequences (\d+) steps (\d+) placed (\d+) refused (\d+) wrapped (\d+) matched (\d+) retired (\d+) cleared (\d+)$", stage_out, re.M)
    assert m
    sequences, steps, placed, refused, wrapped, matched, retired, cleared = map(int, m.groups())
    assert sequences >= 100000 and steps >= 8 * sequences
    assert min(placed, refused, wrapped, matched, retired, cleared) >= 10000


def test_the_header_needs_no_runtime():
    with open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_stage_plan.h"), encoding="utf-8") as fh:
        includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", fh.read(), re.M)
    assert includes and not [i for i in includes if "hip" in i.lower() or i.startswith("mm_")], includes
