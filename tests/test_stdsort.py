"""mashmap_amd/csrc/mm_stdsort.h -- libstdc++'s std::sort restated (introsort with its depth limit, median-of-three to first, the
unguarded partition, the heap fallback, the final insertion sort) -- beside the toolchain's std::sort: tests/hostlogic/stdsort_check.cpp,
a stand-alone program built with -fsanitize=address,undefined, sorts ids through a logging comparator both ways; the logs of comparator
calls and the final permutations must be identical.  Every n in 0 .. 600 and some up to 5000; all keys equal, 2 / 3 / 17 distinct keys
random and interleaved, sorted, reversed, organ-pipe, random distinct, and inputs frozen from McIlroy's adversary that reach the depth
limit.  Runs without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sort_out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stdsort_check") / "stdsort_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "stdsort_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "stdsort_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def test_comparisons_and_permutations_are_std_sorts(sort_out):
    assert re.search(r"^differences 0$", sort_out, re.M)
    m = re.search(r"^inputs (\d+) comparisons (\d+)$", sort_out, re.M)
    assert m and int(m.group(1)) >= 601 * 11 and int(m.group(2)) > 10_000_000


def test_the_depth_limit_fallback_was_taken(sort_out):
    m = re.search(r"^fallback inputs (\d+) taken (\d+)$", sort_out, re.M)
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) >= int(m.group(1))


def test_the_first_of_all_equal_elements_is_the_toolchains(sort_out):
    """which of n equal elements std::sort puts first -- the representative of a chain of n mappings -- as measured on libstdc++: a
    toolchain whose std::sort differs (the reference is then another program) shows up here as such"""
    got = {int(n): int(f) for n, f in re.findall(r"^allequal n (\d+) first (\d+)$", sort_out, re.M)}
    assert got == {17: 8, 20: 10, 33: 25}
