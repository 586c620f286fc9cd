"""mashmap_amd/csrc/mm_paf_core.h -- the second half of MapPost::finishRead for one row (filterFalseHighIdentity,
mappingBoundarySanityCheck) and the bytes of its PAF line as k_paf_measure and k_paf_write produce them (mm_paf_g6, the mapQ table,
mm_paf_numeric) -- on the CPU: tests/hostlogic/paf_check.cpp, a stand-alone program built with -fsanitize=address,undefined, runs the
header beside std::to_chars, MapPost::fakeMapQOf and MapPost::finishRows + appendReadMappings and compares every byte.  Runs without a GPU.

The program prints one line per check with what it covered; the assertions below hold each line against what the check is there for."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["default", "legacy", "ani_percentage", "merge_off", "length_filter", "legacy_length_filter"]


@pytest.fixture(scope="module")
def paf_out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("paf_check") / "paf_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "paf_check.cpp")])
    p = subprocess.run([exe, "20000"], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "paf_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def line(out, pattern):
    m = re.search("^" + pattern + "$", out, re.M)
    assert m, pattern
    return [int(x) for x in m.groups()]


def test_nothing_differs(paf_out):
    assert re.search(r"^differences 0$", paf_out, re.M)


def test_g6_is_to_chars_general_6(paf_out):
    """every float of the identity tables of s 1, 80, 130, 2048 at k 16 and 19, x1 and x100: sum of (s + 1)^2 over the four sizes, x2 x2"""
    n, bad = line(paf_out, r"g6 identity table values (\d+) bad (\d+)")
    assert n == 4 * (2 ** 2 + 81 ** 2 + 131 ** 2 + 2049 ** 2) and bad == 0
    ties, n, bad = line(paf_out, r"g6 representable ties (\d+) values (\d+) bad (\d+)")
    # every D.5 is a double from 10^5 up to where (2D + 1) * 5^(X - 5) outgrows 53 bits: nine exponents hold all 900 000 of them
    assert ties > 9 * 900000 and n == 4 * ties and bad == 0
    for what, least in (("powers of ten", 2 * 39 * 9), ("powers of two and zeros", 2 * 128 * 3 + 2), ("random doubles", 2000000), ("random floats", 1000000),
                        ("out of range", 15)):
        n, bad = line(paf_out, r"g6 %s values (\d+) bad (\d+)" % what)
        assert n >= least and bad == 0, what
    longest, scientific = line(paf_out, r"g6 longest (\d+) scientific (\d+)")
    assert longest == 12 and scientific > 1000000


def test_the_mapq_table_is_the_hosts_expression(paf_out):
    m = re.search(r"^mapq table entries (\d+) first '(.*)' second '(.*)' last '(.*)' last_below_one '(.*)'$", paf_out, re.M)
    assert m and 60 <= int(m.group(1)) <= 128
    assert m.groups()[1:] == ("-0", "0", "255", "72")                  # an identity of exactly 0 prints -0, 1 - 2^-24 prints 72
    n, bad = line(paf_out, r"mapq around thresholds values (\d+) bad (\d+)")
    assert n > 64 * int(m.group(1)) and bad == 0
    n, bad = line(paf_out, r"mapq identity table values (\d+) bad (\d+)")
    assert n > 2 * 2049 * 2049 // 2 and bad == 0
    n, bad = line(paf_out, r"mapq random values (\d+) bad (\d+)")
    assert n == 1000003 and bad == 0
    assert line(paf_out, r"mapq outside refused (\d+) of 4") == [4]


def test_the_length_filter_on_both_sides_of_its_threshold_and_a_query_span_of_zero(paf_out):
    assert line(paf_out, r"scenario length_filter delta_385_lines (\d+) delta_386_lines (\d+) zero_length_delta_0_lines (\d+) zero_length_delta_1_lines (\d+)") == [1, 0, 1, 0]


def test_every_clamp_identity_0_and_1_and_a_row_that_is_not_formattable(paf_out):
    t = "\t"
    assert "scenario clamps text read\t5000\t0\t900\t+\tchr1\t60000\t0\t800\t70\t" in paf_out
    assert t.join(["read", "5000", "5000", "5000", "-", "chr1", "60000", "59999", "59999", "71"]) in paf_out
    assert t.join(["read", "5000", "300", "300", "+", "chr1", "60000", "500", "500", "72"]) in paf_out
    assert t.join(["read", "5000", "4000", "5000", "+", "chr1", "60000", "59000", "59999", "73"]) in paf_out
    assert "\t-0\tid:f:0\tkc:f:1e-07\n" in paf_out and "\t255\tid:f:1\tkc:f:0\n" in paf_out
    assert line(paf_out, r"scenario not_formattable handed (\d+) complexity_0_handed (\d+)") == [1, 0]


def test_the_longest_numeric_part_is_reached_and_never_exceeded(paf_out):
    n, most, before, most_before, untouched = line(paf_out, r"scenario longest_numeric length (\d+) of (\d+) before_ref (\d+) of (\d+) untouched_behind (\d+)")
    assert n == most == 161 and before == most_before == 39 and untouched == 1
    n, most = line(paf_out, r"scenario longest_numeric_legacy length (\d+) of (\d+)")
    assert n <= most == 88


def test_generated_reads_in_every_mode(paf_out):
    total = 0
    for mode in MODES:
        reads, rows, lines, dropped, emptied, handed, every_clamp, zkept, zdropped, longest = line(
            paf_out, r"generated mode %s reads (\d+) rows (\d+) lines (\d+) dropped (\d+) reads_emptied (\d+) handed (\d+) every_clamp (\d+) "
                     r"zero_length_kept (\d+) zero_length_dropped (\d+) longest_numeric (\d+)" % mode)
        total += reads
        assert rows > 4 * reads and lines > 0 and every_clamp == 1 and longest <= 161, mode
        if "length_filter" in mode:
            assert dropped > 1000 and emptied > 100 and zkept > 100 and zdropped > 100, mode
        else:
            assert dropped == 0 and lines + 16 * handed >= rows, mode
    assert total == 20000
