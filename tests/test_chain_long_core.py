"""mm_chain_read_long (mashmap_amd/csrc/mm_chain_core.h) -- the tail of Map::mapModule for a read of up to 512 records, the steps
k_chain_reads_long runs -- on the CPU: tests/hostlogic/chain_long_check.cpp, a stand-alone program built with
-fsanitize=address,undefined, runs it beside MapPost::chainedFromRecords on generated reads of 17 to 512 records and compares every field
of every row bit for bit.  Above 16 elements the host's std::sort calls are introsort, whose order among equal keys picks a chain's
representative; the header's sorts are mm_stdsort.h.  Runs without a GPU.

k 16, segLength 1000, sketch 80.  5 200 generated reads: one to four interleaved colinear chains, fragments out of a tandem array with
more than 16 records of their own, reads of one fragment, ties in (refSeqId, refStartPos, queryStartPos), merge off, the three filter
modes, secondaryToKeep 0, 2 and 65535; every size from 17 to 40 and a hundred reads of 512."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def long_out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_long_check") / "chain_long_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "chain_long_check.cpp")])
    p = subprocess.run([exe, "5200"], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "chain_long_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def scenario(out, name):
    m = re.search(r"^scenario %s rows (\d+)(.*)$" % re.escape(name), out, re.M)
    assert m, name
    rows = [(int(a), int(b), int(c), int(d), int(e), f, int(g), int(h)) for a, b, c, d, e, f, g, h in
            re.findall(r"\[(-?\d+)-(-?\d+) (\d+):(-?\d+)-(-?\d+) ([+-]) cons (\d+) merged (\d+)\]", m.group(2))]
    assert len(rows) == int(m.group(1))
    return rows


def test_every_row_of_every_long_read_is_the_hosts_bit_for_bit(long_out):
    assert re.search(r"^differences 0$", long_out, re.M)
    m = re.search(r"^generated (.*)$", long_out, re.M)
    assert m
    f = dict(zip(m.group(1).split()[0::2], (int(x) for x in m.group(1).split()[1::2])))
    print(f)
    assert f["reads"] >= 5000 and f["rows"] > f["reads"] and f["largest_read"] == 512 and f["reads_of_512"] >= 20 and f["sizes_17_to_40"] == 24
    assert f["chains_of_two_or_more"] > 5000 and f["chains_over_16"] > 500 and f["several_chains"] > 500 and f["reverse"] > 1000
    assert f["fragment_over_16"] > 300 and f["not_split"] > 100 and f["merge_off"] > 100 and f["tied"] > 1000
    assert min(f["keep0"], f["keep2"], f["keep65535"]) > 1000 and min(f["filter_none"], f["filter_map"], f["filter_one2one"]) > 500


def test_the_representative_of_a_long_chain_is_the_one_std_sort_puts_first(long_out):
    """17 colinear members with conservedSketches 50 + segment: all tie in the sort by splitMappingId; libstdc++'s introsort leaves the
    ninth in key order in front (tests/test_stdsort.py: element 8 of 17, 10 of 20), and the row carries its conservedSketches -- a
    stable sort would leave the first, 50.  On the reverse strand key order is the reverse of segment order: element 10 is segment 9."""
    assert scenario(long_out, "chain_of_17") == [(0, 17000, 0, 10000, 27000, "+", 58, 17)]
    assert scenario(long_out, "chain_of_20_rev") == [(0, 20000, 1, 21000, 41000, "-", 50 + (19 - 10), 20)]


def test_the_limit_is_512_records_and_a_bad_record_is_an_error(long_out):
    assert re.search(r"^scenario limits records_513 -1 records_512 rows 1 merged 512 bad_record -2$", long_out, re.M)


def test_short_reads_through_the_long_entry_point_are_mm_chain_reads_rows(long_out):
    m = re.search(r"^short reads (\d+) rows (\d+) sizes (\d+)$", long_out, re.M)
    assert m and int(m.group(1)) == 2000 and int(m.group(2)) > 2000 and int(m.group(3)) == 16
