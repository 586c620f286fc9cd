"""mashmap_amd/csrc/mm_chain_core.h -- the tail of Map::mapModule for one read as k_chain_reads runs it (the kmerComplexity gate, the
coordinates of a split read, mergeMappingsInRange with its union-find, filterWeakMappings, filterByGroup on the query axis with the
plane sweep and its std::set status) -- on the CPU: tests/hostlogic/chain_check.cpp, a stand-alone program built with
-fsanitize=address,undefined, runs the header's function beside MapPost::chainedFromRecords (mapModuleFromRecords stopped behind
filterByGroup) on generated reads of 1 to 16 records and compares every field of every row bit for bit, floats included.  Runs without a GPU.

k 16, segLength 1000, sketch 80.  The named scenarios print what they leave, and the assertions below check that each really shows
what it is there for; 20 000 generated reads vary minMerged (1, 3), secondaryToKeep (0, 2), merge, the filter, chain_gap and the
complexity threshold.  kmerComplexity's integer derivation of (double)((long double)maxHash / UINT64_MAX) is checked apart."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chain_out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_check") / "chain_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "chain_check.cpp")])
    p = subprocess.run([exe, "20000"], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "chain_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def scenario(out, name):
    """(rows, [(qs, qe, ref, rs, re, strand, cons, merged)])"""
    m = re.search(r"^scenario %s rows (\d+)(.*)$" % re.escape(name), out, re.M)
    assert m, name
    rows = [(int(a), int(b), int(c), int(d), int(e), f, int(g), int(h)) for a, b, c, d, e, f, g, h in
            re.findall(r"\[(-?\d+)-(-?\d+) (\d+):(-?\d+)-(-?\d+) ([+-]) cons (\d+) merged (\d+)\]", m.group(2))]
    assert len(rows) == int(m.group(1))
    return rows


def test_every_row_of_every_read_is_the_hosts_bit_for_bit(chain_out):
    assert re.search(r"^differences 0$", chain_out, re.M)
    m = re.search(r"^generated reads (\d+) rows (\d+) chains_of_two_or_more (\d+) reads_without_rows (\d+) largest_read (\d+) reads_of_16 (\d+)$", chain_out, re.M)
    assert m
    reads, rows, chains, without, largest, full = (int(x) for x in m.groups())
    assert reads == 20000 and rows > reads and chains > 2000 and without > 500 and largest == 16 and full >= 20


def test_colinear_chains_on_both_strands_and_the_gap_at_chain_gap(chain_out):
    assert scenario(chain_out, "colinear_fwd") == [(0, 5000, 0, 10000, 15000, "+", 70, 5)]
    assert scenario(chain_out, "colinear_rev") == [(0, 5000, 1, 16000, 21000, "-", 74, 5)]          # the representative: lowest reference position
    assert [r[7] for r in scenario(chain_out, "gap_below")] == [3]                                  # dist 999 < chain_gap 1000: one chain
    assert [r[7] for r in scenario(chain_out, "gap_at")] == [1, 2]                                  # dist 1000: not < chain_gap


def test_two_chains_and_records_with_equal_keys(chain_out):
    assert [r[7] for r in scenario(chain_out, "two_chains_filter_none")] == [3, 3]
    assert len(scenario(chain_out, "two_chains")) == 2
    # three records at one (refSeqId, refStartPos, queryStartPos): the chain's representative -- the conservedSketches of the PAF line -- is
    # the one that came first, in either input order; a sort that is not stable puts another there
    a, b = scenario(chain_out, "equal_keys"), scenario(chain_out, "equal_keys_other_order")
    assert (a[0][6], a[0][7]) == (61, 6) and (b[0][6], b[0][7]) == (69, 6)


def test_the_status_set_keeps_one_of_several_equivalent_mappings(chain_out):
    """three chains of equal identity, queryStartPos and refSeqId: the sweep's std::set holds one of them, so one survives whatever
    secondaryToKeep says -- the behaviour is restated, not fixed"""
    assert len(scenario(chain_out, "sweep_equivalent_filter_none")) == 3
    assert len(scenario(chain_out, "sweep_equivalent_keep0")) == 1
    assert len(scenario(chain_out, "sweep_equivalent_keep2")) == 1


def test_weak_mappings_short_reads_secondaries_merge_off_and_the_complexity_gate(chain_out):
    assert scenario(chain_out, "lone_record") == []                                                  # filterWeakMappings: n_merged 0 < 1
    assert len(scenario(chain_out, "short_read_keep0")) == 2 and len(scenario(chain_out, "short_read_keep2")) == 3
    assert all(r[7] == 0 and r[1] == 600 for r in scenario(chain_out, "short_read_keep2"))          # not a split read: nothing merged
    assert len(scenario(chain_out, "read_of_one_segment")) == 2
    assert [r[7] for r in scenario(chain_out, "min_merged_1")] == [2, 1]
    assert scenario(chain_out, "min_merged_3") == [] and [r[7] for r in scenario(chain_out, "min_merged_3_chain_of_5")] == [5]
    assert len(scenario(chain_out, "merge_off")) == 4 and len(scenario(chain_out, "merge_off_filter_none")) == 5
    assert all(r[7] == 0 for r in scenario(chain_out, "merge_off_filter_none"))
    assert [(r[0], r[1], r[7]) for r in scenario(chain_out, "complexity_gate")] == [(0, 1000, 1), (2000, 4000, 2)]   # the gated fragment splits the chain


def test_a_mapping_count_of_zero_is_the_casts_65535(chain_out):
    """numMappings 0: MapPost::filterByGroup and the reference pass (uint16_t)(0 - 1) = 65535 as secondaryToKeep, and so does the header --
    every mapping the status set holds is kept, where a count of 1 keeps the best"""
    assert len(scenario(chain_out, "num_mappings_0")) == 3 and len(scenario(chain_out, "num_mappings_1")) == 1


def test_complexities_of_a_chain_up_to_2_to_the_24_apart(chain_out):
    """the assumption of the header's note on the averages, at its edge: maxHash 2^63 next to 2^40 in one chain (the generated reads draw
    maxHash from 2^40 .. 2^64 throughout); compared with the host inside the program like every other row"""
    m = re.search(r"^scenario complexities_far_apart rows 1 merged 3 kc ([0-9.e+]+)$", chain_out, re.M)
    assert m and float(m.group(1)) > 1e5


def test_seventeen_records_are_refused(chain_out):
    """... and a record that names an entry outside the identity table is an error of its own (-2), not a hand-over"""
    assert re.search(r"^scenario seventeen_records returns -1 sixteen 1 bad_record -2$", chain_out, re.M)


def test_kmer_complexity_without_an_80_bit_type(chain_out):
    assert re.search(r"^hash01 edge values 191 bad 0$", chain_out, re.M)                            # 1, 2^64 - 1, 2^p and 2^p +- 1 for p = 1..63
    assert re.search(r"^hash01 random values 1000000 bad 0$", chain_out, re.M)
    assert re.search(r"^kmerComplexity random values 200000 bad 0$", chain_out, re.M)
