"""mm_chain_read and mm_chain_read_long (mashmap_amd/csrc/mm_chain_core.h) with the reference groups of -Y (mm_chain_env::refGroup: the
filter of filterByGroup run by run) and with --noSplit (mm_chain_env::noSplit), on the CPU: tests/hostlogic/chain_modes_check.cpp, a
stand-alone program built with -fsanitize=address,undefined, runs both beside MapPost::chainedFromRecords with skip_prefix / split set
accordingly and compares every field of every row bit for bit, and every read's run count with the runs of MapPost's own input to
filterByGroup.  Runs without a GPU.

k 16, segLength 1000, sketch 80; ten contigs in eight groups numbered 0 0 1 1 2 3 4 5 6 7 or 0 1 0 2 1 3 4 5 6 7.  4 000 generated reads
of 1 to 512 records and 2 000 reads without groups."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def modes_out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_modes_check") / "chain_modes_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "chain_modes_check.cpp")])
    p = subprocess.run([exe, "4000"], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "chain_modes_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def scenario(out, name):
    """(runs, rows) of a named scenario"""
    m = re.search(r"^scenario %s runs (\d+) rows (\d+)(.*)$" % re.escape(name), out, re.M)
    assert m, name
    rows = [(int(a), int(b), int(c), int(d), int(e), f, int(g), int(h)) for a, b, c, d, e, f, g, h in
            re.findall(r"\[(-?\d+)-(-?\d+) (\d+):(-?\d+)-(-?\d+) ([+-]) cons (\d+) merged (\d+)\]", m.group(3))]
    assert len(rows) == int(m.group(2))
    return int(m.group(1)), rows


def figures(out, line):
    m = re.search(r"^%s (.*)$" % line, out, re.M)
    assert m, line
    f = dict(zip(m.group(1).split()[0::2], (int(x) for x in m.group(1).split()[1::2])))
    print(f)
    return f


def test_every_row_and_every_run_count_is_the_hosts(modes_out):
    assert re.search(r"^differences 0$", modes_out, re.M)
    f = figures(modes_out, "generated")
    assert f["reads"] == 4000 and f["rows"] > f["reads"] and f["chains_of_two_or_more"] > 4000
    assert f["largest_read"] == 512 and f["sizes_1_to_16"] == 16 and f["reads_up_to_16"] > 500 and f["reads_over_16"] > 2000
    assert min(f["no_groups"], f["groups_in_order"], f["groups_out_of_order"]) >= 800
    assert min(f["in_1_group"], f["in_2_groups"], f["in_3_groups"], f["in_8_groups"]) > 400
    assert f["several_groups_same_interval"] > 1000 and f["two_contigs_of_a_group"] > 1000
    assert f["runs"] > f["reads"] and f["reads_with_several_runs"] > 1000
    assert f["runs_of_one"] > 500 and f["runs_over_16"] > 1000 and f["group_in_two_runs"] > 400
    assert min(f["nosplit_short"], f["nosplit_short_grouped"], f["nosplit_long"], f["nosplit_long_grouped"]) > 50 and f["split_short"] > 200
    assert f["merge_off"] > 300 and f["reverse"] > 1000
    assert min(f["keep0"], f["keep2"], f["keep65535"]) > 1000 and min(f["filter_none"], f["filter_map"], f["filter_one2one"]) > 400


def test_three_groups_leave_three_rows_and_no_groups_one(modes_out):
    """a 3-segment read with a colinear chain on a contig of each of three groups, secondaryToKeep 0: every group is swept by itself
    and keeps its chain; the same records without groups are one run, of which the best identity is left"""
    runs, rows = scenario(modes_out, "three_groups_three_rows")
    assert runs == 3 and rows == [(0, 3000, 0, 10000, 13000, "+", 70, 3), (0, 3000, 2, 10000, 13000, "+", 66, 3), (0, 3000, 4, 10000, 13000, "+", 62, 3)]
    runs, rows = scenario(modes_out, "three_groups_no_groups")
    assert runs == 1 and rows == [(0, 3000, 0, 10000, 13000, "+", 70, 3)]


def test_a_group_whose_contigs_are_not_consecutive_forms_two_runs(modes_out):
    """refGroup 0 1 0 ...: contigs 0 and 2 share a group but contig 1 lies between them in the order sorted by the reference key, as
    std::find_if_not sees it: three runs and three rows.  With 0 0 1 ... contigs 0 and 1 are one run: two runs, and contig 1's row is gone"""
    runs, rows = scenario(modes_out, "group_in_two_runs")
    assert runs == 3 and rows == [(0, 2000, 0, 20000, 22000, "+", 72, 2), (0, 2000, 1, 20000, 22000, "+", 69, 2), (0, 2000, 2, 20000, 22000, "+", 66, 2)]
    runs, rows = scenario(modes_out, "group_in_one_run")
    assert runs == 2 and rows == [(0, 2000, 0, 20000, 22000, "+", 72, 2), (0, 2000, 2, 20000, 22000, "+", 66, 2)]


def test_a_contig_outside_the_group_array_is_a_bad_record(modes_out):
    """MM_CHAIN_BAD_RECORD (-2) from both entry points, no run counted; the last contig is taken, and without refGroup nothing is looked up"""
    assert re.search(r"^scenario bad_refseqid past_the_end -2 long -2 runs 0 negative -2 last_contig 3 no_groups 3$", modes_out, re.M)


def test_without_groups_the_filter_leaves_the_rows_of_before(modes_out):
    """2 000 reads without refGroup through the filter that now walks runs, against MapPost: one run for every read that reaches it"""
    assert re.search(r"^differences 0$", modes_out, re.M)
    f = figures(modes_out, "ungrouped")
    assert f["reads"] == 2000 and f["rows"] > 2000 and 0 < f["runs"] <= 2000 and f["reads_with_several_runs"] == 0
