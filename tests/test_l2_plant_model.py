"""The inputs of tests/test_gpu_l2_edges.py sit on the edges they are named after -- held here, without a GPU, with the oracle's
map_fragment and tests/l2plant.py's slice_model over the planted index.  A case that loses its edge (another seed, another read
position) fails here, not silently on the device.  The counts in the assertions are the ones these inputs give.

Two edges of the stream format have no input:
  * first_gap (the slide's first insert further than MAXDELTA from rangeStart) and no_insert (a slide without an insert).  An L1 range
    begins at the first position whose overlap count reaches minimumHits; the count rises only at an OPEN point, and an OPEN point is the
    wpos of an index record.  That record is the slide's first event (its key is rangeStart * 2 + 1, the slide's lower bound): the
    first delta of every stream is 0.  test_no_candidate_without_an_insert_at_range_start holds that over every candidate of every
    case.  (The range's END may be a CLOSE point: that is what puts evictions behind the last insert.)
  * a gap beyond 2^27 (the bigSkip branch of k_l2_locate) needs a contig of hundreds of Mbp and is still uncovered."""
import pytest

import l2plant as P


def count(c, pred):
    return sum(1 for m in c["facts"] if pred(m))


def edges(c):
    return dict(candidates=len(c["facts"]), gap_in=count(c, lambda m: m["gap_in"]), end_skip=count(c, lambda m: m["end_skip"]),
                tail64=count(c, lambda m: m["tail_evictions"] >= 64), tail128=count(c, lambda m: m["tail_evictions"] >= 128),
                behind64=count(c, lambda m: m["behind_evictions"] >= 64), last=count(c, lambda m: m["last_of_contig"]),
                last_tail64=count(c, lambda m: m["last_of_contig"] and m["tail_evictions"] >= 64))


@pytest.mark.parametrize("s,want", [(3, dict(candidates=12, gap_in=7, end_skip=5)), (5, dict(candidates=12, gap_in=6, end_skip=2))])
def test_skip_jb11(s, want):
    """inserts further apart than 8191 inside a slide (the single-skip path of k_l2_locate, the skip term of the sweep's position), and an end
    marker further than that behind the last insert"""
    c = P.skip_jb11(s)
    print(P.summary(c))
    e = edges(c)
    assert {k: e[k] for k in want} == want
    assert P.jb_of(s) == 11 and max(m["max_gap"] for m in c["facts"]) > 8191 and max(m["end_gap"] for m in c["facts"]) > 8191
    shown = [m for m in c["facts"] if m["end_skip"] and any(x[4] == m["next_w"] for x in c["l2"][m["frag"]])]
    assert shown, "no locus ends at the position an end marker behind a skip carries"


def test_skip_jb13():
    """the 13-bit field: the hole's 2 507 bases against a MAXDELTA of 2047, inside a slide (once before the read's own position, once
    behind it) and behind one; 64 evictions and more at the end of a slide and behind it, in one candidate"""
    c = P.skip_jb13()
    print(P.summary(c))
    assert P.jb_of(c["s"]) == 13
    assert edges(c) == dict(candidates=5, gap_in=2, end_skip=3, tail64=2, tail128=1, behind64=2, last=0, last_tail64=0)
    assert count(c, lambda m: m["end_skip"] and m["tail_evictions"] >= 64 and m["behind_evictions"] >= 64) == 1
    assert sorted(m["max_gap"] for m in c["facts"])[-1] == 2507 and [m["end_gap"] for m in c["facts"]] == [2507, 2507, 6, 3, 21911]
    assert [(x[3], x[4]) for x in c["l2"][3]] == [(102999, 103012)]                # behind the skip: positions that went through it
    m = c["facts"][4]
    assert m["tail_evictions"] == 2047 and [x[4] for x in c["l2"][4]] == [m["next_w"]] == [162005]   # the end marker's position is the locus's end


def test_tail_and_behind():
    """the look-back for the last insert runs once (64 .. 127 evictions at the end of a slide) and more than once (128 and more); the look-ahead
    for the next insert goes beyond the 64 events behind the slide"""
    c = P.tail_and_behind()
    print(P.summary(c))
    assert edges(c) == dict(candidates=29, gap_in=0, end_skip=0, tail64=7, tail128=6, behind64=3, last=0, last_tail64=0)
    assert max(m["tail_evictions"] for m in c["facts"]) == 209 and max(m["behind_evictions"] for m in c["facts"]) == 203


def test_last_of_contig():
    """no insert behind the slide: the end marker carries the last insert's own wpos, and the look-ahead runs to the contig's end"""
    c = P.last_of_contig()
    print(P.summary(c))
    assert edges(c) == dict(candidates=16, gap_in=0, end_skip=0, tail64=7, tail128=0, behind64=4, last=11, last_tail64=7)
    assert all(m["end_gap"] == 0 for m in c["facts"] if m["last_of_contig"])


@pytest.mark.parametrize("L,s", [(5000, 130), (21000, 2100)])
def test_hash_neighbours(L, s):
    """every q[p] - 1 and q[p] + 1, 0, qmax + 1 and 2^64 - 1 are inserted in the slide of the fragment's candidate"""
    c = P.hash_neighbours(L, s)
    m, qs = c["facts"][0], c["sketch"]
    assert len(c["facts"]) == 1 and len(qs) == s
    want = [v for v in P.neighbour_values(qs) if v not in set(qs)]
    assert len(want) == len(set(want)) == 2 * s + 2 == c["placed"] and c["values"] == want, (len(want), c["placed"])   # no two query hashes are neighbours: none was left out
    assert all(v in m["slide_hashes"] for v in want)
    assert {0, qs[-1] + 1, P.U64} <= m["slide_hashes"]


LADDER = [("cell_31", "cell_slide", 31, ("narrow",)), ("cell_32", "cell_slide", 32, ("narrow", "wide")),
          ("cell_4095", "cell_slide", 4095, ("narrow", "wide")), ("cell_4096", "cell_slide", 4096, ("narrow", "wide", "exact")),
          ("preload_cell_31", "cell_preload", 31, ("narrow",)), ("preload_cell_32", "cell_preload", 32, ("narrow", "wide")),
          ("preload_3999", "preload_records", 3999, ("narrow",)), ("preload_4000", "preload_records", 4000, ("narrow", "wide", "exact"))]


@pytest.mark.parametrize("name,fact,want,route", LADDER, ids=[x[0] for x in LADDER])
def test_counter_ladder(name, fact, want, route):
    """One candidate, its counter exactly at the step.  The steps, from the kernels' own rules: an insert into a cell of CMASK counts or
    more sends the candidate on (IN & neg((CMASK - 1) - cnt): the cell would have to hold CMASK + 1), so a narrow cell (CMASK 31) carries
    a count of 31 and a wide one (CMASK 4095) 4095, the query hash's own 1 included; a pre-load cell beyond CMASK trips tooBig in the
    narrow sweep's row copy; a pre-load of nOpen + nPre >= 4000 records goes to the exact kernel through both sweeps"""
    c = P.CASES[name]()
    print(P.summary(c))
    m = c["facts"][0]
    assert len(c["facts"]) == 1 and m[fact] == want and m["route"] == route and c["launches"] == len(route)
    others = {"cell_slide": 12, "cell_preload": 12, "preload_records": 300}
    for k, cap in others.items():
        if k != fact: assert m[k] <= cap, (k, m[k])              # only the named counter is anywhere near a step


def test_ladder_steps_are_the_planted_counts():
    """each pair of the ladder differs by one planted record, on one read over one contig"""
    for a, b in (("cell_31", "cell_32"), ("cell_4095", "cell_4096"), ("preload_cell_31", "preload_cell_32")):
        ca, cb = P.CASES[a](), P.CASES[b]()
        assert cb["planted"] == ca["planted"] + 1 and ca["facts"][0]["cand"] == cb["facts"][0]["cand"]
    assert (P.cell_slide(31)["planted"], P.cell_slide(4095)["planted"], P.cell_preload(31)["planted"]) == (26, 4090, 26)


def test_no_candidate_without_an_insert_at_range_start():
    """first_gap and no_insert are unreachable (see the module's docstring): every slide of every case begins with an insert at rangeStart"""
    n = 0
    for name, f in P.CASES.items():
        for m in f()["facts"]:
            assert not m["no_insert"] and not m["first_gap"] and m["first_delta"] == 0, (name, m["cand"])
            n += 1
    assert n == 84
