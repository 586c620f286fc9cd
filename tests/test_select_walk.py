"""doL2Mapping's best-first walk -- mm_select_fragment (mashmap_amd/csrc/mm_select_core.h over mm_heap.h), the code k_l2_select compiles -- on
the planted inputs of tests/selplant.py, without a GPU.  For every fragment of every case: the facts the case is named for (from the oracle's
one session and mmhost::replayTables: a case that has left its edge fails here), walker (b) = the integer walk pushes exactly what walker
(a) = the float replay with libstdc++'s heap pushes, in its order, and what (a) pushes is, as a set, what the oracle's mapSingleQueryFrag
reports.  tests/test_gpu_select_edges.py runs the same cases on the device.

The cut-off table.  minIsz[Qs][best] is md2j(j2md(best / Qs)) counted up to an integer, which is not the identity in floating point: at
k = 16, s = 130, pi 0.85 it is best + 1 for 4284 of the 8515 pairs 1 <= best <= Qs and best for the other 4231 (test_cut_off_table).  At a
best + 1 entry a candidate whose intersectionSize EQUALS the best reported count is cut, and which one of a tie survives is decided by the
element movements of std::make_heap alone.

Two inputs no planted index gives (a locus shares at most its candidate's intersectionSize there) are walked as plain integers:
test_refused_locus_above_later_candidates and test_walkers_agree_on_random_integers."""
import numpy as np
import pytest

import mmutil as U
import selplant as P


def ids(c, f):
    return "%s fragment %d" % (c["name"], f)


def isz(fr): return [x[3] for x in fr["l1"]]
def shared(fr): return [x[5] for x in fr["l2"]]
def pushed(fr, w="a"): return [c for c, _ in fr[w]]


@pytest.mark.parametrize("name", list(P.CASES))
def test_walkers_and_oracle_agree(name):
    """(b) == (a) as sequences; (a) == the oracle's maps_i as sets; every planted candidate is there with the counts it was planted for"""
    c = P.CASES[name]()
    for f, fr in enumerate(c["per"]):
        assert [(q, m) for q, m, _ in fr["planted"]] == [(x[0], x[3]) for x in fr["l1"]] or name == "skip_prefix", ids(c, f)
        assert [x[0] for x in fr["l2"]] == list(range(len(fr["l1"]))), ids(c, f) + ": not one locus per candidate"
        if name != "skip_prefix": assert [sh for _, _, sh in fr["planted"]] == shared(fr), ids(c, f)
        assert fr["b"] == fr["a"], "%s: the integer walk pushes %r, the float replay %r" % (ids(c, f), fr["b"], fr["a"])
        got = sorted(P.pushed_records(fr))
        exp = sorted((m[5], m[1], m[9], m[10]) for m in fr["maps_i"])
        assert got == exp and len(set(got)) == len(got), ids(c, f)


def test_cut_off_table():
    acc, mi = P.tables()
    pairs = [(q, b) for q in range(1, P.S + 1) for b in range(1, q + 1)]
    assert sum(1 for q, b in pairs if mi[q, b] == b + 1) == 4284 and sum(1 for q, b in pairs if mi[q, b] == b) == 4231 and len(pairs) == 8515
    assert [b for b in range(1, 28) if mi[130, b] == b + 1] == [1, 2, 9, 10, 11, 12, 14, 15, 16, 19, 21, 24, 25, 26, 27]
    assert [b for b in range(1, 26) if mi[129, b] == b + 1] == [2, 4, 5, 6, 7, 8, 13, 14, 15, 21, 22, 23, 25]
    # the entries the cases stand on
    assert [int(mi[130, b]) for b in (3, 4, 5, 6, 7, 8, 9, 12)] == [3, 4, 5, 6, 7, 8, 10, 13] and int(mi[129, 9]) == 9 and int(mi[130, 0]) == 0
    assert P.first_accepted(130) == 3 and P.first_accepted(130, keep_low=False) == 6


def test_tie_at_a_cut_entry_leaves_one():
    c = P.CASES["ties_cut"]()
    assert int(P.tables()[1][130, P.T_CUT]) == P.T_CUT + 1
    winners = []
    for f, (n, fr) in enumerate(zip(P.TIE_N, c["per"])):
        assert fr["qs"] == 130 and isz(fr) == [P.T_CUT] * n and shared(fr) == [P.T_CUT] * n, ids(c, f)
        assert len(fr["maps_i"]) == 1 and len(fr["a"]) == 1, ids(c, f)
        winners.append(pushed(fr)[0])
        print("tie of %2d at %d: candidate %d is reported" % (n, P.T_CUT, winners[-1]))
    assert sum(1 for w in winners if w != 0) * 2 >= len(P.TIE_N), "taking the first maximum would pass: %r" % winners
    assert len(set(winners)) >= 6


def test_tie_at_a_plain_entry_keeps_all():
    c = P.CASES["ties_kept"]()
    assert int(P.tables()[1][130, P.T_KEPT]) == P.T_KEPT
    for f, (n, fr) in enumerate(zip(P.TIE_N, c["per"])):
        assert fr["qs"] == 130 and isz(fr) == [P.T_KEPT] * n and shared(fr) == [P.T_KEPT] * n, ids(c, f)
        assert len(fr["maps_i"]) == n and sorted(pushed(fr)) == list(range(n)), ids(c, f)
        assert pushed(fr) != list(range(n)), ids(c, f)                              # not the emission order
        if n > 3: assert pushed(fr) != list(range(n))[::-1], ids(c, f)              # nor (beyond three) its reverse
        print("tie of %2d at %d: push order %r" % (n, P.T_KEPT, pushed(fr)))


def test_levels():
    c = P.CASES["levels"]()
    for f, fr in enumerate(c["per"]):
        assert list(zip(isz(fr), shared(fr))) == c["expect"]["planted"][f], ids(c, f)
        assert [fr["l2"][i][5] for _, i in fr["a"]] == c["expect"]["reported"][f], ids(c, f)
    per = c["per"]
    assert isz(per[0])[pushed(per[0])[0]] == 12                                     # one 12; the other two 12s and the 9s are cut
    assert sorted(pushed(per[1])) == [i for i, m in enumerate(isz(per[1])) if m == 8]
    p2 = pushed(per[2])
    assert [isz(per[2])[i] for i in p2] == [8] * 3 + [5] * 5                         # best-first over two levels, each in heap order
    p3 = pushed(per[3])
    assert [isz(per[3])[i] for i in p3] == [11] * 2 + [7] * 4 + [4] * 5 and all(isz(per[3])[i] == 3 for i in set(range(13)) - set(p3))


def test_cut_between_two_lower_levels():
    c = P.CASES["cut_between"]()
    mi = P.tables()[1]
    for f, fr in enumerate(c["per"]):
        best = c["expect"]["best"][f]
        assert max(fr["l2"][i][5] for _, i in fr["a"]) == best and shared(fr)[2] == best and isz(fr)[2] > best + 2, ids(c, f)
        cut = int(mi[130, best])
        assert all(isz(fr)[i] == cut for i in (1, 3)) and all(isz(fr)[i] == cut - 1 for i in (0, 4)), ids(c, f)
        assert pushed(fr)[0] == 2 and sorted(pushed(fr)) == c["expect"]["walked"][f], ids(c, f)
    assert int(mi[130, 7]) == 7 and int(mi[130, 9]) == 10


@pytest.mark.parametrize("name,drop_low", [("acceptance", False), ("acceptance_drop_low_id", True)])
def test_acceptance_edge(name, drop_low):
    c = P.CASES[name]()
    a, fr = c["expect"]["a"], c["per"][0]
    acc, mi = P.tables(keep_low=not drop_low)
    assert acc[130, a] == 1 and acc[130, a - 1] == 0 and a == (6 if drop_low else 3) and int(mi[130, a]) == a and int(mi[130, 0]) == 0
    assert list(zip(isz(fr), shared(fr))) == c["expect"]["spec"]
    # candidate 1 is the heap's front and is refused: had it raised best to a - 1, or had a been one lower, the output would differ
    assert isz(fr)[1] == max(isz(fr)) and shared(fr)[1] == a - 1
    assert sorted(pushed(fr)) == [0, 3] and [m[9] for m in fr["maps_i"]] == [a, a]
    assert shared(fr)[2] == a - 1 and isz(fr)[2] == a                                # walked behind a reported one (minIsz[a] == a), refused
    if drop_low: assert isz(fr)[4] == a - 1 == shared(fr)[4]


def test_row_is_the_fragments_sketch_size():
    c = P.CASES["rows"]()
    f0, f1 = c["per"]
    mi = P.tables()[1]
    assert (f0["qs"], f1["qs"]) == (129, 130) and int(mi[129, 9]) == 9 and int(mi[130, 9]) == 10
    assert isz(f0) == isz(f1) == [9] * 6 and shared(f0) == shared(f1) == [9] * 6
    assert len(f0["maps_i"]) == 6 and len(f1["maps_i"]) == 1 and sorted(pushed(f0)) == list(range(6)) and len(f1["a"]) == 1


def test_without_the_hg_filter_candidate_order():
    c = P.CASES["hg_off"]()
    fr = c["per"][0]
    assert list(zip(isz(fr), shared(fr))) == c["expect"]["spec"]
    assert pushed(fr) == [i for i, sh in enumerate(shared(fr)) if sh >= 3] == [0, 2, 3, 4, 5, 6]


def test_best_starts_again_in_every_reference_group():
    c = P.CASES["skip_prefix"]()
    f0, f1 = c["per"]
    assert [x[0] for x in f0["l1"]] == [0] + [1] * 6 + [2] and isz(f0) == [12] + [9] * 6 + [5]
    p = pushed(f0)
    assert p[0] == 0 and p[-1] == 7 and len(p) == 3 and 1 <= p[1] <= 6 and p[1] != 1
    assert int(P.tables()[1][130, 12]) > 9 and int(P.tables()[1][130, 9]) > 5       # either best, kept, would have cut what follows
    assert [x[0] for x in f1["l1"]] == [0, 2] and len(f1["planted"]) == 8 and pushed(f1) == [0, 1]   # the read's own group B is skipped


def test_fragments_without_candidates_between():
    c = P.CASES["placement"]()
    assert [(fr["qs"], len(fr["l1"]), len(fr["a"])) for fr in c["per"]] == [(130, 6, 1), (130, 0, 0), (0, 0, 0), (130, 5, 1), (130, 0, 0), (130, 4, 4)]
    c = P.CASES["seam"]()
    assert len(c["per"]) == 257 and [f for f, fr in enumerate(c["per"]) if fr["l1"]] == [0, 255, 256]
    assert [len(c["per"][f]["a"]) for f in (0, 255, 256)] == [1, 1, 5]


def test_many_candidates():
    c = P.CASES["many"]()
    fr = c["per"][0]
    assert len(fr["l1"]) == P.MANY and list(zip(isz(fr), shared(fr))) == c["expect"]["planted"]
    p = pushed(fr)
    assert len(p) == c["expect"]["reported"] == len(set(p)) and all(isz(fr)[i] == 4 for i in set(range(P.MANY)) - set(p))
    lv = [isz(fr)[i] for i in p]
    assert lv == sorted(lv, reverse=True) and p != sorted(p, key=lambda i: (-isz(fr)[i], i))


# ----------------------------------------------------------------------------- plain integers
def walk_ints(flags, qs, cands, groups=None, s=P.S):
    """cands: [(seqId, intersectionSize, [shared of each locus])]"""
    l1 = [(q, 0, 0, m) for q, m, _ in cands]
    l2 = [(ci, q, 0, 0, 0, sh, 1) for ci, (q, _, shs) in enumerate(cands) for sh in shs]
    return P.walk(P.K, s, P.PI, flags, qs, l1, l2, groups, len(groups) if groups else 1 + max(q for q, _, _ in cands))


def test_refused_locus_above_later_candidates():
    """FLAG_DROP_LOW_ID, row 130: 6 is the first accepted count.  The front candidate's locus shares 5 and is refused; a candidate of
    intersectionSize 4 with a locus sharing 6 follows (a locus above its candidate's intersectionSize: nothing planted gives one).  A refused
    locus that raised best to 5 would cut it (minIsz[130][5] == 5)"""
    a, b = walk_ints(P.HG | U.FLAG_DROP_LOW_ID, 130, [(0, 20, [5]), (0, 4, [6])])
    assert a == [(1, 1)] and b == a


def test_count_beyond_the_sketch_reads_no_other_row():
    """A locus cannot share more hashes than the fragment's sketch holds, and the float expressions have no meaning there (a Jaccard above 1), so
    walker (a) is not asked.  The integer walk must refuse such a count by its own guard and not look it up: row Qs ends at Qs, and entry
    134 of row 129 IS entry 3 of row 130 -- an accepted count"""
    acc = P.tables()[0]
    assert acc.shape == (131, 131) and acc.reshape(-1)[129 * 131 + 134] == acc[130, 3] == 1
    _, b = walk_ints(0, 129, [(0, 9, [134])])
    assert b == []
    _, b = walk_ints(P.HG, 129, [(0, 10, [134]), (0, 9, [9])])
    assert [c for c, _ in b] == [1]


def test_walkers_agree_on_random_integers():
    """400 fragments of random integers -- up to 40 candidates of 0 .. 3 loci each, counts drawn from a narrow band so that ties are the rule,
    shared independent of intersectionSize but never above Qs, every flag combination, reference groups of random length"""
    r = iter(U.splitmix64(424242, 400 * 400).tolist())
    nxt = lambda n: next(r) % n
    pushes = 0
    for it in range(400):
        qs = (130, 129, 64, 17)[nxt(4)]
        flags = (P.HG if nxt(4) else 0) | (U.FLAG_SKIP_PREFIX if nxt(3) == 0 else 0) | (U.FLAG_DROP_LOW_ID if nxt(3) == 0 else 0)
        lo = nxt(12); span = 1 + nxt(6)
        nC = 1 + nxt(40)
        seqs = sorted(nxt(6) for _ in range(nC))
        cands = [(seqs[i], min(qs, lo + nxt(span)), [min(qs, lo + nxt(span + 2)) for _ in range(nxt(4))]) for i in range(nC)]
        groups = None
        if flags & U.FLAG_SKIP_PREFIX:
            groups, g = [], 0
            for q in range(6):
                groups.append(g)
                if nxt(2): g += 1
        a, b = walk_ints(flags, qs, cands, groups)
        assert a == b, (it, flags, qs, cands, groups, a, b)
        pushes += len(a)
    assert pushes > 2000
