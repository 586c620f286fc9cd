"""MM_OPT_L1_GROUP_FUSED: under -Y reference groups (MM_FLAG_SKIP_PREFIX) the fragments k_lookup_l1 queued go through k_lookup_groups --
one wave per fragment, the points of one reference group at a time sorted in registers and swept by the fused L1 -- and the HBM point path
(gather, sort, k_l1_stream_groups / k_l1_sweep) is left with what that kernel hands over.

Every case first derives its figures from the oracle on the CPU and asserts them -- the condition a case exists for holds for the oracle
alone --, states the expected hand-over list with `handover_reasons`, a restatement of the kernel's rules over the oracle's per-fragment
point lists, and then maps the batch on fresh contexts without the option, with it, and with it beside MM_OPT_L1_GROUP_STREAM: stats,
L1, L2 and candidate mappings byte-identical, L1 per fragment the oracle's, offered = fragments with points, fused = offered - expected
hand-overs, pass_l1_literal()[0] = offered - fused.

k = 16, segLength 500, s = 32, pi 0.90; kmerThreshold 0 where copies are planted (no seed is frequent)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import gpucheck
import mmutil as U
import test_gpu_group_stream as G
import test_gpu_skip_prefix_stream as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BIN = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
GOLDEN_PAF = os.path.join(ROOT, "tests", "golden", "paf", "group_fused_case_groups.paf")
K, L, S, PI = T.K, T.L, T.S, T.PI
# mm_map.hip: MM_GRP_MAXPTS, MM_GRP_MAXGROUPS, MM_GRP_MAXKEEP, MM_GRP_MAXCAND, MM_FUSE_MAXRUNS
MAXPTS, MAXGROUPS, MAXKEEP, MAXCAND, MAXRUNS = 8192, 64, 1024, 128, 64
MM_ERR_STATE = -3
COMMAND_LINE_SETS_THE_OPTION = False                             # what the probe of profiles/NOTES.md decided for skch::Sketch under -Y


# ----------------------------------------------------------------------------- the oracle's view and the model of the hand-over rules
def read_ids(contigs, reads):
    """what the host derives from a read's name: its reference group (the group of the first contig with the same prefix, -1 when none)
    and the contig that carries its name (-1 when none)"""
    names = [n for n, _ in contigs]
    pre, grp = gpucheck.prefix_groups(names, "#")
    rgs, selfs = [], []
    for name, _ in reads:
        p = name[:name.rfind("#")] if "#" in name else name
        rgs.append(next((grp[i] for i in range(len(pre)) if pre[i] == p), -1))
        selfs.append(names.index(name) if name in names else -1)
    return rgs, selfs


def oracle_view(oracle, contigs, reads, flags, kmerPct=0.0, base=0):
    """per fragment, in the device's fragment order: the sorted interval points after the seqId filters, Q.sketchSize, the oracle's L1, and
    `raw`, the number of interval points before the filters (the same index asked without them); and the sketch cutoffs"""
    h = oracle.session(contigs, K, L, S, PI, U.FILTER_MAP, flags, b"#", kmerPct)
    h0 = oracle.session(contigs, K, L, S, PI, U.FILTER_MAP, flags & U.FLAG_HG, b"#", kmerPct)
    out = []
    for ri, (name, a) in enumerate(reads):
        for at, ln in T.fragments_of(a):
            e = oracle.map_fragment(h, a[at:at + ln], base + ri, name.encode(), len(a), S)
            e0 = oracle.map_fragment(h0, a[at:at + ln], base + ri, name.encode(), len(a), S)
            out.append(dict(points=[p[:3] for p in e["points"]], q=e["sketchSize"], l1=e["l1"], raw=len(e0["points"])))
    cut = oracle.cutoffs(h)
    oracle.free(h); oracle.free(h0)
    return out, cut


def runs_of(x, q, base, cut, hg):
    """candidate runs of one computeL1CandidateRegions call before they are joined: maximal runs of consecutive position groups on one
    contig -- the last group excluded -- whose overlap count reaches minimumHits (after the sketchCutoffs step under hg)"""
    groups, run = [], 0
    for i, p in enumerate(x):
        run += 1 if p[2] == 1 else -1
        if i + 1 == len(x) or x[i + 1][1] != p[1]: groups.append((p[0], run))
    mh = base
    if hg:
        mh = G.raised_min_hits(max([0] + [c for _, c in groups]), q, base, cut)
        if mh is None: return 0
    flag = [i < len(groups) - 1 and c >= mh for i, (_, c) in enumerate(groups)]
    return sum(1 for i in range(len(groups)) if flag[i] and not (i > 0 and flag[i - 1] and groups[i - 1][0] == groups[i][0]))


def handover_reasons(fr, mh_tab, cut, hg, rg):
    """k_lookup_groups' rules on one fragment, from the oracle's lists: every reason it is handed over for (none: it is finished there)"""
    pts, q = fr["points"], fr["q"]
    why = []
    if fr["raw"] > MAXPTS: why.append("points")
    if len({rg[p[0]] for p in pts}) > MAXGROUPS: why.append("groups")
    ext = G.extents(pts, rg)
    if any(e - b > MAXKEEP for b, e in ext): why.append("extent")
    base = int(mh_tab[q]) if q > 0 else 0
    if base <= 0: why.append("minimumHits")
    for b, e in ext:
        x = pts[b:e]
        if any(x[i][1] == x[i - 1][1] and x[i][0] != x[i - 1][0] for i in range(1, len(x))): why.append("mixed")
        elif base > 0 and runs_of(x, q, base, cut, hg) > MAXRUNS: why.append("runs")
    if len(fr["l1"]) > MAXCAND: why.append("candidates")
    return why


def max_runs(per, mh_tab, cut, hg, rg):
    return max([0] + [runs_of(fr["points"][b:e], fr["q"], int(mh_tab[fr["q"]]), cut, hg) for fr in per for b, e in G.extents(fr["points"], rg)])


# ----------------------------------------------------------------------------- the device's view
def run_y(oracle, contigs, reads, hg, fused, stream=False, kmerPct=0.0, extra=0, base=0, rg=None, keep=False, min_hits=None, points_of=None):
    """one sized -Y pass over the batch on a fresh context; `extra`: FLAG_SKIP_SELF / FLAG_LOWER_TRI on top; rg: the refGroup array
    passed to index_upload instead of the names' groups; min_hits: the table passed to set_tables instead of the oracle's"""
    from mashmap_amd import capi
    flags = U.FLAG_SKIP_PREFIX | (U.FLAG_HG if hg else 0) | extra
    h = oracle.session(contigs, K, L, S, PI, U.FILTER_MAP, flags, b"#", kmerPct)
    ix = oracle.export_index(h)
    ctx = capi.Context(k=K, segLength=L, sketchSize=S, flags=flags)       # (FLAG_HG .. FLAG_LOWER_TRI are MM_FLAG_*'s values)
    assert (capi.MM_FLAG_HG_FILTER, capi.MM_FLAG_SKIP_SELF, capi.MM_FLAG_SKIP_PREFIX, capi.MM_FLAG_LOWER_TRIANGULAR) == \
        (U.FLAG_HG, U.FLAG_SKIP_SELF, U.FLAG_SKIP_PREFIX, U.FLAG_LOWER_TRI)
    if fused: ctx.l1_group_fused(True)
    if stream: ctx.l1_group_stream(True)
    if keep: ctx.keep_points(True)
    if rg is None: rg = gpucheck.prefix_groups([n for n, _ in contigs], "#")[1]
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"], rg)
    ctx.set_tables(oracle.min_hits_table(S, K, PI) if min_hits is None else min_hits, oracle.cutoffs(h))
    ctx.set_replay_tables(*capi.stat_replay_tables(S, K, PI, 0.0, True))
    rgs, selfs = read_ids(contigs, reads)
    ctx.reads_upload([a for _, a in reads], rgs, selfs, base)
    ctx.map()
    offered, nfused = ctx.pass_l1_group_fused()
    queued, literal = ctx.pass_l1_literal()
    stats, l1, l2 = ctx.results()
    per = {}
    for c in l1:
        per.setdefault(int(c["frag"]), []).append((int(c["seqId"]), int(c["rangeStartPos"]), int(c["rangeEndPos"]), int(c["intersectionSize"])))
    out = dict(offered=offered, fused=nfused, queued=queued, literal=literal, stats=stats.tobytes(), l1=l1.tobytes(), l2=l2.tobytes(),
               mappings=ctx.mappings().tobytes(), l1_per_frag=[per.get(f, []) for f in range(len(stats))],
               n_points=[int(x) for x in stats["nPoints"]])
    if points_of is not None:
        try:
            ctx.points(points_of); out["points_error"] = None
        except capi.MashmapError as e:
            out["points_error"] = str(e)
    ctx.close(); oracle.free(h)
    return out


def check_all_ways(oracle, contigs, reads, hg, per, cut, kmerPct=0.0, extra=0, base=0):
    """the batch without the option, with it, and with it beside MM_OPT_L1_GROUP_STREAM; returns (run with the option alone, expected
    hand-overs as {fragment: reasons})"""
    rg = gpucheck.prefix_groups([n for n, _ in contigs], "#")[1]
    mh = oracle.min_hits_table(S, K, PI)
    queued_by_lookup = [i for i, fr in enumerate(per) if fr["raw"] > 0]            # k_lookup_l1 queues by the points before the filters
    expected = {i: handover_reasons(per[i], mh, cut, hg, rg) for i in queued_by_lookup}
    expected = {i: why for i, why in expected.items() if why}
    off = run_y(oracle, contigs, reads, hg, False, False, kmerPct, extra, base)
    on = run_y(oracle, contigs, reads, hg, True, False, kmerPct, extra, base)
    both = run_y(oracle, contigs, reads, hg, True, True, kmerPct, extra, base)
    print("offered %d, fused %d, expected hand-overs %r; point path: queued %d, literal %d alone / %d beside the grouped wave kernel"
          % (on["offered"], on["fused"], expected, on["queued"], on["literal"], both["literal"]))
    assert (off["offered"], off["fused"]) == (0, 0) and off["queued"] == len(queued_by_lookup)
    for r in (on, both):
        assert r["offered"] == len(queued_by_lookup)
        assert r["fused"] == r["offered"] - len(expected), (r["fused"], expected)
        assert r["queued"] == r["offered"] - r["fused"]
        for what in ("stats", "l1", "l2", "mappings"):
            assert len(r[what]) > 0 and r[what] == off[what], "with the option the pass disagrees on " + what
    assert on["literal"] == on["queued"]                          # without MM_OPT_L1_GROUP_STREAM the literal kernel takes every handed-over fragment
    assert both["literal"] <= both["queued"]
    assert len(on["l1_per_frag"]) == len(per)
    for f, fr in enumerate(per):
        assert on["l1_per_frag"][f] == fr["l1"], ("fragment %d" % f, on["l1_per_frag"][f][:4], fr["l1"][:4])
        assert on["n_points"][f] == len(fr["points"]), ("fragment %d" % f, on["n_points"][f], len(fr["points"]))
    return on, expected


def describe(per, rg):
    return [(fr["raw"], len(fr["points"]), [e - b for b, e in G.extents(fr["points"], rg)], len(fr["l1"])) for fr in per]


def groups_of(contigs):
    return gpucheck.prefix_groups([n for n, _ in contigs], "#")[1]


# ----------------------------------------------------------------------------- 1: the group batch of test_gpu_skip_prefix_stream
@functools.lru_cache(maxsize=None)
def _case_groups():
    return T.case_groups(U.Oracle())


@pytest.mark.gpu
@pytest.mark.parametrize("hg", [True, False], ids=["hg", "nohg"])
def test_group_batch_is_fused_but_for_the_mixed_position_group(oracle, hg):
    cs, reads = _case_groups()
    rg = groups_of(cs)
    assert rg == [0, 0, 1, 1, 2, 2, 3, 4]                         # A#1 comes back behind C#1 as a group of its own: ascending group = extent order
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX | (U.FLAG_HG if hg else 0), kmerPct=0.001)
    mh = oracle.min_hits_table(S, K, PI)
    assert max_runs(per, mh, cut, hg, rg) < MAXRUNS
    assert any(len({rg[p[0]] for p in fr["points"]}) == 5 for fr in per)          # a fragment with an extent in every group, A#1's second one included
    on, expected = check_all_ways(oracle, cs, reads, hg, per, cut, kmerPct=0.001)
    frag_of_r12 = sum(len(T.fragments_of(a)) for _, a in reads[:12])
    assert reads[12][0] == "r12" and expected == {frag_of_r12: ["mixed"]}         # its points in B#1#x / B#1#y share a position inside one extent
    assert on["offered"] == 43 and 0 < on["fused"] < on["offered"]


@pytest.mark.gpu
def test_group_batch_with_the_tagged_seed_table(oracle, monkeypatch):
    """the kernel's other instantiation: MM_SEED_TAGS=1 puts the tag layer in front of the seed table whatever its size (the library
    reads the switch when a context is created)"""
    monkeypatch.setenv("MM_SEED_TAGS", "1")
    cs, reads = _case_groups()
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX | U.FLAG_HG, kmerPct=0.001)
    on, expected = check_all_ways(oracle, cs, reads, True, per, cut, kmerPct=0.001)
    assert list(expected.values()) == [["mixed"]] and on["fused"] == 42


# ----------------------------------------------------------------------------- 2: a position shared across a group boundary
@pytest.mark.gpu
def test_position_shared_across_a_group_boundary_is_finished_by_the_kernel(oracle):
    cs, reads = G.case_boundary(oracle)
    rg = groups_of(cs)
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX | U.FLAG_HG, kmerPct=0.001)
    pts = per[0]["points"]
    last1 = [p for p in pts if p[0] == 1][-1]; first2 = [p for p in pts if p[0] == 2][0]
    assert last1[1] == first2[1] and rg[1] != rg[2]               # neighbours in the sorted list that share a position, of two extents
    assert max_runs(per, oracle.min_hits_table(S, K, PI), cut, True, rg) < MAXRUNS
    on, expected = check_all_ways(oracle, cs, reads, True, per, cut, kmerPct=0.001)
    assert expected == {} and on["fused"] == on["offered"] > 0


# ----------------------------------------------------------------------------- 3: reads that belong to a reference group
def case_own_group():
    """four groups of two contigs, one locus in every contig at 1 % (its own haplotype) to 6 % (the others); reads cut from group B's
    copy and named with B's prefix -- one of them with the very name of a contig"""
    names = ["A#1#x", "A#1#y", "B#1#x", "B#1#y", "C#1#x", "C#1#y", "D#1#x", "D#1#y"]
    src = U.random_dna(611, 3000)
    cs = T.genome(29, names, 12000)
    for ci, (nm, _) in enumerate(cs): T.plant(cs, nm, 1500 + ci * 700, T.subst(src, 620 + ci, 0.004 if nm.startswith("B") else 0.06))
    b_copy = dict(cs)["B#1#x"][1500 + 2 * 700:1500 + 2 * 700 + 3000]
    reads = [("B#1#q%d" % i, a) for i, (_, a) in enumerate(T.reads_from(b_copy, 70, 3, 2 * L + 41, 0.01))]
    reads.append(("B#1#y", T.subst(b_copy[400:400 + L + 200], 71, 0.01)))
    reads.append(("r4", T.subst(b_copy[900:900 + L + 100], 72, 0.01)))             # of no group: nothing dropped
    return cs, reads


@pytest.mark.gpu
@pytest.mark.parametrize("extra,base", [(0, 0), (U.FLAG_SKIP_SELF | U.FLAG_LOWER_TRI, 5)], ids=["prefix", "prefix_self_lowertri_base5"])
def test_reads_of_a_reference_group_lose_their_own_group(oracle, extra, base):
    cs, reads = case_own_group()
    rg = groups_of(cs)
    rgs, selfs = read_ids(cs, reads)
    assert rgs == [1, 1, 1, 1, -1] and selfs == [-1, -1, -1, 3, -1]
    free, _ = oracle_view(oracle, cs, reads, U.FLAG_HG, base=base)
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX | U.FLAG_HG | extra, base=base)
    n_own = 0
    for fr0, fr in zip(free[:-2], per[:-2]):                     # the fragments of the reads of group B
        best = max(fr0["l1"], key=lambda c: c[3])
        assert rg[best[0]] == 1                                   # without -Y their own group holds the best candidate ...
        assert fr["points"] and all(rg[p[0]] != 1 for p in fr["points"])           # ... with it no point of that group remains
        n_own += sum(1 for p in fr0["points"] if rg[p[0]] == 1)
    assert n_own > 0 and all(fr["raw"] < MAXPTS // 8 for fr in per)
    if extra:                                                     # lower-triangular: seqCounter = 5 + read > seqId keeps the contigs below it only
        assert any(len(fr["points"]) < sum(1 for p in fr0["points"] if rg[p[0]] != 1) for fr0, fr in zip(free, per))
        assert all(p[0] < base + len(reads) for fr in per for p in fr["points"])
    assert max_runs(per, oracle.min_hits_table(S, K, PI), cut, True, rg) < MAXRUNS
    on, expected = check_all_ways(oracle, cs, reads, True, per, cut, extra=extra, base=base)
    assert expected == {} and on["fused"] == on["offered"] == len(per)


# ----------------------------------------------------------------------------- 4: sorter tiers and the extent cap
TIER_COPIES = (3, 4, 9, 20)                                      # an exact copy brings 70 .. 105 points with it, by the locus


def case_tiers():
    """group T<c> holds locus c (600 bp) c times, far apart, over its two contigs; group P holds every locus once.  A read cut from
    locus c has two extents: c copies' points in T<c> and one copy's in P"""
    loci = {c: U.random_dna(sd, 600) for c, sd in zip(TIER_COPIES, (703, 706, 712, 720))}
    names = ["T%d#1#%s" % (c, x) for c in TIER_COPIES for x in "xy"] + ["P#1#x"]
    cs = T.genome(31, names, 20000)
    for c in TIER_COPIES:
        for j in range(c): T.plant(cs, "T%d#1#%s" % (c, "xy"[j % 2]), 700 + (j // 2) * 1900, loci[c])
    for i, c in enumerate(TIER_COPIES): T.plant(cs, "P#1#x", 1000 + i * 2500, loci[c])
    reads = [("r%d" % i, np.ascontiguousarray(loci[c][50:50 + L])) for i, c in enumerate(TIER_COPIES)]
    return cs, reads


@pytest.mark.gpu
def test_sorter_tiers_and_the_extent_cap(oracle):
    cs, reads = case_tiers()
    rg = groups_of(cs)
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX | U.FLAG_HG)
    sizes = [[e - b for b, e in G.extents(fr["points"], rg)] for fr in per]
    print("(raw, kept, extents, nL1) per fragment: %r" % describe(per, rg))
    assert [len(s) for s in sizes] == [2, 2, 2, 2]
    assert 129 <= sizes[0][0] <= 256 and 257 <= sizes[1][0] <= 512 and 513 <= sizes[2][0] <= 1024 and sizes[3][0] > 1024          # 4-, 8-, 16-per-lane sorters, over the cap
    assert all(64 < s[1] <= 128 for s in sizes)                   # the plain group: the two-per-lane sorter
    assert max_runs(per, oracle.min_hits_table(S, K, PI), cut, True, rg) < MAXRUNS
    on, expected = check_all_ways(oracle, cs, reads, True, per, cut)
    assert expected == {3: ["extent"]} and on["fused"] == 3


# ----------------------------------------------------------------------------- 5: the fragment's point cap
def case_point_cap():
    """locus X 13 times in each of 9 groups (over the cap of 8 192 points, every extent under 1 024), locus Y 13 times in 8 of them (under it)"""
    X, Y = U.random_dna(801, 600), U.random_dna(802, 600)
    names = ["g%d#1#x" % g for g in range(9)]
    cs = T.genome(37, names, 52000)
    for g, (nm, _) in enumerate(cs):
        for j in range(13):
            T.plant(cs, nm, 500 + j * 3400, X)
            if g < 8: T.plant(cs, nm, 500 + j * 3400 + 1700, Y)
    reads = [("r0", np.ascontiguousarray(X[40:40 + L])), ("r1", np.ascontiguousarray(Y[40:40 + L]))]
    return cs, reads


@pytest.mark.gpu
def test_more_points_than_the_tag_array_holds(oracle):
    cs, reads = case_point_cap()
    rg = groups_of(cs)
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX | U.FLAG_HG)
    print("(raw, kept, extents, nL1) per fragment: %r" % describe(per, rg))
    ext = [[e - b for b, e in G.extents(fr["points"], rg)] for fr in per]
    assert per[0]["raw"] > MAXPTS and max(ext[0]) <= MAXKEEP and len(ext[0]) == 9 and len(per[0]["l1"]) <= MAXCAND
    assert MAXPTS - 1024 < per[1]["raw"] <= MAXPTS and max(ext[1]) <= MAXKEEP and len(ext[1]) == 8 and len(per[1]["l1"]) <= MAXCAND
    assert max_runs(per, oracle.min_hits_table(S, K, PI), cut, True, rg) < MAXRUNS
    on, expected = check_all_ways(oracle, cs, reads, True, per, cut)
    assert expected == {0: ["points"]} and on["fused"] == 1


# ----------------------------------------------------------------------------- 6: the group table
def case_group_cap():
    """65 groups of one contig; locus X once in each of them, locus Y in the first 64"""
    X, Y = U.random_dna(811, 600), U.random_dna(812, 600)
    names = ["g%02d#1#x" % g for g in range(65)]
    cs = T.genome(41, names, 4000)
    for g, (nm, _) in enumerate(cs):
        T.plant(cs, nm, 500, X)
        if g < 64: T.plant(cs, nm, 2300, Y)
    reads = [("r0", np.ascontiguousarray(X[40:40 + L])), ("r1", np.ascontiguousarray(Y[40:40 + L]))]
    return cs, reads


@pytest.mark.gpu
def test_more_groups_than_the_group_table_holds(oracle):
    cs, reads = case_group_cap()
    rg = groups_of(cs)
    assert rg == list(range(65))
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX | U.FLAG_HG)
    ngroups = [len({rg[p[0]] for p in fr["points"]}) for fr in per]
    print("(raw, kept, extents, nL1) per fragment: %r" % describe(per, rg))
    assert ngroups == [65, 64] and all(fr["raw"] <= MAXPTS and len(fr["l1"]) <= MAXCAND for fr in per)
    assert max_runs(per, oracle.min_hits_table(S, K, PI), cut, True, rg) < MAXRUNS
    on, expected = check_all_ways(oracle, cs, reads, True, per, cut)
    assert expected == {0: ["groups"]} and on["fused"] == 1


# ----------------------------------------------------------------------------- 7: the candidate list
def case_candidate_cap():
    """copies with 5 % substitutions (about half the seeds of an exact copy: the points stay under the cap), 7 per group, more than a
    segment apart so that none are joined: locus X in 21 groups (147 copies), locus Y in 16 (112)"""
    X, Y = U.random_dna(821, 600), U.random_dna(822, 600)
    names = ["g%02d#1#x" % g for g in range(21)]
    cs = T.genome(43, names, 24000)
    for g, (nm, _) in enumerate(cs):
        for j in range(7):
            T.plant(cs, nm, 500 + j * 3300, T.subst(X, 9000 + g * 16 + j, 0.05))
            if g < 16: T.plant(cs, nm, 500 + j * 3300 + 1650, T.subst(Y, 9500 + g * 16 + j, 0.05))
    reads = [("r0", np.ascontiguousarray(X[40:40 + L])), ("r1", np.ascontiguousarray(Y[40:40 + L]))]
    return cs, reads


@pytest.mark.gpu
def test_more_candidates_than_the_output_list_holds(oracle):
    cs, reads = case_candidate_cap()
    rg = groups_of(cs)
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX)
    print("(raw, kept, extents, nL1) per fragment: %r" % describe(per, rg))
    for fr in per:
        ext = [e - b for b, e in G.extents(fr["points"], rg)]
        assert fr["raw"] <= MAXPTS and len(ext) <= MAXGROUPS and max(ext) <= MAXKEEP
    assert len(per[0]["l1"]) > MAXCAND and 100 <= len(per[1]["l1"]) <= MAXCAND
    assert max_runs(per, oracle.min_hits_table(S, K, PI), cut, False, rg) < MAXRUNS
    on, expected = check_all_ways(oracle, cs, reads, False, per, cut)
    assert expected == {0: ["candidates"]} and on["fused"] == 1


# ----------------------------------------------------------------------------- 8: minimumHits <= 0
@pytest.mark.gpu
def test_minimum_hits_zero_is_handed_over(oracle):
    """The oracle's table of minimum hits never holds a 0 for a sketch with a seed (and every sketch of this batch is full), so a
    table of zeros is passed to set_tables -- the table is the caller's: every fragment is handed over, and the bytes are those of the
    pass without the option over the same table.  (No oracle L1 here: the oracle has its own table.)"""
    cs, reads = _case_groups()
    rg = groups_of(cs)
    per, cut = oracle_view(oracle, cs, reads, U.FLAG_SKIP_PREFIX | U.FLAG_HG, kmerPct=0.001)
    mh = oracle.min_hits_table(S, K, PI)
    assert all(int(x) > 0 for x in mh[1:])
    mh = np.zeros_like(mh)
    queued = [i for i, fr in enumerate(per) if fr["raw"] > 0]
    assert len(queued) == 43 and all("minimumHits" in handover_reasons(per[i], mh, cut, True, rg) for i in queued)
    off = run_y(oracle, cs, reads, True, False, False, 0.001, min_hits=mh)
    for stream in (False, True):
        on = run_y(oracle, cs, reads, True, True, stream, 0.001, min_hits=mh)
        assert (on["offered"], on["fused"], on["queued"], on["literal"]) == (43, 0, 43, 43)      # the grouped wave kernel leaves them to the literal one too
        for what in ("stats", "l1", "l2", "mappings"):
            assert len(on[what]) > 0 and on[what] == off[what], "with the option the pass disagrees on " + what


# ----------------------------------------------------------------------------- 9: the conditions under which the kernel is not launched
@pytest.mark.gpu
def test_not_launched_for_groups_out_of_order_or_kept_points(oracle):
    cs, reads = _case_groups()
    jumbled = [0, 1, 0, 1, 2, 2, 3, 4]                            # a refGroup array no Map::setRefGroups would number: not non-decreasing
    assert any(a > b for a, b in zip(jumbled, jumbled[1:]))
    for kw in (dict(rg=jumbled), dict(keep=True)):
        off = run_y(oracle, cs, reads, True, False, True, 0.001, **kw)
        on = run_y(oracle, cs, reads, True, True, True, 0.001, **kw)
        assert (on["offered"], on["fused"]) == (0, 0), kw
        assert on["queued"] == off["queued"] > 0 and on["literal"] == off["literal"]
        for what in ("stats", "l1", "l2", "mappings"):
            assert len(on[what]) > 0 and on[what] == off[what], "an option that does nothing here changed " + what
    launched = run_y(oracle, cs, reads, True, True, True, 0.001)  # the same batch with its groups in order and no kept points: launched
    assert launched["offered"] == 43 and launched["fused"] > 0


# ----------------------------------------------------------------------------- 10: mm_points_download
@pytest.mark.gpu
def test_points_download_names_the_option(oracle):
    cs, reads = _case_groups()
    on = run_y(oracle, cs, reads, True, True, False, 0.001, points_of=0)
    assert on["points_error"] is not None and "(%d)" % MM_ERR_STATE in on["points_error"] and "MM_OPT_L1_GROUP_FUSED" in on["points_error"]
    assert run_y(oracle, cs, reads, True, False, False, 0.001, points_of=0)["points_error"] is None          # without the option: today's answer
    assert run_y(oracle, cs, reads, True, True, False, 0.001, keep=True, points_of=0)["points_error"] is None   # MM_OPT_KEEP_POINTS keeps them


# ----------------------------------------------------------------------------- the command line
def write_case_groups_fasta(tmp_path):
    cs, reads = _case_groups()
    ref, qry = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    U.write_fasta(ref, cs); U.write_fasta(qry, reads)
    return ref, qry


CLI_ARGS = ["-Y", "#", "-k", "16", "-s", "500", "--pi", "90", "-t", "4"]


@pytest.mark.gpu
def test_command_line_paf_is_the_stock_binarys(tmp_path):
    """mashmap_hip -Y '#' on case 1's sequences: the PAF is the stock binary's -- the copy of it under tests/golden/paf/, and a live run
    where oracle/_ref/mashmap_ref is there"""
    assert os.path.exists(HIP_BIN), "mashmap_hip not built"
    ref, qry = write_case_groups_fasta(tmp_path)
    paf = str(tmp_path / "hip.paf")
    p = subprocess.run([HIP_BIN, "-r", ref, "-q", qry, "-o", paf] + CLI_ARGS, capture_output=True, text=True, timeout=240, env=dict(os.environ, MM_DEBUG="1"))
    assert p.returncode == 0, p.stderr[-3000:]
    got = open(paf, "rb").read()
    took = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"(\d+) fragments offered to k_lookup_groups, (\d+) fused, (\d+) handed over", p.stderr)]
    print("%d PAF lines; (offered, fused, handed over) per pass %r" % (got.count(b"\n"), took))
    assert got.count(b"\n") > 0 and got == open(GOLDEN_PAF, "rb").read()
    if os.path.exists(U.REF_BIN):
        live = str(tmp_path / "ref.paf")
        q = subprocess.run([U.REF_BIN, "-r", ref, "-q", qry, "-o", live] + CLI_ARGS, capture_output=True, text=True, timeout=240)
        assert q.returncode == 0, q.stderr[-3000:]
        assert got == open(live, "rb").read()
    assert all(a == b + c for a, b, c in took)
    assert COMMAND_LINE_SETS_THE_OPTION == bool(took and sum(b for _, b, _ in took) > 0)
