"""MM_OPT_L2_WINDOW_WAVE: the L2 stage of a batch with a read longer than segLength (MM_FLAG_NO_SPLIT, windowLen != 0) on k_l2_window_wave,
one wave per L1 candidate with the candidate's sketch, SlideMapper cells and heap of open records in LDS and 64 events of the index per
step; the literal k_l2_window takes the candidates it hands over.

Every case first derives its figures on the CPU -- from the oracle and tests/winmodel.py's model of the reference's window bookkeeping
over the oracle's index -- and asserts the conditions it exists for, then maps the batch twice on fresh contexts, with the option and
without it: stats, L1, L2 and candidate mappings byte-identical, L2 equal to the oracle's per fragment and candidate, and pass_l2_window()
(n, n) without the option and (n, the model's count of handed-over candidates) with it.

k 16, segLength 1000, s 80, pi 0.85, kmerThreshold 0 (tests/winmodel.py); contigs of 90 kbp."""
import os
import re

import numpy as np
import pytest

import gpucheck
import mmutil as U
import winmodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_batch(orc, contigs, reads, hg, grouped=False):
    """per read: the oracle's L1, its loci per candidate, and the model's figures per candidate"""
    flags = U.FLAG_NOSPLIT | (U.FLAG_HG if hg else 0) | (U.FLAG_SKIP_PREFIX if grouped else 0)
    h = orc.session(contigs, M.K, M.L, M.S, M.PI, U.FILTER_MAP, flags, b"#" if grouped else b"\0", 0.0)
    idx = orc.index_array(h)
    per = []
    for name, a in reads:
        e = orc.map_fragment(h, a, len(per), name.encode(), len(a), M.S)
        loci = [[] for _ in e["l1"]]
        for x in e["l2"]: loci[x[0]].append(x[1:])
        W = max(0, len(a) - M.L)
        per.append(dict(l1=e["l1"], l2=loci, W=W, fig=[M.figures(idx, c, W) for c in e["l1"]]))
    orc.free(h)
    return per


def run(orc, contigs, reads, hg, option, grouped=False, nosplit=True, passes=1):
    """`passes` map() calls over the batch on a fresh context, with or without the option: (candidates, literal), pass_stats of the last
    pass, and everything it leaves, as bytes and per fragment"""
    from mashmap_amd import capi
    flags = (U.FLAG_NOSPLIT if nosplit else 0) | (U.FLAG_HG if hg else 0) | (U.FLAG_SKIP_PREFIX if grouped else 0)
    h = orc.session(contigs, M.K, M.L, M.S, M.PI, U.FILTER_MAP, flags, b"#" if grouped else b"\0", 0.0)
    ix = orc.export_index(h)
    cflags = (capi.MM_FLAG_NO_SPLIT if nosplit else 0) | (capi.MM_FLAG_HG_FILTER if hg else 0) | (capi.MM_FLAG_SKIP_PREFIX if grouped else 0)
    ctx = capi.Context(k=M.K, segLength=M.L, sketchSize=M.S, flags=cflags)
    if option: ctx.l2_window_wave(True)
    rg = gpucheck.prefix_groups([n for n, _ in contigs], "#")[1] if grouped else None
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"], rg)
    ctx.set_tables(orc.min_hits_table(M.S, M.K, M.PI), orc.cutoffs(h))
    ctx.set_replay_tables(*capi.stat_replay_tables(M.S, M.K, M.PI, 0.0, True))
    ctx.reads_upload([a for _, a in reads], [-1] * len(reads) if grouped else None, [-1] * len(reads), 0)
    for _ in range(passes): ctx.map()
    cands, literal = ctx.pass_l2_window()
    stats, l1, l2 = ctx.results()
    l2_by_c = {}
    for x in l2:
        l2_by_c.setdefault(int(x["cand"]), []).append((int(x["seqId"]), int(x["meanOptimalPos"]), int(x["optimalStart"]), int(x["optimalEnd"]),
                                                       int(x["sharedSketchSize"]), int(x["strand"])))
    per = [dict(l1=[], l2=[]) for _ in range(len(stats))]
    for gi, c in enumerate(l1):
        f = per[int(c["frag"])]
        f["l1"].append((int(c["seqId"]), int(c["rangeStartPos"]), int(c["rangeEndPos"]), int(c["intersectionSize"])))
        f["l2"].append(l2_by_c.get(gi, []))
    out = dict(cands=cands, literal=literal, pass_stats=ctx.pass_stats(), stats=stats.tobytes().hex(), l1=l1.tobytes().hex(), l2=l2.tobytes().hex(),
               mappings=ctx.mappings().tobytes().hex(), per=per)
    ctx.close(); orc.free(h)
    return out


def check_both_ways(orc, contigs, reads, hg, per, grouped=False):
    """the batch with the option and without it: the same bytes, the oracle's loci per candidate, the model's literal count"""
    n = sum(len(p["l1"]) for p in per)
    expected = [(ri, ci) for ri, p in enumerate(per) for ci in range(len(p["l1"])) if M.takes_literal(p["fig"][ci], len(p["l2"][ci]))]
    on = run(orc, contigs, reads, hg, True, grouped)
    off = run(orc, contigs, reads, hg, False, grouped)
    print("%d candidates; with the option: %r, expected literal %r; without: %r" % (n, (on["cands"], on["literal"]), expected, (off["cands"], off["literal"])))
    assert n > 0 and (off["cands"], off["literal"]) == (n, n)
    assert (on["cands"], on["literal"]) == (n, len(expected))
    for what in ("stats", "l1", "l2", "mappings"):
        assert len(on[what]) > 0 and on[what] == off[what], "the wave kernel disagrees with the literal one on " + what
    assert len(on["per"]) == len(per)
    for f, (g, p) in enumerate(zip(on["per"], per)):
        assert g["l1"] == p["l1"], ("fragment %d" % f, g["l1"][:4], p["l1"][:4])
        assert g["l2"] == p["l2"], ("fragment %d" % f, [x[:3] for x in g["l2"]][:3], [x[:3] for x in p["l2"]][:3])
    return on, expected


# ----------------------------------------------------------------------------- 1: the gate
GATING_SEEDS = (1, 2, 3, 5)


def case_gating(names=None):
    cs = [M.tandem_contig(seed) for seed in GATING_SEEDS]
    contigs = [(names[i] if names else "s%d" % seed, c) for i, (seed, c) in enumerate(zip(GATING_SEEDS, cs))]
    reads = [("r%d" % seed, M.tandem_read(seed, c)) for seed, c in zip(GATING_SEEDS, cs)]
    return contigs, reads


def assert_gating(per):
    assert all(len(p["l1"]) >= 1 for p in per)
    for i, p in enumerate(per):
        # every candidate has records the gate skips; the candidate over the read's own locus (contig i, from before position 5100 on) has
        # records that re-enter after an expiry as well.  (In one batch the reads of seeds 2 and 3 have a second candidate, a hundred-odd
        # records at the head of another contig and too short for an expiry: it stays in, with its skipped records.)
        assert all(fig["skipped"] > 0 for fig in p["fig"]), p["fig"]
        own = [fig for c, fig in zip(p["l1"], p["fig"]) if c[0] == i and c[1] <= 5100 <= c[2] + p["W"]]
        assert len(own) == 1 and own[0]["reentered"] > 0, (p["l1"], p["fig"])
    assert any(fig["same_hash_in_a_step"] for fig in per[3]["fig"])             # seed 5: the copies are 150 bp apart
    assert not any(M.takes_literal(fig, len(l)) for p in per for fig, l in zip(p["fig"], p["l2"]))


@pytest.mark.gpu
def test_gated_candidates_go_through_the_wave_kernel(oracle):
    contigs, reads = case_gating()
    per = oracle_batch(oracle, contigs, reads, False)
    print([(len(p["l1"]), [(f["walked"], f["entering"], f["skipped"], f["reentered"], f["largest_heap"]) for f in p["fig"]]) for p in per])
    assert_gating(per)
    on, expected = check_both_ways(oracle, contigs, reads, False, per)
    assert on["literal"] == 0


# ----------------------------------------------------------------------------- 2: the grid of 64 events per step
def case_grid():
    contigs, reads = case_gating()
    small = U.random_dna(4201, 3000)
    contigs = contigs + [("small", small)]
    reads = reads + [("few", small[0:1200].copy()), ("short", contigs[1][1][40000:40900].copy()), ("rc", U.revcomp(M.tandem_read(2, contigs[1][1]))),
                     ("plain", contigs[0][1][60000:62500].copy()),
                     ("mixed410", M.mixed_strand_read(1, contigs[0][1], 410)), ("mixed950", M.mixed_strand_read(1, contigs[0][1], 950))]
    return contigs, reads


@pytest.mark.gpu
@pytest.mark.parametrize("hg", [False, True], ids=["nohg", "hg"])
def test_steps_off_the_grid_short_and_reversed_reads(oracle, hg):
    contigs, reads = case_grid()
    per = oracle_batch(oracle, contigs, reads, hg)
    few, short, rc = per[4], per[5], per[6]
    print("few: %r; short: %r; first slide events %r" % (few["fig"], short["fig"], [f["first_slide_event"] for p in per for f in p["fig"]]))
    # the smallest candidate this shape has: every position of a contig has s = 80 records open, so none walks fewer than 64 -- this one walks a
    # few steps' worth, the fewest of the batch without the HG filter, and ends inside its last step
    assert len(few["l1"]) == 1 and few["fig"][0]["walked"] < 4 * 64 and few["fig"][0]["steps"] <= 8
    assert any(f["first_slide_event"] % 64 != 0 and f["setup"] > 0 for p in per for f in p["fig"])  # the set-up phase ends inside a step
    assert short["W"] == 0 and len(short["l1"]) >= 1
    assert len(rc["l1"]) >= 1 and all(x[5] == -1 for l in rc["l2"] for x in l)
    # reads whose pieces alternate in strand: loci of both strands, so the strand of a closing run depends on when the votes are sampled --
    # behind the evictions of the skipped slide records before the entering one, whose wpos the kernel takes from the lanes below or, where
    # that record lies in an earlier step of 64 events, from the carry
    for p in per[8:10]:
        assert {x[5] for l in p["l2"] for x in l} == {1, -1}, p["l2"]
        assert any(f["behind_skipped_earlier_step"] > 0 for f in p["fig"]) and any(f["behind_skipped"] > f["behind_skipped_earlier_step"] for f in p["fig"])
    on, expected = check_both_ways(oracle, contigs, reads, hg, per)
    assert on["literal"] == 0


# ----------------------------------------------------------------------------- 3: more tied loci than slots
@pytest.mark.gpu
@pytest.mark.parametrize("hg", [False, True], ids=["nohg", "hg"])
def test_more_tied_loci_than_slots_are_handed_over(oracle, hg):
    contigs = [("s1", M.planted_contig(4101, 4100, 1800, 14, 0.0))]
    reads = [("unit", U.random_dna(4100, 1800)[100:1500].copy())]
    per = oracle_batch(oracle, contigs, reads, hg)
    print([(c, len(l)) for c, l in zip(per[0]["l1"], per[0]["l2"])])
    if not hg:
        assert [c[:3] for c in per[0]["l1"]] == [(0, 3751, 29442)] and [len(l) for l in per[0]["l2"]] == [14]
        assert all(x[4] == 79 for x in per[0]["l2"][0]) and 14 > M.LOCAP0 + 1
    else:
        assert len(per[0]["l1"]) == 14 and all(len(l) == 1 for l in per[0]["l2"])
    on, expected = check_both_ways(oracle, contigs, reads, hg, per)
    assert on["literal"] == (0 if hg else 1)


@pytest.mark.gpu
def test_a_handed_over_candidate_behind_loci_the_wave_kernel_wrote(oracle):
    """the 14 tied loci in one batch with case 1: the literal kernel runs out of slots once and is run again alone, from the cursor the
    wave kernel left -- which is not 0 here --, and the wave kernel's loci stay where they are"""
    contigs, reads = case_gating()
    contigs = contigs + [("tied", M.planted_contig(4101, 4100, 1800, 14, 0.0))]
    reads = reads + [("unit", U.random_dna(4100, 1800)[100:1500].copy())]
    per = oracle_batch(oracle, contigs, reads, False)
    print([(c[:3], len(l)) for p in per for c, l in zip(p["l1"], p["l2"])])
    assert [len(l) for c, l in zip(per[4]["l1"], per[4]["l2"]) if c[0] == 4] == [14]
    assert sum(len(l) for p in per[:4] for l in p["l2"]) > 0
    on, expected = check_both_ways(oracle, contigs, reads, False, per)
    assert on["literal"] == 1 and expected == [(4, [c[0] for c in per[4]["l1"]].index(4))]


# ----------------------------------------------------------------------------- 4: a heap beyond the LDS capacity
@pytest.mark.gpu
def test_a_heap_beyond_the_lds_capacity_is_handed_over(oracle):
    c = M.tandem_contig(4)
    contigs = [("s4", c)]
    reads = [("long", M.tandem_read(4, c, 36000)), ("seed4", M.tandem_read(4, c)), ("mid", c[50000:53000].copy())]
    per = oracle_batch(oracle, contigs, reads, False)
    heaps = [[f["largest_heap"] for f in p["fig"]] for p in per]
    print("largest heaps per read and candidate: %r" % heaps)
    assert max(heaps[0]) > M.WW_HEAP and 739 <= max(heaps[1]) <= M.WW_HEAP and 0 < max(heaps[2]) < M.WW_HEAP
    on, expected = check_both_ways(oracle, contigs, reads, False, per)
    assert 0 < on["literal"] < on["cands"]


# ----------------------------------------------------------------------------- 5: -Y reference groups
@pytest.mark.gpu
def test_reference_groups(oracle):
    contigs, reads = case_gating(names=["A#1#s1", "A#1#s2", "B#1#s3", "B#1#s5"])
    reads = [("C#1#" + n, a) for n, a in reads]
    per = oracle_batch(oracle, contigs, reads, False, grouped=True)
    assert_gating(per)
    on, expected = check_both_ways(oracle, contigs, reads, False, per, grouped=True)
    assert on["literal"] == 0


# ----------------------------------------------------------------------------- 6: the option without a windowed batch
@pytest.mark.gpu
@pytest.mark.parametrize("nosplit", [True, False], ids=["nosplit_short_reads", "split"])
def test_the_option_leaves_other_batches_alone(oracle, nosplit):
    contigs, _ = case_gating()
    # --noSplit: reads that all fit a segment (no fragment is longer than segLength); split mode: long reads, cut into segments
    reads = [("r%d" % i, c[5100 + 700 * i:5100 + 700 * i + (900 if nosplit else 3300)].copy()) for i, (_, c) in enumerate(contigs)]
    on = run(oracle, contigs, reads, True, True, nosplit=nosplit, passes=2)
    off = run(oracle, contigs, reads, True, False, nosplit=nosplit, passes=2)
    assert on["pass_stats"] == (1, True) and off["pass_stats"] == (1, True)     # the second pass is a steady-state pass, as it is today
    assert (on["cands"], on["literal"]) == (0, 0) and (off["cands"], off["literal"]) == (0, 0)
    for what in ("stats", "l1", "l2", "mappings"):
        assert len(on[what]) > 0 and on[what] == off[what], what


@pytest.mark.gpu
def test_loci_outgrow_the_buffer_behind_the_window_wave_kernel(oracle):
    """k_l2_window_wave's claim running past l2Cap: tests/largewave.py's loci8 batch out of eight exact copies (s = 32), under --noSplit and with
    a read of three segments in front, which makes the batch a windowed one -- more loci than the 2 n1 + 1 024 the buffer starts with
    (mm_launch_l2_window: l2w_extents), of candidates the wave kernel keeps.  Its first launch raises MM_PC_L2_OVERFLOW, the launcher
    grows l2Cap to the cursor's demand and launches it again (the first pass closes more MM_K_L2 timer brackets than a second pass of the
    same batch on the same context: loci8_pass): the bytes of the pass without the option (the literal kernel)"""
    import largewave as T
    from mashmap_amd import capi
    ub = U.random_dna(9052, 1300)
    long_read = U.mutate(np.concatenate([ub, ub, ub]), 9057, 0.02)[:3 * T.LOCI8_L].copy()
    reads = [long_read] + T.loci8_reads(700)
    off = T.loci8_pass(reads, capi.MM_FLAG_NO_SPLIT, lambda c: c.l2_window_wave(False))
    on = T.loci8_pass(reads, capi.MM_FLAG_NO_SPLIT, lambda c: c.l2_window_wave(True))
    n1, n2 = off["counts"]
    print("%d candidates, %d loci (at most %d in one), the buffer starts at %d; windowed: %r without the option, %r with it; MM_K_L2 brackets of the first and the second pass %r"
          % (n1, n2, off["per"].max(), 2 * n1 + 1024, off["window"], on["window"], on["l2_brackets"]))
    assert off["window"] == (n1, n1) and on["window"][0] == n1
    assert n2 - on["window"][1] * int(off["per"].max()) > 2 * n1 + 1024, "the loci of the candidates the wave kernel keeps fit the buffer it is first launched with"
    assert on["l2_brackets"][0] > on["l2_brackets"][1] > 0, "the first pass did not repeat an attempt: l2Cap did not grow"
    for a, b, what in zip(on["bytes"], off["bytes"], ("stats", "l1", "l2", "mappings", "query sketches")):
        assert a == b, what


# ----------------------------------------------------------------------------- 7: CPU
def test_the_option_and_the_query_are_declared_exported_and_bound():
    import ctypes
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert re.search(r"enum \{[^}]*MM_OPT_L2_WINDOW_WAVE = 5[^}]*\};", hdr)
    assert "int mm_pass_l2_window(const mm_ctx* ctx, uint64_t* candidates, uint64_t* literal);" in hdr
    assert "#define MM_ABI_VERSION 2" in hdr or re.search(r"MM_ABI_VERSION\s*=?\s*2\b", hdr)
    assert "mm_pass_l2_window" in capi.EXPORTS and hasattr(ctypes.CDLL(capi.LIB_PATH), "mm_pass_l2_window")
    assert capi.MM_OPT_L2_WINDOW_WAVE == 5
    assert callable(getattr(capi.Context, "l2_window_wave")) and callable(getattr(capi.Context, "pass_l2_window"))
    assert capi.load().mm_abi_version() == 2                     # additive: the ABI version stays
    src = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_l2.hip")).read()
    assert re.search(r"#define MM_WW_HEAP %d\b" % M.WW_HEAP, src) and re.search(r"#define MM_LOCAP0 %d\b" % M.LOCAP0, src)   # the mirrored capacities
