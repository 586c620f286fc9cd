"""MM_OPT_L2_LARGE_WAVE: the L2 stage of a split batch on the literal route (a sketch beyond 8190) on k_l2_large_wave, one wave per L1
candidate with the candidate's SlideMapper cells in LDS and 64 events of its slice of the index per step; the literal k_l2_window takes the
candidates it hands over.  Bit 1 of the option sends split batches down that route at any sketch size, so the kernel's edges are checked at
s = 80 (values 3 and 2 against 0, the fast split path) and its sizes at s = 8 200 and 19 998 (value 1 against 0, the literal kernel alone).

Every case first derives its figures on the CPU -- the oracle per fragment, and tests/largewave.py's cut of a candidate's slice out of the
oracle's index -- and asserts the conditions it exists for, then maps the batch on a fresh context per value: stats, L1, L2 and candidate
mappings byte-identical, L1 and L2 equal to the oracle's per fragment and candidate, and pass_l2_large() as expected.

Small shapes: k 16, segLength 1000, s 80, pi 0.85, kmerThreshold 0; contigs of at most 90 kbp."""
import os
import subprocess
import time

import numpy as np
import pytest

import largewave as W
import mmutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, L, S, PI = 16, 1000, 80, 0.85
TAILLEN = 400


def n_cands(per):
    return sum(len(p["l1"]) for p in per)


# ----------------------------------------------------------------------------- 1: a plain batch
def case_plain():
    a, b, small = U.random_dna(7101, 90000), U.random_dna(7102, 60000), U.random_dna(7103, 1200)
    unit = b[20000:21100].copy()
    for i in range(4): b[30000 + 1100 * i:30000 + 1100 * (i + 1)] = unit          # four copies in tandem: one candidate over all of them, more than ten steps
    contigs = [("a", a), ("b", b), ("small", small)]
    reads = [("three%d" % i, U.mutate(a[x:x + 2 * L + 777 + 200], 7110 + i, 0.08)[:2 * L + 777].copy()) for i, x in enumerate((5000, 41234, 77000))]
    reads += [("short", b[50000:50600].copy()), ("rc", U.revcomp(U.mutate(a[60000:61100], 7120, 0.04)[:L])), ("n_runs", U.with_n_runs(a[20000:22500], 7121, 4, 40)),
              ("head", a[0:L].copy()), ("tail", a[len(a) - L:].copy()), ("small", small.copy()), ("tandem", U.mutate(unit, 7122, 0.02)[:L].copy()),
              ("end", a[len(a) - 150:].copy())]
    return contigs, reads


@pytest.mark.gpu
@pytest.mark.parametrize("hg", [False, True], ids=["nohg", "hg"])
def test_a_plain_batch_on_the_wave_kernel_and_on_the_literal_one(oracle, hg):
    contigs, reads = case_plain()
    flags = U.FLAG_HG if hg else 0
    h, per = W.oracle_batch(oracle, contigs, reads, K, L, S, PI, flags)
    try:
        figs = [f for p in per for f in p["fig"]]
        print([(p["read"], p["l1"], [(f["slide"], f["before"], f["last_is_contig_last"]) for f in p["fig"]]) for p in per])
        n = n_cands(per)
        assert n >= len(reads) and all(len(p["l1"]) >= 1 for p in per)
        assert [len(a) for _, a in reads[:3]] == [2 * L + 777] * 3 and sum(1 for p in per if p["read"] == 0) == 3
        assert any(f["slide"] < 64 for f in figs)                                # a slide that ends inside its first step of 64 events
        assert any(f["slide"] > 640 for f in figs)                               # ... and one of more than ten steps
        assert any(f["before"] == 0 for f in figs)                               # no record before rangeStart: nothing to pre-load
        # (no candidate's last insert is the contig's last record: L1 positions are read starts, rangeEnd stays a segment short of the
        # contig's end -- 88 993 of 90 000 for "tail" and "end" -- and the last record lies in the contig's last window; the record behind
        # the slice always exists here)
        assert not any(f["last_is_contig_last"] for f in figs)
        assert all(x[5] == -1 for p in per if reads[p["read"]][0] == "rc" for l in p["l2"] for x in l)
        assert not any(len(l) > W.LOCAP0 + 1 for p in per for l in p["l2"])
        W.check_values(oracle, h, reads, per, K, L, S, PI, flags, {3: (n, 0), 2: (n, n), 0: (0, 0)})
    finally:
        oracle.free(h)


# ----------------------------------------------------------------------------- 2: more tied loci than slots
@pytest.mark.gpu
def test_more_tied_loci_than_slots_are_handed_over_behind_loci_of_the_wave_kernel(oracle):
    """candidates over a tandem array of twelve exact copies have a locus per copy: more than MM_LOCAP0 + 1, so the wave kernel hands them over;
    the reads in front of them stay on it, so the literal kernel -- which runs out of its own eight slots once -- is run again alone, from the
    cursor the wave kernel left, which is not 0"""
    unit = U.random_dna(7201, 1100)
    contigs = [("unique", U.random_dna(7202, 40000)), ("array", W.arrayed(7203, unit, 12, 0))]
    two = np.concatenate([unit, unit])
    reads = [("u%d" % i, U.mutate(contigs[0][1][x:x + L + 100], 7210 + i, 0.05)[:L].copy()) for i, x in enumerate((3000, 17000, 30000))]
    reads += [("unit%d" % i, U.mutate(two[x:x + L + 60], 7220 + i, 0.02)[:L].copy()) for i, x in enumerate((0, 400, 900))]
    h, per = W.oracle_batch(oracle, contigs, reads, K, L, S, PI, 0)
    try:
        tied = [(fi, ci) for fi, p in enumerate(per) for ci, l in enumerate(p["l2"]) if len(l) > W.LOCAP0 + 1]
        print([(p["read"], [c[:3] for c in p["l1"]], [len(l) for l in p["l2"]]) for p in per], tied)
        n = n_cands(per)
        assert len(tied) >= 1 and min(fi for fi, _ in tied) >= 3
        assert sum(len(l) for p in per[:3] for l in p["l2"]) > 0 and not any(len(l) > W.LOCAP0 + 1 for p in per[:3] for l in p["l2"])
        W.check_values(oracle, h, reads, per, K, L, S, PI, 0, {3: (n, len(tied)), 2: (n, n), 0: (0, 0)})
    finally:
        oracle.free(h)


# ----------------------------------------------------------------------------- 3: a query hash open twice
def overlap(recs):
    """tests/test_gpu_steady.py: every fifth window of contig 1 is there twice, shifted by 13 bases"""
    pick = recs[recs["seqId"] == 1][::5].copy()
    pick["wpos"] += 13; pick["wpos_end"] += 13
    allr = np.concatenate([recs, pick])
    return allr[np.lexsort((np.arange(len(allr)), allr["wpos"], allr["seqId"]))]


@pytest.mark.gpu
def test_a_query_hash_open_twice_stays_on_the_wave_kernel(oracle):
    """an index in which two windows of one hash overlap: `active` stays a boolean, the vote accumulates, the shared count moves once per
    insert and once per delete -- the literal rule, which WinSlide states; nothing is handed over"""
    cs = [U.random_dna(7301, 60000), U.random_dna(7302, 60000)]
    contigs = [("c0", cs[0]), ("c1", cs[1])]
    reads = [("a%d" % i, U.mutate(cs[0][x:x + L + 100], 7310 + i, 0.04)[:L].copy()) for i, x in enumerate((1000, 30000))]
    reads += [("b%d" % i, U.mutate(cs[1][x:x + 2 * L + 300], 7320 + i, 0.04)[:2 * L + 123].copy()) for i, x in enumerate((2000, 25000, 47000))]
    h, per = W.oracle_batch(oracle, contigs, reads, K, L, S, PI, 0, mutate_index=overlap, with_sketch_hashes=True)
    try:
        n = n_cands(per)
        twice = sum(1 for p in per for f in p["fig"] if f["doubly_open"])
        print("%d candidates, %d with a doubly open query hash" % (n, twice))
        assert twice >= 3 and not any(f["doubly_open"] for p in per if p["read"] < 2 for f in p["fig"])
        assert not any(len(l) > W.LOCAP0 + 1 for p in per for l in p["l2"])
        W.check_values(oracle, h, reads, per, K, L, S, PI, 0, {3: (n, 0), 2: (n, n), 0: (0, 0)})
    finally:
        oracle.free(h)


# ----------------------------------------------------------------------------- 4: no candidates
@pytest.mark.gpu
def test_a_batch_without_candidates(oracle):
    """no candidate at all: nothing is launched; with a read shorter than k (12 bases: skipped, computeMap.hpp:325) and one whose sketch has
    fewer than s entries (40 bases: 25 k-mers)"""
    contigs = [("c0", U.random_dna(7401, 30000))]
    reads = [("unrelated", U.random_dna(7402, 2 * L + 50)), ("tiny", contigs[0][1][100:112].copy()), ("few", U.random_dna(7403, 40))]
    h, per = W.oracle_batch(oracle, contigs, reads, K, L, S, PI, 0)
    try:
        print([(p["read"], p["len"], p["sketchSize"], p["l1"]) for p in per])
        assert n_cands(per) == 0 and len(per) == 4 and per[-1]["len"] == 40 and 0 < per[-1]["sketchSize"] < S
        W.check_values(oracle, h, reads, per, K, L, S, PI, 0, {3: (0, 0), 2: (0, 0), 0: (0, 0)}, empty_ok=True)
    finally:
        oracle.free(h)


# ----------------------------------------------------------------------------- 5: s = 8 200
@pytest.mark.gpu
def test_sketch_8200_with_twelve_tied_loci(oracle):
    """the first size of the literal route.  Checked on the CPU: the unit read has one candidate spanning 0..128 000 with 12 tied loci (more
    than MM_LOCAP0 + 1: handed over), every other fragment one candidate with one locus; 205 022 index records; no HG filter (the oracle's
    cut-off table is cubic in s)"""
    k, Ls, s, pi = 16, 10000, 8200, 0.80
    unit = U.random_dna(9101, 11000)
    uniq = U.random_dna(9104, 60000)
    contigs = [("unique", uniq), ("array", W.arrayed(9101, unit, 12, 0))]
    reads = [("unit", U.mutate(unit[300:300 + Ls + 300], 9110, 0.02)[:Ls].copy()), ("long", U.mutate(uniq[20000:20000 + 20777 + 1500], 9111, 0.05)[:20777].copy()),
             ("head", uniq[:Ls].copy()), ("tail", uniq[len(uniq) - Ls:].copy()), ("rc", U.revcomp(U.mutate(uniq[45000:45000 + Ls + 300], 9112, 0.03)[:Ls]))]
    t0 = time.time()
    h, per = W.oracle_batch(oracle, contigs, reads, k, Ls, s, pi, 0, figures=False)
    try:
        print("oracle: %.2f s; %r" % (time.time() - t0, [([c[:3] for c in p["l1"]], [len(l) for l in p["l2"]]) for p in per]))
        assert oracle.f("session_index_size")(h) == 205022
        assert [len(l) for l in per[0]["l2"]] == [12] and per[0]["l1"][0][1] == 0 and 12 > W.LOCAP0 + 1
        assert all([len(l) for l in p["l2"]] == [1] for p in per[1:])
        n = n_cands(per)
        W.check_values(oracle, h, reads, per, k, Ls, s, pi, 0, {1: (n, 1), 0: (n, n)})
    finally:
        oracle.free(h)


# ----------------------------------------------------------------------------- 6: the LDS edge
def case_edge():
    g = U.random_dna(9201, 120000)
    Ls = 24000
    reads = [("fwd", U.mutate(g[30000:30000 + Ls + 1500], 9210, 0.05)[:Ls].copy()), ("rc", U.revcomp(U.mutate(g[80000:80000 + Ls + 900], 9211, 0.03)[:Ls])), ("head", g[:Ls].copy())]
    return [("g", g)], reads


@pytest.fixture(scope="module")
def min_hits_edge(oracle):
    """Stat::estimateMinimumHitsRelaxed(q, k, pi) for q up to MM_LW_MAX_SKETCH + 1: entry q does not depend on the sketch size, so both cases
    at the LDS edge take their table from this one (some seconds of host time; shared, unchanged)"""
    return oracle.min_hits_table(W.LW_MAX_SKETCH + 1, 16, 0.80)


@pytest.mark.gpu
def test_sketch_19998_one_wave_per_cu(oracle, min_hits_edge):
    """s = 19 998: 160 112 of a CU's 163 840 B of LDS.  No replay tables (1.2 GB at this size): the pass stops at the loci"""
    k, Ls, s, pi = 16, 24000, 19998, 0.80
    contigs, reads = case_edge()
    h, per = W.oracle_batch(oracle, contigs, reads, k, Ls, s, pi, 0, figures=False)
    try:
        print([([c[:3] for c in p["l1"]], [len(l) for l in p["l2"]]) for p in per])
        assert all(len(p["l1"]) == 1 and [len(l) for l in p["l2"]] == [1] for p in per)
        W.check_values(oracle, h, reads, per, k, Ls, s, pi, 0, {1: (3, 0), 0: (3, 3)}, min_hits=min_hits_edge[:s + 1], replay=False)
    finally:
        oracle.free(h)


@pytest.mark.gpu
def test_one_sketch_entry_more_than_the_lds_holds_is_the_literal_kernels(oracle, min_hits_edge):
    """the same batch at sketchSize = MM_LW_MAX_SKETCH + 1 (segLength raised to match): the wave kernel is not launched"""
    k, s, pi = 16, W.LW_MAX_SKETCH + 1, 0.80
    Ls = 24600
    contigs, reads0 = case_edge()
    g = contigs[0][1]
    reads = [("fwd", U.mutate(g[30000:30000 + Ls + 1500], 9210, 0.05)[:Ls].copy()), ("rc", U.revcomp(U.mutate(g[80000:80000 + Ls + 900], 9211, 0.03)[:Ls])), ("head", g[:Ls].copy())]
    h, per = W.oracle_batch(oracle, contigs, reads, k, Ls, s, pi, 0, figures=False)
    try:
        n = n_cands(per)
        assert n >= 3
        W.check_values(oracle, h, reads, per, k, Ls, s, pi, 0, {1: (n, n), 0: (n, n)}, min_hits=min_hits_edge[:s + 1], replay=False)
    finally:
        oracle.free(h)


# ----------------------------------------------------------------------------- the locus buffer behind the wave kernel
@pytest.mark.gpu
def test_loci_outgrow_the_buffer_behind_the_large_wave_kernel(oracle):
    """k_l2_large_wave's claim running past l2Cap: 700 one-segment reads out of eight exact copies -- up to eight tied loci in a candidate,
    which its slots hold, so every candidate stays on the wave kernel -- bring more loci than the 2 n1 + 1 024 the literal route's buffer
    starts with on a fresh context (mm_launch_l2_window: l2w_extents).  The kernel's first launch raises MM_PC_L2_OVERFLOW, the launcher
    grows l2Cap to the cursor's demand and launches it again -- seen as the first pass closing more MM_K_L2 timer brackets than a second
    pass of the same batch on the same context, which finds the grown buffer (tests/largewave.py: loci8_pass) -- and the pass leaves the
    bytes of the pass with the option off (the fast split kernels).
    At s = 32, the sketch size of the "loci8" case: at this module's s = 80 the same index cuts a read's candidates at every copy (400
    reads: 1 749 candidates with 2 943 loci), fewer than the two loci per candidate the buffer starts with, at any number of reads"""
    reads = W.loci8_reads(700)
    off = W.loci8_pass(reads, 0, lambda c: c.l2_large_wave(0))
    on = W.loci8_pass(reads, 0, lambda c: c.l2_large_wave(3))
    n1, n2 = off["counts"]
    print("%d candidates, %d loci (at most %d in one), the buffer starts at %d; with the option %r, MM_K_L2 brackets of the first and the second pass %r"
          % (n1, n2, off["per"].max(), 2 * n1 + 1024, on["large"], on["l2_brackets"]))
    assert off["per"].max() <= W.LOCAP0 + 1, "a candidate has more loci than the wave kernel holds"
    assert n2 > 2 * n1 + 1024, "the loci fit the buffer the kernel is first launched with"
    assert off["large"] == (0, 0) and on["large"] == (n1, 0)       # every candidate, and its loci, on the wave kernel
    assert on["l2_brackets"][0] > on["l2_brackets"][1] > 0, "the first pass did not repeat an attempt: l2Cap did not grow"
    for a, b, what in zip(on["bytes"], off["bytes"], ("stats", "l1", "l2", "mappings", "query sketches")):
        assert a == b, what


# ----------------------------------------------------------------------------- 7: the command line
def case_command_line():
    cs = [U.random_dna(9301, 400000), U.random_dna(9302, 380000)]
    reads = [("r0", U.mutate(cs[0][50000:50000 + 252000], 9310, 0.03)[:250000].copy()), ("r1", U.revcomp(U.mutate(cs[1][100000:100000 + 246000], 9311, 0.05)[:245000])),
             ("r2", U.mutate(cs[0][140000:140000 + 256000], 9312, 0.01)[:255000].copy())]
    return [("chrA", cs[0]), ("chrB", cs[1])], reads


@pytest.mark.gpu
def test_command_line_dense_s100000_against_the_stock_binary(tmp_path):
    """mashmap_hip --dense --pi 80 -s 100000 (sketchSize 9 998; skch::Sketch's setting of the option as the probe decided it) byte for byte
    against tests/golden/paf/large_wave_dense_s100000.paf, which the stock binary wrote:

        import sys; sys.path.insert(0, "tests")
        import mmutil as U, test_gpu_large_wave as T, subprocess
        ref, reads = T.case_command_line()
        U.write_fasta("/tmp/lw.ref.fa", ref); U.write_fasta("/tmp/lw.q.fa", reads)
        subprocess.check_call([U.REF_BIN, "-r", "/tmp/lw.ref.fa", "-q", "/tmp/lw.q.fa", "-t", "4", "--dense", "--pi", "80", "-s", "100000",
                               "-o", "tests/golden/paf/large_wave_dense_s100000.paf"])
    """
    hip = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
    assert os.path.exists(hip), "mashmap_hip not built (python -c 'import __graft_entry__ as g; g.build()')"
    ref, reads = case_command_line()
    rf, qf, out = str(tmp_path / "ref.fa"), str(tmp_path / "q.fa"), str(tmp_path / "hip.paf")
    U.write_fasta(rf, ref); U.write_fasta(qf, reads)
    p = subprocess.run([hip, "-r", rf, "-q", qf, "-t", "4", "--dense", "--pi", "80", "-s", "100000", "-o", out], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = open(out, "rb").read()
    exp = open(os.path.join(ROOT, "tests", "golden", "paf", "large_wave_dense_s100000.paf"), "rb").read()
    assert len(exp) > 0 and exp.count(b"\n") >= 3
    assert got == exp, (got[:400], exp[:400])
