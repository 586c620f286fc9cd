"""Steady-state passes at their edges.  A steady-state pass launches every stage against the capacities an earlier sized pass left and reads
one counter block back at its end; a batch that outgrows one of those capacities must stop short of the buffer's end, raise its flag, be
redone the sized way (mm_pass_totals, mm_pass_redo_cause) and come out with the bytes a fresh context gives -- and nothing behind the stage
that overflowed may have touched the index, the tables or a parked batch.  One A/B pair per cause: a context is sized on batch A, batch B --
no more fragments than A, so that the steady attempt really happens -- outgrows ONE capacity A left, shown from the counts of two fresh
contexts and the project's own capacity formulas before the pass under test runs.

Findings written down here because the tests pin them:
  * MM_L2F_CANDS (MM_REDO_L2_CANDS) cannot fire on its own: k_l1_gate compares the candidate count with min(candCap, dense L1 buffer) first,
    raises the L1 flag and zeroes the count, so k_l2_extents never sees more candidates than candCap.  Its test expects L1 and NOT CANDS:
    the bit would mean that the gate let a count through.
  * after three redone attempts in a row a context makes no further steady attempt, and nothing resets that: steadyFails is only cleared by
    a steady-state pass that went through, which needs an attempt (test_three_redone_attempts_in_a_row_...).
  * a batch with more wide-cell or doubly open candidates than MM_WIDE_CAP / MM_EXACT_CAP is redone on EVERY steady attempt, its own sized
    pass notwithstanding (the steady launches cover a fixed number of them), until the third failure ends the attempts.

The pairs of the later stages rest on one lever: B's streams must fit what A left, or k_l2_gate fires first.  Reads shorter than a
segment, and candidates that run over a long array, bring two to seven times the stream entries of an ordinary candidate: A is made of
those, and the flag of the stage behind the gate is the one that fires.
"""
import numpy as np
import pytest

import mmutil as U
import gpucheck

pytestmark = pytest.mark.gpu

K, L, PI = 16, 1000, 0.95                                 # (at 0.95 minimumHits is above 1: k_lookup_mid takes what the fused kernel cannot sort)
WIDE_CAP, EXACT_CAP, LOCAP0 = 4096, 1024, 8               # mm_l2.hip: MM_WIDE_CAP, MM_EXACT_CAP, MM_LOCAP0


# the capacities a sized pass leaves, restated, and the tandem arrays with their reads: tests/mmutil.py (other modules use them too)
from mmutil import (arrayed, cand_cap, dense_cap, devbuf, loci_cap, map_cap, ops_cap, pts_cap, region_cap, unit_reads)  # noqa: E402,F401


class Fresh:
    """what a fresh context makes of a batch: the bytes, and the counts the preconditions are stated in"""
    def __init__(self, make_ctx, reads):
        c = make_ctx()
        self.nF = c.reads_upload(reads); c.map()
        assert not c.pass_stats()[1] and c.pass_redo_cause() == 0
        self.bytes = gpucheck.pass_bytes(c)
        self.stats, self.l1, _ = c.results()
        self.n1, self.n2 = c.result_counts()
        self.nmap = len(c.mappings())
        self.counts = c.pass_counts()
        self.ops, self.queued = self.counts["stream_entries"], self.counts["queued"]
        c.close()

    def points_demand(self):
        """an upper bound of the slots this batch reserves in the interval-point buffer: a power of two, 128 at least, per queued fragment"""
        top = np.sort(self.stats["nPoints"].astype(np.int64))[::-1][:self.queued]      # whichever fragments were queued, they bring no more than the largest lists
        return int(sum(max(128, 1 << int(n - 1).bit_length()) for n in top))

    def fits_l1_of(self, a):
        """this batch's L1 candidates fit the output regions and the dense buffer of a pass sized for a (region = fragment mod 64; a bound:
        it counts the sweep path's candidates, which only go to the dense buffer, into the regions as well)"""
        per = np.bincount(self.l1["frag"] & 63, minlength=64).max() if self.n1 else 0
        return per <= region_cap(a.nF) and self.n1 <= dense_cap(a.nF)

    def __repr__(self):
        return "nF %d, L1 %d, L2 %d, mappings %d, stream entries %d, queued %d" % (self.nF, self.n1, self.n2, self.nmap, self.ops, self.queued)


def redone_pair(make_ctx, A, B, expect, beside=0, pre=None, b_never_steady=False, a_outgrows_b=0):
    """Sized on A; B's steady attempt is redone for `expect` (at least one of its bits, and no bit outside expect | beside); B again is a
    steady-state pass; A, back out of its slot, is a steady-state pass -- the bytes of a fresh context every time.
    pre(fa, fb): the precondition, stated on the fresh contexts' counts.
    b_never_steady: B is redone again, for the same cause, on the buffers its own sized pass left (FINDING: the steady launches of the wide
    re-run and the exact kernel cover a fixed number of candidates, so such a batch never goes steady).
    a_outgrows_b: the bits A's return is redone for, where A needs more candidates than B's sized pass leaves (candCap follows the last pass)."""
    from mashmap_amd import capi
    fa, fb = Fresh(make_ctx, A), Fresh(make_ctx, B)
    print("A: %r\nB: %r" % (fa, fb))
    assert fb.nF <= fa.nF + fa.nF // 10, "B would be sized without a steady attempt"
    assert fa.nF <= fb.nF + fb.nF // 10, "A would be sized without a steady attempt when it comes back"
    assert fa.n1 > 0       # (a sized pass that grows a buffer leaves MORE than the formulas say: they are lower bounds wherever B is shown to fit)
    if pre:
        pre(fa, fb)
    ctx = make_ctx()
    assert ctx.reads_upload(A) == fa.nF
    ctx.map()
    assert gpucheck.pass_bytes(ctx) == fa.bytes and not ctx.pass_stats()[1]
    ctx.reads_exchange(0)                                                        # A waits in slot 0 while B is mapped
    assert ctx.reads_upload(B) == fb.nF
    t0 = ctx.pass_totals()
    ctx.map()
    cause, t1 = ctx.pass_redo_cause(), ctx.pass_totals()
    print("B's steady attempt: cause %#x" % cause)
    assert t1["redone"] == t0["redone"] + 1 and not ctx.pass_stats()[1], "B went through (cause %#x): %r" % (cause, ctx.pass_stats())
    assert not (cause & capi.MM_REDO_L2_STREAM), "MM_L2F_STREAM: an internal error (cause %#x)" % cause
    assert cause & expect, "redone for %#x, expected %#x" % (cause, expect)
    assert not (cause & ~(expect | beside)), "redone for %#x: bits beside the expected %#x other than %#x" % (cause, expect, beside)
    assert gpucheck.pass_bytes(ctx) == fb.bytes, "the redone pass is not exact"
    ctx.map()
    if b_never_steady:
        assert not ctx.pass_stats()[1] and ctx.pass_redo_cause() == cause and ctx.pass_totals()["redone"] == t1["redone"] + 1, (ctx.pass_stats(), ctx.pass_redo_cause())
    else:
        assert ctx.pass_stats() == (1, True) and ctx.pass_redo_cause() == 0, (ctx.pass_stats(), ctx.pass_redo_cause())
    assert gpucheck.pass_bytes(ctx) == fb.bytes
    ctx.reads_exchange(0); ctx.map()                                             # A again, out of its slot
    if a_outgrows_b:
        assert not ctx.pass_stats()[1] and ctx.pass_redo_cause() == a_outgrows_b, (ctx.pass_stats(), ctx.pass_redo_cause())
    else:
        assert ctx.pass_stats() == (1, True) and ctx.pass_redo_cause() == 0, "A does not fit what B left: %r, cause %#x" % (ctx.pass_stats(), ctx.pass_redo_cause())
    assert gpucheck.pass_bytes(ctx) == fa.bytes, "something written during B's passes reached the index, the tables or the parked batch"
    redone = 1 + (1 if b_never_steady else 0) + (1 if a_outgrows_b else 0)
    assert ctx.pass_totals() == {"passes": 4, "steady": 3 - redone, "redone": redone}
    ctx.close()
    return fa, fb


def built(contigs, s, k=K, seg=L, pi=PI):
    """make_ctx for an index built on the device from the contigs"""
    from mashmap_amd import capi
    def make():
        c = capi.Context(k=k, segLength=seg, sketchSize=s, flags=capi.MM_FLAG_HG_FILTER)
        c.index_build(contigs, kmerPct=0.0); c.set_tables_default(pi)
        return c
    return make


def named(prefix, reads): return [("%s%d" % (prefix, i), a) for i, a in enumerate(reads)]


def reads_of(seqs, seed, n, err=0.02, rl=L): return [a[:rl].copy() for _, a, _ in U.sample_reads(seqs, seed, n, rl + 60, err)]


def strewn(seed, unit, copies, div, spacing=6000):
    """a contig with `copies` copies of the unit, every one further than segLength from the next (a candidate each), diverged by div"""
    g = U.random_dna(seed, copies * spacing + 4000)
    for i in range(copies):
        m = unit if div == 0 else U.mutate(unit, seed * 131 + i, div)
        n = min(len(m), len(unit)); g[2000 + i * spacing:2000 + i * spacing + n] = m[:n]
    return g


UNIQ = U.random_dna(9001, 500000)


# ---- the L1 stage -------------------------------------------------------------------------------------------------------------------------
def test_points_of_the_hbm_path_outgrow_their_buffer(oracle):
    """B: as many fragments as A out of a 24-copy repeat -- ~1 500 interval points per fragment at s = 32, more than k_lookup_mid keeps, so
    every fragment reserves slots in dPts, which a pass over unique reads sized at 8 per fragment"""
    from mashmap_amd import capi
    unit = U.random_dna(9011, 3000)
    contigs = [UNIQ, strewn(9012, unit, 24, 0.004)]
    A, B = reads_of([UNIQ], 9013, 1000), reads_of([unit], 9014, 1000)
    def pre(fa, fb):
        assert fa.queued == 0, "A grew the point buffer itself"
        assert fb.queued * 128 > pts_cap(fa.nF), "B's queued fragments (at least 128 slots each) fit the point buffer"
    redone_pair(built(contigs, 32), A, B, capi.MM_REDO_POINTS, beside=capi.MM_REDO_L1, pre=pre)
    gpucheck.run_and_compare(oracle, named("c", contigs), named("a", A[:30]) + named("b", B[:10]), k=K, L=L, s=32, kmerPct=0.0, pi=PI, device_index=True, verbose=False)


def test_l1_candidates_outgrow_an_output_region(oracle):
    """B: 10 clean, well-separated copies -- 10 candidates per fragment from k_lookup_mid (640 points: next to no HBM point path), more than a region
    of the L1 buffer holds: the flag is k_lookup_l1's / k_lookup_mid's own"""
    from mashmap_amd import capi
    unit = U.random_dna(9021, 3000)
    contigs = [UNIQ, strewn(9022, unit, 10, 0.004)]
    A, B = reads_of([UNIQ], 9023, 1000), reads_of([unit], 9024, 1000)
    def pre(fa, fb):
        per = np.bincount(fb.l1["frag"] & 63, minlength=64)
        assert fa.fits_l1_of(fa), "A itself grew an L1 buffer: region_cap does not describe what it leaves"
        assert fb.points_demand() <= pts_cap(fa.nF), "B overflows the point buffer"
        assert per.max() > region_cap(fa.nF), "B's candidates fit the regions: %d <= %d" % (per.max(), region_cap(fa.nF))
    redone_pair(built(contigs, 32), A, B, capi.MM_REDO_L1, pre=pre)


def test_more_candidates_than_the_staging_behind_l1_holds(oracle):
    """B: 3 copies -- its candidates fit the L1 buffers (2 per fragment + 1 024, and 64 per region, of head room) but not candCap, which the
    L2 launcher left at 9/8 of A's count + 1 024.  k_l1_gate is what notices (MM_PC_L1_OVERFLOW); MM_L2F_CANDS, behind it, is never reached
    (module docstring): this is the test of both bits, and MM_REDO_L2_CANDS must stay clear."""
    from mashmap_amd import capi
    unit = U.random_dna(9031, 3000)
    contigs = [UNIQ, strewn(9032, unit, 3, 0.004)]
    A, B = reads_of([UNIQ], 9033, 1000), reads_of([unit], 9034, 1000)
    def pre(fa, fb):
        assert fb.points_demand() <= pts_cap(fa.nF) and fb.fits_l1_of(fa), "B overflows the L1 stage's own buffers"
        assert fb.n1 > cand_cap(fa.n1), "B's candidates fit candCap: %d <= %d" % (fb.n1, cand_cap(fa.n1))
    redone_pair(built(contigs, 32), A, B, capi.MM_REDO_L1, pre=pre)


# ---- the L2 stage -------------------------------------------------------------------------------------------------------------------------
def test_l2_streams_outgrow_their_buffer(oracle):
    """same candidates, longer streams: A's reads are whole segments, B's a third of a segment out of the same places (a short read's
    candidate region, and the stream over it, is several times as long: measured 296 064 entries against 115 008 for 1 000 reads)"""
    from mashmap_amd import capi
    A = reads_of([UNIQ], 9043, 1000)
    B = [a[300:640].copy() for a in A]
    def pre(fa, fb):
        assert fb.points_demand() <= pts_cap(fa.nF) and fb.fits_l1_of(fa) and fb.n1 <= cand_cap(fa.n1), "B overflows a stage before the streams"
        assert fb.ops > ops_cap(fa.ops), "B's streams fit: %d <= %d" % (fb.ops, ops_cap(fa.ops))
    redone_pair(built([UNIQ], 64), A, B, capi.MM_REDO_L2_OPS, pre=pre)
    gpucheck.run_and_compare(oracle, [("u", UNIQ)], named("a", A[:25]) + named("b", B[:25]), k=K, L=L, s=64, kmerPct=0.0, pi=PI, device_index=True, verbose=False)


def test_more_wide_cell_candidates_than_the_re_run_covers(oracle):
    """reads a tenth of a segment long: over a hundred reference-only hashes pile up below their first query hash, more than the 5-bit cells of
    the narrow sweep count, so the candidate goes on the list of the 16-bit re-run -- which a steady-state pass launches for MM_WIDE_CAP
    candidates.  (The list's length is not reported by any pass: the precondition is that B has more candidates than the re-run covers and
    fits everything before it; that more than MM_WIDE_CAP of them are listed is what the flag says.)"""
    from mashmap_amd import capi
    g = U.random_dna(9071, 400000)
    unit = U.random_dna(9072, 8000)
    B = [g[41 * i:41 * i + 300 + (i % 11) * 40].copy() for i in range(8000)]
    A = reads_of([unit], 9073, 8000, rl=5000)                                   # three candidates each: streams no shorter than the short reads' (theirs are long)
    contigs = [g, strewn(9074, unit, 3, 0.004, spacing=14000)]
    def pre(fa, fb):
        assert fb.points_demand() <= pts_cap(fa.nF) and fb.fits_l1_of(fa) and fb.n1 <= cand_cap(fa.n1) and fb.ops <= ops_cap(fa.ops), "B overflows a stage before the sweep"
        assert fb.n1 > WIDE_CAP and fb.n2 <= loci_cap(fa.n1, fa.n2)
    redone_pair(built(contigs, 130, k=19, seg=5000, pi=0.85), A, B, capi.MM_REDO_L2_LIST, pre=pre, b_never_steady=True,
                a_outgrows_b=capi.MM_REDO_L1)          # (A's 24 000 candidates against the candCap B's 8 000 leave: k_l1_gate)


def test_more_doubly_open_candidates_than_the_exact_kernel_covers(oracle):
    """an index in which every fifth window of ONE contig is there twice, shifted (test_map_overlapping_windows_of_one_hash): candidates on
    that contig have a query hash open twice and go on the exact kernel's list, launched for MM_EXACT_CAP in a steady-state pass; A's reads
    fall on the other contig.  (Precondition as for the wide list.)"""
    from mashmap_amd import capi
    cs = [U.random_dna(9081, 300000), U.random_dna(9082, 300000)]
    def overlap(recs):
        pick = recs[recs["seqId"] == 1][::5].copy()
        pick["wpos"] += 13; pick["wpos_end"] += 13
        allr = np.concatenate([recs, pick])
        return allr[np.lexsort((np.arange(len(allr)), allr["wpos"], allr["seqId"]))]
    h = oracle.session(named("c", cs), 19, 5000, 130, PI, mutate_index=overlap)
    ix = oracle.export_index(h)
    def make():
        c = capi.Context(k=19, segLength=5000, sketchSize=130, flags=capi.MM_FLAG_HG_FILTER)
        c.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"]); c.set_tables_default(PI)
        return c
    A, B = reads_of([cs[0]], 9083, 1500, rl=5000), reads_of([cs[1]], 9084, 1500, rl=5000)
    def pre(fa, fb):
        assert fb.points_demand() <= pts_cap(fa.nF) and fb.fits_l1_of(fa) and fb.n1 <= cand_cap(fa.n1) and fb.ops <= ops_cap(fa.ops), "B overflows a stage before the sweep"
        assert fb.n1 > EXACT_CAP and fb.n2 <= loci_cap(fa.n1, fa.n2)
    try:
        redone_pair(make, A, B, capi.MM_REDO_L2_LIST, pre=pre, b_never_steady=True)
        gpucheck.run_and_compare(oracle, named("c", cs), named("a", A[:15]) + named("b", B[:15]), pi=PI, mutate_index=overlap, verbose=False)
    finally:
        oracle.free(h)


def loci_per_candidate(make_ctx, reads):
    c = make_ctx(); c.reads_upload(reads); c.map()
    l2 = c.results()[2]; c.close()
    return np.bincount(l2["cand"]) if len(l2) else np.zeros(1, dtype=np.int64)


def test_l2_loci_outgrow_their_buffer(oracle):
    """A's reads come out of an array of six diverged copies (long candidates, one best locus); B's out of an array of six EXACT copies of a
    unit longer than a segment: about as many candidates and stream entries, five or six tied loci in most of them -- no more than the
    slots per candidate hold, more in all than l2Cap = 2 candCap + 1 024"""
    from mashmap_amd import capi
    ua, ub = U.random_dna(9051, 1100), U.random_dna(9052, 1300)
    contigs = [UNIQ[:200000], arrayed(9053, ua, 6, 0.03), arrayed(9054, ub, 6, 0)]
    A, B = unit_reads(ua, 9055, 1500), unit_reads(ub, 9056, 1500)
    make = built(contigs, 32)
    def pre(fa, fb):
        assert fb.points_demand() <= pts_cap(fa.nF) and fb.fits_l1_of(fa) and fb.n1 <= cand_cap(fa.n1) and fb.ops <= ops_cap(fa.ops), "B overflows a stage before the loci"
        assert loci_per_candidate(make, A).max() <= LOCAP0 and loci_per_candidate(make, B).max() <= LOCAP0, "a candidate has more loci than slots"
        assert fb.n2 > loci_cap(fa.n1, fa.n2), "B's loci fit: %d <= %d" % (fb.n2, loci_cap(fa.n1, fa.n2))
    redone_pair(make, A, B, capi.MM_REDO_L2_LOCI, pre=pre)
    gpucheck.run_and_compare(oracle, named("c", contigs), named("a", A[:12]) + named("b", B[:12]), k=K, L=L, s=32, kmerPct=0.0, pi=PI, device_index=True, verbose=False)


def test_a_candidate_ties_in_more_loci_than_it_has_slots(oracle):
    """B: 100 reads out of twelve exact copies -- eleven or twelve tied loci in a candidate, more than the 8 staging slots (and the one pending
    locus) a pass over A leaves (prevLocap) -- and reads that map nowhere; A: long candidates over twelve diverged copies, unique reads,
    and no more candidates in all than the candCap B leaves, so that A's return is a steady-state pass"""
    from mashmap_amd import capi
    ua, ub = U.random_dna(9061, 1100), U.random_dna(9062, 1100)
    contigs = [UNIQ[:300000], arrayed(9063, ua, 12, 0.03), arrayed(9064, ub, 12, 0)]
    A = unit_reads(ua, 9065, 300) + reads_of([UNIQ[:300000]], 9066, 500) + [U.random_dna(9600 + i, L) for i in range(200)]
    B = unit_reads(ub, 9067, 100) + [U.random_dna(9700 + i, L) for i in range(900)]
    make = built(contigs, 32)
    def pre(fa, fb):
        assert fb.points_demand() <= pts_cap(fa.nF) and fb.fits_l1_of(fa) and fb.n1 <= cand_cap(fa.n1) and fb.ops <= ops_cap(fa.ops) \
            and fb.n2 <= loci_cap(fa.n1, fa.n2), "B overflows a stage before the slots, or the locus buffer"
        assert loci_per_candidate(make, A).max() <= LOCAP0, "A's sized pass doubled the slots itself"
        assert fa.n1 <= cand_cap(fb.n1), "A's return would outgrow the candCap B leaves"
        assert loci_per_candidate(make, B).max() > LOCAP0 + 1, "no candidate of B ties in more loci than %d slots and the pending one hold" % LOCAP0
    redone_pair(make, A, B, capi.MM_REDO_L2_SLOTS, pre=pre)


# ---- the selection ------------------------------------------------------------------------------------------------------------------------
def test_candidate_mappings_outgrow_their_buffer(oracle):
    """A: reads half a segment long, one candidate and one mapping each, long streams; B: whole segments of a unit that is there twice, far
    apart and exact -- two candidates, both accepted: twice the mappings on fewer stream entries"""
    from mashmap_amd import capi
    ub = U.random_dna(9092, 1500)
    contigs = [UNIQ[:300000], strewn(9097, ub, 2, 0)]
    A = [a[300:800].copy() for a in reads_of([UNIQ[:300000]], 9098, 600)]
    B = reads_of([ub], 9099, 600)
    def pre(fa, fb):
        assert fb.points_demand() <= pts_cap(fa.nF) and fb.fits_l1_of(fa) and fb.n1 <= cand_cap(fa.n1) and fb.ops <= ops_cap(fa.ops) \
            and fb.n2 <= loci_cap(fa.n1, fa.n2), "B overflows a stage before the selection"
        assert fb.nmap > map_cap(fa.nmap), "B's mappings fit: %d <= %d" % (fb.nmap, map_cap(fa.nmap))
    redone_pair(built(contigs, 64), A, B, capi.MM_REDO_MAPPINGS, pre=pre)
    gpucheck.run_and_compare(oracle, named("c", contigs), named("a", A[:20]) + named("b", B[:20]), k=K, L=L, s=64, kmerPct=0.0, pi=PI, device_index=True, verbose=False)


# ---- the launcher -------------------------------------------------------------------------------------------------------------------------
def test_three_redone_attempts_in_a_row_end_the_steady_attempts_of_a_context(oracle):
    """mm_launch_map: batches that alternate between few and many candidates have every steady attempt redone (steadyFails); after the third
    the context sizes every pass without an attempt.  FINDING: nothing lets it return -- steadyFails is cleared only by a steady-state pass
    that went through, and without an attempt there is none; a sized pass, however well the next batch would fit, does not clear it.
    Pinned here as it is: the same batch twice in a row, which any other context maps as a steady-state pass, stays sized."""
    from mashmap_amd import capi
    unit = U.random_dna(9101, 3000)
    contigs = [UNIQ, strewn(9102, unit, 3, 0.004)]
    make = built(contigs, 32)
    small, big = reads_of([UNIQ], 9103, 1000), reads_of([unit], 9104, 1000)
    more = small + small[:150]                                                   # over a tenth more fragments than `big`: sized without an attempt
    fs, fb, fm = Fresh(make, small), Fresh(make, big), Fresh(make, more)
    assert fm.nF > fb.nF + fb.nF // 10 and fb.nF <= fm.nF + fm.nF // 10
    assert fb.n1 > cand_cap(fs.n1) and fb.n1 > cand_cap(fm.n1), "the many-candidate batch fits what the few-candidate ones leave"
    ctx = make()
    def run(reads, want):
        ctx.reads_upload(reads); ctx.map()
        assert gpucheck.pass_bytes(ctx) == want.bytes
        return ctx.pass_stats()[1], ctx.pass_redo_cause(), ctx.pass_totals()["redone"]
    assert run(small, fs) == (False, 0, 0)
    for i in range(3):
        steady, cause, redone = run(big, fb)                                     # an attempt against candCap of a few-candidate batch: redone
        assert not steady and cause & capi.MM_REDO_L1 and redone == i + 1, (i, steady, cause, redone)
        if i < 2:                                                                # candCap made small again by a pass that is sized outright (a steady-state pass would clear the count)
            assert run(more, fm) == (False, 0, i + 1)
    for reads, want in ((big, fb), (big, fb), (small, fs), (small, fs)):         # three in a row: no attempt any more, whatever comes
        assert run(reads, want) == (False, 0, 3)
    ctx.close()


def test_a_chunked_sized_pass_is_not_followed_by_a_steady_one(oracle, monkeypatch):
    """MM_L2_STREAM_MIB small enough that the sized pass takes its streams through in chunks (l2Chunks != 1): the next pass over the same
    batch is sized again, without an attempt, and exact"""
    from mashmap_amd import capi
    reads = reads_of([UNIQ], 9113, 600)
    make = built([UNIQ], 64)
    want = Fresh(make, reads)
    monkeypatch.setenv("MM_L2_STREAM_MIB", "0.05")
    assert want.ops * 4 > 4 * 0.05 * (1 << 20), "the streams fit one chunk"
    ctx = make()
    ctx.reads_upload(reads)
    for _ in range(3):
        ctx.map()
        assert gpucheck.pass_bytes(ctx) == want.bytes and not ctx.pass_stats()[1] and ctx.pass_redo_cause() == 0
    assert ctx.pass_totals() == {"passes": 3, "steady": 0, "redone": 0}
    ctx.close()


# ---- the steady leg of the parity cases -----------------------------------------------------------------------------------------------------
# run_and_compare calls of tests/test_gpu_map.py whose second pass the rule (gpucheck.must_be_steady) exempts, by their flags and sketch size
EXEMPT_IN_TEST_GPU_MAP = {
    "test_map_against_the_device_built_index[5-#-0.001]": ["skip_prefix"],
    "test_map_self_skip_prefix_lower_triangular": ["skip_prefix"],              # the first of its three calls
    "test_map_sketch_beyond_8190": ["sketch"],
    "test_map_no_split_reads_longer_than_the_segment[default]": ["nosplit"],
    "test_map_no_split_reads_longer_than_the_segment[dup_nohg]": ["nosplit"],
    "test_map_no_split_reads_longer_than_the_segment[prefix]": ["skip_prefix"],
    "test_map_no_split_read_longer_than_the_lds": ["nosplit"],
    "test_map_no_split_window_with_many_candidates[False]": ["nosplit"],
    "test_map_no_split_window_with_many_candidates[True]": ["skip_prefix"],
}
CALLS_IN_TEST_GPU_MAP = 51


def test_every_parity_case_the_rule_does_not_exempt_took_the_steady_leg(oracle, request):
    """run_and_compare logs the second pass of every call (gpucheck.STEADY_LOG).  Over the calls made here, one of each kind, and over the
    calls of every test of tests/test_gpu_map.py that this session collected ahead of this one: the exempt ones are exactly those the
    rule names from their flags and sketch size (7 of the module's 46 calls: none for want of candidates), and every other took the
    steady leg in one wait.  A collected parity test that left nothing in the log (it ran in another process) fails this test."""
    g = [("hapA#1#c", UNIQ[:120000]), ("hapB#1#c", U.random_dna(9121, 90000))]
    rd = named("hapA#1#r", reads_of([UNIQ[:120000]], 9122, 12, rl=2500))
    at = len(gpucheck.STEADY_LOG)
    gpucheck.run_and_compare(oracle, g, rd, k=K, L=L, s=64, verbose=False)
    gpucheck.run_and_compare(oracle, g, rd, k=K, L=L, s=64, flags=U.FLAG_HG | U.FLAG_SKIP_PREFIX, delim="#", verbose=False)
    gpucheck.run_and_compare(oracle, g, rd, k=K, L=L, s=64, flags=U.FLAG_HG | U.FLAG_NOSPLIT, verbose=False)
    gpucheck.run_and_compare(oracle, g, named("r", reads_of([UNIQ[:120000]], 9123, 12, rl=900)), k=K, L=L, s=64, flags=U.FLAG_HG | U.FLAG_NOSPLIT, verbose=False)
    assert [(e["want"], e["why"]) for e in gpucheck.STEADY_LOG[at:]] == [(True, None), (False, "skip_prefix"), (False, "nosplit"), (True, None)]
    for e in gpucheck.STEADY_LOG:
        assert e["cause"] == 0 and e["stats"][1] == e["want"] and (not e["want"] or e["stats"][0] == 1), e
    name = lambda e: e["test"].split("::", 1)[1].split(" ")[0]
    mine = [e for e in gpucheck.STEADY_LOG if "test_gpu_map.py::" in e["test"]]
    ahead = []                                                                   # the parity module's tests this session runs before this one
    for item in request.session.items:
        if item.nodeid == request.node.nodeid:
            break
        if "test_gpu_map.py::" in item.nodeid:
            ahead.append(item.name)
    exempt = {}
    for e in mine:
        if not e["want"]:
            exempt.setdefault(name(e), []).append(e["why"])
    print("steady leg: %d of %d run_and_compare calls of test_gpu_map.py (%d of its tests collected ahead), exempt: %r"
          % (len(mine) - sum(map(len, exempt.values())), len(mine), len(ahead), exempt))
    expected = {n: why for n, why in EXEMPT_IN_TEST_GPU_MAP.items() if n in ahead}
    assert exempt == expected, "exempt by the rule: %r, logged: %r (a test that ran in another process leaves no log here)" % (expected, exempt)
    assert {name(e) for e in mine} <= set(ahead)
    if len(expected) == len(EXEMPT_IN_TEST_GPU_MAP):                             # the whole module, not a selection
        assert len(mine) == CALLS_IN_TEST_GPU_MAP, len(mine)
