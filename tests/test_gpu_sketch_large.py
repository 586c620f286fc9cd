"""MM_OPT_SKETCH_LARGE: sketches beyond 8190 entries on k_sketch_large -- the strip hashers of the LDS sketch kernels, the survivors of
k_sketch_global's cut sorted in LDS tiles of MM_SKL_TILE entries with sweeps through HBM only between tiles, k_sketch_global's emission.

Every sketch-only case derives its figures on the CPU first -- the oracle's sketch per fragment, the cut (mm_sketch_cut, restated here)
and from the two which fragments the kernel must sort without a cut -- asserts the conditions it exists for, and then sketches the batch
on two fresh contexts, option on and off: the bytes identical, every checked fragment equal to the oracle's, sketch_large_counts() as
predicted.  k = 16 unless a case says otherwise.

The cut and the shapes.  The cut T aims at s + 5 sqrt(s) + 64 of the 2n strand hashes, but what survives it are canonical hashes, the smaller
of a position's two: n (1 - (1 - t)^2) = 2nt - nt^2 of them at t = T / 2^64.  At the small shapes of cases 1, 2, 4, 5 and 6 (s = 0.82 n) that
is 0.68 n, fewer than s: every fragment with a real cut is done again without one there -- the oracle says so per fragment, the cases
assert it, and those cases check the retry, the sort without a cut and every edge of the input.  The cut that stands needs s well below n:
case 8 (s = 8 200 over 100 kbp, nt^2 = 190 of a margin of 517) is there for it."""
import math

import numpy as np
import pytest

import largewave as W
import mmutil as U

pytestmark = pytest.mark.gpu

SKL_TILE = 4096                        # mm_sketch_large_plan.h: MM_SKL_TILE (tests/test_sketch_large_abi.py holds the two together)
K = 16


def sketch_cut(s, n):
    """mm_sketch_cut: None = no cut (MM_HASH_MAX)"""
    want = float(s) + 5.0 * math.sqrt(float(s)) + 64.0
    return None if want >= float(n) else int(want / (2.0 * float(n)) * 18446744073709551616.0)


def expected(oracle, reads, k, s, L, every=1):
    """per fragment, in the order Map::mapModule cuts them: (read, offset, length); for every `every`-th the oracle's sketch and whether
    k_sketch_large must end up sorting it without a cut.  No s-th hash may lie within a relative 1e-6 of the cut (another seed then)"""
    frs, exp, uncut, why = [], {}, {}, {}
    for ri, a in enumerate(reads):
        if len(a) < k: continue
        for off, ln in W.fragments_of(len(a), L):
            f = len(frs)
            frs.append((ri, off, ln))
            if f % every: continue
            e = oracle.sketch_sequence(a[off:off + ln], k, s, ri)
            T = sketch_cut(s, ln - k + 1)
            if T is not None and len(e) >= s:
                assert abs(e[s - 1][0] - T) > 1e-6 * T, "fragment %d: the s-th hash lies at the cut" % f
            exp[f] = e
            why[f] = "no cut" if T is None else "few" if len(e) < s else "cut too low" if e[s - 1][0] >= T else ""
            uncut[f] = why[f] != ""
    return frs, exp, uncut, why


def rows(got, cnt, f):
    c = int(cnt[f])
    return list(zip(got["hash"][f, :c].tolist(), got["wpos"][f, :c].tolist(), got["wpos_end"][f, :c].tolist(), got["seqId"][f, :c].tolist(), got["strand"][f, :c].tolist()))


def sketch_both(reads, k, s, L, frs, exp, n_uncut):
    """the batch on two fresh contexts; n_uncut None: predicted from the sketches themselves (a case that does not ask the oracle about every fragment)"""
    from mashmap_amd import capi
    out = {}
    for on in (False, True):
        ctx = capi.Context(k=k, segLength=L, sketchSize=s)
        if on: ctx.sketch_large()
        nF = ctx.reads_upload(reads)
        got, cnt = ctx.sketch()
        out[on] = (nF, got, cnt, ctx.sketch_large_counts(), [(int(x["readId"]), int(x["fragStart"]), int(x["len"])) for x in ctx.fragments()])
        ctx.close()
    (nF, got, cnt, counts_off, frags), (nF1, got1, cnt1, counts_on, _) = out[False], out[True]
    assert nF == nF1 == len(frs) and frags == frs
    assert cnt.tobytes() == cnt1.tobytes(), "counts differ between k_sketch_large and k_sketch_global: %r" % (np.nonzero(cnt != cnt1)[0][:8],)
    assert got.tobytes() == got1.tobytes(), "sketch bytes differ in fragments %r" % (np.nonzero((got != got1).any(axis=1))[0][:8],)
    bad = [f for f in sorted(exp) if rows(got1, cnt1, f) != exp[f]]
    assert not bad, ("fragments that differ from the oracle", bad[:8], [(int(cnt1[f]), len(exp[f])) for f in bad[:8]])
    if n_uncut is None:
        n_uncut = sum(1 for f, (_, _, ln) in enumerate(frs) if sketch_cut(s, ln - k + 1) is None or cnt[f] < s or int(got["hash"][f, s - 1]) >= sketch_cut(s, ln - k + 1))
    print("%d fragments, %d without a cut; counts off %r, on %r" % (nF, n_uncut, counts_off, counts_on))
    assert counts_off == (0, 0)
    assert counts_on == (nF, n_uncut)
    return got1, cnt1


# ----------------------------------------------------------------------------- 1: the first size of the route
def test_s8200_every_kind_of_fragment_in_one_batch(oracle):
    s, L = 8200, 10000
    rnd = U.random_dna(8101, L)
    pal = U.random_dna(8106, L); pal[4000:4400] = np.frombuffer(b"ACGT" * 100, dtype=np.uint8)      # palindromic 16-mers: the two strands hash alike
    named = [("random", rnd), ("three", U.random_dna(8102, 20777)), ("n_runs", U.with_n_runs(U.random_dna(8103, L), 8104, 5, 40)),
             ("rc", U.revcomp(U.mutate(rnd, 8105, 0.04)[:L])), ("short", U.random_dna(8107, 3000)), ("k_bases", U.random_dna(8108, K)),
             ("k_minus_1", U.random_dna(8109, K - 1)), ("all_n", np.frombuffer(b"N" * L, dtype=np.uint8).copy()), ("tandem", U.tandem_repeat(8110, L, 37)),
             ("palindromes", pal)]
    reads = [a for _, a in named]
    frs, exp, uncut, why = expected(oracle, reads, K, s, L)
    name_of = [named[ri][0] for ri, _, _ in frs]
    print([(nm, len(exp[f]), why[f]) for f, nm in enumerate(name_of)])
    assert name_of.count("three") == 3 and "k_minus_1" not in name_of and len(frs) == 11
    # the short reads have no cut to begin with, the tandem and the all-N read too few hashes under any cut; the others have s hashes and a cut
    # below the s-th of them (the module's docstring): all eleven are sorted without a cut, nine of them on the second attempt
    assert {nm: why[f] for f, nm in enumerate(name_of)} == dict(short="no cut", k_bases="no cut", all_n="few", tandem="few", random="cut too low", three="cut too low",
                                                               n_runs="cut too low", rc="cut too low", palindromes="cut too low")
    by = {nm: exp[name_of.index(nm)] for nm in ("short", "k_bases", "all_n", "tandem", "random", "palindromes")}
    assert 0 < len(by["short"]) < s and len(by["k_bases"]) == 1 and len(by["all_n"]) == 0 and len(by["tandem"]) <= 37 and len(by["random"]) == s
    assert any(a[1] != a[2] for a in by["tandem"])                                         # runs of equal hashes: first and last position differ
    assert not any(4000 <= a[1] <= 4384 and a[1] % 2 == 0 for a in by["palindromes"])      # the planted palindromes are skipped (ACGT... at even offsets)
    sketch_both(reads, K, s, L, frs, exp, sum(uncut.values()))


# ----------------------------------------------------------------------------- 2: several tiles, sweeps at three values of k2
def test_s19998_sorts_32768_entries(oracle):
    """the three reads of test_gpu_large_wave.py's case_edge: the cut aims at 20 770 survivors, the sort without a cut takes 23 985 positions;
    either way 32 768 entries in tiles of 4 096: the sweeps of k2 = 8 192, 16 384 and 32 768"""
    s, L = 19998, 24000
    g = U.random_dna(9201, 120000)
    reads = [U.mutate(g[30000:30000 + L + 1500], 9210, 0.05)[:L].copy(), U.revcomp(U.mutate(g[80000:80000 + L + 900], 9211, 0.03)[:L]), g[:L].copy()]
    frs, exp, uncut, why = expected(oracle, reads, K, s, L)
    want = s + 5.0 * math.sqrt(s) + 64.0
    assert 4 * SKL_TILE < want <= 8 * SKL_TILE and len(frs) == 3 and all(len(e) == s for e in exp.values())
    # ... in either attempt: 0.68 n = 16 300 distinct hashes below the cut, fewer than s, then all 23 985 positions without one
    assert all(w == "cut too low" for w in why.values()) and 4 * SKL_TILE < L - K + 1 <= 8 * SKL_TILE
    sketch_both(reads, K, s, L, frs, exp, 3)


# ----------------------------------------------------------------------------- 3: the strand sum is an int16
def test_the_strand_sum_wraps_as_the_references_int16(oracle):
    s, L = 8200, 40000
    A = lambda n: np.full(n, ord("A"), dtype=np.uint8)
    reads = [A(40000), np.concatenate([A(33000), U.random_dna(8301, 7000)]), A(20000)]
    frs, exp, uncut, why = expected(oracle, reads, K, s, L)
    assert len(frs) == 3 and len(exp[0]) == 1 and len(exp[2]) == 1 and exp[0][0][0] == exp[2][0][0]
    poly = exp[0][0][0]
    mixed = [a for a in exp[1] if a[0] == poly]
    assert len(mixed) == 1 and (mixed[0][1], mixed[0][2]) == (0, 33000 - K) and (exp[0][0][1], exp[0][0][2]) == (0, 40000 - K)
    control = exp[2][0][4]
    assert control in (1, -1) and exp[0][0][4] == -control and mixed[0][4] == -control     # 39 985 and 32 985 occurrences: past 32 767, the sum wraps
    assert uncut[0] and uncut[2]
    sketch_both(reads, K, s, L, frs, exp, sum(uncut.values()))


# ----------------------------------------------------------------------------- 4: every hasher
@pytest.mark.parametrize("k", [11, 19, 32, 40, 57])
def test_every_strip_hasher(oracle, k):
    """k = 11: the generic tables; 19: the tuned tail; 32: the product tables' largest; 40: wide strips of 4 words; 57: of 5"""
    s, L = 8200, 10000
    reads = [U.random_dna(8400 + k, L), U.with_n_runs(U.random_dna(8500 + k, L), 8600 + k, 4, 50)]
    frs, exp, uncut, why = expected(oracle, reads, k, s, L)
    assert len(frs) == 2 and len(exp[0]) == s
    sketch_both(reads, k, s, L, frs, exp, sum(uncut.values()))


# ----------------------------------------------------------------------------- 5: more fragments than workgroups
def test_more_fragments_than_workgroups(oracle):
    """1 100 one-fragment reads: every workgroup takes several fragments through the same LDS tables and the same slice"""
    s, L = 8200, 10000
    g = U.random_dna(8701, 300000)
    starts = (U.splitmix64(8702, 1100) % np.uint64(len(g) - L)).astype(np.int64)
    reads = [g[x:x + L] for x in starts]
    frs, exp, uncut, why = expected(oracle, reads, K, s, L, every=20)
    assert len(frs) == 1100 and len(exp) == 55 and all(w == "cut too low" for w in why.values())
    sketch_both(reads, K, s, L, frs, exp, None)


# ----------------------------------------------------------------------------- 6: a whole pass
def test_a_whole_pass_at_s8200(oracle):
    """the shape of test_gpu_large_wave.py's test_sketch_8200_with_twelve_tied_loci (its contigs and reads), MM_OPT_L2_LARGE_WAVE = 1 on both
    contexts: everything the pass leaves is the same with the sketches from k_sketch_large, and the pass has no host wait more"""
    import gpucheck
    from mashmap_amd import capi
    k, L, s, pi = 16, 10000, 8200, 0.80
    unit = U.random_dna(9101, 11000)
    uniq = U.random_dna(9104, 60000)
    contigs = [("unique", uniq), ("array", W.arrayed(9101, unit, 12, 0))]
    reads = [U.mutate(unit[300:300 + L + 300], 9110, 0.02)[:L].copy(), U.mutate(uniq[20000:20000 + 20777 + 1500], 9111, 0.05)[:20777].copy(),
             uniq[:L].copy(), uniq[len(uniq) - L:].copy(), U.revcomp(U.mutate(uniq[45000:45000 + L + 300], 9112, 0.03)[:L])]
    h = oracle.session(contigs, k, L, s, pi, U.FILTER_MAP, 0, b"\0", 0.0)
    try:
        assert oracle.f("session_index_size")(h) == 205022
        ix = oracle.export_index(h)
        min_hits, cutoffs = oracle.min_hits_table(s, k, pi), oracle.cutoffs(h)
    finally:
        oracle.free(h)
    frs, _, uncut, _ = expected(oracle, reads, k, s, L)
    assert len(frs) == 7
    out = {}
    for on in (False, True):
        ctx = capi.Context(k=k, segLength=L, sketchSize=s, flags=0)
        ctx.l2_large_wave(1)
        if on: ctx.sketch_large()
        ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"])
        ctx.set_tables(min_hits, cutoffs)
        ctx.set_replay_tables(*W.replay_tables(s, k, pi))
        nF = ctx.reads_upload(reads, None, [-1] * len(reads), 0)
        ctx.map()
        out[on] = dict(bytes=gpucheck.pass_bytes(ctx), stats=ctx.pass_stats(), counts=ctx.pass_counts(), large=ctx.sketch_large_counts(), l2=ctx.pass_l2_large(),
                       n=ctx.result_counts(), nF=nF)
        ctx.close()
    print({on: (o["stats"], o["counts"], o["large"], o["l2"], o["n"]) for on, o in out.items()})
    assert out[True]["nF"] == 7 and out[True]["n"][0] >= 7 and out[True]["n"][1] >= 7
    for a, b, what in zip(out[True]["bytes"], out[False]["bytes"], ("stats", "l1", "l2", "mappings", "query sketches")):
        assert len(a) > 0 and a == b, what
    assert out[True]["stats"] == out[False]["stats"] and out[True]["stats"][1] is False
    assert out[True]["counts"] == out[False]["counts"] and out[True]["counts"]["hard"] == 0
    assert out[True]["l2"] == out[False]["l2"]
    assert out[False]["large"] == (0, 0) and out[True]["large"] == (7, sum(uncut.values()))


# ----------------------------------------------------------------------------- 7: other sizes are left alone
def test_the_option_does_nothing_at_sketch_130(oracle):
    from mashmap_amd import capi
    k, L, s = 19, 5000, 130
    g = U.random_dna(1, 400000)
    reads = [a for _, a, _ in U.sample_reads([g], 2, 40, 10000, 0.1)]
    reads += [a for _, a, _ in U.sample_reads([g], 3, 10, 12345, 0.05)]
    reads += [U.random_dna(50, 700), U.random_dna(51, 19), U.random_dna(52, 18), U.random_dna(53, 5000), U.random_dna(54, 5001)]
    out = {}
    for on in (False, True):
        ctx = capi.Context(k=k, segLength=L, sketchSize=s)
        if on: ctx.sketch_large()
        ctx.reads_upload(reads)
        got, cnt = ctx.sketch()
        counts = ctx.sketch_large_counts()
        ctx.index_build([g], kmerPct=0.0); ctx.set_tables_default(0.85)
        ctx.map(); first = ctx.pass_stats()
        ctx.map()
        out[on] = (got.tobytes(), cnt.tobytes(), counts, first[1], ctx.pass_stats(), ctx.sketch_large_counts())
        ctx.close()
    assert out[True][0] == out[False][0] and out[True][1] == out[False][1] and len(out[True][0]) > 0
    for on in (False, True):
        assert out[on][2] == (0, 0) and out[on][5] == (0, 0)
        assert out[on][3] is False and out[on][4] == (1, True), out[on][3:5]
    ctx = capi.Context(k=k, segLength=L, sketchSize=s)
    with pytest.raises(capi.MashmapError):
        ctx.sketch_large_counts()                                  # MM_ERR_STATE: no sketch launch yet
    ctx.close()


# ----------------------------------------------------------------------------- 8: the cut that stands
def test_the_cut_stands_at_100_kbp(oracle):
    """s = 8 200 over fragments of 100 kbp: some 8 500 distinct hashes below the cut, so the first attempt is the final one -- 16 384 entries,
    four tiles, the sweeps of k2 = 8 192 and 16 384 -- and the emission stops at the s-th of them.  A 20 kbp read beside them has no cut"""
    s, L = 8200, 100000
    reads = [U.random_dna(8901, L), U.with_n_runs(U.random_dna(8902, L), 8903, 6, 60), U.revcomp(U.random_dna(8904, L + 4321)), U.random_dna(8905, 20000)]
    frs, exp, uncut, why = expected(oracle, reads, K, s, L)
    print([(fr, len(exp[f]), why[f]) for f, fr in enumerate(frs)])
    want = s + 5.0 * math.sqrt(s) + 64.0
    assert 2 * SKL_TILE < want <= 4 * SKL_TILE and len(frs) == 5
    assert [why[f] for f in range(5)] == ["", "", "", "", "cut too low"] and all(len(e) == s for e in exp.values())
    sketch_both(reads, K, s, L, frs, exp, 1)
