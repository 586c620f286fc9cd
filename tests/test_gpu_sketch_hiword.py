"""k_sketch_fast tests a position on the high words of its two hashes (one v_min_u32, one 32-bit compare), stores the smaller hash by two
exec-masked writes, sends a fragment with a tie of high words to the exact kernel, and leaves the range and N tests to the drain
(mm_sketch.hip, mm_sketch_dev.h).  Every sketch here is compared entry for entry with the CPU oracle (hash, first and last position, strand,
count) at the places where that form can go wrong: fragments of no, one, 20 and 21 positions (strips of 20 at k = 19 and segments of 5 kbp),
a fragment whose strip loop runs twice, k-mers that are their own reverse complement with every position passing, an N next to a strip's
edge, an N run, a tandem repeat and a homopolymer; sketch sizes 4 and 130."""
import numpy as np
import pytest

import mmutil as U

pytestmark = pytest.mark.gpu

L = 5000


def entries(rows):
    return [(int(x["hash"]), int(x["wpos"]), int(x["wpos_end"]), int(x["seqId"]), int(x["strand"])) for x in rows]


def sketch_and_compare(oracle, reads, k, s, seg=L):
    """every read is at most one segment long: one fragment per read of at least k bases, none for a shorter one"""
    from mashmap_amd import capi
    ctx = capi.Context(k=k, segLength=seg, sketchSize=s)
    nF = ctx.reads_upload(reads)
    got, cnt = ctx.sketch()
    ctx.close()
    frs = [(ri, a) for ri, a in enumerate(reads) if len(a) >= k]
    assert all(len(a) <= seg for a in reads) and nF == len(frs)
    for f, (ri, a) in enumerate(frs):
        exp = oracle.sketch_sequence(a, k, s, ri)
        assert entries(got[f, :cnt[f]]) == exp, ("read %d of %d bases" % (ri, len(a)), cnt[f], len(exp), entries(got[f, :3]), exp[:3])
    return cnt


def cut(s, n):
    """mm_sketch_fast_cut (mm_sketch_plan.h), in float as it is there; None = no cut"""
    want = int(s + 4.2 * np.sqrt(float(s)) + 0.999)
    if want >= n:
        return None
    return int(np.float32(want) / np.float32(2 * n) * np.float32(18446744073709551616.0))


def palindrome(seed, k):
    half = U.random_dna(seed, k // 2)
    return np.concatenate([half, U.revcomp(half)])


@pytest.mark.parametrize("s", [4, 130])
def test_short_fragments_and_strip_edges(oracle, s):
    k = 19
    reads = [U.random_dna(900 + i, n) for i, n in enumerate((k - 1, k, k + 19, k + 20, k + 21, k + 39, k + 40, 700, L))]
    for off in (19, 20, 21):                           # an N at offsets 19, 20, 21 of the fourth strip of 20, one read each, and all three in one
        a = U.random_dna(920 + off, L); a[60 + off] = ord("N"); reads.append(a)
    a = U.random_dna(930, L); a[[79, 80, 81]] = ord("N"); reads.append(a)
    a = U.random_dna(931, L); a[L - 1] = ord("N"); reads.append(a)         # the last base: only the last k-mer goes
    a = U.random_dna(932, L); a[0] = ord("n"); reads.append(a)
    cnt = sketch_and_compare(oracle, reads, k, s)
    assert cnt[0] == min(s, 1) and cnt[1] == min(s, 20) and cnt[2] == min(s, 21)      # fragments of k, k + 19, k + 20 bases (the first read makes none)


@pytest.mark.parametrize("s", [4, 130])
def test_the_strip_loop_runs_twice(oracle, s):
    """segments of 20 kbp: 1 249 strips of 16 positions on 1 024 threads"""
    reads = [U.random_dna(940, 20000), U.random_dna(941, 16384 + 18), U.random_dna(942, 16384 + 19), U.with_n_runs(U.random_dna(943, 20000), 5, 3, 50)]
    sketch_and_compare(oracle, reads, 19, s, seg=20000)


@pytest.mark.parametrize("s", [4, 130])
@pytest.mark.parametrize("k", [16, 20])
def test_own_reverse_complements_vanish_when_every_position_passes(oracle, k, s):
    """s >= n: no cut.  A k-mer that is its own reverse complement hashes alike on both strands and is no sketch entry (commonFunc.hpp:237)"""
    reads = []
    for i, n in enumerate((4,) if s == 4 else (4, 60, 130)):
        a = U.random_dna(950 + i, n + k - 1)
        for at in (1, k + 2, 2 * k + 2, 3 * k + 9):       # apart, back to back, and anywhere
            if at + k <= len(a):
                a[at:at + k] = palindrome(960 + at, k)
        reads.append(a)
        assert cut(s, n) is None and n <= s
        pal = bytes(a[1:1 + k])
        assert pal == bytes(U.revcomp(a[1:1 + k])) and oracle.get_hash(pal) not in [e[0] for e in oracle.sketch_sequence(a, k, s, 0)]
    # ... and under a cut, in a whole segment
    a = U.random_dna(970, L)
    for at in range(100, L - k, 400):
        a[at:at + k] = palindrome(980 + at, k)
    reads.append(a)
    sketch_and_compare(oracle, reads, k, s)


@pytest.fixture(scope="module")
def mapper():
    """contexts with a small index, for pass_counts()["hard"] of a mapped batch"""
    from mashmap_amd import capi
    g = U.random_dna(990, 60000)
    made = {}

    def get(s):
        if s not in made:
            made[s] = capi.Context(k=19, segLength=L, sketchSize=s, flags=capi.MM_FLAG_HG_FILTER)
            made[s].index_build([g], kmerPct=0.0); made[s].set_tables_default(0.85)
        return made[s]
    yield get
    for c in made.values():
        c.close()


def hard_fragments(ctx, reads):
    ctx.reads_upload(reads); ctx.map()
    return ctx.pass_counts()["hard"]


@pytest.mark.parametrize("s", [4, 130])
def test_random_segments_stay_off_the_hard_list_and_hard_cases_are_exact(oracle, mapper, s):
    k = 19
    random_reads = [U.random_dna(1000 + i, L) for i in range(4)]
    T = cut(s, L - k + 1)
    for a in random_reads:                             # what the input has to offer for the assertion below: s distinct hashes under the cut
        assert sum(e[0] < T for e in oracle.sketch_sequence(a, k, 64 + s, 0)) >= s
    sketch_and_compare(oracle, random_reads, k, s)
    ctx = mapper(s)
    assert hard_fragments(ctx, random_reads) == 0
    nrun = U.random_dna(1010, L); nrun[2000:2300] = ord("N")                      # an N run of 300: hashed as poly-A in the loop, dropped by the drain
    nruns = U.with_n_runs(U.random_dna(1011, L), 7, 6, 45)
    period7 = U.tandem_repeat(1012, L, 7)                                          # 7 distinct k-mers: the duplicate list overflows
    polyA = np.full(L, ord("A"), dtype=np.uint8)                                   # one hash, 4 982 times
    mixed = U.random_dna(1013, L); mixed[1000:1600] = ord("A"); mixed[3000:3700] = np.tile(U.random_dna(1014, 7), 100)
    hard_cases = [nrun, nruns, period7, polyA, mixed]
    sketch_and_compare(oracle, hard_cases, k, s)
    n_hard = hard_fragments(ctx, random_reads + hard_cases)
    print("s = %d: %d of the %d special fragments went to the hard list" % (s, n_hard, len(hard_cases)))
    assert 2 <= n_hard <= len(hard_cases)              # the repeat and the homopolymer have fewer than s distinct hashes (s = 4: overflow their duplicate list)
