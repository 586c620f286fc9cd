"""MM_OPT_L1_GROUP_STREAM: under -Y reference groups (MM_FLAG_SKIP_PREFIX) the queued fragments' L1 stage on k_l1_stream_groups, the
wave-per-fragment kernel that runs one body per reference-group extent of the sorted points; the literal k_l1_sweep takes what it leaves.

Every case first derives its figures from the oracle on the CPU and asserts them -- the conditions a case exists for hold for the oracle
alone --, then maps the batch twice on fresh contexts, with the option and without it (the literal kernel, which the CPU suite holds
against the oracle): stats, L1, L2 and candidate mappings byte-identical, L1 equal to the oracle's per fragment, `literal` equal to the
number of fragments the grouped form of the hand-over rule names.

k = 16, segLength 500, s = 32, pi 0.90; kmerThreshold 0 where repeats are planted (no seed is frequent).  Reads are named r<i>: they
belong to no reference group, so none of their points is dropped and the oracle's point list is the device's."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gpucheck
import mmutil as U
import test_gpu_skip_prefix_stream as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BIN = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
K, L, S, PI = T.K, T.L, T.S, T.PI
STREAM_BUF = 64                                                  # mm_map.hip: MM_STREAM_BUF
SORT_LDSCAP = 4096                                               # mm_map.hip: MM_SORT_LDSCAP, the largest list the LDS sorter takes


# ----------------------------------------------------------------------------- the oracle's view, per reference-group extent
def extents(points, rg):
    """[b, e) of the maximal runs of sorted points whose contigs share a reference group (computeMap.hpp:1146-1165)"""
    out, b = [], 0
    while b < len(points):
        e = b
        while e < len(points) and rg[points[e][0]] == rg[points[b][0]]: e += 1
        out.append((b, e)); b = e
    return out


def best_count(points):
    """the best overlap count of one computeL1CandidateRegions call: the running sum of OPEN / CLOSE at the end of a position group"""
    run, best = 0, 0
    for i, p in enumerate(points):
        run += 1 if p[2] == 1 else -1
        if i + 1 == len(points) or points[i + 1][1] != p[1]: best = max(best, run)
    return best


def raised_min_hits(best, q_sketch, min_hits, cutoffs):
    """computeMap.hpp:984-998: None when the call yields nothing"""
    if best < min_hits: return None
    return max(min_hits, int(cutoffs[min(int(min(best, q_sketch) / max(S / 1000.0, 1.0)), len(cutoffs) - 1)]))


def takes_literal_grouped(points, q_sketch, min_hits_tab, rg):
    """k_l1_stream_groups' two rules: a position group spans two contigs inside ONE extent, or minimumHits <= 0"""
    for b, e in extents(points, rg):
        if any(points[i][1] == points[i - 1][1] and points[i][0] != points[i - 1][0] for i in range(b + 1, e)): return True
    return int(min_hits_tab[q_sketch]) <= 0


def run_y(oracle, contigs, reads, hg, option, kmerPct=0.001, before=None, brackets=False):
    """one sized -Y pass over the batch on a fresh context, with or without MM_OPT_L1_GROUP_STREAM: (queued, literal) and everything it
    leaves, as bytes and per fragment.  before: a batch the context maps first, which leaves it its buffers.  brackets: the kernel timers
    are on and the batch is mapped once more at the end; `l1_brackets` = the MM_K_L1 timer brackets of its first and of its second pass
    (pass_l1_sweeps closes one per attempt and the grown buffer stays with the context, so the first pass has more exactly when it had to
    launch the sweep again)"""
    from mashmap_amd import capi
    flags = U.FLAG_SKIP_PREFIX | (U.FLAG_HG if hg else 0)
    h = oracle.session(contigs, K, L, S, PI, U.FILTER_MAP, flags, b"#", kmerPct)
    ix = oracle.export_index(h)
    ctx = capi.Context(k=K, segLength=L, sketchSize=S, flags=capi.MM_FLAG_SKIP_PREFIX | (capi.MM_FLAG_HG_FILTER if hg else 0))
    if option: ctx.l1_group_stream(True)
    rg = gpucheck.prefix_groups([n for n, _ in contigs], "#")[1]
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"], rg)
    ctx.set_tables(oracle.min_hits_table(S, K, PI), oracle.cutoffs(h))
    ctx.set_replay_tables(*capi.stat_replay_tables(S, K, PI, 0.0, True))
    for batch in ([before] if before else []) + [reads]:
        ctx.reads_upload([a for _, a in batch], [-1] * len(batch), [-1] * len(batch), 0)
        if brackets and batch is reads: ctx.synchronize(); ctx.profile(True); ctx.profile_read(True)
        ctx.map()
    if brackets: ctx.synchronize(); first = ctx.profile_read(True)["l1"][1]
    queued, literal = ctx.pass_l1_literal()
    stats, l1, l2 = ctx.results()
    per = {}
    for c in l1:
        per.setdefault(int(c["frag"]), []).append((int(c["seqId"]), int(c["rangeStartPos"]), int(c["rangeEndPos"]), int(c["intersectionSize"])))
    out = dict(queued=queued, literal=literal, stats=stats.tobytes().hex(), l1=l1.tobytes().hex(), l2=l2.tobytes().hex(),
               mappings=ctx.mappings().tobytes().hex(), l1_per_frag=[per.get(f, []) for f in range(len(stats))],
               steady=ctx.pass_stats()[1], cause=ctx.pass_redo_cause(), totals=ctx.pass_totals())
    if brackets:
        ctx.map(); ctx.synchronize()
        out["l1_brackets"] = (first, ctx.profile_read(True)["l1"][1])
        assert ctx.results()[1].tobytes().hex() == out["l1"]
    ctx.close(); oracle.free(h)
    return out


def check_both_ways(oracle, cs, reads, hg, per, kmerPct=0.001):
    """the batch with the option and without it: the same bytes, the oracle's candidates, the expected literal count; returns the
    run with the option"""
    rg = gpucheck.prefix_groups([n for n, _ in cs], "#")[1]
    mh = oracle.min_hits_table(S, K, PI)
    with_points = [i for i, (p, q, _) in enumerate(per) if p]
    expected = [i for i in with_points if takes_literal_grouped(per[i][0], per[i][1], mh, rg)]
    on = run_y(oracle, cs, reads, hg, True, kmerPct)
    off = run_y(oracle, cs, reads, hg, False, kmerPct)
    print("with the option: queued %d, literal %d (expected %r); without: queued %d, literal %d"
          % (on["queued"], on["literal"], expected, off["queued"], off["literal"]))
    assert off["literal"] == off["queued"] == on["queued"] == len(with_points)
    assert on["literal"] == len(expected), (on["literal"], expected)
    for what in ("stats", "l1", "l2", "mappings"):
        assert len(on[what]) > 0 and on[what] == off[what], "the grouped wave kernel disagrees with the literal one on " + what
    assert len(on["l1_per_frag"]) == len(per)
    for f, (_, _, l1) in enumerate(per):
        assert on["l1_per_frag"][f] == l1, ("fragment %d" % f, on["l1_per_frag"][f][:4], l1[:4])
    return on, expected


# ----------------------------------------------------------------------------- 1: the group batch of test_gpu_skip_prefix_stream
def oracle_case_groups(oracle, hg):
    cs, reads = T.case_groups(oracle)
    per, cut = T.oracle_points(oracle, cs, reads, U.FLAG_SKIP_PREFIX | (U.FLAG_HG if hg else 0))
    return cs, reads, per, cut


@pytest.mark.gpu
@pytest.mark.parametrize("hg", [True, False], ids=["hg", "nohg"])
def test_group_batch_goes_to_the_wave_kernel(oracle, hg):
    cs, reads, per, _ = oracle_case_groups(oracle, hg)
    on, expected = check_both_ways(oracle, cs, reads, hg, per)
    frag_of_r12 = sum(len(T.fragments_of(a)) for _, a in reads[:12])
    assert reads[12][0] == "r12" and expected == [frag_of_r12]  # the fragment whose points in B#1#x / B#1#y share a position
    assert on["queued"] == 43 and on["literal"] == 1
    assert 0 < on["literal"] < on["queued"]


# ----------------------------------------------------------------------------- 2: a position shared across a group boundary
BOUNDARY_NAMES = ["A#1#x", "A#1#y", "B#1#x", "B#1#y"]


def case_boundary(oracle):
    """a locus in A#1#y (the last contig of its group) and in B#1#x (the first of the next), placed so that the fragment's last point
    in the one and its first in the other share a position: neighbours in the sorted list, but of two extents"""
    src = U.random_dna(91, 3000)
    small = U.random_dna(92, L + 600)
    small_read = ("r0", T.subst(small[300:300 + L], 19, 0.05))

    def build(shift):
        cs = T.genome(13, BOUNDARY_NAMES, 24000)
        for ci, (nm, _) in enumerate(cs): T.plant(cs, nm, 1000 + ci * 4000, T.subst(src, 700 + ci, 0.01))
        T.plant(cs, "A#1#y", 21000, small); T.plant(cs, "B#1#x", 21000 + shift, small)
        return cs
    cs = T.close_boundary(oracle, build, small_read, 1, 2)
    reads = [small_read] + T.reads_from(src, 50, 3, 2 * L + 57, 0.05, first=1)
    return cs, reads


@pytest.mark.gpu
@pytest.mark.parametrize("hg", [True, False], ids=["hg", "nohg"])
def test_position_shared_across_a_group_boundary_is_no_mixed_group(oracle, hg):
    cs, reads = case_boundary(oracle)
    per, cut = T.oracle_points(oracle, cs, reads, U.FLAG_SKIP_PREFIX | (U.FLAG_HG if hg else 0))
    pts = per[0][0]
    last1 = [p for p in pts if p[0] == 1][-1]; first2 = [p for p in pts if p[0] == 2][0]
    print("fragment 0: %d points, last in contig 1 %r, first in contig 2 %r, oracle L1 %r" % (len(pts), last1, first2, per[0][2]))
    assert last1[1] == first2[1]                                 # the ungrouped rule would hand this fragment over ...
    assert T.takes_literal(pts, per[0][1], oracle.min_hits_table(S, K, PI), cut, hg)
    assert len(per[0][2]) >= 2 and {c[0] for c in per[0][2]} == {1, 2}
    on, expected = check_both_ways(oracle, cs, reads, hg, per)
    assert 0 not in expected and on["literal"] == 0              # ... the grouped one does not: the two points belong to two calls


# ----------------------------------------------------------------------------- 3: extents against the 64-point chunks, > MM_STREAM_BUF candidates
def case_repeats(oracle_unused=None):
    """twelve contigs in six groups; an 800 bp unit planted seven times per contig, 2 900 bp apart (more than segLength + unit); the
    copies of group g carry g-dependent substitutions, the last group's so many that only a few seeds survive"""
    names = ["%s#1#%s" % (g, c) for g in "ABCDEF" for c in "xy"]
    unit = U.random_dna(301, 800)
    rates = [0.005, 0.01, 0.02, 0.03, 0.04, 0.16]
    cs = T.genome(17, names, 22000)
    for ci, (nm, _) in enumerate(cs):
        for j in range(7): T.plant(cs, nm, 600 + j * 2900 + ci * 13, T.subst(unit, 900 + ci * 16 + j, rates[ci // 2]))
    reads = [("r0", T.subst(unit[150:150 + L], 5, 0.01)), ("r1", T.subst(unit[20:20 + L + 240], 6, 0.02)),
             ("r2", T.subst(cs[3][1][300:300 + L + 33].copy(), 7, 0.05))]
    return cs, reads


@pytest.mark.gpu
@pytest.mark.parametrize("hg", [True, False], ids=["hg", "nohg"])
def test_extents_off_the_chunk_grid_and_more_candidates_than_the_lds_buffer(oracle, hg):
    cs, reads = case_repeats()
    per, cut = T.oracle_points(oracle, cs, reads, U.FLAG_SKIP_PREFIX | (U.FLAG_HG if hg else 0), kmerPct=0.0)
    rg = gpucheck.prefix_groups([n for n, _ in cs], "#")[1]
    sizes = [[e - b for b, e in extents(p, rg)] for p, _, _ in per]
    print("points per fragment %r, extents %r, oracle nL1 %r" % ([len(p) for p, _, _ in per], sizes, [len(l1) for _, _, l1 in per]))
    assert any(len(l1) > STREAM_BUF for _, _, l1 in per)         # the writing pass, across extents
    assert any(0 < n < 64 for s in sizes for n in s)             # an extent inside one chunk, the next one starting off the grid
    assert any(n > 128 for s in sizes for n in s)                # the chunk carry inside an extent
    assert any(len(s) >= 6 for s in sizes)
    assert all(len(p) <= SORT_LDSCAP for p, _, _ in per)
    check_both_ways(oracle, cs, reads, hg, per, kmerPct=0.0)


@pytest.mark.gpu
def test_candidates_outgrow_the_buffer_inside_the_grouped_wave_kernel(oracle):
    """k_l1_stream_groups' claim running past l1Cap: the context is sized on the three reads above, then maps 120 one-segment reads of the
    unit -- every fragment a candidate per copy it still sees, thousands in all, none from the fused kernels (under -Y every fragment is
    queued) and none from the literal one, against the dense buffer a pass over 120 fragments starts with (tests/mmutil.py: dense_cap):
    the kernel's first launch raises MM_PC_L1_OVERFLOW and the sweep is launched again -- the pass closes more MM_K_L1 timer brackets than a
    second pass of the same batch on the same context, which finds the grown buffer.
    FINDING: there is no MM_REDO_L1 to expect.  mm_launch_map makes no steady attempt under MM_FLAG_SKIP_PREFIX (mm_never_steady), so the batch is
    a sized pass, and a sized pass absorbs the flag itself: pass_l1_sweeps grows the buffer to the cursor's demand, rewinds the cursor
    and launches the kernel again.  Pinned: no attempt, nothing redone, cause 0 -- and the bytes of a fresh context with the option and
    of one without it (the literal kernel)."""
    cs, few = case_repeats()
    unit = U.random_dna(301, 800)
    B = [("r%d" % i, T.subst(unit[x:x + L], 40 + i, 0.01)) for i, x in enumerate(np.linspace(0, len(unit) - L, 120).astype(int))]
    assert all(len(T.fragments_of(a)) == 1 for _, a in B) and len(B) > sum(len(T.fragments_of(a)) for _, a in few)
    behind = run_y(oracle, cs, B, True, True, kmerPct=0.0, before=few, brackets=True)
    fresh = run_y(oracle, cs, B, True, True, kmerPct=0.0)
    off = run_y(oracle, cs, B, True, False, kmerPct=0.0)
    n1 = len(fresh["l1"]) // (2 * 20)                              # (hex digits of 20-byte records)
    print("%d fragments, %d candidates, dense buffer of a pass over them %d; queued %d, literal %d; MM_K_L1 brackets of the first and the second pass %r"
          % (len(B), n1, U.dense_cap(len(B)), behind["queued"], behind["literal"], behind["l1_brackets"]))
    assert behind["queued"] == len(B) and behind["literal"] == 0   # every candidate is the wave kernel's
    assert n1 > U.dense_cap(len(B)), "the candidates fit the buffer the kernel is first launched with"
    assert behind["l1_brackets"][0] > behind["l1_brackets"][1] > 0, "the sweep was not launched again: the buffer did not grow"
    for what in ("stats", "l1", "l2", "mappings"):
        assert len(behind[what]) > 0 and behind[what] == fresh[what] == off[what], what
    assert not behind["steady"] and behind["cause"] == 0 and behind["totals"] == {"passes": 2, "steady": 0, "redone": 0}


# ----------------------------------------------------------------------------- 4: the HG rule, per extent
def case_hg_extents():
    """three groups.  A: the unit nearly exact in one place and, further on, a copy with 9 % substitutions -- the extent's best count
    raises minimumHits above what the weak copy reaches.  B: copies with 15 % substitutions only: some seeds hit, the best count misses
    minimumHits.  C: a 5 % copy: an ordinary extent"""
    names = ["A#1#x", "A#1#y", "B#1#x", "B#1#y", "C#1#x"]
    unit = U.random_dna(401, 900)
    cs = T.genome(23, names, 20000)
    T.plant(cs, "A#1#x", 2000, T.subst(unit, 1, 0.002)); T.plant(cs, "A#1#y", 9000, T.subst(unit, 2, 0.09))
    T.plant(cs, "A#1#x", 12000, T.subst(unit, 3, 0.09))
    T.plant(cs, "B#1#x", 3000, T.subst(unit, 4, 0.15)); T.plant(cs, "B#1#y", 7000, T.subst(unit, 5, 0.15))
    T.plant(cs, "C#1#x", 5000, T.subst(unit, 6, 0.05))
    reads = [("r0", T.subst(unit[200:200 + L], 8, 0.003)), ("r1", T.subst(unit[0:L + 300], 9, 0.01))]
    return cs, reads


@pytest.mark.gpu
def test_hg_rule_per_extent(oracle):
    cs, reads = case_hg_extents()
    per, cut = T.oracle_points(oracle, cs, reads, U.FLAG_SKIP_PREFIX | U.FLAG_HG, kmerPct=0.0)
    per_nohg, _ = T.oracle_points(oracle, cs, reads, U.FLAG_SKIP_PREFIX, kmerPct=0.0)
    rg = gpucheck.prefix_groups([n for n, _ in cs], "#")[1]
    mh = oracle.min_hits_table(S, K, PI)
    missed = raised = dropped = False
    for (p, q, l1), (_, _, l1_nohg) in zip(per, per_nohg):
        base = int(mh[q]); figures = []
        for b, e in extents(p, rg):
            best = best_count(p[b:e]); r = raised_min_hits(best, q, base, cut)
            g = rg[p[b][0]]
            n_here = sum(1 for c in l1 if rg[c[0]] == g); n_nohg = sum(1 for c in l1_nohg if rg[c[0]] == g)
            figures.append((g, e - b, best, base, r, n_here, n_nohg))
            if r is None and best > 0 and len(l1) > 0: assert n_here == 0; missed = True      # this extent yields nothing, another one does
            if r is not None and r != base: raised = True
            if r is not None and r != base and n_here < n_nohg: dropped = True                 # a position that passes the base minimumHits only
        print("sketch %d: (group, points, best, minHits, raised, nL1 hg, nL1 no hg) %r" % (q, figures))
    assert missed and raised and dropped
    check_both_ways(oracle, cs, reads, True, per, kmerPct=0.0)


# ----------------------------------------------------------------------------- 5: MM_L1_LITERAL still forces the literal kernel
@pytest.mark.gpu
@pytest.mark.parametrize("hg", [True, False], ids=["hg", "nohg"])
def test_forced_literal_run_with_the_option_set(oracle, hg):
    cs, reads, per, _ = oracle_case_groups(oracle, hg)
    here = run_y(oracle, cs, reads, hg, True)
    assert here["queued"] == 43 and here["literal"] == 1
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "1" if hg else "0"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MM_L1_LITERAL="1"))
    assert p.returncode == 0, p.stderr[-3000:]
    there = json.loads(p.stdout.strip().splitlines()[-1])
    assert there["literal"] == there["queued"] == here["queued"]
    for what in ("stats", "l1", "l2", "mappings"):
        assert len(here[what]) > 0 and there[what] == here[what], "the forced literal run disagrees on " + what


# ----------------------------------------------------------------------------- 6: the command line
@pytest.mark.gpu
def test_command_line_sets_the_option(tmp_path):
    """mashmap_hip -Y '#', all against all, 8 contigs of 25 kbp in four groups (haplotypes of one genome, 1 % apart): the PAF is the
    forced literal run's, and MM_DEBUG shows the literal kernel taking fewer fragments than were queued"""
    assert os.path.exists(HIP_BIN), "mashmap_hip not built"
    base = [U.random_dna(500 + j, 25000) for j in range(2)]
    recs = [("h%d#1#c%d" % (hpl, j), T.subst(base[j], 600 + hpl * 2 + j, 0.01)) for hpl in range(4) for j in range(2)]
    fa = str(tmp_path / "groups.fa")
    U.write_fasta(fa, recs)
    out = {}
    for name, extra in (("stream", {}), ("literal", {"MM_L1_LITERAL": "1"})):
        paf = str(tmp_path / (name + ".paf"))
        p = subprocess.run([HIP_BIN, "-r", fa, "-q", fa, "-Y", "#", "-s", "1000", "--pi", "90", "-n", "3", "-t", "4", "-o", paf],
                           capture_output=True, text=True, timeout=240, env=dict(os.environ, MM_DEBUG="1", **extra))
        assert p.returncode == 0, p.stderr[-3000:]
        took = [(int(a), int(b)) for a, b in re.findall(r"of (\d+) queued fragments the literal L1 kernel took (\d+)", p.stderr)]
        out[name] = (open(paf, "rb").read(), took)
        print("%s: %d PAF lines, (queued, literal) per pass %r" % (name, out[name][0].count(b"\n"), took))
    assert out["stream"][0].count(b"\n") > 0 and out["stream"][0] == out["literal"][0]
    took = out["stream"][1]
    assert took and sum(b for _, b in took) < sum(a for a, _ in took)
    assert not out["literal"][1]                                 # the forced run never starts the wave kernel: no such line


# ----------------------------------------------------------------------------- 7: CPU
def test_the_option_is_declared_and_bound():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert re.search(r"enum \{[^}]*MM_OPT_L1_GROUP_STREAM = 4[^}]*\};", hdr)
    assert "#define MM_ABI_VERSION 2" in hdr or re.search(r"MM_ABI_VERSION\s*=?\s*2\b", hdr)
    assert capi.MM_OPT_L1_GROUP_STREAM == 4
    assert callable(getattr(capi.Context, "l1_group_stream"))
    assert capi.load().mm_abi_version() == 2                     # additive: the ABI version stays


if __name__ == "__main__":                                       # the child of test 5: case 1 with the option set, hg = argv[1]
    sys.path.insert(0, ROOT)
    orc_ = U.Oracle()
    cs_, reads_ = T.case_groups(orc_)
    r_ = run_y(orc_, cs_, reads_, sys.argv[1] == "1", True)
    del r_["l1_per_frag"]
    print(json.dumps(r_))
