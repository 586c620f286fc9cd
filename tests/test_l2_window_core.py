"""mashmap_amd/csrc/mm_l2_window_core.h -- computeL2MappedRegions with windowLen != 0 (computeMap.hpp:1276-1451) as k_l2_window_wave runs it:
SlideMapper on located records, the presence rule in place of hash_to_freq, the evictions of skipped records made by the next entering one,
the evaluation with its "- windowLen" offsets, the join of loci -- on the CPU: tests/hostlogic/l2_window_check.cpp, a stand-alone program
built with -fsanitize=address,undefined, runs the header's serial driver over the oracle's index records, query sketch and L1 candidates
(written to a file here) and every candidate's loci must equal the oracle's byte for byte.  Runs without a GPU.

k 16, segLength 1000, s 80, pi 0.85, --noSplit, kmerThreshold 0.  The tandem cases (tests/winmodel.py: TANDEM), what the oracle and the
Python model of the reference's counter + heap yield on them without the HG filter (one candidate each; `walked` leaves out the records
before rangeStart that are closed by then, which the set-up loop passes over).  The floors asserted below are half of what the reference
alone was measured at when the cases were chosen (2 927 / 1 020 skipped / re-entered for seed 1, 943 / 610 for seed 3, a heap of 1 478 for seed 4):

    seed  period x copies, err   read     W       walked  entering  skipped  re-entered  largest heap
    1     1800 x 14, 0           3 000    2 000   4 379   1 524     2 855    1 020       263
    2     700 x 30, 0.01         2 500    1 500   2 843   1 325     1 518    558         228
    3     300 x 60, 0.02         1 400    400     2 437   1 565     872      610         122
    4     1800 x 6, 0.03         21 000   20 000  4 131   2 006     2 125    0           1 478
    5     150 x 100, 0           5 000    4 000   2 177   929       1 248    181         506
"""
import os
import subprocess

import numpy as np
import pytest

import mmutil as U
import winmodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOORS = {1: dict(skipped=1460, reentered=510), 3: dict(skipped=470, reentered=305), 4: dict(largest_heap=739)}
BIG = 1 << 16                                                   # a heap and locus slots no case outgrows


@pytest.fixture(scope="module")
def l2_window_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("l2_window_check") / "l2_window_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "l2_window_check.cpp")])
    return exe


def run_program(exe, idx, reads, tmp_path, heap_cap=BIG, locap=64):
    """reads: dicts(sketch = the oracle's [(hash, .., strand)], W, l1 = [(seqId, rangeStart, rangeEnd, ..)]); per read and candidate
    (done, overflow, counts, loci as the oracle's (seqId, mean, start, end, shared, strand) tuples)"""
    rec = np.stack([idx["hash"].astype(np.int64), idx["wpos"].astype(np.int64), idx["wpos_end"].astype(np.int64), idx["seqId"].astype(np.int64),
                    idx["strand"].astype(np.int64)], axis=1).reshape(-1)
    words = [np.array([len(reads)], dtype=np.int64)]
    for r in reads:
        sk = r["sketch"]
        assert [x[0] for x in sk] == sorted(x[0] for x in sk)
        words.append(np.array([len(sk), M.L, r["W"], heap_cap, locap, len(idx), len(r["l1"])], dtype=np.int64))
        words.append(np.array([x[0] for x in sk], dtype=np.uint64).view(np.int64)); words.append(np.array([x[4] for x in sk], dtype=np.int64))
        words.append(rec)
        words.append(np.array([c[:3] for c in r["l1"]], dtype=np.int64).reshape(-1))
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    np.concatenate(words).tofile(fin)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert p.returncode == 0, "l2_window_check (sanitized) failed with status %d:\n%s" % (p.returncode, p.stderr[-4000:])
    out = np.fromfile(fout, dtype="<i4")
    got, at = [], 0
    for r in reads:
        per = []
        for c in r["l1"]:
            done, over, counts, n = int(out[at]), int(out[at + 1]), [int(x) for x in out[at + 2:at + 7]], int(out[at + 7])
            loci = [tuple(int(x) for x in out[at + 8 + 4 * i:at + 12 + 4 * i]) for i in range(n)]
            at += 8 + 4 * n
            per.append((done, over, counts, [(c[0], (a + b) // 2 if a + b >= 0 else -((-(a + b)) // 2), a, b, sh, st) for a, b, sh, st in loci]))
        got.append(per)
    assert at == len(out)
    return got


def oracle_reads(orc, h, reads):
    out = []
    for a in reads:
        e, per = M.oracle_read(orc, h, a)
        assert e["sketchSize"] == len(e["sketch"])
        out.append(dict(sketch=e["sketch"], W=max(0, len(a) - M.L), l1=e["l1"], l2=per))
    return out


def check(orc, exe, contigs, reads, hg, tmp_path):
    """every candidate of every read: the program's loci are the oracle's, its counts are the model's, and the model's two gates agree
    (winmodel.figures asserts that); returns the figures per read and candidate"""
    h = M.session(orc, contigs, hg)
    idx = orc.index_array(h)
    rs = oracle_reads(orc, h, reads)
    orc.free(h)
    got = run_program(exe, idx, rs, tmp_path)
    figs, n_loci = [], 0
    for ri, (r, per) in enumerate(zip(rs, got)):
        figs.append([])
        for ci, (cand, (done, over, counts, loci)) in enumerate(zip(r["l1"], per)):
            fig = M.figures(idx, cand, r["W"])
            figs[-1].append(fig)
            assert done == 1 and over == 0
            assert counts == [fig["walked"], fig["entering"], fig["skipped"], fig["reentered"], fig["largest_heap"]], (ri, ci, counts, fig)
            assert loci == r["l2"][ci], ("read %d candidate %d %r, W %d" % (ri, ci, cand, r["W"]), loci[:3], r["l2"][ci][:3])
            n_loci += len(loci)
    return rs, figs, n_loci


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "revcomp"])
@pytest.mark.parametrize("hg", [False, True], ids=["nohg", "hg"])
def test_tandem_cases_equal_the_oracle(oracle, l2_window_check, tmp_path, hg, rc):
    total = 0
    for seed in sorted(M.TANDEM):
        c = M.tandem_contig(seed)
        read = M.tandem_read(seed, c)
        rs, figs, n = check(oracle, l2_window_check, [("c", c)], [U.revcomp(read) if rc else read], hg, tmp_path)
        total += n
        best = {k: max(f[k] for f in figs[0]) for k in ("walked", "entering", "skipped", "reentered", "largest_heap")} if figs[0] else {}
        print("seed %d, %s, %s: %d candidates, %d loci, the largest figures over them %r" % (seed, "hg" if hg else "nohg", "rc" if rc else "fwd", len(figs[0]), n, best))
        assert len(figs[0]) >= 1 and n >= 1
        for key, floor in (FLOORS.get(seed, {}) if not hg else {}).items():   # (the HG filter narrows the candidates: the table is without it)
            assert best[key] >= floor, (seed, key, best[key], floor)
        if rc:
            assert all(x[5] == -1 for per in rs[0]["l2"] for x in per)           # negative votes all the way
    assert total >= 5


@pytest.mark.parametrize("piece", [410, 700, 950])
@pytest.mark.parametrize("hg", [False, True], ids=["nohg", "hg"])
def test_mixed_strand_reads_pin_when_the_votes_are_sampled(oracle, l2_window_check, tmp_path, hg, piece):
    """seed 1's read with every second piece reverse-complemented: loci of both strands.  The strand of a closing run comes from the votes
    behind the evictions of the skipped slide records before the entering one and before its own (mm_win_enter): with either order
    changed a strand flips on these reads"""
    c = M.tandem_contig(1)
    rs, figs, n = check(oracle, l2_window_check, [("c", c)], [M.mixed_strand_read(1, c, piece)], hg, tmp_path)
    strands = [x[5] for per in rs[0]["l2"] for x in per]
    print("piece %d, %s: loci per candidate %r, strands %r, entering records behind a skipped slide record %r"
          % (piece, "hg" if hg else "nohg", [len(per) for per in rs[0]["l2"]], strands, [f["behind_skipped"] for f in figs[0]]))
    assert set(strands) == {1, -1}
    assert any(f["behind_skipped"] > 0 for f in figs[0])


def test_a_read_shorter_than_a_segment_and_random_reads(oracle, l2_window_check, tmp_path):
    """windowLen == 0 through the same driver (the gate off), and reads sampled from random contigs with errors, both strands"""
    cs = [U.random_dna(700 + i, n) for i, n in enumerate((60000, 40000, 30000))]
    reads = [a for _, a, _ in U.sample_reads(cs, 13, 12, 2469, 0.08)] + [a for _, a, _ in U.sample_reads(cs, 14, 4, 6200, 0.05)]
    reads += [cs[1][1000:1600].copy(), cs[0][38000:41000].copy(), cs[1][7000:8001].copy(), U.mutate(cs[2][2000:29000], 5, 0.03)]
    for hg in (True, False):
        rs, figs, n = check(oracle, l2_window_check, [("chr%d" % i, c) for i, c in enumerate(cs)], reads, hg, tmp_path)
        assert n >= len(reads) - 2
        short = rs[16]
        assert short["W"] == 0 and len(short["l1"]) >= 1 and all(f["skipped"] == 0 for f in figs[16])
        assert any(x[5] == -1 for r in rs for per in r["l2"] for x in per) and any(x[5] == 1 for r in rs for per in r["l2"] for x in per)


def test_the_capacities_are_checked_before_the_write(oracle, l2_window_check, tmp_path):
    """the heap at the model's largest size holds the candidate, one entry less does not -- and the program, whose heap has exactly that
    size under the sanitizer, says so instead of writing; likewise locus slots: unit[100:1500] of a unit planted 14 times has 14 tied loci"""
    c = M.tandem_contig(4)
    h = M.session(oracle, [("c", c)], False)
    idx = oracle.index_array(h)
    rs = oracle_reads(oracle, h, [M.tandem_read(4, c)])
    oracle.free(h)
    fig = M.figures(idx, rs[0]["l1"][0], rs[0]["W"])
    assert run_program(l2_window_check, idx, rs, tmp_path, heap_cap=fig["largest_heap"])[0][0][0] == 1
    assert run_program(l2_window_check, idx, rs, tmp_path, heap_cap=fig["largest_heap"] - 1)[0][0][0] == 0
    c1 = M.planted_contig(4101, 4100, 1800, 14, 0.0)
    h = M.session(oracle, [("c", c1)], False)
    idx = oracle.index_array(h)
    rs = oracle_reads(oracle, h, [U.random_dna(4100, 1800)[100:1500]])
    oracle.free(h)
    assert [len(x) for x in rs[0]["l2"]] == [14]
    (done, over, _, loci), = run_program(l2_window_check, idx, rs, tmp_path, locap=13)[0]
    assert (done, over) == (1, 0) and loci == rs[0]["l2"][0]
    (done, over, _, loci), = run_program(l2_window_check, idx, rs, tmp_path, locap=12)[0]
    assert (done, over) == (1, 1)
    assert M.takes_literal(M.figures(idx, rs[0]["l1"][0], rs[0]["W"]), 14)
