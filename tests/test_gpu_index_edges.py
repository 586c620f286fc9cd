"""The device index build (mm_index_build: k_ref_hash<K>, the candidate compaction, k_winnow_tiles, the host stitch and tail,
mm_finalize_index_device) against the CPU oracle where tests/test_gpu_index.py does not reach: every k-mer size from 1 to 64 on contigs
a few windows long (the reference kernel's own N handling and the host patch for the reference's unnoticed leading N at every size; at
k <= 3 no sparse tile can fill its sketch and every one is spliced from the dense re-run), the edges of the frequency threshold
(k_freq_threshold: exact hit, tie, more seeds to ignore than there are), and the mapping stages on top of such indexes."""
import numpy as np
import pytest

import gpucheck
import mmutil as U
from gpucheck import compare_index

pytestmark = pytest.mark.gpu

QUALIFYING = {0, 1, 3, 4, 5}          # the contigs of U.index_edge_contigs that are at least a window long


def edge_case(oracle, k, s):
    """one (k, sketch size) build over U.index_edge_contigs(k), compared record for record; returns the number of k_winnow_tiles
    launches.  Two conditions on the oracle's side keep the case from passing empty."""
    out = {}
    n, _ = compare_index(oracle, U.index_edge_contigs(k), k=k, L=U.index_edge_window(k), s=s, out=out)
    ids = set(out["oracle"]["minmers"]["seqId"].tolist())
    launches = out["profile"]["winnow"][1]
    print("k %d s %d: %d records, seqIds %r, %d k_winnow_tiles launches" % (k, s, n, sorted(ids), launches))
    assert ids == QUALIFYING and n >= 100
    return launches


@pytest.mark.parametrize("k", range(1, 65))
def test_index_at_every_kmer_size(oracle, k):
    """k_winnow_tiles is launched once per contig of at least a window (5 of the 7) and once more for a contig with a tile that failed.
    At sketch size 12 the launch is sparse, and the tandem repeat (at most 7 distinct k-mers in any window) cannot fill a sketch from
    its candidates: its tiles are re-run dense and spliced.  At the second size the launch is dense from the start."""
    sparse, dense = U.index_edge_sketch_sizes(k)
    assert edge_case(oracle, k, sparse) > len(QUALIFYING)
    assert edge_case(oracle, k, dense) >= len(QUALIFYING)


@pytest.mark.parametrize("k", [1, 3, 9, 31, 33, 64])
def test_index_at_kmer_size_edges_with_the_blocked_window_sketch(oracle, monkeypatch, k):
    """the same contigs through k_winnow_tiles<.., GSK> (the window's sketch as blocks in HBM, tiles of w / 16 windows)"""
    monkeypatch.setenv("MM_WINNOW_GSK", "1")
    sparse, dense = U.index_edge_sketch_sizes(k)
    assert edge_case(oracle, k, sparse) > len(QUALIFYING)
    assert edge_case(oracle, k, dense) >= len(QUALIFYING)


# ---- the frequency threshold (computeFreqHist, winSketch.hpp:410-453) -------------------------------------------------------------------
FREQ = dict(k=19, L=1000, s=50)


@pytest.fixture(scope="module")
def freq_hist(oracle):
    """(contigs, nk, [(point count, number of seeds with at least that many)] from the largest count down, seeds per count)"""
    contigs = U.freq_edge_contigs()
    h = oracle.session(contigs, FREQ["k"], FREQ["L"], FREQ["s"], 0.85, U.FILTER_MAP, U.FLAG_HG, b"\0", 0.0)
    e = oracle.export_index(h)
    oracle.free(h)
    counts = np.diff(e["offsets"].astype(np.int64))
    values, group = np.unique(counts, return_counts=True)
    values, group = values[::-1], group[::-1]
    return contigs, len(counts), list(zip(values.tolist(), np.cumsum(group).tolist())), group.tolist()


def to_ignore(nk, pct):
    """minmerToIgnore as winSketch.hpp:425 computes it: int64 * float / int, in float"""
    return int(np.int64(np.float32(nk) * np.float32(pct) / np.float32(100)))


# kmerPct -> (frequent seeds, threshold) of the oracle; beyond 100 there are more seeds to ignore than there are seeds: every step of the
# reference's walk stays below, the threshold ends at the smallest count and every seed is frequent
FIXED = {-1.0: (0, 0x7fffffff), 0.0: (0, 0x7fffffff), 0.001: (0, 0x7fffffff), 0.5: (8, 88), 5.0: (67, 24), 50.0: (503, 4), 100.0: (1717, 2),
         150.0: (1717, 2)}


@pytest.mark.parametrize("pct", sorted(FIXED))
def test_frequency_threshold_sweep(oracle, freq_hist, pct):
    contigs, nk, _, _ = freq_hist
    out = {}
    _, nf = compare_index(oracle, contigs, kmerPct=pct, out=out, **FREQ)
    print("kmerPct %g: %d keys, threshold %d, %d frequent seeds" % (pct, nk, out["freqThreshold"], nf))
    assert nk == 1717 and (nf, out["freqThreshold"]) == FIXED[pct]


def boundary(freq_hist):
    """the third boundary between two point counts, from the top, whose next group has at least two seeds: (T = seeds at or above the
    boundary, the count there)"""
    _, _, cum, group = freq_hist
    at = [i for i in range(len(cum) - 1) if group[i + 1] >= 2][2]
    return cum[at][1], cum[at][0]


def test_frequency_threshold_exact_hit(oracle, freq_hist):
    """minmerToIgnore equals the number of seeds at or above a count: that count is the threshold (`sum == toIgnore`, :433)"""
    contigs, nk, _, _ = freq_hist
    T, v = boundary(freq_hist)
    pct = 100 * (T + 0.5) / nk
    assert to_ignore(nk, pct) == T
    out = {}
    _, nf = compare_index(oracle, contigs, kmerPct=pct, out=out, **FREQ)
    print("exact hit: T %d, threshold %d, %d frequent seeds" % (T, out["freqThreshold"], nf))
    assert nf == T and out["freqThreshold"] == v


def test_frequency_threshold_inside_a_tie(oracle, freq_hist):
    """minmerToIgnore one beyond a boundary, inside the next group of equal counts: the group does not fit, the threshold stays at the
    count above it (k_freq_threshold's tie branch)"""
    contigs, nk, _, _ = freq_hist
    T, v = boundary(freq_hist)
    pct = 100 * (T + 1.5) / nk
    assert to_ignore(nk, pct) == T + 1
    out = {}
    _, nf = compare_index(oracle, contigs, kmerPct=pct, out=out, **FREQ)
    print("tie: T + 1 = %d, threshold %d, %d frequent seeds" % (T + 1, out["freqThreshold"], nf))
    assert nf == T and out["freqThreshold"] == v


# ---- mapping on top ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome_and_reads():
    g = U.random_dna(1, 120000)
    return [("chr0", g)], [("read%d" % i, a) for i, (_, a, _) in enumerate(U.sample_reads([g], 2, 8, 10000, 0.1))]


def n_fragments(reads, L):
    """Map::mapModule: full segments and, where bases are left over, one more that ends with the read"""
    return sum(len(a) // L + (1 if len(a) % L else 0) for _, a in reads if len(a) >= L)


@pytest.mark.parametrize("pct", [100.0, 150.0])
def test_map_with_every_seed_frequent(oracle, genome_and_reads, pct):
    """every seed of the index is frequent: minmerIndex is empty (no event, no open record), every query seed that is in the index is
    removed from its sketch, no fragment has an interval point, L1 finds nothing"""
    contigs, reads = genome_and_reads
    nF, nloci = gpucheck.run_and_compare(oracle, contigs, reads, kmerPct=pct, device_index=True, verbose=True)
    assert nF == n_fragments(reads, 5000) and nloci == 0


@pytest.mark.parametrize("k", [11, 28])
def test_map_on_a_device_built_index_at_other_kmer_sizes(oracle, genome_and_reads, k):
    contigs, reads = genome_and_reads
    nF, nloci = gpucheck.run_and_compare(oracle, contigs, reads, k=k, L=1000, s=50, device_index=True, verbose=True)
    assert nF == n_fragments(reads, 1000) and nloci > 0
