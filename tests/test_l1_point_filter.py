"""The interval-point pre-filter of the HBM point path (tests/l1filter.py states the rule; mm_map.hip k_filter_points is the device form) must
leave computeL1CandidateRegions' output (computeMap.hpp:916-1116) exactly as it is: checked here on the CPU against the oracle's literal L1
over fuzzed point sets -- clusters that reach minimumHits, scattered noise, long merged intervals, contigs whose last and first points share a
position (the reference groups by `pos` alone), with and without the HG filter.  Runs without a GPU."""
import numpy as np
import pytest

import l1filter
import mmutil as U
from l1points import KINDS, l1 as _l1, scenario as _scenario

@pytest.mark.parametrize("flags", [U.FLAG_HG, 0])
def test_filtered_points_give_the_same_l1_candidates(oracle, flags):
    h = oracle.session([("c", U.random_dna(5, 30000))], 19, 5000, 60, 0.85, U.FILTER_MAP, flags)
    rng = np.random.default_rng(20260927 + flags)
    dropped = kept = with_candidates = 0
    for it in range(1500):
        kind = KINDS[it % 5]
        seq, o, c = _scenario(rng, kind)
        if len(seq) == 0:
            continue
        qs = int(rng.integers(10, 61))
        min_hits = int(rng.integers(1, 7))
        want, n = _l1(oracle, h, seq, o, c, qs, min_hits)
        with_candidates += n > 0
        for slots in (None, 64, 2048):
            m = l1filter.keep_mask(seq, o, c, min_hits, slots)
            got, _ = _l1(oracle, h, seq[m], o[m], c[m], qs, min_hits)
            assert got == want, (it, kind, min_hits, slots, int(m.sum()), len(m))
        m = l1filter.keep_mask(seq, o, c, min_hits, None)
        dropped += int((~m).sum()); kept += int(m.sum())
    oracle.free(h)
    assert with_candidates > 300 and dropped > 20000 and kept > 20000, (with_candidates, dropped, kept)


def test_the_bin_rule_alone_is_not_enough_at_a_contig_seam(oracle):
    """what the boundary rule is for (and that this test file can fail): without it the seam2 scenarios change their candidates"""
    h = oracle.session([("c", U.random_dna(5, 30000))], 19, 5000, 60, 0.85, U.FILTER_MAP, U.FLAG_HG)
    rng = np.random.default_rng(7)
    differ = 0
    for _ in range(200):
        seq, o, c = _scenario(rng, "seam2")
        min_hits = int(rng.integers(2, 6))
        want, _ = _l1(oracle, h, seq, o, c, 60, min_hits)
        m = l1filter.keep_mask(seq, o, c, min_hits, None)
        assert _l1(oracle, h, seq[m], o[m], c[m], 60, min_hits)[0] == want
        cnt = {}
        for i in range(len(seq)):
            for b in range(int(o[i]) >> l1filter.BIN_SHIFT, ((int(c[i]) - 1) >> l1filter.BIN_SHIFT) + 1):
                cnt[(int(seq[i]), b)] = cnt.get((int(seq[i]), b), 0) + 1
        pure = np.array([any(cnt[(int(seq[i]), b)] >= min_hits for b in range(int(o[i]) >> l1filter.BIN_SHIFT, ((int(c[i]) - 1) >> l1filter.BIN_SHIFT) + 1)) for i in range(len(seq))])
        differ += _l1(oracle, h, seq[pure], o[pure], c[pure], 60, min_hits)[0] != want
    oracle.free(h)
    assert differ > 20, differ
