"""mashmap_amd/csrc/mm_l1_core.h -- the literal computeL1CandidateRegions (computeMap.hpp:916-1116) that k_l1_sweep and k_l1_window run one
thread per fragment, and that every faster L1 path is compared against -- on the CPU: tests/hostlogic/l1_check.cpp, a stand-alone program
built with -fsanitize=address,undefined, runs it over fuzzed point lists (tests/l1points.py) and every case's candidates must equal the
oracle's byte for byte.  Both forms (WINDOWED false: windowLen == 0; true: windowLen in {1, 400, 5000, 40000} with seeds whose windows overlap,
and windowLen == 0 again), with and without the HG filter, with and without -Y reference groups.  Runs without a GPU.

What the oracle alone yields on the seeds below, per mode (1500 cases each): cases with a candidate / with three or more / whose list has a
position group spanning two contigs (of one reference group); the test asserts at least half of each.

    form            windowLen  HG   -Y      >=1    >=3   spanning
    split+windowed  0          on   no     1399    566    300      (>=1: the floor is 300, as test_l1_point_filter.py asserts for this generator)
    split+windowed  0          on   yes    1406    707    186
    split+windowed  0          off  no     1395    761    300      (>=1: 300, likewise)
    split+windowed  0          off  yes    1408    798    193
    windowed        != 0       on   no     1442    549    300
    windowed        != 0       on   yes    1426    610    180
    windowed        != 0       off  no     1432    743    300
    windowed        != 0       off  yes    1430    758    191
"""
import os
import subprocess

import numpy as np
import pytest

import mmutil as U
from l1points import KINDS, L1_DT, l1_of_points, points, scenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG, SKETCH, CAP = 5000, 60, 4096
# (windowLen != 0, hg, groups) -> floors: half of the docstring's figures
FLOORS = {(0, 1, 0): (300, 283, 150), (0, 1, 1): (703, 353, 93), (0, 0, 0): (300, 380, 150), (0, 0, 1): (704, 399, 96),
          (1, 1, 0): (721, 274, 150), (1, 1, 1): (713, 305, 90), (1, 0, 0): (716, 371, 150), (1, 0, 1): (715, 379, 95)}


@pytest.fixture(scope="module")
def l1_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("l1_check") / "l1_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "l1_check.cpp")])
    return exe


def run_program(exe, windowed, cases, cutoffs, tmp_path):
    """cases: dicts(pts, ids, W, nFreq, qs, min_hits, hg, groups); returns each case's candidates as the oracle's bytes"""
    words = [np.array([len(cases), CAP, SKETCH, len(cutoffs)] + list(cutoffs), dtype=np.int64)]
    for cs in cases:
        pts, grp = cs["pts"], cs["groups"]
        words.append(np.array([len(pts), cs["W"], cs["nFreq"], cs["qs"], cs["min_hits"], SEG, cs["hg"], grp is not None, 5] +
                              (list(grp) if grp is not None else [0] * 5), dtype=np.int64))
        words.append((pts["seqId"].astype(np.int64) << 33) | (pts["pos"].astype(np.int64) << 1) | (pts["side"] == 1))
        words.append(cs["ids"].astype(np.int64))
    fin, fout = str(tmp_path / ("cases%d.bin" % windowed)), str(tmp_path / ("out%d.bin" % windowed))
    np.concatenate(words).tofile(fin)
    p = subprocess.run([exe, str(windowed), fin, fout], capture_output=True, text=True)
    assert p.returncode == 0, "l1_check (sanitized) failed with status %d:\n%s" % (p.returncode, p.stderr[-4000:])
    out = np.fromfile(fout, dtype="<i4")
    got, at = [], 0
    for _ in cases:
        n = int(out[at]); assert n >= 0, "more than %d candidates" % CAP
        got.append(out[at + 1:at + 1 + 4 * n].tobytes()); at += 1 + 4 * n
    assert at == len(out)
    return got


def oracle_l1(orc, h, cs):
    """what doL1Mapping does (l1_mapping in oracle.cpp): one computeL1CandidateRegions call per reference-group slice of the list"""
    pts, grp = cs["pts"], cs["groups"]
    if grp is None:
        return l1_of_points(orc, h, pts, cs["qs"], cs["min_hits"], SEG + cs["W"])
    g = np.asarray(grp)[pts["seqId"]]
    cut = [0] + [i for i in range(1, len(pts)) if g[i] != g[i - 1]] + [len(pts)]
    parts = [l1_of_points(orc, h, np.ascontiguousarray(pts[a:b]), cs["qs"], cs["min_hits"], SEG + cs["W"]) for a, b in zip(cut[:-1], cut[1:])]
    return b"".join(x for x, _ in parts), sum(n for _, n in parts)


def make_cases(orc, h, seed, n, windows, hg, with_groups, kinds=KINDS):
    """n cases with the oracle's answer (`want`, `n_want`) and whether a position group of the list spans two contigs (`spans`)"""
    rng = np.random.default_rng(seed)
    cases = []
    while len(cases) < n:
        seq, o, c = scenario(rng, kinds[len(cases) % len(kinds)])
        if len(seq) == 0:
            continue
        W = int(rng.choice(windows))
        # every interval has a seed; about a third share theirs with another interval (overlapping windows of one hash); ids number the seeds
        hashes = np.arange(len(seq))
        share = rng.random(len(seq)) < 1 / 3
        hashes[share] = rng.integers(0, len(seq), int(share.sum()))
        uniq, ids = np.unique(hashes, return_inverse=True)
        # -Y: contigs 0..4 in 2-3 reference groups, numbered in contig order as Map::refIdGroup is
        groups = None
        if with_groups:
            cuts = sorted(rng.choice(np.arange(1, 5), int(rng.integers(1, 3)), replace=False).tolist())
            groups = [sum(q >= x for x in cuts) for q in range(5)]
        pts = points(seq, o, c, ids)
        cs = dict(pts=pts, ids=pts["hash"].astype(np.int64), W=W, nFreq=len(uniq), qs=int(rng.integers(10, 61)), min_hits=int(rng.integers(0, 7)),
                  hg=int(hg), groups=groups)
        same_group = np.ones(len(pts) - 1, dtype=bool) if groups is None else np.asarray(groups)[pts["seqId"][1:]] == np.asarray(groups)[pts["seqId"][:-1]]
        cs["spans"] = bool(np.any((pts["seqId"][1:] != pts["seqId"][:-1]) & (pts["pos"][1:] == pts["pos"][:-1]) & same_group))
        cs["want"], cs["n_want"] = oracle_l1(orc, h, cs)
        cases.append(cs)
    return cases


def check_floors(cases, floors, what):
    have = (sum(cs["n_want"] >= 1 for cs in cases), sum(cs["n_want"] >= 3 for cs in cases), sum(cs["spans"] for cs in cases))
    print("oracle,", what, ": cases with a candidate / with three or more / with a position group across contigs:", have)
    assert all(x >= f for x, f in zip(have, floors)), (what, have, floors)


_SPLIT = {}                                            # (hg, groups) -> the windowLen == 0 cases, made once for both forms


@pytest.mark.parametrize("with_groups", [0, 1])
@pytest.mark.parametrize("hg", [1, 0])
@pytest.mark.parametrize("windowed", [0, 1])
def test_literal_l1_core_equals_the_oracle(oracle, l1_check, tmp_path, windowed, hg, with_groups):
    h = oracle.session([("c", U.random_dna(5, 30000))], 19, SEG, SKETCH, 0.85, U.FILTER_MAP, U.FLAG_HG if hg else 0)
    cutoffs = oracle.cutoffs(h)
    seed = 20261018 + 2 * hg + with_groups
    if (hg, with_groups) not in _SPLIT:                                                # windowLen == 0: both forms take these
        _SPLIT[(hg, with_groups)] = make_cases(oracle, h, seed, 1500, [0], hg, with_groups)
    split = _SPLIT[(hg, with_groups)]
    check_floors(split, FLOORS[(0, hg, with_groups)], "windowLen == 0")
    got = run_program(l1_check, 0, split, cutoffs, tmp_path)
    if windowed:
        assert run_program(l1_check, 1, split, cutoffs, tmp_path) == got, "WINDOWED with windowLen == 0 differs from the split form"
        cases = make_cases(oracle, h, seed + 100, 1500, [1, 400, 5000, 40000], hg, with_groups)
        check_floors(cases, FLOORS[(1, hg, with_groups)], "windowLen != 0")
        got = run_program(l1_check, 1, cases, cutoffs, tmp_path)
    else:
        cases = split
    oracle.free(h)
    for i, (cs, g) in enumerate(zip(cases, got)):
        assert g == cs["want"], (i, KINDS[i % 5], cs["W"], cs["min_hits"], cs["qs"], cs["groups"], np.frombuffer(g, dtype=L1_DT)[:4],
                                 np.frombuffer(cs["want"], dtype=L1_DT)[:4])


def l1_grouped_by_seq_and_pos(pts, qs, min_hits, cutoffs):
    """the sweep with ONE thing changed: a position group is a run of equal (seqId, pos), not of equal pos (windowLen == 0, HG on)"""
    K = [(int(s) << 32) | int(p) for s, p in zip(pts["seqId"], pts["pos"])]
    opens = [int(s) == 1 for s in pts["side"]]
    groups, overlap, trail, lead = [], 0, 0, 0                  # per group: (overlap before it, its key)
    while lead < len(K):
        prev = overlap
        while trail < len(K) and K[trail] <= K[lead]:
            overlap -= not opens[trail]; trail += 1
        cur = K[lead]
        while lead < len(K) and K[lead] == cur:
            overlap += opens[lead]; lead += 1
        groups.append((prev, cur, overlap))
    best = max(g[2] for g in groups)
    if best < min_hits:
        return b""
    min_hits = max(min_hits, cutoffs[min(int(min(best, qs) / max(SKETCH / 1000.0, 1.0)), len(cutoffs) - 1)])
    runs, cur, prev_key = [], None, 0
    for prev, key, _ in groups:
        seq, pos = prev_key >> 32, prev_key & 0xFFFFFFFF
        if prev >= min_hits:
            if cur and cur[0] != seq:
                runs.append(cur); cur = None
            cur = [seq, pos, pos, prev] if cur is None else [cur[0], cur[1], pos, max(cur[3], prev)]
        elif cur:
            runs.append(cur); cur = None
        prev_key = key
    if cur:
        runs.append(cur)
    out = []
    for r in runs:
        if out and r[0] == out[-1][0] and not r[1] > out[-1][2] + SEG:
            out[-1][2] = r[2]; out[-1][3] = max(out[-1][3], r[3])
        else:
            out.append(list(r))
    return np.array([tuple(r) for r in out], dtype=L1_DT).tobytes()


def test_grouping_by_contig_and_position_is_not_the_reference(oracle, l1_check, tmp_path):
    """what the seam cases are for (and that this test file can fail): a sweep that groups by (seqId, pos) differs from the oracle on the
    seam2 lists, on which the header's sweep equals it"""
    h = oracle.session([("c", U.random_dna(5, 30000))], 19, SEG, SKETCH, 0.85, U.FILTER_MAP, U.FLAG_HG)
    cutoffs = oracle.cutoffs(h)
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(200):
        seq, o, c = scenario(rng, "seam2")
        pts = points(seq, o, c)
        cs = dict(pts=pts, ids=np.zeros(len(pts), dtype=np.int64), W=0, nFreq=0, qs=60, min_hits=int(rng.integers(2, 6)), hg=1, groups=None)
        cs["want"], _ = oracle_l1(oracle, h, cs)
        cases.append(cs)
    oracle.free(h)
    assert run_program(l1_check, 0, cases, cutoffs, tmp_path) == [cs["want"] for cs in cases]
    differ = sum(l1_grouped_by_seq_and_pos(cs["pts"], cs["qs"], cs["min_hits"], cutoffs) != cs["want"] for cs in cases)
    assert differ > 20, differ
