"""The default L1 kernels -- k_lookup_l1<MAXPTS>, k_lookup_mid, mm_l1_fused (mashmap_amd/csrc/mm_map.hip) -- at the point counts and
capacities that decide what a fragment goes through, on a planted index (tests/l1plant.py): reads of random DNA, one fragment each, whose
hits are exactly the minmer records a plan puts under their sketch hashes.

Every case (a batch of fragments over one planted index) first derives its figures from the oracle alone and asserts them -- P, seeds
with points, kept points, runs, and the route l1plant.route names for every fragment: a case that does not sit on the edge it is named
for fails on the CPU side --, then runs gpucheck.run_and_compare over the planted index (sized, steady-state, kept-points and filtered
pass against the oracle on every integer), and holds pass_l1_mid() and pass_l1_literal()[0] of the sized pass against the model's counts
and stats["nPoints"] against the oracle's filtered point count.  Every batch runs once more behind the tagged seed table.

k = 16, segLength = 1000; kmerPct 0 (no seed is frequent) but for the frequent-seed case.

Not built: "the only group that reaches minimumHits is the last one".  A fragment's points are whole intervals, so the overlap count
behind the last position group of a list is 0 and cannot reach a minimumHits of 1 or more: the rule has no input that shows it."""
import functools

import numpy as np
import pytest

import gpucheck
import l1plant as P
import mmutil as U

pytestmark = pytest.mark.gpu
K, L = 16, 1000
HG = U.FLAG_HG


def reads_of(n, seed, names=None):
    return [((names or {}).get(i, "r%d" % i), U.random_dna(seed + i, L)) for i in range(n)]


def contigs_of(seed, lens):
    return [("c%d" % i, U.random_dna(seed + i, n)) for i, n in enumerate(lens)]


def finish(oracle, name, contigs, reads, plan, s, pi, flags, expect, kmerPct=0.0, notes=None):
    """the oracle's view of the batch, the model's routes, and the CPU-side check that every fragment takes the route it was planted for"""
    per, cut, thr = P.view(oracle, contigs, reads, K, L, s, pi, flags, kmerPct, plan)
    mh = oracle.min_hits_table(s, K, pi)
    routes = [P.route(fr, s, mh, cut, bool(flags & HG)) for fr in per]
    for f, ((r, i), fr) in enumerate(zip(routes, per)):
        print("%s[%d] %-22s raw sketch %d, Q.sketchSize %d, minHits %d, P %d, valid %d, seeds %d, kept %s, runs %s, nL1 %d -> %s%s"
              % (name, f, (notes or {}).get(f, ""), fr["raw"], fr["q"], i["minHits"], i["P"], i["valid"], i["seeds"], i["kept"], i["runs"], len(fr["l1"]), r[0],
                 " (%s)" % r[1] if r[1] else ""))
    for f, want in expect.items():
        assert routes[f][0][0] == want, "%s fragment %d (%s): planted for %r, the model says %r with %r" % (name, f, (notes or {}).get(f, ""), want, routes[f][0], routes[f][1])
    assert any(fr["l1"] for fr in per), name + ": no fragment with an L1 candidate"
    return dict(name=name, contigs=contigs, reads=reads, plan=plan, s=s, pi=pi, flags=flags, kmerPct=kmerPct, per=per, cut=cut, thr=thr, routes=routes, mh=mh)


def run_case(oracle, case):
    """the batch on the device: every integer of four passes against the oracle, the sized pass's counts against the model"""
    stats_out, pass_out = [], {}
    gpucheck.run_and_compare(oracle, case["contigs"], case["reads"], k=K, L=L, s=case["s"], pi=case["pi"], flags=case["flags"], kmerPct=case["kmerPct"],
                             mutate_index=case["plan"].mutate, stats_out=stats_out, pass_out=pass_out)
    mid, queued = P.counts(case["routes"])
    print("%s: the model expects %d through k_lookup_mid and %d queued; the sized pass had %d and %r" % (case["name"], mid, queued, pass_out["mid"], pass_out["literal"]))
    assert pass_out["mid"] == mid, (pass_out, mid, [r for r, _ in case["routes"]])
    assert pass_out["literal"][0] == queued, (pass_out, queued, [r for r, _ in case["routes"]])
    assert [int(x) for x in stats_out[0]["nPoints"]] == [len(fr["points"]) for fr in case["per"]]


# ----------------------------------------------------------------------------- a, b: the fused tiers, and runs per seed
TIERS = {130: (2, 62, 64, 66, 126, 128, 130), 200: (128, 130, 254, 256, 258), 310: (256, 258, 510, 512, 514)}
FULL = {130: (64, 128), 200: (128, 256), 310: (256, 512)}


def width_of(m):
    """long enough for m intervals 3 apart to lie over one position, and for more to follow"""
    return 3 * m + 100


def tier_of(n):
    return 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8 if n <= 512 else 16


def plant_tier(plan, f, n, m, place, self_seq=None):
    """n points: a cluster of m overlapping intervals (2 m points; m = minHits + 1) and single intervals, one seed each (dealt to 250 - m
    seeds where there are more: k_lookup_mid lists 256 seeds).  place: the
    cluster sorts to the `start` or the `end` of the list, or lies in the `mid`dle and starts two points before a lane boundary.
    self_seq: five of the single intervals (fewer where there are not six) lie on that contig (the read carries its name:
    MM_FLAG_SKIP_SELF drops them).  Returns the (seqId, first OPEN, last CLOSE) of the cluster and the number of intervals dropped"""
    if n < 2 * m:
        plan.singles(f, list(range(n // 2)), 0, 300, n // 2, 50, 20)
        return None, 0
    R, ns = tier_of(n), (n - 2 * m) // 2
    ranks = [m + i % (250 - m) for i in range(ns)]
    nself = min(5, ns - 1) if self_seq is not None else 0
    if place == "start": nb = 0
    elif place == "end": nb = ns - nself
    else:
        nb = (ns - nself) // 2
        while R >= 4 and (2 * nb) % R != R - 2: nb -= 1
    cq = 1
    plan.singles(f, ranks[:nb], 0, 300, nb, 50, 20)                                # before the cluster: contig 0
    plan.cluster(f, list(range(m)), cq, 100 if place == "start" or nb == 0 else 20000, width=width_of(m))
    rest = ns - nb - nself
    plan.singles(f, ranks[nb:nb + rest], 1, 25000, rest, 50, 20)                  # behind it: the same contig
    if nself: plan.singles(f, ranks[nb + rest:], self_seq, 700, nself, 50, 20)
    at = 100 if place == "start" or nb == 0 else 20000
    return (cq, at, at + (m - 1) * 3 + width_of(m)), nself


@functools.lru_cache(maxsize=None)
def case_tiers(s, pi=0.85):
    oracle = U.Oracle()
    m = int(oracle.min_hits_table(s, K, pi)[s]) + 1
    specs = [(n, "mid", False) for n in TIERS[s]]
    for n in FULL[s]: specs += [(n, "end", False), (n, "start", False), (n, "mid", True)]
    extra = []
    if s == 310 and pi < 0.9:                                                                 # b: runs per seed (c <= 8: the owning lane copies; above: the wave)
        extra = ["8 and 10 points", "one seed, 400 points", "long runs at 0, 63, 255", "two long runs, one batch"]
    n = len(specs) + len(extra)
    names = {i: "c2" for i, sp in enumerate(specs) if sp[2]}
    reads = reads_of(n, 5000 + s, names)
    contigs = contigs_of(300 + s, [40000, 40000, 40000])
    plan = P.Plan(oracle, reads, K, s)
    where, nself, notes, expect = {}, {}, {}, {}
    for f, (npt, place, selfv) in enumerate(specs):
        where[f], nself[f] = plant_tier(plan, f, npt, m, place, 2 if selfv else None)
        notes[f] = "P=%d %s%s" % (npt, place, " self" if selfv else "")
        expect[f] = "fused" if npt <= P.fused_cap(s) else "mid"
    f0 = len(specs)
    if extra:
        plan.cluster(f0, list(range(20, 20 + m)), 1, 5000, width=width_of(m))
        plan.singles(f0, [5], 0, 1000, 4, 300, 20); plan.singles(f0, [6], 0, 9000, 5, 300, 20)
        plan.cluster(f0 + 1, list(range(20, 20 + m)), 1, 5000, width=width_of(m))
        plan.singles(f0 + 1, [300], 0, 1000, 200, 40, 20)
        plan.cluster(f0 + 2, list(range(20, 20 + m)), 1, 5000, width=width_of(m))
        for r_, at in ((0, 1000), (63, 6000), (255, 11000)): plan.singles(f0 + 2, [r_], 0, at, 6, 300, 20)
        plan.singles(f0 + 2, [256], 2, 1000, 7, 300, 20)                          # and one in the second probing batch
        plan.cluster(f0 + 3, list(range(20, 20 + m)), 1, 5000, width=width_of(m))
        plan.singles(f0 + 3, [3], 0, 1000, 9, 300, 20); plan.singles(f0 + 3, [40], 0, 7000, 30, 300, 20); plan.singles(f0 + 3, [130], 2, 1000, 12, 300, 20)
        for i, e in enumerate(extra): notes[f0 + i] = e; expect[f0 + i] = "fused"
    case = finish(oracle, "tiers s=%d pi=%.2f" % (s, pi), contigs, reads, plan, s, pi, HG | U.FLAG_SKIP_SELF, expect, notes=notes)
    for f, (npt, place, selfv) in enumerate(specs):
        fr, R = case["per"][f], tier_of(npt)
        assert fr["raw"] == fr["q"] == s and fr["P"] == npt and fr["seeds"] == min(npt // 2, 250), (f, fr["raw"], fr["q"], fr["P"], fr["seeds"])
        assert len(fr["points"]) == npt - 2 * nself[f] and (nself[f] > 0) == selfv   # MM_EMPTY keys inside P: nValid < P
        if where[f] is None: continue
        cq, o, c = where[f]
        i0, i1 = fr["points"].index((cq, o, 1)), fr["points"].index((cq, c, -1))
        assert i1 - i0 == 2 * m - 1 and len(fr["l1"]) == 1, (f, i0, i1, fr["l1"])
        if place == "start": assert i0 == 0
        elif place == "end": assert i1 == len(fr["points"]) - 1
        else: assert i0 // R != i1 // R and (R < 4 or i0 % R == R - 2), (f, i0, i1, R)
    if extra:
        per = case["per"]
        assert [per[f0 + i]["P"] for i in range(4)] == [2 * m + 18, 2 * m + 400, 2 * m + 50, 2 * m + 102]
    return case


@pytest.mark.parametrize("pi", [0.85, 0.95])
@pytest.mark.parametrize("s", [130, 200, 310])
def test_fused_tiers(oracle, s, pi):
    """minimumHits 3 / 4 / 7 at pi 0.85, 28 / 45 / 73 at 0.95: above 1 either way, so P = MAXPTS + 2 goes through k_lookup_mid"""
    run_case(oracle, case_tiers(s, pi))


@functools.lru_cache(maxsize=None)
def case_min_hits_one():
    """pi 0.80 at s = 130: minimumHits is 1 -- a list beyond the fused kernel's 128 points is queued, not passed to k_lookup_mid"""
    oracle = U.Oracle()
    s, pi = 130, 0.80
    assert int(oracle.min_hits_table(s, K, pi)[s]) == 1
    reads, contigs = reads_of(3, 5500), contigs_of(350, [40000, 40000])
    plan = P.Plan(oracle, reads, K, s)
    for f, npt in enumerate((128, 130, 258)): plant_tier(plan, f, npt, 3, "mid")
    case = finish(oracle, "minHits 1", contigs, reads, plan, s, pi, HG, {0: "fused", 1: "HBM", 2: "HBM"})
    assert [r[1] for r, _ in case["routes"]] == [None, "minHits", "minHits"] and P.counts(case["routes"]) == (0, 2)
    return case


def test_min_hits_one_is_queued_not_passed_to_mid(oracle):
    run_case(oracle, case_min_hits_one())


# ----------------------------------------------------------------------------- c: a sketch of several probing batches with a frequent seed
@functools.lru_cache(maxsize=None)
def case_frequent(s):
    """fragment 0: its seed of rank 270 is frequent (the first removal comes in the second probing batch and back-fills the first);
    fragment 1: its seeds of ranks 10 and 300; fragment 2: none.  The three hashes carry 40 records each, more than any other hash, and
    kmerPct is 3.5 hashes' share of the index: the frequency threshold comes out at their 80 points"""
    oracle = U.Oracle()
    pi = 0.85
    reads, contigs = reads_of(3, 5600 + s), contigs_of(360 + s, [20000, 20000])
    plan = P.Plan(oracle, reads, K, s)
    m = int(oracle.min_hits_table(s, K, pi)[s]) + 1
    for f, freq in enumerate(((270,), (10, 300), ())):
        for r_ in freq: plan.singles(f, [r_], 0, 1000, 40, 300, 20)
        plan.cluster(f, list(range(100, 100 + m)), 1, 5000)
        plan.cluster(f, list(range(280, 280 + m)), 1, 9000)
        plan.singles(f, list(range(150, 250)), 0, 14000, 100, 50, 20)
    keys = plan.keys_after(np.concatenate([oracle.add_minmers(a, K, L, s, i) for i, (_, a) in enumerate(contigs)]))   # the contigs' own records, as a session adds them
    kmerPct = 100.0 * 3.5 / keys
    case = finish(oracle, "frequent s=%d" % s, contigs, reads, plan, s, pi, HG, {0: "fused", 1: "fused", 2: "fused"}, kmerPct=kmerPct)
    per = case["per"]
    assert case["thr"] == 80 and [(fr["raw"], fr["q"]) for fr in per] == [(s, s - 1), (s, s - 2), (s, s)], (case["thr"], [(fr["raw"], fr["q"]) for fr in per])
    assert plan.hashes[0][270] not in per[0]["sketch"] and plan.hashes[1][10] not in per[1]["sketch"] and plan.hashes[1][300] not in per[1]["sketch"]
    assert all(fr["P"] == 4 * m + 200 and len(fr["l1"]) == 2 for fr in per)
    return case


@pytest.mark.parametrize("s", [310, 498])
def test_frequent_seed_in_a_later_probing_batch(oracle, s):
    run_case(oracle, case_frequent(s))


# ----------------------------------------------------------------------------- d: k_lookup_mid's limits
KEPT = (62, 64, 66, 126, 128, 130, 254, 256, 258, 510, 512, 514, 1022, 1024, 1026)


def plant_kept(plan, f, kept, mh, seq=0, dense_ranks=200, sparse_ranks=(200, 256), nsparse=None, sparse_per_bin=10):
    """kept points = kept / 2 intervals: all but one packed into the 4 096-position bin 1 of the contig, 6 apart and 100 long (each
    position under 16 of them: candidates); single intervals behind it, ten to a bin -- below minimumHits, dropped by the filter but for
    the one that closes last on the contig.  At least 514 points in all."""
    nd = kept // 2 - 1
    plan.singles(f, list(range(dense_ranks)), seq, 4096, nd, 6, 100)
    ns = max(12, 258 - kept // 2) if nsparse is None else nsparse
    ranks = list(range(*sparse_ranks))
    for i in range(ns):
        b = 3 + i // sparse_per_bin
        plan.add(f, ranks[i % len(ranks)], seq, b * 4096 + 100 + (i % sparse_per_bin) * 300, b * 4096 + 100 + (i % sparse_per_bin) * 300 + 20)
    return nd, ns


@functools.lru_cache(maxsize=None)
def case_mid_kept():
    """s = 498, pi 0.85 (minimumHits 13): one value below, at and above every sorter tier of k_lookup_mid, the 16-per-lane one included;
    1 026 kept points are handed over"""
    oracle = U.Oracle()
    s, pi = 498, 0.85
    mh = int(oracle.min_hits_table(s, K, pi)[s])
    assert mh == 13
    reads, contigs = reads_of(len(KEPT), 5700), contigs_of(370, [125000])
    plan = P.Plan(oracle, reads, K, s)
    for f, kept in enumerate(KEPT): plant_kept(plan, f, kept, mh)
    expect = {f: "mid" if kept <= P.MID_MAXKEEP else "mid>HBM" for f, kept in enumerate(KEPT)}
    case = finish(oracle, "mid kept", contigs, reads, plan, s, pi, HG, expect, notes={f: "kept=%d" % kept for f, kept in enumerate(KEPT)})
    for f, kept in enumerate(KEPT):
        fr, ((r, why), info) = case["per"][f], case["routes"][f]
        assert fr["P"] > 512 and fr["seeds"] <= P.MID_MAXSEEDS and (info["kept"] == kept if kept <= 1024 else why == "kept"), (f, kept, info, why)
        # the interval that closes last on the contig lies in a bin of ten intervals, below minimumHits, and is kept all the same
        why_, pts = P.kept_points(fr, mh)
        assert why_ is None and len(pts) == kept and pts[-1][1] == max(c for _, _, c, _ in fr["iv"]) and pts[-1][1] > 3 * 4096
        assert len(fr["l1"]) >= 1
    return case


def test_mid_kept_point_tiers(oracle):
    run_case(oracle, case_mid_kept())


@functools.lru_cache(maxsize=None)
def case_mid_limits():
    """s = 498, pi 0.85: 256 / 257 seeds with points; 16 384 / 16 386 points; lists of 4 096 and 4 098 points (the LDS and the global
    sorter behind a hand-over and in the kept-points pass); an interval over 64 / 65 bins"""
    oracle = U.Oracle()
    s, pi = 498, 0.85
    mh = int(oracle.min_hits_table(s, K, pi)[s])
    reads, contigs = reads_of(8, 5800), contigs_of(380, [275000])
    plan = P.Plan(oracle, reads, K, s)
    notes = {0: "256 seeds", 1: "257 seeds", 2: "P=16384", 3: "P=16386", 4: "P=4096", 5: "P=4098", 6: "64 bins", 7: "65 bins"}
    for f, nseeds in ((0, 256), (1, 257)):                                         # kept 64: 31 dense intervals on the first seeds, the rest sparse, one per seed
        plan.singles(f, list(range(31)), 0, 4096, 31, 6, 100)
        for i in range(nseeds - 31 + 1):
            b = 3 + i // 10
            plan.add(f, 31 + (i % (nseeds - 31)), 0, b * 4096 + 100 + (i % 10) * 300, b * 4096 + 120 + (i % 10) * 300)
    for f, npt in ((2, 16384), (3, 16386), (4, 4096), (5, 4098)):                  # intervals 12 apart, 100 long: every position under eight or nine of them
        plan.singles(f, list(range(250)), 0, 1000, npt // 2, 12, 100)
    for f, nbins in ((6, 64), (7, 65)):
        plant_kept(plan, f, 64, mh, sparse_ranks=(200, 255))
        plan.add(f, 255, 0, 2 * 4096, (2 + nbins - 1) * 4096 + 1)                  # [o, c): c - 1 lies in bin 2 + nbins - 1
    expect = {0: "mid", 1: "mid>HBM", 2: "mid>HBM", 3: "HBM", 4: "mid>HBM", 5: "mid>HBM", 6: "mid", 7: "mid>HBM"}
    case = finish(oracle, "mid limits", contigs, reads, plan, s, pi, HG, expect, notes=notes)
    per, why = case["per"], [r[1] for r, _ in case["routes"]]
    assert [(fr["P"], fr["seeds"]) for fr in per[:2]] == [(514, 256), (516, 257)] and why[:2] == [None, "seeds"]
    assert [fr["P"] for fr in per[2:6]] == [16384, 16386, 4096, 4098] and why[2:6] == ["kept", "points", "kept", "kept"]
    assert [P.hbm_slots(fr["P"]) for fr in per[2:6]] == [16384, 32768, 4096, 8192]
    assert why[6:] == [None, "span"] and per[6]["P"] == per[7]["P"] and case["routes"][6][1]["kept"] == 64
    return case


def test_mid_seed_point_and_span_limits(oracle):
    run_case(oracle, case_mid_limits())


@functools.lru_cache(maxsize=None)
def case_mid_contigs():
    """130 contigs of 1 500 bp; fragment 0 has intervals on 128 of them (finished by k_lookup_mid), fragment 1 on 129 (handed over)"""
    oracle = U.Oracle()
    s, pi = 498, 0.85
    reads, contigs = reads_of(2, 5900), contigs_of(390, [1500] * 130)
    plan = P.Plan(oracle, reads, K, s)
    for f, nc in ((0, 128), (1, 129)):
        plan.cluster(f, list(range(14)), 0, 200, step=3, width=150)
        for q in range(nc):
            plan.add(f, 20 + q, q, 500, 520); plan.add(f, 20 + q, q, 700, 720)
    case = finish(oracle, "mid contigs", contigs, reads, plan, s, pi, HG, {0: "mid", 1: "mid>HBM"})
    assert [len({q for q, _, _, _ in fr["iv"]}) for fr in case["per"]] == [128, 129] and case["routes"][1][0][1] == "contigs"
    assert all(fr["P"] > 512 for fr in case["per"])
    return case


def test_mid_contig_table(oracle):
    run_case(oracle, case_mid_contigs())


@functools.lru_cache(maxsize=None)
def case_sketch_limit(s):
    """s = 512: the largest sketch k_lookup_mid serves; s = 513: the pass has no k_lookup_mid"""
    oracle = U.Oracle()
    pi = 0.85
    mh = int(oracle.min_hits_table(s, K, pi)[s])
    reads, contigs = reads_of(2, 6000 + s), contigs_of(400 + s, [125000])
    plan = P.Plan(oracle, reads, K, s)
    plant_kept(plan, 0, 2 * mh + 40, mh)
    plan.cluster(1, list(range(mh + 1)), 0, 3000)
    case = finish(oracle, "sketch s=%d" % s, contigs, reads, plan, s, pi, HG, {0: "mid" if s == 512 else "HBM", 1: "fused"})
    assert all(fr["raw"] == fr["q"] == s for fr in case["per"]) and case["per"][0]["P"] > 512 and mh > 1
    assert case["routes"][0][0][1] == (None if s == 512 else "sketch") and P.counts(case["routes"])[0] == (1 if s == 512 else 0)
    return case


@pytest.mark.parametrize("s", [512, 513])
def test_largest_sketch_of_mid(oracle, s):
    run_case(oracle, case_sketch_limit(s))


# ----------------------------------------------------------------------------- e: mm_l1_fused's edges, on k_lookup_l1 and through k_lookup_mid
def plant_fused_edges(plan, f0, mh, filler):
    """five fragments from f0 on: 64 runs, 65 runs, a position shared by the last point of contig 0 and the first of contig 1, two runs
    segLength apart, two runs segLength + 1 apart.  A run: mh intervals of one extent [x, x + 30).  filler(f): what brings the list
    beyond the fused kernel's capacity, for the cases through k_lookup_mid; called first, with the points the fragment is about to get"""
    ranks = list(range(mh))
    for f, nruns in ((f0, 64), (f0 + 1, 65)):
        for j in range(nruns):
            for r_ in ranks: plan.add(f, r_ + mh * (j % 3), 0, 4096 + j * 50, 4096 + j * 50 + 30)
        filler(f, 2 * mh * nruns)
    f = f0 + 2
    for r_ in ranks: plan.add(f, r_, 0, 4096, 4096 + 777 - r_)                     # contig 0's last point closes at 4873 ...
    for r_ in ranks: plan.add(f, mh + r_, 1, 4096 + 777, 4096 + 900 + r_)          # ... where contig 1's first one opens
    filler(f, 4 * mh)
    for f, gap in ((f0 + 3, L), (f0 + 4, L + 1)):
        for r_ in ranks: plan.add(f, r_, 0, 4096, 4096 + 30)
        for r_ in ranks: plan.add(f, mh + r_, 0, 4096 + gap, 4096 + gap + 30)
        filler(f, 4 * mh)


@functools.lru_cache(maxsize=None)
def case_fused_edges(through_mid):
    oracle = U.Oracle()
    s, pi = (498, 0.80) if through_mid else (310, 0.80)
    mh = int(oracle.min_hits_table(s, K, pi)[s])
    assert mh == (4 if through_mid else 2)
    reads, contigs = reads_of(5, 6100 + s), contigs_of(410 + s, [125000, 40000])
    plan = P.Plan(oracle, reads, K, s)

    def filler(f, have):
        # intervals at the head of contig 0, 6 apart and 4 long -- never two over a position, all in bin 0, which they fill beyond
        # minimumHits: kept --, as many as bring the fragment to 520 points or more
        if through_mid: plan.singles(f, list(range(100, 300)), 0, 100, max(4, (520 - have + 1) // 2), 6, 4)
    plant_fused_edges(plan, 0, mh, filler)
    mid = "mid" if through_mid else "fused"
    over = "mid>HBM" if through_mid else "HBM"
    case = finish(oracle, "fused edges %s" % mid, contigs, reads, plan, s, pi, 0, {0: mid, 1: over, 2: over, 3: mid, 4: mid},
                  notes={0: "64 runs", 1: "65 runs", 2: "shared position", 3: "runs %d apart" % L, 4: "runs %d apart" % (L + 1)})
    per, routes = case["per"], case["routes"]
    assert [i["runs"] for _, i in routes[:2]] == [64, 65] and [r[1] for r, _ in routes[:3]] == [None, "runs", "mixed"]
    assert all((fr["P"] > 512) == through_mid and fr["P"] <= 1024 for fr in per)
    last0 = [p for p in per[2]["points"] if p[0] == 0][-1]; first1 = [p for p in per[2]["points"] if p[0] == 1][0]
    assert last0[1] == first1[1] and last0[2] == -1 and first1[2] == 1
    assert [len(fr["l1"]) for fr in per[3:]] == [1, 2] and per[3]["l1"][0][1:3] == (4096, 4096 + L) and [c[1] for c in per[4]["l1"]] == [4096, 4096 + L + 1]
    return case


@pytest.mark.parametrize("through_mid", [False, True], ids=["k_lookup_l1", "k_lookup_mid"])
def test_fused_sweep_edges(oracle, through_mid):
    run_case(oracle, case_fused_edges(through_mid))


# ----------------------------------------------------------------------------- f: the sorters behind a hand-over
def all_cases():
    return [case_tiers(130), case_tiers(200), case_tiers(310), case_tiers(130, 0.95), case_tiers(200, 0.95), case_tiers(310, 0.95), case_min_hits_one(), case_frequent(310), case_frequent(498), case_mid_kept(),
            case_mid_limits(), case_mid_contigs(), case_sketch_limit(512), case_sketch_limit(513), case_fused_edges(False), case_fused_edges(True)]


def test_lists_for_every_sorter_and_every_route():
    """The kept-points pass of run_and_compare sends every list to HBM unfiltered: the batches above hold lists of 128, 512, 514, 4 096
    and 4 098 points -- the wave, the LDS and the global sorter at the ends of their ranges, in slots of exactly their size and of the
    next power of two.  And every route of the model is taken by some fragment (the tests above hold the model's counts against the
    device's)."""
    cases = all_cases()
    sizes = {fr["P"] for c in cases for fr in c["per"]}
    assert {128, P.SORT_WAVECAP, P.SORT_WAVECAP + 2, P.SORT_LDSCAP, P.SORT_LDSCAP + 2} <= sizes
    tally = {}
    for c in cases:
        for r, _ in c["routes"]: tally[r] = tally.get(r, 0) + 1
    print("routes taken: %r" % sorted(tally.items(), key=str))
    want = [("fused", None), ("mid", None)] + [("mid>HBM", w) for w in ("seeds", "span", "contigs", "kept", "mixed", "runs")] + \
           [("HBM", w) for w in ("minHits", "sketch", "points", "mixed", "runs")]
    assert all(tally.get(r, 0) > 0 for r in want), [r for r in want if not tally.get(r)]


# ----------------------------------------------------------------------------- g: the tagged seed table
TAGGED = [("tiers130", lambda: case_tiers(130)), ("tiers200", lambda: case_tiers(200)), ("tiers310", lambda: case_tiers(310)), ("mid_kept", case_mid_kept),
          ("mid_limits", case_mid_limits), ("mid_contigs", case_mid_contigs), ("s512", lambda: case_sketch_limit(512)), ("s513", lambda: case_sketch_limit(513))]


@pytest.mark.parametrize("which", range(len(TAGGED)), ids=[n for n, _ in TAGGED])
def test_behind_the_tagged_seed_table(oracle, monkeypatch, which):
    """k_lookup_l1<.., true> and k_lookup_mid<true>: MM_SEED_TAGS=1 puts the tag layer in front of the seed table whatever its size (the
    library reads the switch when a context is created)"""
    monkeypatch.setenv("MM_SEED_TAGS", "1")
    run_case(oracle, TAGGED[which][1]())
