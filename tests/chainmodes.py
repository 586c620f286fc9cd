"""Helpers of tests/test_gpu_chain_modes.py: the batch every case of MM_OPT_CHAIN_MODES is in -- mm_chain_reads under -Y reference groups
(MM_FLAG_SKIP_PREFIX) and under --noSplit (MM_FLAG_NO_SPLIT) --, the host's rows for it (mmh_chain_rows_modes: MapPost with skip_prefix,
refIdGroup and split set), the run counts derived from those rows, and the CPU check that the batch really holds its cases
(tests/test_chain_modes_batch.py runs it on the oracle's records, the GPU test again on the device's).

k 16, segLength 1000, s 80, pi 0.85, kmerThreshold 0 (chainbatch's).  About 200 kbp in six contigs and four groups:
  A#1#c0   60 kbp of random sequence
  A#1#c1   30 kbp of random sequence holding a copy (3 % diverged) of 3 kbp of A#1#c0: two contigs of one group that the same read hits
  B#1#c0   A#1#c0 mutated 1.5 %
  B#1#arr  the array below once more, between other flanks: a fragment out of it has twelve records in group B and twelve in group D
  C#1#c0   A#1#c0 mutated 3 %
  D#1#arr  a unit of 1 100 bp twelve times in tandem between flanks: twelve records per fragment and group
(the contigs of a group are consecutive, as Map::setRefGroups numbers groups: gpucheck.prefix_groups gives 0 0 1 1 2 3).  Mapped WITHOUT
the top-ANI filter of L1 (no FLAG_HG): with it a group's second-best contig never reaches L2, and no two contigs of a group would meet
in the filter."""
import numpy as np

import chainbatch as B
import gpucheck
import mmutil as U

K, L, S, PI = B.K, B.L, B.S, B.PI
LONG_MAX = 512
COPY_AT, COPY_LEN, COPY_TO = 20000, 3000, 10000


def case():
    """(contigs, reads, refGroup, readRefGroup)"""
    a0 = U.random_dna(8501, 60000)
    a1 = U.random_dna(8502, 30000)
    a1[COPY_TO:COPY_TO + COPY_LEN] = U.mutate(a0[COPY_AT:COPY_AT + COPY_LEN + 200], 8503, 0.03)[:COPY_LEN]
    unit = U.random_dna(8506, 1100)
    arr = U.arrayed(8507, unit, 12, 0)
    contigs = [("A#1#c0", a0), ("A#1#c1", a1), ("B#1#c0", U.mutate(a0, 8504, 0.015)), ("B#1#arr", U.arrayed(8508, unit, 12, 0)),
               ("C#1#c0", U.mutate(a0, 8505, 0.03)), ("D#1#arr", arr)]
    pre, grp = gpucheck.prefix_groups([n for n, _ in contigs], "#")
    assert grp == [0, 0, 1, 1, 2, 3]

    def cut(a, x, n, seed, err=0.04):
        return U.mutate(a[x:x + n + n // 8 + 64], seed, err)[:n].copy()

    reads = [("three", cut(a0, 5000, 3 * L, 8510)),                                    # 3 segments: nine records in three groups, the one-thread kernel's
             ("eight_tail", cut(a0, 30000, 8 * L + 345, 8511)),                        # 8 segments and a tail: 27 records, the wave kernel's
             ("eight_tail_rc", U.revcomp(cut(a0, 40000, 8 * L + 345, 8512))),
             ("copied", cut(a0, COPY_AT, COPY_LEN, 8513, 0.02)),                       # over the copied block: two contigs of group A compete inside one run
             ("short", cut(a0, 50000, 600, 8514)),                                     # shorter than a segment
             ("one_record", cut(a1, 20000, L, 8515)),                                  # a stretch only A#1#c1 has
             ("unrelated", U.random_dna(8516, 3 * L + 10)),                            # no record at all
             ("array_two", cut(arr, 3000 + 500, 2 * L, 8517, 0.02)),                   # more than 16 records in each of two groups
             ("array_many", np.concatenate([cut(arr, 3000 + 100 + 50 * i, 10 * L, 8540 + i, 0.02) for i in range(3)])),   # above 512 records: handed over
             ("A#1#own", cut(a0, 10000, 4 * L, 8520)),                                 # uploaded with readRefGroup = group A: no record in A
             ("six", cut(a0, 1000, 6 * L, 8521)),                                      # 18 records: just over the one-thread kernel's 16
             ("rc4", U.revcomp(cut(a0, 15000, 4 * L, 8522))),
             ("fwd2", cut(a0, 25000, 2 * L, 8523)),
             ("array_one", cut(arr, 3000 + 300, L, 8524, 0.02)),                       # one fragment, its records in two groups, not split
             ("rc5_tail", U.revcomp(cut(a0, 53000, 5 * L + 500, 8525))),
             ("last", cut(a0, 9000, 3 * L, 8526))]                                     # an ordinary read last
    read_grp = [grp[pre.index(n[:n.rfind("#")])] if "#" in n and n[:n.rfind("#")] in pre else -1 for n, _ in reads]
    assert read_grp.count(-1) == len(reads) - 1 and read_grp[[n for n, _ in reads].index("A#1#own")] == 0
    return contigs, reads, grp, read_grp


def nosplit_reads(contigs):
    """reads of 600, 1 000, 2 500 and 6 000 bp out of A#1#c0: under --noSplit each is one fragment"""
    a0 = contigs[0][1]
    return [("ns%d" % n, U.mutate(a0[x:x + n + n // 8 + 64], 8530 + i, 0.04)[:n].copy()) for i, (x, n) in enumerate(((2000, 600), (8000, 1000), (14000, 2500), (33000, 6000)))]


def oracle_records(orc, h, reads, split=True):
    """chainbatch.oracle_records with --noSplit: a read is then one fragment whatever its length"""
    from mashmap_amd import capi
    out = []
    for ri, (name, a) in enumerate(reads):
        if len(a) < K:
            continue
        for off, ln in (B.fragments_of(len(a)) if split else [(0, len(a))]):
            e = orc.map_fragment(h, a[off:off + ln], ri, name.encode(), len(a), S)
            for m in e["maps_i"]:
                out.append((ri, off, ln, m[5], m[1], m[9], m[8], m[10], e["rawSketchSize"], 0, e["sketch"][-1][0]))
    return np.array(out, dtype=capi.MAPPING_DT)


def host_rows(contig_lens, reads, recs, num_mappings=1, filter_mode=U.FILTER_MAP, ref_group=None, split=True, max_records=LONG_MAX):
    """mmh_chain_rows_modes: MapPost::chainedFromRecords of every read with at most max_records records, with skip_prefix and refIdGroup
    set when ref_group is given and Parameters::split as given, as capi.CHAIN_ROW_DT"""
    from mashmap_amd import capi, shard
    lib = shard.host_lib()
    cl = np.ascontiguousarray(contig_lens, dtype=np.int32); rl = np.array([len(a) for _, a in reads], dtype=np.int32)
    rg = None if ref_group is None else np.ascontiguousarray(ref_group, dtype=np.int32)
    assert rg is None or len(rg) == len(cl)
    recs = np.ascontiguousarray(recs)
    out = np.zeros(len(recs) + 1, dtype=capi.CHAIN_ROW_DT)
    n = lib.mmh_chain_rows_modes(K, L, S, PI, filter_mode, num_mappings, num_mappings, L, L, len(cl), cl.ctypes.data, recs.ctypes.data if len(recs) else None, len(recs),
                                 rl.ctypes.data, len(rl), 0, max_records, out.ctypes.data, len(out), None if rg is None else rg.ctypes.data, 1 if split else 0)
    assert 0 <= n <= len(out)
    return out[:n]


def records_per_read(reads, recs):
    return np.bincount(recs["querySeqId"], minlength=len(reads))


def expected_counts(nrec, long_on=True):
    """chain_counts() / chain_long_counts() of the batch from its record histogram (chainlong.expected_counts)"""
    top = LONG_MAX if long_on else 16
    return (dict(offered=int((nrec > 0).sum()), finished=int(((nrec > 0) & (nrec <= top)).sum()), leftover=int(nrec[nrec > top].sum())),
            dict(offered=int((nrec > 16).sum()), finished=int(((nrec > 16) & (nrec <= LONG_MAX)).sum()) if long_on else 0))


def group_counts(n_reads, rows, ref_group, filter_mode=U.FILTER_MAP):
    """chain_group_counts() from the host's rows of the finished reads.  Every run of filterByGroup leaves at least one row (the sweep keeps
    the best mapping at the run's first event; a run of one member is kept), and with a non-decreasing refGroup array a group's members
    are one run: a read's runs are the groups among its rows -- one, without groups, for a read that has a row.  Filter mode none: no run"""
    if filter_mode == U.FILTER_NONE:
        return dict(reads=0, runs=0)
    assert ref_group is None or list(ref_group) == sorted(ref_group)
    g = np.zeros(len(rows), dtype=np.int64) if ref_group is None else np.asarray(ref_group)[rows["refSeqId"]]
    per = [len(set(g[rows["querySeqId"] == r].tolist())) for r in range(n_reads)]
    return dict(reads=sum(1 for x in per if x > 1), runs=sum(per))


def check_holds(reads, recs, rows0, rows2, ref_group):
    """the batch holds every case test_gpu_chain_modes.py is about; rows0 / rows2: the host's rows (host_rows with ref_group) of every read of
    at most 512 records at secondaryToKeep 0 / 2"""
    names = [n for n, _ in reads]
    nrec = records_per_read(reads, recs)
    per = dict(zip(names, nrec.tolist()))
    rg = np.asarray(ref_group)

    def of(a, name):
        return a[a["querySeqId"] == names.index(name)]

    def groups(a):
        return sorted(rg[a["refSeqId"]].tolist())

    three = of(recs, "three")
    assert len(three) == 9 and groups(three) == [0] * 3 + [1] * 3 + [2] * 3                                      # nine records in three groups
    assert groups(of(rows0, "three")) == [0, 1, 2] and all(int(x) == 3 for x in of(rows0, "three")["n_merged"])   # one row per group, each a chain of 3
    for name, strand in (("eight_tail", 1), ("eight_tail_rc", -1)):
        assert 27 <= per[name] <= LONG_MAX and len(dict(reads)[name]) % L != 0
        rw = of(rows0, name)
        assert groups(rw) == [0, 1, 2] and all(int(x) == strand for x in rw["strand"]) and int(rw["n_merged"].min()) >= 8, (name, rw)
        a, b = rw[0], rw[1]                                                                                      # chains of several groups over the same query interval
        assert a["queryStartPos"] < b["queryEndPos"] and b["queryStartPos"] < a["queryEndPos"]
    cp = of(recs, "copied")
    assert set(cp["refSeqId"].tolist()) >= {0, 1, 2, 4} and int(((cp["refSeqId"] == 0) | (cp["refSeqId"] == 1)).sum()) >= 4    # both contigs of group A
    assert groups(of(rows0, "copied")).count(0) == 1 and int(of(rows0, "copied")[rg[of(rows0, "copied")["refSeqId"]] == 0]["refSeqId"][0]) == 0   # A#1#c0 wins at 0
    assert groups(of(rows2, "copied")).count(0) == 2                                                             # ... and A#1#c1 is kept at 2
    assert len(dict(reads)["short"]) < L and per["short"] == 3 and groups(of(rows0, "short")) == [0, 1, 2]       # runs of one member
    assert per["one_record"] == 1 and len(of(rows0, "one_record")) == 1
    assert per["unrelated"] == 0
    two = of(recs, "array_two")
    assert int((rg[two["refSeqId"]] == 1).sum()) > 16 and int((rg[two["refSeqId"]] == 3).sum()) > 16 and per["array_two"] <= LONG_MAX
    assert set(groups(of(rows0, "array_two"))) == {1, 3}
    assert per["array_many"] > LONG_MAX and len(of(rows0, "array_many")) == 0                                    # handed over
    own = of(recs, "A#1#own")
    assert len(own) >= 6 and 0 not in groups(own) and set(groups(of(rows0, "A#1#own"))) == {1, 2}                # no record in its own group
    assert 16 < per["six"] <= 27 and 2 <= per["fwd2"] <= 16 and 16 < per["array_one"] <= LONG_MAX and len(dict(reads)["array_one"]) <= L
    assert per["last"] == 9 and groups(of(rows0, "last")) == [0, 1, 2]
    assert int(((nrec > 0) & (nrec <= 16)).sum()) >= 6 and int(((nrec > 16) & (nrec <= LONG_MAX)).sum()) >= 5
