"""Helpers of tests/test_gpu_chain.py: the batch every case of mm_chain_reads is in, its candidate mappings from the oracle (for the
CPU check that the batch really holds those cases), and the host stage through libmashmap_host.so (mmh_post_batch, mmh_post_chained,
mmh_chain_rows).

k 16, segLength 1000, s 80, pi 0.85, kmerThreshold 0: three contigs of tens of kbp --
  uniq    60 kbp of random sequence
  triple  a unit of 1 100 bp three times in tandem (exact copies) between flanks: a fragment out of it has a record per copy, of equal identity
  array   a unit of 1 100 bp twelve times in tandem (exact copies, as tests/largewave.py's): twelve records per fragment
"""
import ctypes as C

import numpy as np

import mmutil as U

K, L, S, PI = 16, 1000, 80, 0.85
ROW_DT = np.dtype([("querySeqId", "<i4"), ("queryLen", "<i4"), ("queryStartPos", "<i4"), ("queryEndPos", "<i4"), ("refSeqId", "<i4"),
                   ("refStartPos", "<i4"), ("refEndPos", "<i4"), ("strand", "<i4"), ("conservedSketches", "<i4"), ("blockLength", "<i4"),
                   ("nucIdentity", "<f4"), ("kmerComplexity", "<f4")])          # mmh_row (mashmap_amd/host/host_capi.cpp)


def case():
    uniq = U.random_dna(8101, 60000)
    unit3, unit12 = U.random_dna(8102, 1100), U.random_dna(8103, 1100)
    contigs = [("uniq", uniq), ("triple", U.arrayed(8104, unit3, 3, 0)), ("array", U.arrayed(8107, unit12, 12, 0))]
    tri, arr = contigs[1][1], contigs[2][1]

    def cut(a, x, n, seed, err=0.04):
        return U.mutate(a[x:x + n + n // 8 + 64], seed, err)[:n].copy()

    reads = []
    for i, (x, nseg, extra) in enumerate(((1000, 2, 0), (7000, 3, 0), (12000, 4, 345), (20000, 5, 0), (27000, 6, 777), (34000, 7, 0), (43000, 8, 1))):
        reads.append(("fwd%d" % nseg, cut(uniq, x, nseg * L + extra, 8110 + i)))
    for i, (x, nseg, extra) in enumerate(((3000, 2, 500), (15000, 4, 0), (50000, 8, 0))):
        reads.append(("rc%d" % nseg, U.revcomp(cut(uniq, x, nseg * L + extra, 8120 + i))))
    # 1 500 unrelated bases in the middle of the read: the two halves are more than chain_gap apart on the query axis
    reads.append(("insertion", np.concatenate([cut(uniq, 30000, 2 * L, 8130), U.random_dna(8131, 1500), cut(uniq, 32000, 2 * L + 500, 8132)])))
    reads.append(("tandem", cut(tri, 3000 + 50, 2 * L, 8140, 0.02)))                  # out of the three exact copies: records that tie
    reads.append(("tandem_rc", U.revcomp(cut(tri, 3000 + 700, 2 * L + 300, 8141, 0.02))))
    reads.append(("short", cut(uniq, 56000, 600, 8150)))                               # shorter than a segment
    reads.append(("one_segment_maps", np.concatenate([cut(uniq, 25000, L, 8160), U.random_dna(8161, 2 * L)])))   # a lone record of a longer read
    reads.append(("array_one", cut(arr, 3000 + 300, L, 8170, 0.02)))                    # twelve records: still taken
    reads.append(("array_two", cut(arr, 3000 + 500, 2 * L, 8171, 0.02)))                # more than 16 records: handed over
    reads.append(("unrelated", U.random_dna(8180, 3 * L + 10)))                        # no record at all
    reads.append(("array_three", cut(arr, 3000 + 100, 3 * L + 200, 8172, 0.02)))       # handed over, behind a read without records
    reads.append(("last", cut(uniq, 9000, 3 * L, 8190)))
    return contigs, reads


def fragments_of(n):
    if n <= L:
        return [(0, n)]
    fr = [(i * L, L) for i in range(n // L)]
    if n % L:
        fr.append((n - L, L))
    return fr


def oracle_records(orc, h, reads):
    """the batch's candidate mappings from the oracle alone, as capi.MAPPING_DT (inside a fragment in the order of its final sort, which
    is all the CPU check of the batch needs); kmerThreshold 0: the query sketch is the raw sketch, its last hash is maxHash"""
    from mashmap_amd import capi
    out = []
    for ri, (name, a) in enumerate(reads):
        if len(a) < K:
            continue
        for off, ln in fragments_of(len(a)):
            e = orc.map_fragment(h, a[off:off + ln], ri, name.encode(), len(a), S)
            for m in e["maps_i"]:
                out.append((ri, off, ln, m[5], m[1], m[9], m[8], m[10], e["rawSketchSize"], 0, e["sketch"][-1][0]))
    return np.array(out, dtype=capi.MAPPING_DT)


def _lens(reads):
    return np.array([len(a) for _, a in reads], dtype=np.int32)


def post(contig_lens, reads, recs, rows=None, num_mappings=1, threads=2, filter_mode=U.FILTER_MAP):
    """mmh_post_chained: the reported mappings (mmh_row + n_merged + approxMatches) of the batch from `rows` (mm_chain_row, may be None)
    and the records `recs`"""
    from mashmap_amd import shard
    lib = shard.host_lib()
    cl = np.ascontiguousarray(contig_lens, dtype=np.int32); rl = _lens(reads)
    recs = np.ascontiguousarray(recs); nrow = 0 if rows is None else len(rows)
    rows = np.ascontiguousarray(rows) if nrow else None
    cap = len(recs) + nrow + 1
    out = np.zeros(cap, dtype=ROW_DT); nm = np.zeros(cap, dtype=np.int32); am = np.zeros(cap, dtype=np.int32)
    n = lib.mmh_post_chained(K, L, S, PI, filter_mode, 1, num_mappings, num_mappings, L, L, len(cl), cl.ctypes.data, rows.ctypes.data if nrow else None, nrow,
                             recs.ctypes.data if len(recs) else None, len(recs), rl.ctypes.data, len(rl), 0, threads, None, out.ctypes.data, nm.ctypes.data,
                             am.ctypes.data, cap)
    assert 0 <= n <= cap
    return out[:n], nm[:n], am[:n]


def post_batch(contig_lens, reads, recs, num_mappings=1, threads=2):
    """mmh_post_batch, the stage as it was"""
    from mashmap_amd import shard
    lib = shard.host_lib()
    cl = np.ascontiguousarray(contig_lens, dtype=np.int32); rl = _lens(reads)
    recs = np.ascontiguousarray(recs)
    out = np.zeros(len(recs) + 1, dtype=ROW_DT)
    n = lib.mmh_post_batch(K, L, S, PI, U.FILTER_MAP, 1, num_mappings, len(cl), cl.ctypes.data, recs.ctypes.data, len(recs), rl.ctypes.data, len(rl), 0, threads,
                           None, out.ctypes.data, len(out))
    return out[:n]


def host_rows(contig_lens, reads, recs, num_mappings=1, max_records=16):
    """mmh_chain_rows: MapPost::chainedFromRecords of every read with at most max_records records, as capi.CHAIN_ROW_DT"""
    from mashmap_amd import capi, shard
    lib = shard.host_lib()
    cl = np.ascontiguousarray(contig_lens, dtype=np.int32); rl = _lens(reads)
    recs = np.ascontiguousarray(recs)
    out = np.zeros(len(recs) + 1, dtype=capi.CHAIN_ROW_DT)
    n = lib.mmh_chain_rows(K, L, S, PI, U.FILTER_MAP, num_mappings, num_mappings, L, L, len(cl), cl.ctypes.data, recs.ctypes.data if len(recs) else None, len(recs),
                           rl.ctypes.data, len(rl), 0, max_records, out.ctypes.data, len(out))
    assert 0 <= n <= len(out)
    return out[:n]


def figures(reads, recs, reported, n_merged):
    """what the batch holds, from its records and the host's reported mappings: per read the number of records, of reported mappings and
    the n_merged of each"""
    nrec = np.bincount(recs["querySeqId"], minlength=len(reads))
    per = {name: dict(records=int(nrec[i]), reported=[], merged=[]) for i, (name, _) in enumerate(reads)}
    for r, m in zip(reported, n_merged):
        d = per[reads[int(r["querySeqId"])][0]]
        d["reported"].append((int(r["queryStartPos"]), int(r["queryEndPos"]), int(r["refSeqId"]), int(r["refStartPos"]), int(r["strand"])))
        d["merged"].append(int(m))
    return per


def check_holds(reads, recs, per):
    """the batch holds every case test_gpu_chain.py is about (asserted on the CPU from the oracle's records, and again on the device's)"""
    for name, a in reads:
        if name.startswith(("fwd", "rc")):
            nseg = int(name[3:] if name.startswith("fwd") else name[2:])
            assert len(a) // L == nseg and max(per[name]["merged"]) >= nseg, (name, per[name])         # one chain over every full segment
            assert all(x[4] == (1 if name.startswith("fwd") else -1) for x in per[name]["reported"])
    assert sorted(len(a) // L for n, a in reads if n.startswith(("fwd", "rc"))) == [2, 2, 3, 4, 4, 5, 6, 7, 8, 8]
    ins = per["insertion"]
    assert len(ins["reported"]) == 2 and ins["reported"][0][1] <= 2 * L + 1500 // 2 <= ins["reported"][1][0], ins     # two chains, one on either side
    for name in ("tandem", "tandem_rc"):
        rt = recs[recs["querySeqId"] == [n for n, _ in reads].index(name)]
        first = rt[rt["fragStart"] == 0]
        assert len(first) >= 2 and len(set(first["conservedSketches"].tolist())) < len(first), (name, first)          # several records in a fragment, identities tie
    assert per["tandem"]["records"] >= 4 and per["tandem_rc"]["records"] >= 4
    assert per["short"]["records"] >= 1 and per["short"]["merged"] == [0] and len(dict(reads)["short"]) < L
    assert per["one_segment_maps"]["records"] == 1 and per["one_segment_maps"]["reported"] == []                       # dropped by filterWeakMappings
    assert 2 <= per["array_one"]["records"] <= 16
    assert per["array_two"]["records"] > 16 and per["array_three"]["records"] > 16
    assert per["unrelated"]["records"] == 0 and per["last"]["records"] == 3
