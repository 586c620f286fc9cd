"""Helpers of tests/test_gpu_chain_long.py: the batch every case of MM_OPT_CHAIN_LONG is in (reads of 17 .. 512 candidate mappings,
which k_chain_reads_long chains on the device, around reads of fewer and of more), and the CPU check that the batch really holds those
cases.  The host stage and the oracle's records come from tests/chainbatch.py, unchanged.

k 16, segLength 1000, s 80, pi 0.85, kmerThreshold 0 (chainbatch's), three contigs --
  uniq     60 kbp of random sequence (chainbatch's)
  array    a unit of 1 100 bp twelve times in tandem (chainbatch's): twelve records per fragment
  array40  a unit of 1 100 bp forty times in tandem, exact copies: about forty records per fragment, of equal identity
"""
import numpy as np

import chainbatch as B
import mmutil as U

K, L, S, PI = B.K, B.L, B.S, B.PI
LONG_MAX = 512


def case():
    uniq = U.random_dna(8101, 60000)
    unit12, unit40 = U.random_dna(8103, 1100), U.random_dna(8203, 1100)
    contigs = [("uniq", uniq), ("array", U.arrayed(8107, unit12, 12, 0)), ("array40", U.arrayed(8207, unit40, 40, 0))]
    arr, arr40 = contigs[1][1], contigs[2][1]

    def cut(a, x, n, seed, err=0.04):
        return U.mutate(a[x:x + n + n // 8 + 64], seed, err)[:n].copy()

    reads = [("fwd17", cut(uniq, 1000, 17 * L, 8210)),                                 # 17 colinear segments: one chain of 17
             ("fwd2", cut(uniq, 1000, 2 * L, 8110)),
             ("fwd3", cut(uniq, 7000, 3 * L, 8111)),
             ("array_two", cut(arr, 3000 + 500, 2 * L, 8171, 0.02)),                   # 2 fragments x 12 copies: interleaved chains
             ("unrelated", U.random_dna(8180, 3 * L + 10)),                            # no record at all, between long reads
             ("array_three", cut(arr, 3000 + 100, 3 * L + 200, 8172, 0.02)),
             ("fwd21", cut(uniq, 20000, 20 * L + 345, 8211)),                          # 20 segments and a remainder
             ("array40_one", cut(arr40, 3000 + 300, L, 8270, 0.02)),                   # one fragment, not split, more than 16 records
             ("fwd8", cut(uniq, 43000, 8 * L + 1, 8116)),
             ("array_one", cut(arr, 3000 + 300, L, 8170, 0.02)),                       # twelve records: the one-thread kernel's
             ("array40_two", cut(arr40, 3000 + 500, 2 * L, 8271, 0.02)),               # two fragments with more than 16 records each
             ("array40_many", cut(arr40, 3000 + 100, 15 * L, 8272, 0.02)),             # more than 512 records: handed over
             ("rc4", U.revcomp(cut(uniq, 15000, 4 * L, 8121))),
             ("rc33", U.revcomp(cut(uniq, 25000, 33 * L, 8212)))]                      # 33 segments on the reverse strand, last in the batch
    return contigs, reads


def host_rows(contig_lens, reads, recs, num_mappings=1, filter_mode=U.FILTER_MAP):
    """mmh_chain_rows: MapPost::chainedFromRecords of every read with at most 512 records, as capi.CHAIN_ROW_DT (chainbatch.host_rows with
    the filter mode as a parameter)"""
    from mashmap_amd import capi, shard
    lib = shard.host_lib()
    cl = np.ascontiguousarray(contig_lens, dtype=np.int32); rl = np.array([len(a) for _, a in reads], dtype=np.int32)
    recs = np.ascontiguousarray(recs)
    out = np.zeros(len(recs) + 1, dtype=capi.CHAIN_ROW_DT)
    n = lib.mmh_chain_rows(K, L, S, PI, filter_mode, num_mappings, num_mappings, L, L, len(cl), cl.ctypes.data, recs.ctypes.data if len(recs) else None, len(recs),
                           rl.ctypes.data, len(rl), 0, LONG_MAX, out.ctypes.data, len(out))
    assert 0 <= n <= len(out)
    return out[:n]


def records_per_read(reads, recs):
    return np.bincount(recs["querySeqId"], minlength=len(reads))


def expected_counts(nrec, option):
    """chain_counts() / chain_long_counts() of the batch from its record histogram"""
    top = LONG_MAX if option else 16
    return (dict(offered=int((nrec > 0).sum()), finished=int(((nrec > 0) & (nrec <= top)).sum()), leftover=int(nrec[nrec > top].sum())),
            dict(offered=int((nrec > 16).sum()), finished=int(((nrec > 16) & (nrec <= LONG_MAX)).sum()) if option else 0))


def check_holds(reads, recs, rows):
    """the batch holds every case test_gpu_chain_long.py is about; rows: the host's rows of every read of at most 512 records
    (chainbatch.host_rows(..., max_records=512)).  Returns the names of the colinear reads whose row carries another member's
    conservedSketches than the first in key order."""
    names = [n for n, _ in reads]
    nrec = records_per_read(reads, recs)
    per = dict(zip(names, nrec.tolist()))
    other = []
    for name, nseg, strand in (("fwd17", 17, 1), ("fwd21", 21, 1), ("rc33", 33, -1)):
        i = names.index(name)
        rr, rw = recs[recs["querySeqId"] == i], rows[rows["querySeqId"] == i]
        assert len(rr) == nseg and len(set(rr["fragStart"].tolist())) == nseg, (name, len(rr))           # a record per fragment
        assert len(rw) == 1 and int(rw["n_merged"][0]) == nseg and int(rw["strand"][0]) == strand, (name, rw)   # one chain of all of them
        first = rr[np.lexsort((rr["fragStart"], rr["refStartPos"], rr["refSeqId"]))][0]                  # the first member in key order
        if int(rw["conservedSketches"][0]) != int(first["conservedSketches"]):
            other.append(name)
    assert len(dict(reads)["fwd21"]) % L != 0
    assert other, "no colinear read whose representative differs from the first member in key order"
    for name in ("array_two", "array_three"):
        i = names.index(name)
        assert 16 < per[name] <= LONG_MAX and len(rows[rows["querySeqId"] == i]) >= 1 and (recs[recs["querySeqId"] == i]["fragStart"] > 0).any()
    assert len(dict(reads)["array40_one"]) <= L and 16 < per["array40_one"] <= LONG_MAX                # one fragment
    two = recs[recs["querySeqId"] == names.index("array40_two")]
    per_fragment = np.bincount(two["fragStart"] // L)
    assert len(per_fragment) == 2 and per_fragment.min() > 16 and len(two) <= LONG_MAX
    assert per["array40_many"] > LONG_MAX
    assert per["unrelated"] == 0 and 0 < names.index("unrelated") < len(names) - 1
    assert nrec[names.index("unrelated") - 1] > 16 and nrec[names.index("unrelated") + 1] > 16            # between long ones
    assert set(range(2, 17)) & set(nrec.tolist()) and per["array_one"] <= 16 and 2 <= per["fwd2"] <= 16 and 2 <= per["fwd8"] <= 16
    assert 16 < nrec[-1] <= LONG_MAX                                                                     # a long read last
    return other
