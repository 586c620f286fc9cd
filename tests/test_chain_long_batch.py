"""The batch of tests/test_gpu_chain_long.py (tests/chainlong.py) really holds every case that test is about -- checked here on the CPU,
from the oracle's candidate mappings and the host stage (mmh_chain_rows, mmh_post_chained), before any device sees it: colinear reads
of 17, 21 and 33 segments (the last on the reverse strand) that come out as one chain each, at least one of them with a
representative that is not the first member in key order (introsort's doing: a stable sort would report another conservedSketches);
reads out of tandem arrays with interleaved chains; a read of one fragment and a read of two fragments with more than 16 records per
fragment; a read with more than 512 records; reads of 2 to 16 records; a read without records between long ones; a long read last.
Also on the host alone: the rows of the reads of at most 512 records plus the records of the others give what all records give.
Runs without a GPU."""
import numpy as np
import pytest

import chainbatch as B
import chainlong as CL
import mmutil as U


@pytest.fixture(scope="module")
def batch(oracle):
    contigs, reads = CL.case()
    h = oracle.session(contigs, CL.K, CL.L, CL.S, CL.PI, U.FILTER_MAP, U.FLAG_HG, b"\0", 0.0)
    try:
        recs = B.oracle_records(oracle, h, reads)
    finally:
        oracle.free(h)
    return [len(a) for _, a in contigs], reads, recs


def test_the_batch_holds_every_case(batch):
    clens, reads, recs = batch
    nrec = CL.records_per_read(reads, recs)
    print(dict(zip([n for n, _ in reads], nrec.tolist())))
    rows = B.host_rows(clens, reads, recs, 1, max_records=CL.LONG_MAX)
    other = CL.check_holds(reads, recs, rows)
    print("representative is not the first member in key order:", other)
    cnt, lcnt = CL.expected_counts(nrec, True)
    assert lcnt["offered"] >= 8 and lcnt["finished"] == lcnt["offered"] - 1 and cnt["finished"] == cnt["offered"] - 1


@pytest.mark.parametrize("num_mappings", [1, 3], ids=["secondary0", "secondary2"])
def test_rows_of_reads_up_to_512_records_plus_the_rest_are_all_records_on_the_host(batch, num_mappings):
    clens, reads, recs = batch
    nrec = CL.records_per_read(reads, recs)
    rows = B.host_rows(clens, reads, recs, num_mappings, max_records=CL.LONG_MAX)
    left = recs[nrec[recs["querySeqId"]] > CL.LONG_MAX]
    assert len(left) > CL.LONG_MAX and len(rows) > len(B.host_rows(clens, reads, recs, num_mappings))
    want = B.post(clens, reads, recs, None, num_mappings)
    got = B.post(clens, reads, left, rows, num_mappings)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
