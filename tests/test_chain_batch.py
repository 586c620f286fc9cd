"""The batch of tests/test_gpu_chain.py (tests/chainbatch.py) really holds every case that test is about -- checked here on the CPU,
from the oracle's candidate mappings and the host stage (mmh_post_batch, mmh_post_chained, mmh_chain_rows), before any device sees it:
reads of 2 to 8 segments on both strands that chain over every full segment, an insertion longer than chain_gap that leaves two
chains, tandem copies with several records per fragment whose identities tie, a read shorter than a segment, a read of which one
segment maps (dropped by filterWeakMappings), a read of twelve records, two reads with more than 16, a read without any.  Also on the
host alone: the rows of the reads of at most 16 records plus the records of the others give what all records give.  Runs without a GPU."""
import numpy as np
import pytest

import chainbatch as B
import mmutil as U


@pytest.fixture(scope="module")
def batch(oracle):
    contigs, reads = B.case()
    h = oracle.session(contigs, B.K, B.L, B.S, B.PI, U.FILTER_MAP, U.FLAG_HG, b"\0", 0.0)
    try:
        recs = B.oracle_records(oracle, h, reads)
    finally:
        oracle.free(h)
    return [len(a) for _, a in contigs], reads, recs


def test_the_batch_holds_every_case(batch):
    clens, reads, recs = batch
    rep, merged, _ = B.post(clens, reads, recs, None, 1)
    per = B.figures(reads, recs, rep, merged)
    print(per)
    B.check_holds(reads, recs, per)
    assert B.post_batch(clens, reads, recs, 1).tobytes() == rep.tobytes()              # the stage as it was says the same


@pytest.mark.parametrize("num_mappings", [1, 3], ids=["secondary0", "secondary2"])
def test_rows_plus_left_over_records_are_all_records_on_the_host(batch, num_mappings):
    clens, reads, recs = batch
    nrec = np.bincount(recs["querySeqId"], minlength=len(reads))
    rows = B.host_rows(clens, reads, recs, num_mappings)
    left = recs[nrec[recs["querySeqId"]] > 16]
    assert len(rows) >= 17 and len(left) == int(nrec[nrec > 16].sum()) > 32
    want = B.post(clens, reads, recs, None, num_mappings)
    got = B.post(clens, reads, left, rows, num_mappings)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
