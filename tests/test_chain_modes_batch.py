"""The batch of tests/test_gpu_chain_modes.py (tests/chainmodes.py) really holds every case that test is about -- checked here on the CPU,
from the oracle's candidate mappings under -Y '#' (oracle.session(..., b"#", ...)) and the host's rows (mmh_chain_rows_modes: MapPost with
skip_prefix, its refIdGroup and split), before any device sees it: reads whose chains stand in three groups over the same query
interval, one of them short enough for the one-thread kernel and two for the wave kernel, on both strands; two contigs of one group
competing inside a run; runs of one member; more than 16 records in each of two groups; a read above 512 records; a read that skips its
own group; and the --noSplit reads.  Runs without a GPU."""
import numpy as np
import pytest

import chainmodes as M
import mmutil as U


@pytest.fixture(scope="module")
def batch(oracle):
    contigs, reads, grp, read_grp = M.case()
    h = oracle.session(contigs, M.K, M.L, M.S, M.PI, U.FILTER_MAP, U.FLAG_SKIP_PREFIX, b"#", 0.0)
    try:
        recs = M.oracle_records(oracle, h, reads)
    finally:
        oracle.free(h)
    return [len(a) for _, a in contigs], contigs, reads, grp, recs


def test_the_batch_holds_every_case(batch):
    clens, _, reads, grp, recs = batch
    rows0, rows2 = M.host_rows(clens, reads, recs, 1, ref_group=grp), M.host_rows(clens, reads, recs, 3, ref_group=grp)
    print(dict(zip([n for n, _ in reads], M.records_per_read(reads, recs).tolist())), len(rows0), len(rows2))
    M.check_holds(reads, recs, rows0, rows2, grp)
    assert len(rows2) > len(rows0)
    cnt = M.group_counts(len(reads), rows0, grp)
    print(cnt)
    assert cnt["reads"] >= 10 and cnt["runs"] > 2 * cnt["reads"]


def test_groups_are_what_separates_the_rows(batch):
    """the same records without groups: one run a read, and of three chains over the same interval one row is left"""
    clens, _, reads, grp, recs = batch
    grouped, plain = M.host_rows(clens, reads, recs, 1, ref_group=grp), M.host_rows(clens, reads, recs, 1)
    i = [n for n, _ in reads].index("three")
    assert len(grouped[grouped["querySeqId"] == i]) == 3 and len(plain[plain["querySeqId"] == i]) == 1 and len(plain) < len(grouped)
    cnt = M.group_counts(len(reads), plain, None)
    assert cnt["reads"] == 0 and cnt["runs"] == len(set(plain["querySeqId"].tolist()))
    none = M.host_rows(clens, reads, recs, 1, U.FILTER_NONE, ref_group=grp)
    assert len(none) > len(grouped) and M.group_counts(len(reads), none, grp, U.FILTER_NONE) == dict(reads=0, runs=0)


@pytest.mark.parametrize("grouped", [False, True], ids=["nosplit", "nosplit_Y"])
def test_the_nosplit_reads(oracle, batch, grouped):
    """--noSplit: every read is one fragment; its row is the fragment's, n_merged 0, queryLen the read's length"""
    clens, contigs, _, grp, _ = batch
    reads = M.nosplit_reads(contigs)
    assert [len(a) for _, a in reads] == [600, 1000, 2500, 6000]
    flags = U.FLAG_NOSPLIT | (U.FLAG_SKIP_PREFIX if grouped else 0)
    h = oracle.session(contigs, M.K, M.L, M.S, M.PI, U.FILTER_MAP, flags, b"#" if grouped else b"\0", 0.0)
    try:
        recs = M.oracle_records(oracle, h, reads, split=False)
    finally:
        oracle.free(h)
    nrec = M.records_per_read(reads, recs)
    print(nrec.tolist())
    assert (nrec >= (3 if grouped else 1)).all() and (recs["fragStart"] == 0).all()
    assert (recs["fragLen"] == np.array([len(a) for _, a in reads])[recs["querySeqId"]]).all()
    rows = M.host_rows(clens, reads, recs, 1, ref_group=grp if grouped else None, split=False)
    assert len(rows) == (3 if grouped else 1) * len(reads)
    assert (rows["n_merged"] == 0).all() and (rows["queryStartPos"] == 0).all()
    assert (rows["queryLen"] == np.array([len(a) for _, a in reads])[rows["querySeqId"]]).all() and (rows["queryEndPos"] == rows["queryLen"]).all()
    split_rows = M.host_rows(clens, reads, recs, 1, ref_group=grp if grouped else None, split=True)                # the flag is what decides
    assert split_rows.tobytes() != rows.tobytes()
