"""Every device buffer of the library is a DevBuf (mashmap_amd/csrc/mm_devbuf.h) that frees itself: what a context, an index build or a
failed call allocated is back when the context is closed -- measured with mm_device_bytes (capi.device_bytes()), the library's own count
of the bytes its buffers hold, not with the shared device's free memory.

Each test takes its base after a gc.collect(): a context an earlier test left to the garbage collector is destroyed before, not during,
the test.  Small shapes: k 16, segLength 1000, s 80 (the batch of tests/test_gpu_chain_long.py); k 19, segLength 5000, s 130 for the
two contexts on one device."""
import gc

import numpy as np
import pytest

import chainlong as CL
import mmutil as U
from test_gpu_chain_long import batch, context  # noqa: F401  (the module-scoped batch fixture and the context recipe)

pytestmark = pytest.mark.gpu


def base_bytes():
    from mashmap_amd import capi
    gc.collect()
    return capi.device_bytes()


def test_everything_a_context_allocates_comes_back(batch):  # noqa: F811
    """upload, map, chain_reads with MM_OPT_CHAIN_LONG, a parked batch beside a second resident one, index_download: all of it is
    freed by close().  Before DevBuf owned its memory mm_destroy freed the buffers of a hand-written list, and the same sequence left
    the two buffers of the chain-long stage (dChainLongList, dChainStage) behind; that version has no counter, so the sequence cannot
    be measured there."""
    from mashmap_amd import capi
    base = base_bytes()
    reads = batch["reads"]
    ctx = context(batch, 0)
    try:
        ctx.chain_long()
        ctx.reads_upload([a for _, a in reads], None, [-1] * len(reads), 0)
        ctx.map()
        ctx.chain_reads()
        assert ctx.chain_long_counts()["finished"] > 0                     # the chain-long stage ran: its list and staging rows exist
        resident = capi.device_bytes()
        ctx.reads_exchange(0)                                              # parks the batch: no copy, nothing allocated or freed
        assert capi.device_bytes() == resident
        two = [reads[i] for i in (6, 1)]
        ctx.reads_upload([a for _, a in two], None, [-1] * len(two), 0)
        ctx.map()
        assert capi.device_bytes() > resident                              # a second batch beside the parked one
        ix = ctx.index_download()
        assert len(ix["minmers"]) == len(batch["ix"]["minmers"])
        assert capi.device_bytes() > base
    finally:
        ctx.close()
    assert capi.device_bytes() == base


def test_the_scratch_of_an_index_build_is_gone_when_it_returns():
    """a second mm_index_build of the same contigs leaves the count where the first left it: the grow-only buffers of the index are
    large enough, and every temporary of the build -- hashing buffers, winnow scratch, sort keys -- was freed on the way"""
    from mashmap_amd import capi
    base = base_bytes()
    contigs = [U.random_dna(9101, 60000), U.random_dna(9102, 40000)]
    ctx = capi.Context(k=CL.K, segLength=CL.L, sketchSize=CL.S)
    try:
        ctx.index_build(contigs, kmerPct=0.001)
        first = ctx.index_download()                                       # the mirrors of a device-built index: scratch of their own
        after_first = capi.device_bytes()
        assert after_first > base and len(first["minmers"]) > 100
        ctx.index_build(contigs, kmerPct=0.001)
        assert capi.device_bytes() == after_first
        again = ctx.index_download()
        assert again["minmers"].tobytes() == first["minmers"].tobytes() and again["points"].tobytes() == first["points"].tobytes()
        assert capi.device_bytes() == after_first
    finally:
        ctx.close()
    assert capi.device_bytes() == base


def test_an_input_error_frees_its_scratch(batch):  # noqa: F811
    """mm_index_upload of a minmerIndex that is not grouped by ascending seqId: the MM_ERR_ARG of mm_flatten_device_index (an argument
    check on the records, no device fault), returned past the uploaded records and the scratch of the flattening"""
    from mashmap_amd import capi
    base = base_bytes()
    ix = batch["ix"]
    mins = np.array(ix["minmers"], dtype=capi.MINMER_DT)
    edge = int(np.flatnonzero(np.diff(mins["seqId"]) != 0)[0])              # the last record of a contig and the first of the next
    mins[[edge, edge + 1]] = mins[[edge + 1, edge]]
    ctx = capi.Context(k=CL.K, segLength=CL.L, sketchSize=CL.S, flags=capi.MM_FLAG_HG_FILTER)
    try:
        with pytest.raises(capi.MashmapError, match="not grouped by ascending seqId"):
            ctx.index_upload(mins, ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"], None)
    finally:
        ctx.close()
    assert capi.device_bytes() == base


def test_two_contexts_on_one_device():
    """as tests/test_gpu_multigpu.py: an index built on one context and replicated to the other, a local group, a sharded batch whose
    gathered records are the single context's byte for byte -- and both contexts give everything back"""
    from mashmap_amd import capi, shard
    base = base_bytes()
    contigs = [U.random_dna(9111, 120000), U.random_dna(9112, 80000)]
    reads = [a for _, a, _ in U.sample_reads(contigs, 9113, 12, 10000, 0.10)] + [U.random_dna(9114, 300)]
    ctxs = [capi.Context(k=19, segLength=5000, sketchSize=130, device=0) for _ in range(2)]
    try:
        ctxs[0].index_build(contigs, kmerPct=0.001)
        ctxs[1].index_replicate_from(ctxs[0])
        for c in ctxs:
            c.set_tables_default(0.85)
        ctxs[0].reads_upload(reads, seqCounterBase=100)
        ctxs[0].map()
        single = ctxs[0].mappings()
        assert len(single) >= 12
        capi.comm_init_local(ctxs)
        blocks = [shard.read_block_by_bases([len(r) for r in reads], r, len(ctxs)) for r in range(len(ctxs))]
        for c, (a, b) in zip(ctxs, blocks):
            c.reads_upload(reads[a:b], seqCounterBase=100 + a)
            c.map()
        capi.allgatherv_mappings_local(ctxs)
        for c in ctxs:
            got, counts = c.gathered(len(ctxs))
            assert counts.sum() == len(single) and got.tobytes() == single.tobytes()
        both = capi.device_bytes()
        ctxs[1].close()
        assert base < capi.device_bytes() < both
    finally:
        for c in ctxs:
            c.close()
    assert capi.device_bytes() == base
