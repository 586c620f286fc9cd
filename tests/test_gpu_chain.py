"""mm_chain_reads: the tail of Map::mapModule on the device -- every read's candidate mappings chained (mergeMappingsInRange), weeded
(filterWeakMappings) and filtered (filterByGroup, query axis) by k_chain_reads, one mm_chain_row per surviving mapping; a read with
more than 16 records is handed over with its records untouched.

One batch (tests/chainbatch.py) holds reads of 2 to 8 segments on both strands, a read with an insertion longer than chain_gap, reads
out of tandem copies (several records per fragment, identities that tie), a read shorter than a segment, a read of which one segment
maps, a read of twelve records, two reads with more than 16 (twelve tandem copies, two and three segments) and a read without any.
That it holds each of them is checked on the CPU from the oracle's records and the host stage (tests/test_chain_batch.py), and asserted
again here from the device's records (chainbatch.check_holds).

Per secondaryToKeep (0, 2), after a sized pass and after a steady-state one:
  counts        offered == reads with records, finished == those with at most 16
  rows          byte for byte the rows the host's own code leaves (mmh_chain_rows: MapPost::chainedFromRecords of every read of at most
                16 records) -- floats and the double kmerComplexity included
  left-over     byte for byte the records of the reads with more than 16, read-major, in their order
  end to end    rows + the host's result on the left-over records == the host's result on all downloaded records, field for field
                (mmh_post_chained both ways: coordinates, identities, n_merged, approxMatches), and == mmh_post_batch

Small shapes: k 16, segLength 1000, s 80, pi 0.85, kmerThreshold 0; three contigs of 60, 9 and 19 kbp; 21 reads."""
import os
import subprocess

import numpy as np
import pytest

import chainbatch as B
import mmutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BIN = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")


@pytest.fixture(scope="module")
def batch(oracle):
    """the case, the oracle session's index and tables (shared, unchanged)"""
    from mashmap_amd import capi
    contigs, reads = B.case()
    h = oracle.session(contigs, B.K, B.L, B.S, B.PI, U.FILTER_MAP, U.FLAG_HG, b"\0", 0.0)
    try:
        d = dict(contigs=contigs, reads=reads, ix=oracle.export_index(h), min_hits=oracle.min_hits_table(B.S, B.K, B.PI), cutoffs=oracle.cutoffs(h),
                 replay=capi.stat_replay_tables(B.S, B.K, B.PI, 0.0, True), identity=capi.stat_identity_table(B.S, B.K),
                 clens=[len(a) for _, a in contigs])
    finally:
        oracle.free(h)
    return d


def context(batch, flags=None, chain=None, tables=True):
    from mashmap_amd import capi
    ctx = capi.Context(k=B.K, segLength=B.L, sketchSize=B.S, flags=capi.MM_FLAG_HG_FILTER if flags is None else flags)
    ix = batch["ix"]
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"],
                     np.zeros(len(ix["contigLen"]), dtype=np.int32) if flags is not None and flags & capi.MM_FLAG_SKIP_PREFIX else None)
    ctx.set_tables(batch["min_hits"], batch["cutoffs"])
    if tables:
        ctx.set_replay_tables(*batch["replay"])
    if chain is not None:
        ctx.set_chain_tables(B.L, 1, chain, chain, True, capi.MM_CHAIN_FILTER_QUERY, 0.0, batch["identity"])
    return ctx


def check_pass(batch, ctx, keep, what):
    """one mapped pass of the context: mm_chain_reads against the host on the records the pass left"""
    reads, cl, nm = batch["reads"], batch["clens"], keep + 1
    recs = ctx.mappings()
    ctx.chain_reads()
    cnt, rows, left = ctx.chain_counts(), ctx.chain_rows(), ctx.chain_leftover()
    nrec = np.bincount(recs["querySeqId"], minlength=len(reads))
    print(what, cnt, "records per read", nrec.tolist())
    assert cnt == dict(offered=int((nrec > 0).sum()), finished=int(((nrec > 0) & (nrec <= 16)).sum()), rows=len(rows), leftover=len(left)), what
    assert cnt["offered"] - cnt["finished"] == 2 and cnt["finished"] >= 17
    assert left.tobytes() == recs[nrec[recs["querySeqId"]] > 16].tobytes(), what + ": left-over records"
    want = B.host_rows(cl, reads, recs, nm)
    assert len(rows) == len(want) and len(rows) >= 17, (what, len(rows), len(want))
    for i, (a, b) in enumerate(zip(rows, want)):
        assert a.tobytes() == b.tobytes(), (what, "row %d" % i, a, b)
    assert int(rows["pad"].max()) == 0 and (np.diff(rows["querySeqId"]) >= 0).all()               # read order
    allr, allm, alla = B.post(cl, reads, recs, None, nm)
    got, gotm, gota = B.post(cl, reads, left, rows, nm)
    assert got.tobytes() == allr.tobytes() and gotm.tobytes() == allm.tobytes() and gota.tobytes() == alla.tobytes(), what + ": rows + left-over against all records"
    assert B.post_batch(cl, reads, recs, nm).tobytes() == allr.tobytes()
    a, na, b, nb = ctx.chain_device()
    assert (na, nb) == (len(rows), len(left)) and a and b
    return recs, allr, allm


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0, 2], ids=["secondary0", "secondary2"])
def test_rows_and_left_over_records_against_the_host(batch, keep):
    ctx = context(batch, chain=keep)
    try:
        reads = batch["reads"]
        ctx.reads_upload([a for _, a in reads], None, [-1] * len(reads), 0)
        ctx.map()
        assert ctx.pass_stats()[1] is False
        recs, rep, merged = check_pass(batch, ctx, keep, "sized pass, secondaryToKeep %d" % keep)
        if keep == 0:
            B.check_holds(reads, recs, B.figures(reads, recs, rep, merged))                         # the batch holds every case, on the device's records too
        ctx.map()
        assert ctx.pass_stats()[1] is True, "the second pass of the same batch is a steady-state pass"
        recs2, rep2, _ = check_pass(batch, ctx, keep, "steady-state pass, secondaryToKeep %d" % keep)
        assert recs2.tobytes() == recs.tobytes() and rep2.tobytes() == rep.tobytes()
        if keep == 2:
            assert len(rep) > len(B.post(batch["clens"], reads, recs, None, 1)[0])                  # the secondaries are there
    finally:
        ctx.close()


@pytest.mark.gpu
def test_every_refusal_names_its_reason(batch):
    from mashmap_amd import capi
    reads = batch["reads"][:3]

    def refused(ctx, text, code=-3):
        with pytest.raises(capi.MashmapError) as e:
            ctx.chain_reads()
        assert "(%d)" % code in str(e.value) and text in str(e.value), str(e.value)

    ctx = context(batch, chain=0)                                                                    # nothing mapped
    refused(ctx, "nothing mapped")
    with pytest.raises(capi.MashmapError) as e:
        ctx.chain_counts()
    assert "mm_chain_counts: mm_chain_reads has not run" in str(e.value)
    with pytest.raises(capi.MashmapError) as e:
        ctx.chain_device()
    assert "mm_chain_device: mm_chain_reads has not run" in str(e.value)
    ctx.close()
    ctx = context(batch, chain=0, tables=False)                                                      # mapped, but no replay tables: no candidate mappings
    ctx.reads_upload([a for _, a in reads]); ctx.map()
    refused(ctx, "mm_set_replay_tables")
    ctx.close()
    ctx = context(batch)                                                                             # mm_set_chain_tables was not called
    ctx.reads_upload([a for _, a in reads]); ctx.map()
    refused(ctx, "mm_set_chain_tables was not called")
    with pytest.raises(capi.MashmapError) as e:                                                      # ... and refuses a chain gap beyond 1 << 25
        ctx.set_chain_tables((1 << 25) + 1, identity=batch["identity"])
    assert "(-1)" in str(e.value) and "chainGap" in str(e.value)
    with pytest.raises(capi.MashmapError) as e:                                                      # ... and a secondary count below -1 (-1 is a mapping count of 0)
        ctx.set_chain_tables(B.L, 1, -2, 0, identity=batch["identity"])
    assert "(-1)" in str(e.value) and "secondary" in str(e.value)
    ctx.set_chain_tables(1 << 25, 1, -1, -1, identity=batch["identity"])
    ctx.chain_reads()
    ctx.reads_upload([a for _, a in reads])                                                          # a new batch: the results of the old one are gone
    with pytest.raises(capi.MashmapError):
        ctx.chain_rows()
    ctx.close()
    for flag, text in ((capi.MM_FLAG_SKIP_PREFIX, "MM_FLAG_SKIP_PREFIX"), (capi.MM_FLAG_NO_SPLIT, "MM_FLAG_NO_SPLIT")):
        ctx = capi.Context(k=B.K, segLength=B.L, sketchSize=B.S, flags=capi.MM_FLAG_HG_FILTER | flag)   # what the context was created with is refused first
        ctx.set_chain_tables(B.L, identity=batch["identity"])
        refused(ctx, text)
        ctx.close()
    big = capi.Context(k=B.K, segLength=30000, sketchSize=2049)                                      # no index needed: the size is refused first
    with pytest.raises(capi.MashmapError) as e:
        big.set_chain_tables(B.L, identity=np.zeros(2050 * 2050, dtype=np.float32))
    assert "2048" in str(e.value)
    refused(big, "sketchSize above 2048")
    big.close()


@pytest.mark.gpu
def test_an_empty_batch_and_a_batch_without_records(batch):
    ctx = context(batch, chain=0)
    try:
        assert ctx.reads_upload([]) == 0
        ctx.map(); ctx.chain_reads()
        assert ctx.chain_counts() == dict(offered=0, finished=0, rows=0, leftover=0)
        assert len(ctx.chain_rows()) == 0 and len(ctx.chain_leftover()) == 0
        ctx.reads_upload([U.random_dna(8301, 2500), U.random_dna(8302, 700), U.random_dna(8303, 10)])
        ctx.map(); ctx.chain_reads()
        assert len(ctx.mappings()) == 0 and ctx.chain_counts() == dict(offered=0, finished=0, rows=0, leftover=0)
    finally:
        ctx.close()


# (case of tests/golden/cases.py, argv in place of the case's or None, golden PAF to compare with or None)
COMMAND_LINES = {"default": ("default", None, "default"), "pi90_n2": ("pi90_n2", None, "pi90_n2"),
                 "reads_one2one": ("default", ["-f", "one-to-one"], None),      # 10 kbp reads at segLength 5000: two records a read, every read finished on the device
                 "asm_one2one": ("asm_one2one", None, "asm_one2one")}           # whole contigs at segLength 10000: dozens of records a read, handed over


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(COMMAND_LINES))
def test_command_line_paf_is_the_same_with_the_switch(name, tmp_path):
    """mashmap_hip with MASHMAP_HIP_DEVICE_CHAIN set writes the PAF it writes without it (and the stock binary's where tests/golden/paf has
    it), in filter mode map (`default`, and `--pi 90 -n 2` with a secondary) and one-to-one.  The device-stage timing lines say how many
    chained rows and left-over records came back: in `default`, `pi90_n2` and `reads_one2one` rows did (MapPost::finishRows ran), in
    `asm_one2one` left-over records did (contigs as reads have more than 16 records)"""
    import re
    from golden import cases as CS
    assert os.path.exists(HIP_BIN), "mashmap_hip not built (python -c 'import __graft_entry__ as g; g.build()')"
    case, argv, golden = COMMAND_LINES[name]
    _, refrec, qrec, extra = {c[0]: c for c in CS.paf_cases()}[case]
    extra = extra if argv is None else argv
    rf, qf = str(tmp_path / "ref.fa"), str(tmp_path / "q.fa")
    U.write_fasta(rf, refrec); U.write_fasta(qf, qrec)
    outs = {}
    for tag, env in (("off", {}), ("on", {"MASHMAP_HIP_DEVICE_CHAIN": "1", "MASHMAP_HIP_TIMING": "1"})):
        out = str(tmp_path / (tag + ".paf"))
        e = {k: v for k, v in os.environ.items() if k != "MASHMAP_HIP_DEVICE_CHAIN"}
        e.update(env)
        p = subprocess.run([HIP_BIN, "-r", rf, "-q", qf, "-o", out, "-t", "4"] + extra, capture_output=True, text=True, env=e, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[tag] = open(out, "rb").read()
        if tag == "on":
            assert "chaining on the device" in p.stderr, p.stderr[-2000:]
            back = re.findall(r"download of (\d+) left-over candidate mappings and (\d+) chained rows\)", p.stderr)
            left, rows = sum(int(a) for a, _ in back), sum(int(b) for _, b in back)
            print(name, "left-over records", left, "chained rows", rows)
            assert back and (left > 16 if name == "asm_one2one" else rows > 0), (name, back)
    assert len(outs["off"]) > 0 and outs["off"].count(b"\n") >= 3
    if golden:
        assert outs["off"] == open(os.path.join(ROOT, "tests", "golden", "paf", golden + ".paf"), "rb").read()
    assert outs["on"] == outs["off"], (outs["on"][:300], outs["off"][:300])
