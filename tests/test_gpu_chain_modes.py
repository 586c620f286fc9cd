"""MM_OPT_CHAIN_MODES: mm_chain_reads on a context created with MM_FLAG_SKIP_PREFIX (-Y: filterByGroup runs reference group by
reference group, from the index's refGroup array), MM_FLAG_NO_SPLIT (--noSplit: no read is split) or both; mm_chain_group_counts.

One -Y batch (tests/chainmodes.py; that it holds each case is checked on the CPU by tests/test_chain_modes_batch.py and asserted again
here from the device's records): reads whose chains stand in three groups over the same query interval -- nine records for the
one-thread kernel, 27 and more for the wave kernel, both strands --, two contigs of one group competing inside a run, a read shorter
than a segment, reads with one record and with none, more than 16 records in each of two groups, a read above 512 records, a read
uploaded with its own group.

  rows        byte for byte the host's (mmh_chain_rows_modes: MapPost::chainedFromRecords with skip_prefix, refIdGroup and split)
  left-over   byte for byte the records of the reads above 512 (above 16 without MM_OPT_CHAIN_LONG)
  counts      chain_counts() and chain_long_counts() from the record histogram, chain_group_counts() from the host's rows and refGroup
with the option off (refused, in the words of before), on, off and on again, after a second map(); without MM_OPT_CHAIN_LONG, on a
context whose index came through mm_index_replicate; --noSplit alone and with -Y; filter none; and the command line with
MASHMAP_HIP_DEVICE_CHAIN=all.

Small shapes: k 16, segLength 1000, s 80, pi 0.85; six contigs, about 200 kbp, four groups; 16 reads, about 800 records."""
import os
import re
import subprocess

import numpy as np
import pytest

import chainmodes as M
import mmutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BIN = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
REFUSED_Y = "mm_chain_reads: MM_FLAG_SKIP_PREFIX is set (filterByGroup then runs reference group by reference group)"
REFUSED_NOSPLIT = "mm_chain_reads: MM_FLAG_NO_SPLIT is set"


@pytest.fixture(scope="module")
def batch(oracle):
    """the case, the oracle session's index and tables (shared, unchanged)"""
    from mashmap_amd import capi
    contigs, reads, grp, read_grp = M.case()
    h = oracle.session(contigs, M.K, M.L, M.S, M.PI, U.FILTER_MAP, U.FLAG_SKIP_PREFIX, b"#", 0.0)
    try:
        d = dict(contigs=contigs, reads=reads, grp=grp, read_grp=read_grp, ix=oracle.export_index(h), min_hits=oracle.min_hits_table(M.S, M.K, M.PI),
                 cutoffs=oracle.cutoffs(h), replay=capi.stat_replay_tables(M.S, M.K, M.PI, 0.0, True), identity=capi.stat_identity_table(M.S, M.K),
                 clens=[len(a) for _, a in contigs])
    finally:
        oracle.free(h)
    return d


def context(batch, flags, keep=0, filt=None, replica_of=None):
    from mashmap_amd import capi
    ctx = capi.Context(k=M.K, segLength=M.L, sketchSize=M.S, flags=flags)
    ix = batch["ix"]
    if replica_of is not None:
        ctx.index_replicate_from(replica_of)
    else:
        ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"],
                         np.array(batch["grp"], dtype=np.int32) if flags & capi.MM_FLAG_SKIP_PREFIX else None)
    ctx.set_tables(batch["min_hits"], batch["cutoffs"])
    ctx.set_replay_tables(*batch["replay"])
    ctx.set_chain_tables(M.L, 1, keep, keep, True, capi.MM_CHAIN_FILTER_QUERY if filt is None else filt, 0.0, batch["identity"])
    return ctx


def refused(ctx, text):
    from mashmap_amd import capi
    with pytest.raises(capi.MashmapError) as e:
        ctx.chain_reads()
    assert "(-3)" in str(e.value) and text in str(e.value), str(e.value)
    with pytest.raises(capi.MashmapError):
        ctx.chain_group_counts()


def check_on(batch, ctx, reads, keep, what, grp, split=True, long_on=True, filter_mode=U.FILTER_MAP):
    """chain_reads() of the mapped batch with the option set, against the host on the records the pass left; -> (records, rows, left-over)"""
    cl, nm, top = batch["clens"], keep + 1, (M.LONG_MAX if long_on else 16)
    recs = ctx.mappings()
    ctx.chain_reads()
    cnt, lcnt, gcnt, rows, left = ctx.chain_counts(), ctx.chain_long_counts(), ctx.chain_group_counts(), ctx.chain_rows(), ctx.chain_leftover()
    nrec = M.records_per_read(reads, recs)
    print(what, cnt, lcnt, gcnt, "records per read", nrec.tolist())
    want_cnt, want_long = M.expected_counts(nrec, long_on)
    assert cnt == dict(want_cnt, rows=len(rows)) and lcnt == want_long, what
    assert left.tobytes() == recs[nrec[recs["querySeqId"]] > top].tobytes(), what + ": left-over records"
    want = M.host_rows(cl, reads, recs, nm, filter_mode, grp, split, top)
    assert len(rows) == len(want), (what, len(rows), len(want))
    for i, (a, b) in enumerate(zip(rows, want)):
        assert a.tobytes() == b.tobytes(), (what, "row %d" % i, a, b)
    assert (len(rows) == 0 or int(rows["pad"].max()) == 0) and (np.diff(rows["querySeqId"]) >= 0).all()          # read order
    assert gcnt == M.group_counts(len(reads), want, grp, filter_mode), (what, gcnt)
    return recs, rows, left


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0, 2], ids=["secondary0", "secondary2"])
def test_reference_groups_are_filtered_run_by_run_on_the_device(batch, keep):
    """-Y with MM_OPT_CHAIN_LONG: option off, on, off, on; then a second map() of the same batch"""
    from mashmap_amd import capi
    reads, grp, cl = batch["reads"], batch["grp"], batch["clens"]
    ctx = context(batch, capi.MM_FLAG_SKIP_PREFIX, keep)
    try:
        ctx.chain_long()
        ctx.reads_upload([a for _, a in reads], batch["read_grp"], [-1] * len(reads), 0)
        ctx.map()
        refused(ctx, REFUSED_Y)                                                                      # off: the refusal of before, word for word
        ctx.chain_modes()
        recs, rows, left = check_on(batch, ctx, reads, keep, "-Y, option on, secondaryToKeep %d" % keep, grp)
        nrec = M.records_per_read(reads, recs)
        gcnt = ctx.chain_group_counts()
        assert gcnt["reads"] > 0 and gcnt["runs"] > gcnt["reads"]
        assert 0 < len(left) == int(nrec[nrec > M.LONG_MAX].sum())
        # the batch holds every case, on the device's records too: rows per group, the competing pair, the long reads being long
        M.check_holds(reads, recs, M.host_rows(cl, reads, recs, 1, ref_group=grp), M.host_rows(cl, reads, recs, 3, ref_group=grp), grp)
        plain = M.host_rows(cl, reads, recs, keep + 1)                                               # without groups the rows are others
        assert len(plain) < len(rows)

        ctx.chain_modes(False)
        refused(ctx, REFUSED_Y)
        ctx.chain_modes()
        ctx.chain_reads()
        assert ctx.chain_rows().tobytes() == rows.tobytes() and ctx.chain_leftover().tobytes() == left.tobytes() and ctx.chain_group_counts() == gcnt

        ctx.map()
        recs2, rows2, left2 = check_on(batch, ctx, reads, keep, "-Y, second map(), secondaryToKeep %d" % keep, grp)
        assert recs2.tobytes() == recs.tobytes() and rows2.tobytes() == rows.tobytes() and left2.tobytes() == left.tobytes()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_reference_groups_without_the_long_kernel_and_on_a_replicated_index(batch):
    """without MM_OPT_CHAIN_LONG reads above 16 records are handed over and the others' rows are the host's; the same on a context that
    got its index, refGroup included, through mm_index_replicate"""
    from mashmap_amd import capi
    reads, grp = batch["reads"], batch["grp"]
    src = context(batch, capi.MM_FLAG_SKIP_PREFIX, 0)
    ctx = None
    try:
        out = []
        for c, what in ((src, "uploaded index"), (None, "replicated index")):
            if c is None:
                ctx = c = context(batch, capi.MM_FLAG_SKIP_PREFIX, 0, replica_of=src)
            c.chain_modes()
            c.reads_upload([a for _, a in reads], batch["read_grp"], [-1] * len(reads), 0)
            c.map()
            recs, rows, left = check_on(batch, c, reads, 0, "-Y without MM_OPT_CHAIN_LONG, " + what, grp, long_on=False)
            nrec = M.records_per_read(reads, recs)
            assert len(left) == int(nrec[nrec > 16].sum()) > M.LONG_MAX and int((nrec > 16).sum()) >= 6 and len(rows) >= 20
            out.append((recs.tobytes(), rows.tobytes(), left.tobytes()))
        assert out[0] == out[1]
    finally:
        if ctx is not None:
            ctx.close()
        src.close()


@pytest.mark.gpu
@pytest.mark.parametrize("grouped", [False, True], ids=["nosplit", "nosplit_Y"])
def test_no_read_is_split_under_no_split(batch, grouped):
    """MM_FLAG_NO_SPLIT alone and with MM_FLAG_SKIP_PREFIX: reads of 600, 1 000, 2 500 and 6 000 bp are one fragment each"""
    from mashmap_amd import capi
    reads = M.nosplit_reads(batch["contigs"])
    grp = batch["grp"] if grouped else None
    ctx = context(batch, capi.MM_FLAG_NO_SPLIT | (capi.MM_FLAG_SKIP_PREFIX if grouped else 0), 0)
    try:
        ctx.chain_long()
        ctx.reads_upload([a for _, a in reads], [-1] * len(reads), [-1] * len(reads), 0)
        ctx.map()
        refused(ctx, REFUSED_Y if grouped else REFUSED_NOSPLIT)                                      # SKIP_PREFIX is named first, as before
        ctx.chain_modes()
        recs, rows, left = check_on(batch, ctx, reads, 0, "--noSplit" + (" -Y" if grouped else ""), grp, split=False)
        lens = np.array([len(a) for _, a in reads])
        assert [len(a) for _, a in reads] == [600, 1000, 2500, 6000] and len(left) == 0
        assert len(rows) == (3 if grouped else 1) * len(reads) and (rows["n_merged"] == 0).all()
        assert (rows["queryLen"] == lens[rows["querySeqId"]]).all() and (rows["queryStartPos"] == 0).all() and (rows["queryEndPos"] == rows["queryLen"]).all()
        assert ctx.chain_group_counts() == dict(reads=len(reads) if grouped else 0, runs=len(rows))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_filter_none_counts_no_run(batch):
    """MM_CHAIN_FILTER_NONE under -Y: every chain of every group is a row, no run is swept or passed through"""
    from mashmap_amd import capi
    reads, grp = batch["reads"], batch["grp"]
    ctx = context(batch, capi.MM_FLAG_SKIP_PREFIX, 0, capi.MM_CHAIN_FILTER_NONE)
    try:
        ctx.chain_long(); ctx.chain_modes()
        ctx.reads_upload([a for _, a in reads], batch["read_grp"], [-1] * len(reads), 0)
        ctx.map()
        _, rows, _ = check_on(batch, ctx, reads, 0, "-Y, filter none", grp, filter_mode=U.FILTER_NONE)
        assert ctx.chain_group_counts() == dict(reads=0, runs=0)
        assert len(rows) > len(M.host_rows(batch["clens"], reads, ctx.mappings(), 1, ref_group=grp))
    finally:
        ctx.close()


def run_cli(tmp_path, name, refrec, qrec, extra, tag, value):
    rf, qf, out = str(tmp_path / (name + ".ref.fa")), str(tmp_path / (name + ".q.fa")), str(tmp_path / ("%s.%s.paf" % (name, tag)))
    if not os.path.exists(rf):
        U.write_fasta(rf, refrec)
        if qrec is not None:
            U.write_fasta(qf, qrec)
    e = {k: v for k, v in os.environ.items() if k != "MASHMAP_HIP_DEVICE_CHAIN"}
    e["MASHMAP_HIP_TIMING"] = "1"
    if value is not None:
        e["MASHMAP_HIP_DEVICE_CHAIN"] = value
    p = subprocess.run([HIP_BIN, "-r", rf, "-o", out, "-t", "4"] + extra + (["-q", qf] if qrec is not None else []), capture_output=True, text=True, env=e, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return open(out, "rb").read(), p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["allvsall_Y", "nosplit", "nosplit_pi90_n3"])
def test_command_line_with_the_value_all(tmp_path, name):
    """golden cases under -Y '#' and --noSplit (tests/golden/cases.py) with MASHMAP_HIP_DEVICE_CHAIN=all: the PAF of the run without the
    switch and of the stock binary; where the stage runs (a sketch of at most 2048) the timing lines show chained rows and group runs.
    With the value `long` the switch does nothing under -Y and --noSplit, as before"""
    from golden import cases as CS
    assert os.path.exists(HIP_BIN), "mashmap_hip not built (python -c 'import __graft_entry__ as g; g.build()')"
    _, refrec, qrec, extra = {c[0]: c for c in CS.paf_cases()}[name]
    off, err0 = run_cli(tmp_path, name, refrec, qrec, extra, "off", None)
    assert "chaining on the device" not in err0 and off.count(b"\n") >= 3
    golden = os.path.join(ROOT, "tests", "golden", "paf", name + ".paf")
    if os.path.exists(golden):
        assert off == open(golden, "rb").read()
    on, err = run_cli(tmp_path, name, refrec, qrec, extra, "all", "all")
    assert on == off, (on[:300], off[:300])
    if "chaining on the device" in err:
        back = re.findall(r"download of (\d+) left-over candidate mappings and (\d+) chained rows\)", err)
        runs = re.findall(r"\[(\d+) group runs filtered on the device, (\d+) reads with more than one\]", err)
        lng = re.findall(r"\[(\d+) of (\d+) reads of more than 16 records chained on the device\]", err)
        assert back and len(runs) == len(back) == len(lng), err[-2000:]
        n_rows, n_runs, n_multi = sum(int(b) for _, b in back), sum(int(a) for a, _ in runs), sum(int(b) for _, b in runs)
        print(name, "left-over records", sum(int(a) for a, _ in back), "chained rows", n_rows, "group runs", n_runs, "reads with several", n_multi, "long", lng)
        assert n_rows > 0 and n_runs > 0 and n_rows >= n_runs
        assert (n_multi > 0) == ("-Y" in extra)
    else:                                                                                            # a sketch above 2048: the switch did nothing
        print(name, "the stage did not run")
        assert "chained rows" not in err and "group runs" not in err
    lng_paf, err_long = run_cli(tmp_path, name, refrec, qrec, extra, "long", "long")
    assert lng_paf == off and "chaining on the device" not in err_long and "chained rows" not in err_long
