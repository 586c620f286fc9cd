"""MM_OPT_CHAIN_LONG: mm_chain_reads no longer hands over a read of 17 .. 512 candidate mappings -- k_chain_reads_long, one wave per read
with the working set in LDS and libstdc++'s std::sort restated move for move (mm_stdsort.h), chains and filters it; only reads above
512 records are handed over.

One batch (tests/chainlong.py; that it holds each case is checked on the CPU by tests/test_chain_long_batch.py and asserted again here
from the device's records): colinear reads of 17, 21 and 33 segments -- whose representative, hence conservedSketches of the row, is
the member introsort leaves in front --, reads out of tandem arrays with interleaved chains, one and two fragments with more than 16
records each, a read with more than 512 records, reads of 2 to 16 records, a read without any, a long read last.

  rows        byte for byte the host's (mmh_chain_rows: MapPost::chainedFromRecords of every read of at most 512 records)
  left-over   byte for byte the records of the reads with more than 512
  counts      chain_counts() and chain_long_counts() from the record histogram
  end to end  rows + the host's result on the left-over records == the host's result on all records (mmh_post_chained, mmh_post_batch)
with the option on, off and on again on one context, after a sized and a steady-state pass, for a smaller batch after a larger one,
secondaryToKeep 0 and 2, filter none; and the command line with MASHMAP_HIP_DEVICE_CHAIN=long.

Small shapes: k 16, segLength 1000, s 80, pi 0.85; contigs of 60, 19 and 50 kbp; 14 reads, about 1 000 records."""
import os
import re
import subprocess

import numpy as np
import pytest

import chainbatch as B
import chainlong as CL
import mmutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BIN = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")


@pytest.fixture(scope="module")
def batch(oracle):
    """the case, the oracle session's index and tables (shared, unchanged)"""
    from mashmap_amd import capi
    contigs, reads = CL.case()
    h = oracle.session(contigs, CL.K, CL.L, CL.S, CL.PI, U.FILTER_MAP, U.FLAG_HG, b"\0", 0.0)
    try:
        d = dict(contigs=contigs, reads=reads, ix=oracle.export_index(h), min_hits=oracle.min_hits_table(CL.S, CL.K, CL.PI), cutoffs=oracle.cutoffs(h),
                 replay=capi.stat_replay_tables(CL.S, CL.K, CL.PI, 0.0, True), identity=capi.stat_identity_table(CL.S, CL.K),
                 clens=[len(a) for _, a in contigs])
    finally:
        oracle.free(h)
    return d


def context(batch, keep=0, filt=None):
    from mashmap_amd import capi
    ctx = capi.Context(k=CL.K, segLength=CL.L, sketchSize=CL.S, flags=capi.MM_FLAG_HG_FILTER)
    ix = batch["ix"]
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"], None)
    ctx.set_tables(batch["min_hits"], batch["cutoffs"])
    ctx.set_replay_tables(*batch["replay"])
    ctx.set_chain_tables(CL.L, 1, keep, keep, True, capi.MM_CHAIN_FILTER_QUERY if filt is None else filt, 0.0, batch["identity"])
    return ctx


def check_on(batch, ctx, reads, keep, what, filter_mode=U.FILTER_MAP):
    """chain_reads() of the mapped batch with the option set, against the host on the records the pass left; -> (records, rows, left-over)"""
    cl, nm = batch["clens"], keep + 1
    recs = ctx.mappings()
    ctx.chain_reads()
    cnt, lcnt, rows, left = ctx.chain_counts(), ctx.chain_long_counts(), ctx.chain_rows(), ctx.chain_leftover()
    nrec = CL.records_per_read(reads, recs)
    print(what, cnt, lcnt, "records per read", nrec.tolist())
    want_cnt, want_long = CL.expected_counts(nrec, True)
    assert cnt == dict(want_cnt, rows=len(rows)) and lcnt == want_long, what
    assert left.tobytes() == recs[nrec[recs["querySeqId"]] > CL.LONG_MAX].tobytes(), what + ": left-over records"
    want = CL.host_rows(cl, reads, recs, nm, filter_mode)
    assert len(rows) == len(want), (what, len(rows), len(want))
    for i, (a, b) in enumerate(zip(rows, want)):
        assert a.tobytes() == b.tobytes(), (what, "row %d" % i, a, b)
    assert (len(rows) == 0 or int(rows["pad"].max()) == 0) and (np.diff(rows["querySeqId"]) >= 0).all()          # read order
    allr, allm, alla = B.post(cl, reads, recs, None, nm, filter_mode=filter_mode)
    got, gotm, gota = B.post(cl, reads, left, rows, nm, filter_mode=filter_mode)
    assert got.tobytes() == allr.tobytes() and gotm.tobytes() == allm.tobytes() and gota.tobytes() == alla.tobytes(), what + ": rows + left-over against all records"
    if filter_mode == U.FILTER_MAP:
        assert B.post_batch(cl, reads, recs, nm).tobytes() == allr.tobytes()
    return recs, rows, left


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0, 2], ids=["secondary0", "secondary2"])
def test_long_reads_are_chained_on_the_device(batch, keep):
    """option on (sized pass), off, on again, then a steady-state pass: num_mappings 1 and 3"""
    ctx = context(batch, keep)
    try:
        reads, cl = batch["reads"], batch["clens"]
        ctx.chain_long()
        ctx.reads_upload([a for _, a in reads], None, [-1] * len(reads), 0)
        ctx.map()
        assert ctx.pass_stats()[1] is False
        recs, rows, left = check_on(batch, ctx, reads, keep, "sized pass, option on, secondaryToKeep %d" % keep)
        nrec = CL.records_per_read(reads, recs)
        if keep == 0:
            other = CL.check_holds(reads, recs, rows)                                                # the batch holds every case, on the device's records too
            print("representative is not the first member in key order:", other)
        assert 0 < len(left) == int(nrec[nrec > CL.LONG_MAX].sum()) and int(((nrec > 16) & (nrec <= CL.LONG_MAX)).sum()) >= 7

        ctx.chain_long(False)                                                                        # off: the counts and bytes of today
        ctx.chain_reads()
        cnt, lcnt, rows_off, left_off = ctx.chain_counts(), ctx.chain_long_counts(), ctx.chain_rows(), ctx.chain_leftover()
        want_cnt, want_long = CL.expected_counts(nrec, False)
        assert cnt == dict(want_cnt, rows=len(rows_off)) and lcnt == want_long and lcnt["finished"] == 0 and lcnt["offered"] >= 8
        assert left_off.tobytes() == recs[nrec[recs["querySeqId"]] > 16].tobytes()
        assert rows_off.tobytes() == B.host_rows(cl, reads, recs, keep + 1).tobytes() and len(rows_off) < len(rows)

        ctx.chain_long()                                                                             # on again: the first result
        ctx.chain_reads()
        assert ctx.chain_rows().tobytes() == rows.tobytes() and ctx.chain_leftover().tobytes() == left.tobytes()

        ctx.map()
        assert ctx.pass_stats()[1] is True, "the second pass of the same batch is a steady-state pass"
        recs2, rows2, left2 = check_on(batch, ctx, reads, keep, "steady-state pass, option on, secondaryToKeep %d" % keep)
        assert recs2.tobytes() == recs.tobytes() and rows2.tobytes() == rows.tobytes() and left2.tobytes() == left.tobytes()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_smaller_batch_after_a_larger_one_and_filter_none(batch):
    """the buffers of the larger batch are reused: list, staging rows and counts of the smaller one are its own; then filter mode none,
    where every chain of a read survives"""
    from mashmap_amd import capi
    reads = batch["reads"]
    ctx = context(batch, 0)
    try:
        ctx.chain_long()
        ctx.reads_upload([a for _, a in reads], None, [-1] * len(reads), 0)
        ctx.map()
        _, rows_all, _ = check_on(batch, ctx, reads, 0, "the whole batch")
        small = [reads[i] for i in (6, 1, 3, 4, 13)]                                                 # fwd21, fwd2, array_two, unrelated, rc33
        ctx.reads_upload([a for _, a in small], None, [-1] * len(small), 0)
        ctx.map()
        _, rows, left = check_on(batch, ctx, small, 0, "a smaller batch")
        assert len(left) == 0 and ctx.chain_long_counts() == dict(offered=3, finished=3) and 3 <= len(rows) < len(rows_all)
    finally:
        ctx.close()
    ctx = context(batch, 0, capi.MM_CHAIN_FILTER_NONE)
    try:
        ctx.chain_long()
        ctx.reads_upload([a for _, a in reads], None, [-1] * len(reads), 0)
        ctx.map()
        _, rows_none, _ = check_on(batch, ctx, reads, 0, "filter none", U.FILTER_NONE)
        assert len(rows_none) > len(rows_all)
    finally:
        ctx.close()


def run_cli(tmp_path, refrec, qrec, extra, tag, value):
    rf, qf, out = str(tmp_path / "ref.fa"), str(tmp_path / "q.fa"), str(tmp_path / (tag + ".paf"))
    if not os.path.exists(rf):
        U.write_fasta(rf, refrec); U.write_fasta(qf, qrec)
    e = {k: v for k, v in os.environ.items() if k != "MASHMAP_HIP_DEVICE_CHAIN"}
    if value is not None:
        e.update({"MASHMAP_HIP_DEVICE_CHAIN": value, "MASHMAP_HIP_TIMING": "1"})
    p = subprocess.run([HIP_BIN, "-r", rf, "-q", qf, "-o", out, "-t", "4"] + extra, capture_output=True, text=True, env=e, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return open(out, "rb").read(), p.stderr


def timing_figures(err):
    """(left-over records, chained rows, long reads chained on the device, long reads) summed over the device-stage lines"""
    assert "chaining on the device" in err, err[-2000:]
    back = re.findall(r"download of (\d+) left-over candidate mappings and (\d+) chained rows\)", err)
    lng = re.findall(r"\[(\d+) of (\d+) reads of more than 16 records chained on the device\]", err)
    assert back and len(lng) == len(back), err[-2000:]
    return sum(int(a) for a, _ in back), sum(int(b) for _, b in back), sum(int(a) for a, _ in lng), sum(int(b) for _, b in lng)


@pytest.mark.gpu
def test_command_line_with_the_value_long(tmp_path):
    """`asm_one2one` (tests/golden/cases.py: whole contigs at segLength 10000, dozens of records a read, which MASHMAP_HIP_DEVICE_CHAIN=1
    hands over) with MASHMAP_HIP_DEVICE_CHAIN=long: the PAF of the run without the switch and the stock binary's; the timing lines show
    rows and the long reads chained on the device"""
    from golden import cases as CS
    assert os.path.exists(HIP_BIN), "mashmap_hip not built (python -c 'import __graft_entry__ as g; g.build()')"
    _, refrec, qrec, extra = {c[0]: c for c in CS.paf_cases()}["asm_one2one"]
    off, _ = run_cli(tmp_path, refrec, qrec, extra, "off", None)
    on, err = run_cli(tmp_path, refrec, qrec, extra, "long", "long")
    left, rows, fin, offered = timing_figures(err)
    print("asm_one2one: left-over records", left, "chained rows", rows, "long reads chained", fin, "of", offered)
    assert off == open(os.path.join(ROOT, "tests", "golden", "paf", "asm_one2one.paf"), "rb").read() and off.count(b"\n") >= 3
    assert on == off, (on[:300], off[:300])
    assert rows > 0 and fin > 0 and offered >= fin
    if fin == offered:                                                                               # every contig has at most 512 records: nothing is handed over
        assert left == 0
    else:
        assert left > CL.LONG_MAX * (offered - fin)
    one, err1 = run_cli(tmp_path, refrec, qrec, extra, "one", "1")                                   # any other value: as before, no long reads on the device
    assert one == off and "records chained on the device]" not in err1


@pytest.mark.gpu
def test_command_line_on_long_colinear_reads_of_both_strands(tmp_path):
    """reads of 18 to 45 segments of a 150 kbp reference at segLength 1000, half of them reverse-complemented: one chain each, whose
    PAF line carries the conservedSketches-derived fields of the member introsort leaves in front"""
    assert os.path.exists(HIP_BIN), "mashmap_hip not built (python -c 'import __graft_entry__ as g; g.build()')"
    g = U.random_dna(8401, 150000)
    qrec = []
    for i, (x, n) in enumerate(((2000, 18000), (25000, 23400), (52000, 33000), (90000, 45000), (10000, 20000), (60000, 19000), (100000, 2500))):
        a = U.mutate(g[x:x + n + n // 8 + 64], 8410 + i, 0.04)[:n].copy()
        qrec.append(("r%d" % i, U.revcomp(a) if i % 2 else a))
    extra = ["-s", "1000", "--pi", "85"]
    off, _ = run_cli(tmp_path, [("g", g)], qrec, extra, "off", None)
    on, err = run_cli(tmp_path, [("g", g)], qrec, extra, "long", "long")
    left, rows, fin, offered = timing_figures(err)
    print("long reads: left-over records", left, "chained rows", rows, "long reads chained", fin, "of", offered)
    assert off.count(b"\n") >= len(qrec) and on == off, (on[:300], off[:300])
    assert fin == offered == 6 and left == 0 and rows >= 7
    if os.path.exists(U.REF_BIN):
        out = str(tmp_path / "stock.paf")
        p = subprocess.run([U.REF_BIN, "-r", str(tmp_path / "ref.fa"), "-q", str(tmp_path / "q.fa"), "-o", out, "-t", "4"] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert open(out, "rb").read() == on
