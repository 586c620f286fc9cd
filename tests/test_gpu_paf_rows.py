"""mm_paf_rows / mm_paf_format: the PAF lines of a pass written on the device -- filterFalseHighIdentity, mappingBoundarySanityCheck
and the text of every line (k_paf_measure, k_paf_unflag, k_paf_offsets, k_paf_write) -- byte for byte what the host's own code writes
(mmh_paf_text of libmashmap_host.so: MapPost::finishRows + appendReadMappings).

Planted rows through mm_paf_format (tests/pafrows.py; no index, one context): row counts at and around k_paf_write's wave of 64, reads
of 1, 2, 3 and 16 rows and reads without rows, names of 0 to 300 bytes, and in every output mode rows that are dropped, clamped,
of identity 0 and 1, with a complexity in exponent form, and one that is not formattable (its read is handed over as a whole).
The chain batch (tests/chainbatch.py): mm_map_fragments -> mm_chain_reads -> mm_paf_rows after a sized and a steady-state pass.
Every refusal with its code and reason; empty batches; results invalid after the next upload.
The command line with MASHMAP_HIP_DEVICE_CHAIN and MASHMAP_HIP_DEVICE_PAF writes the PAF it writes with neither.

Small shapes: at most 200 rows and 47 reads a planted batch; k 16, segLength 1000, s 80 and 21 reads in the chain batch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chainbatch as B
import mmutil as U
import pafrows as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BIN = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
SENTINEL = 0xA5


def paf_context(mode):
    from mashmap_amd import capi
    ctx = capi.Context(k=P.K, segLength=1000, sketchSize=P.S)
    names, lens = P.contigs()
    ctx.set_paf_tables(names, lens, legacy=mode[0], aniPercentage=mode[1], merge=mode[2], filterLengthMismatches=mode[3], lenIdThreshold=P.len_id_threshold())
    return ctx


def check_planted(ctx, n_rows, mode, what):
    rows, read_lens, names, handed = P.planted(n_rows)
    cn, cl = P.contigs()
    want, woff, wflags, wcounts = P.expected(rows, read_lens, names, cn, cl, mode, handed)
    ctx.paf_format(rows, read_lens, names)
    counts = ctx.paf_counts()
    off, flags = ctx.paf_offsets(len(read_lens))
    buf = ctx.paf_text(slack=64, fill=SENTINEL)
    got = buf[:counts["bytes"]].tobytes()
    print(what, counts, "reads", len(read_lens), "handed", handed)
    assert counts == wcounts, (what, counts, wcounts)
    assert off.tolist() == woff.tolist(), what
    assert flags.tolist() == wflags.tolist(), what
    if got != want:
        at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if got[:len(want)] != want[:len(got)] else min(len(got), len(want))
        raise AssertionError("%s: text differs at byte %d: device %r, host %r" % (what, at, got[max(0, at - 60):at + 60], want[max(0, at - 60):at + 60]))
    assert (buf[counts["bytes"]:] == SENTINEL).all(), what + ": bytes behind off[nReads]"
    return rows, read_lens, names, handed, off, got


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 128, 130])
def test_row_counts_around_the_wave_of_64(n_rows):
    ctx = paf_context(P.MODES["default"])
    try:
        check_planted(ctx, n_rows, P.MODES["default"], "%d rows" % n_rows)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(P.MODES))
def test_every_mode_with_dropped_clamped_and_handed_over_rows(mode):
    ctx = paf_context(P.MODES[mode])
    try:
        rows, read_lens, names, handed, off, text = check_planted(ctx, 193, P.MODES[mode], mode)
        per_read = np.bincount(rows["querySeqId"], minlength=len(read_lens))
        assert sorted(set(per_read.tolist())) == [0, 1, 2, 3, 16] and per_read[0] == 0 and per_read[-1] == 0 and (per_read[1:-1] == 0).any()
        assert sorted(set(len(n) for n in names)) == P.NAME_LENGTHS
        (h,) = handed                                                  # the read of three rows with the row that is not formattable
        before = max(r for r in range(h) if per_read[r]); after = min(r for r in range(h + 1, len(per_read)) if per_read[r])
        assert per_read[h] == 3 and off[h] == off[h + 1] and off[before] < off[before + 1] and off[after] < off[after + 1]   # its neighbours' spans stand
        counts = ctx.paf_counts()
        sep = b" " if mode == "legacy" else b"\t"
        if mode == "length_filter":
            assert counts["dropped"] >= 5 and any(per_read[r] == 2 and off[r] == off[r + 1] for r in range(len(read_lens)))   # first, last, all of a read, q_l == 0
        else:
            assert counts["dropped"] == 0
        if mode != "legacy":
            assert sep + b"-0" + sep + b"id:f:0" + sep in text and sep + b"255" + sep + (b"id:f:100" if mode == "ani_percentage" else b"id:f:1") + sep in text
            assert b"kc:f:1e-07" in text and b"kc:f:1e+06" in text and b"kc:f:0" + (sep if mode == "merge_off" else b"\n") in text
            assert (b"jc:f:" in text) == (mode == "merge_off")
        # a second call on the same context replaces the results (the buffers are reused)
        check_planted(ctx, 65, P.MODES[mode], mode + ", 65 rows behind 193")
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def batch(oracle):
    """the chain batch, the oracle session's index and tables (shared, unchanged)"""
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


def chain_context(batch, keep, paf=True):
    from mashmap_amd import capi
    ctx = capi.Context(k=B.K, segLength=B.L, sketchSize=B.S, flags=capi.MM_FLAG_HG_FILTER)
    ix = batch["ix"]
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"], None)
    ctx.set_tables(batch["min_hits"], batch["cutoffs"])
    ctx.set_replay_tables(*batch["replay"])
    ctx.set_chain_tables(B.L, 1, keep, keep, True, capi.MM_CHAIN_FILTER_QUERY, 0.0, batch["identity"])
    if paf:
        ctx.set_paf_tables([n for n, _ in batch["contigs"]], batch["clens"], lenIdThreshold=min(0.7, float(np.float32(B.PI)) ** 3))
    return ctx


def check_chain_pass(batch, ctx, what):
    reads = batch["reads"]
    names = [n for n, _ in reads]
    lens = [len(a) for _, a in reads]
    ctx.chain_reads()
    rows, left = ctx.chain_rows(), ctx.chain_leftover()
    ctx.paf_rows(names)
    counts = ctx.paf_counts()
    off, flags = ctx.paf_offsets(len(reads))
    text = ctx.paf_text()
    want, woff, rep = P.host_text(rows, lens, names, [n for n, _ in batch["contigs"]], batch["clens"], k=B.K, s=B.S, pi=B.PI)
    print(what, counts, "rows", len(rows), "left-over records", len(left))
    assert text == want and off.tolist() == woff.tolist() and len(text) > 1000, what
    assert not flags.any() and counts == dict(readsWithText=int((np.diff(woff) > 0).sum()), lines=int(rep.sum()), bytes=len(want), dropped=int(len(rows) - rep.sum()),
                                              handedReads=0), what
    for name in ("array_two", "array_three", "unrelated"):             # handed over by the chain stage, or without records: no rows, an empty span
        r = names.index(name)
        assert off[r] == off[r + 1] and flags[r] == 0, name
    assert set(left["querySeqId"].tolist()) == {names.index("array_two"), names.index("array_three")}
    a, n, b = ctx.paf_device()
    assert a and b and n == len(want)
    return text


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0, 2], ids=["secondary0", "secondary2"])
def test_the_chain_batch_after_a_sized_and_a_steady_state_pass(batch, keep):
    from mashmap_amd import capi
    ctx = chain_context(batch, keep)
    try:
        reads = batch["reads"]
        ctx.reads_upload([a for _, a in reads], None, [-1] * len(reads), 0)
        ctx.map()
        assert ctx.pass_stats()[1] is False
        first = check_chain_pass(batch, ctx, "sized pass, secondaryToKeep %d" % keep)
        ctx.map()
        assert ctx.pass_stats()[1] is True, "the second pass of the same batch is a steady-state pass"
        with pytest.raises(capi.MashmapError) as e:                    # a map call: the text of the pass before is gone, and so are its rows
            ctx.paf_text()
        assert "(-3)" in str(e.value)
        with pytest.raises(capi.MashmapError) as e:
            ctx.paf_rows([n for n, _ in reads])
        assert "(-3)" in str(e.value) and "mm_chain_reads has not run on the mapped batch" in str(e.value)
        assert check_chain_pass(batch, ctx, "steady-state pass, secondaryToKeep %d" % keep) == first
        with pytest.raises(capi.MashmapError) as e:                    # nReads is not the batch's
            ctx.paf_rows([n for n, _ in reads][:-1])
        assert "(-1)" in str(e.value) and "nReads" in str(e.value)
        ctx.paf_rows([n for n, _ in reads])
        ctx.reads_upload([a for _, a in reads[:3]])                     # a new batch: the results of the old one are gone
        for call in (ctx.paf_counts, ctx.paf_text, ctx.paf_device, lambda: ctx.paf_offsets(len(reads))):
            with pytest.raises(capi.MashmapError) as e:
                call()
            assert "(-3)" in str(e.value) and "has not run on the current batch" in str(e.value)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_every_refusal_names_its_reason():
    from mashmap_amd import capi
    rows, read_lens, names, _ = P.planted(20)
    cn, cl = P.contigs()

    def refused(call, code, text):
        with pytest.raises(capi.MashmapError) as e:
            call()
        assert "(%d)" % code in str(e.value) and text in str(e.value), str(e.value)

    ctx = capi.Context(k=P.K, segLength=1000, sketchSize=P.S)
    try:
        refused(lambda: ctx.paf_format(rows, read_lens, names), -3, "mm_paf_format: mm_set_paf_tables was not called")
        refused(lambda: ctx.paf_rows(names), -3, "mm_paf_rows: mm_set_paf_tables was not called")
        refused(lambda: ctx.set_paf_tables(cn, cl, sparsityThreshold=1 << 63), -1, "sparsity threshold")
        thr, txt = capi.paf_mapq_table()
        refused(lambda: ctx.set_paf_tables(cn, cl, mapq=(thr[::-1], txt)), -1, "mapQ table")
        refused(lambda: ctx.paf_format(rows, read_lens, names), -3, "mm_set_paf_tables was not called")       # a refused block sets nothing
        ctx.set_paf_tables(cn, cl)
        refused(lambda: ctx.paf_rows(names), -3, "mm_chain_reads has not run on the mapped batch")
        refused(ctx.paf_counts, -3, "has not run on the current batch")
        qn, qo = capi.pack_names(names)
        lib, p = ctx.lib, capi._ptr
        bad_off = qo.copy(); bad_off[3] = bad_off[4] + 1                                                   # name offsets that step back
        assert lib.mm_paf_format(ctx.h, p(rows), len(rows), p(read_lens), 0, p(qn), p(bad_off), len(read_lens)) == -1
        assert b"not non-decreasing" in lib.mm_last_error(ctx.h)
        assert lib.mm_paf_format(ctx.h, p(rows), 1 << 31, p(read_lens), 0, p(qn), p(qo), len(read_lens)) == -1   # refused by the count alone: no row is read
        assert b"more than 2^31 - 1 rows" in lib.mm_last_error(ctx.h)
        for field, value in (("refSeqId", len(cl)), ("refSeqId", -1), ("querySeqId", len(read_lens)), ("querySeqId", -1)):
            bad = rows.copy(); bad[len(bad) - 1][field] = value
            refused(lambda: ctx.paf_format(bad, read_lens, names), -1, "corrupt row %d" % (len(bad) - 1))
        bad = rows.copy(); bad[5]["querySeqId"] = bad[4]["querySeqId"] - 1                                  # read order broken
        refused(lambda: ctx.paf_format(bad, read_lens, names), -1, "corrupt row 5")
        refused(lambda: ctx.paf_format(rows, read_lens, names, firstSeqId=2), -1, "corrupt row 0")                 # read 1 lies in front of firstSeqId
        refused(ctx.paf_counts, -3, "has not run on the current batch")                                     # a refused call leaves no results
        # an empty batch, and a batch without rows
        ctx.paf_format(rows[:0], read_lens[:0], [])
        assert ctx.paf_counts() == dict(readsWithText=0, lines=0, bytes=0, dropped=0, handedReads=0) and ctx.paf_text() == b""
        assert ctx.paf_offsets(0)[0].tolist() == [0]
        ctx.paf_format(rows[:0], read_lens, names)
        assert ctx.paf_counts() == dict(readsWithText=0, lines=0, bytes=0, dropped=0, handedReads=0)
        off, flags = ctx.paf_offsets(len(read_lens))
        assert not off.any() and not flags.any()
        ctx.paf_format(rows, read_lens, names)                                                              # and the context still works
        assert ctx.paf_counts()["lines"] > 0
    finally:
        ctx.close()


@pytest.mark.gpu
def test_an_empty_mapped_batch_and_one_without_records(batch):
    ctx = chain_context(batch, 0)
    try:
        assert ctx.reads_upload([]) == 0
        ctx.map(); ctx.chain_reads(); ctx.paf_rows([])
        assert ctx.paf_counts() == dict(readsWithText=0, lines=0, bytes=0, dropped=0, handedReads=0) and ctx.paf_text() == b""
        ctx.reads_upload([U.random_dna(8301, 2500), U.random_dna(8302, 700), U.random_dna(8303, 10)])
        ctx.map(); ctx.chain_reads(); ctx.paf_rows(["a", "b", "c"])
        assert ctx.paf_counts() == dict(readsWithText=0, lines=0, bytes=0, dropped=0, handedReads=0)
        assert ctx.paf_offsets(3)[0].tolist() == [0, 0, 0, 0]
    finally:
        ctx.close()


# case of tests/golden/cases.py -> (golden PAF to compare with or None, device text expected)
COMMAND_LINES = {"default": ("default", True), "pi90_n2": ("pi90_n2", True), "nomerge": ("nomerge", True), "filter_none": ("filter_none", True),
                 "legacy_pct": ("legacy_pct", True), "k40_asm": ("k40_asm", None), "asm_one2one": ("asm_one2one", False)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(COMMAND_LINES))
def test_command_line_paf_is_the_same_with_both_switches(name, tmp_path):
    """mashmap_hip with MASHMAP_HIP_DEVICE_CHAIN and MASHMAP_HIP_DEVICE_PAF set writes the PAF it writes with neither (and the stock
    binary's where tests/golden/paf has it).  The device-stage timing line says how many bytes of PAF text came back: more than zero in
    the five cases whose reads the chain stage finishes; in `k40_asm` contigs are the reads (handed over by the chain stage, their lines
    interleaved by the post stage); in `asm_one2one` the switch says why it is ignored"""
    from golden import cases as CS
    assert os.path.exists(HIP_BIN), "mashmap_hip not built (python -c 'import __graft_entry__ as g; g.build()')"
    golden, device_text = COMMAND_LINES[name]
    _, refrec, qrec, extra = {c[0]: c for c in CS.paf_cases()}[name]
    rf, qf = str(tmp_path / "ref.fa"), str(tmp_path / "q.fa")
    U.write_fasta(rf, refrec); U.write_fasta(qf, qrec)
    outs = {}
    for tag, env in (("off", {}), ("on", {"MASHMAP_HIP_DEVICE_CHAIN": "1", "MASHMAP_HIP_DEVICE_PAF": "1", "MASHMAP_HIP_TIMING": "1"})):
        out = str(tmp_path / (tag + ".paf"))
        e = {k: v for k, v in os.environ.items() if k not in ("MASHMAP_HIP_DEVICE_CHAIN", "MASHMAP_HIP_DEVICE_PAF")}
        e.update(env)
        p = subprocess.run([HIP_BIN, "-r", rf, "-q", qf, "-o", out, "-t", "4"] + extra, capture_output=True, text=True, env=e, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[tag] = open(out, "rb").read()
        if tag == "on":
            back = [int(x) for x in re.findall(r"(\d+) bytes of PAF text", p.stderr)]
            print(name, "bytes of device text", back)
            if device_text is False:
                assert "MASHMAP_HIP_DEVICE_PAF ignored" in p.stderr and "one-to-one" in p.stderr and not back, p.stderr[-2000:]
            else:
                assert "PAF text on the device" in p.stderr and back, p.stderr[-2000:]
                if device_text:
                    assert sum(back) > 0, (name, back)
    assert len(outs["off"]) > 0 and outs["off"].count(b"\n") >= 3
    gold = os.path.join(ROOT, "tests", "golden", "paf", golden + ".paf")
    if os.path.exists(gold):
        assert outs["off"] == open(gold, "rb").read()
    assert outs["on"] == outs["off"], (outs["on"][:300], outs["off"][:300])
