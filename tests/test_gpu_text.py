"""mm_text_* on the GPU (mashmap_amd/csrc/mm_text.hip) against the record rules restated in tests/textzoo.py: the record table, the names
and `consumed`; the packed piece, uploaded with mm_reads_upload_packed and downloaded again, byte for byte against the same records
packed on the host (mm_pack_read) and uploaded the old way.  Texts at exact multiples of MM_TEXT_TILE and one byte either side, split
appends, keep flags, the staged and the declined hand-over, mm_text_append_inflated, the errors, the thread exception, and the command
line under MASHMAP_HIP_DEVICE_PARSE=1."""
import os
import re
import subprocess
import threading
import zlib

import numpy as np
import pytest

import inflatezoo as IZ
import textzoo as Z
from golden import cases as CS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BIN = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
PAF_DIR = os.path.join(ROOT, "tests", "golden", "paf")


@pytest.fixture(scope="module")
def ctx():
    from mashmap_amd import capi
    c = capi.Context()
    yield c
    c.close()


def _arrays(seqs):
    return [np.frombuffer(s, dtype=np.uint8) for s in seqs]


def _host_words(ctx, seqs):
    """the records packed on the host and uploaded the old way: what mm_reads_packed_download gives back"""
    from mashmap_amd import capi
    ctx.reads_upload_packed(capi.pack_reads(_arrays(seqs)))
    b2, nm, hasn = ctx.reads_packed_download()
    return b2.tobytes(), nm.tobytes(), hasn.tobytes()


def _table(ctx, fmt, final, want, consumed_want):
    n, nb, consumed = ctx.text_scan(fmt, final)
    recs, names = ctx.text_records()
    assert (n, consumed) == (len(want), consumed_want)
    assert [int(x) for x in recs["hdrOff"]] == [o for o, _, _ in want]
    assert names == [nm for _, nm, _ in want] and nb == sum(len(nm) for _, nm, _ in want)
    assert [int(x) for x in recs["seqLen"]] == [len(s) for _, _, s in want]
    assert [int(x) for x in recs["hasN"]] == [Z.has_n(s) for _, _, s in want]
    return recs


def _pack(ctx, recs, keep=None, reserve=0, slack=64):
    """mm_text_pack into fresh host buffers filled with 0xA5; returns (the upload's arguments, nPacked, staged, b2, nm)"""
    lens = np.array([int(l) if keep is None or keep[i] else 0 for i, l in enumerate(recs["seqLen"])], dtype=np.int32)
    total = int(((lens.astype(np.int64) + 31) // 32 * 32).sum())
    b2 = np.full(total // 16 + slack, 0xA5A5A5A5, dtype=np.uint32); nm = np.full(total // 32 + slack, 0xA5A5A5A5, dtype=np.uint32)
    n, staged = ctx.text_pack(b2, nm, keep=keep, reserve=reserve)
    assert n == total
    hasn = np.array([int(h) if lens[i] else 0 for i, h in enumerate(recs["hasN"])], dtype=np.uint8)
    return (b2, nm, hasn, lens), n, staged, b2, nm


def _device_words(ctx, packed):
    ctx.reads_upload_packed(packed)
    b2, nm, hasn = ctx.reads_packed_download()
    return b2.tobytes(), nm.tobytes(), hasn.tobytes()


def _whole(ctx, text, fmt, final=1, keep=None):
    """one append, scan, table, pack, upload: everything compared; returns `staged`"""
    want, consumed = Z.parse(text, fmt, final)
    ctx.text_reset()
    ctx.text_append(text)
    recs = _table(ctx, fmt, final, want, consumed)
    packed, n, staged, b2, nm = _pack(ctx, recs, keep)
    if staged:
        assert bool(np.all(b2 == 0xA5A5A5A5)) and bool(np.all(nm == 0xA5A5A5A5))       # the host buffers are a key only
    seqs = [s if keep is None or keep[i] else b"" for i, (_, _, s) in enumerate(want)]
    if len(want):
        assert _device_words(ctx, packed) == _host_words(ctx, seqs)
    return staged


def _T():
    from mashmap_amd import capi
    return capi.MM_TEXT_TILE


def test_the_edge_texts(ctx):
    T = _T()
    texts = Z.edge_texts(T)
    assert len(texts) >= 60 and len({n for n, _, _ in texts}) == len(texts)
    staged = 0
    for name, fmt, text in texts:
        try:
            for final in (1, 0):
                staged += _whole(ctx, text, fmt, final)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
    assert staged > 0
    # the buffer's length itself at every byte count around two tiles: the last tile's loads end inside the buffer
    base = (Z.fa(b"e", Z.bases(np.random.RandomState(1), 50), 60) * (2 * T // 50 + 2))
    for n in list(range(2 * T - 20, 2 * T + 20)) + [1, 2, 15, 16, 17]:
        _whole(ctx, base[:n], Z.FASTA, 1)
    _whole(ctx, b"", Z.FASTA, 1)
    _whole(ctx, b"", Z.FASTQ, 0)


def _long_text(fmt, seed):
    rng = np.random.RandomState(seed)
    T = _T()
    out = b""
    i = 0
    while len(out) < 20 * T:
        L = int(rng.choice([0, 1, 31, 32, 33, 200, 1500, 7000]))
        seq = Z.bases(rng, L, b"ACGTNacgt" if i % 5 == 0 else b"ACGT")
        out += Z.fa(b"read%d some words" % i, seq, 70 if i % 2 else 0) if fmt == Z.FASTA else Z.fq(b"read%d some words" % i, seq, Z.bases(rng, L, b"@+>I5"))
        i += 1
    return out


@pytest.mark.parametrize("fmt", [Z.FASTA, Z.FASTQ])
def test_split_appends(ctx, fmt):
    """the text in two appends -- final = 0 with the tail held back, then final = 1 -- at about 30 cuts: the records and words of one append"""
    text = _long_text(fmt, 21 + fmt)
    want, _ = Z.parse(text, fmt, 1)
    ctx.text_reset(); ctx.text_append(text)
    recs = _table(ctx, fmt, 1, want, len(text))
    packed, n, _, _, _ = _pack(ctx, recs)
    single = _device_words(ctx, packed)
    assert single == _host_words(ctx, [s for _, _, s in want])
    # cuts: inside a header, right behind a '\n', between '\n' and the mark, inside each line kind, at tile boundaries
    lines = Z.lines_of(text)
    cuts = set()
    for k in (len(lines) // 3, len(lines) // 2):
        k -= k % 4
        for j in range(4):
            off, ln, _ = lines[k + j]
            cuts |= {off, off + 1, off + len(ln) // 2, off + len(ln)}
    T = _T()
    cuts |= {T, T - 1, T + 1, 7 * T, 1, len(text) - 1}
    cuts = sorted(c for c in cuts if 0 < c < len(text))
    assert 25 <= len(cuts) <= 40
    for cut in cuts:
        ctx.text_reset()
        ctx.text_append(text[:cut])
        wa, ca = Z.parse(text[:cut], fmt, 0)
        ra = _table(ctx, fmt, 0, wa, ca)
        pa, na, _, _, _ = _pack(ctx, ra)
        ctx.text_append(text[cut:])
        wb, cb = Z.parse(text[ca:], fmt, 1)
        rb = _table(ctx, fmt, 1, wb, cb)
        pb, nb, _, _, _ = _pack(ctx, rb)
        assert [(o, nm, s) for o, nm, s in wa] + [(o + ca, nm, s) for o, nm, s in wb] == want, cut
        parts = [dict(packed=p) for p, k in ((pa, na), (pb, nb)) if len(p[3])]
        ctx.reads_upload_packed_parts(parts)
        b2, nm, hasn = ctx.reads_packed_download()
        assert (b2.tobytes(), nm.tobytes(), hasn.tobytes()) == single, cut


def test_keep(ctx):
    text = _long_text(Z.FASTA, 5)
    want, _ = Z.parse(text, Z.FASTA, 1)
    rng = np.random.RandomState(9)
    for keep in (rng.randint(0, 2, size=len(want)).astype(np.uint8), np.zeros(len(want), dtype=np.uint8), np.ones(len(want), dtype=np.uint8)):
        _whole(ctx, text, Z.FASTA, 1, keep=keep)
    text = _long_text(Z.FASTQ, 6)
    want, _ = Z.parse(text, Z.FASTQ, 1)
    _whole(ctx, text, Z.FASTQ, 1, keep=(np.arange(len(want)) % 3 != 0).astype(np.uint8))


def test_staged_and_declined(ctx):
    from mashmap_amd import capi
    text = _long_text(Z.FASTA, 7)
    ctx.lib.mm_reads_prefetch_drop(ctx.h)
    assert _whole(ctx, text, Z.FASTA, 1) == 1              # nothing on its way: the area grows to the piece, the host buffers keep their 0xA5
    # a small host piece with a small reserve first: the area cannot grow under it, the text's piece is declined
    ctx.lib.mm_reads_prefetch_drop(ctx.h)
    fresh = capi.Context()
    try:
        small = capi.pack_reads(_arrays([b"ACGT" * 16]))
        st = capi.C.c_int(0)
        fresh._ck(fresh.lib.mm_reads_prefetch_packed_append(fresh.h, capi._ptr(small[0]), capi._ptr(small[1]), small[1].size * 32, 64, capi.C.byref(st)), "append")
        assert st.value == 1
        want, consumed = Z.parse(text, Z.FASTA, 1)
        fresh.text_append(text)
        recs = _table(fresh, Z.FASTA, 1, want, consumed)
        packed, n, staged, b2, nm = _pack(fresh, recs, slack=0)
        assert staged == 0 and n > 64
        hb2, hnm, hasn, lens = capi.pack_reads(_arrays([s for _, _, s in want]))
        assert b2.tobytes() == hb2.tobytes() and nm.tobytes() == hnm.tobytes()      # the host buffers hold the words
        assert _device_words(fresh, packed) == _host_words(fresh, [s for _, _, s in want])
    finally:
        fresh.close()


def _bgzf_blocks(raw, rng):
    """raw as raw-deflate blocks of 1 000 .. 60 000 bytes that cut it anywhere: (comp, descriptors)"""
    from mashmap_amd import capi
    comp, rows, at = bytearray(), [], 0
    while at < len(raw):
        n = int(rng.randint(1000, 60001))
        chunk = raw[at:at + n]
        d = IZ.raw_deflate(chunk)
        rows.append((len(comp), len(d), len(chunk), at, zlib.crc32(chunk), 0))
        comp += d; at += len(chunk)
    return bytes(comp), np.array(rows, dtype=capi.INFLATE_BLOCK_DT)


def test_append_inflated(ctx):
    rng = np.random.RandomState(17)
    text = _long_text(Z.FASTQ, 8) * 3
    comp, blocks = _bgzf_blocks(text, rng)
    assert len(blocks) >= 5
    want, consumed = Z.parse(text, Z.FASTQ, 1)
    ctx.text_reset()
    # a corrupted block in the middle: one refused, nothing appended
    bad = bytearray(comp)
    mid = len(blocks) // 2
    bad[int(blocks[mid]["cOff"]) + int(blocks[mid]["cLen"]) // 2] ^= 0x10
    status, nbad = ctx.text_append_inflated(bytes(bad), blocks.copy())
    assert nbad == 1 and status[mid] != 0 and not np.delete(status, mid).any()
    assert ctx.text_scan(Z.FASTQ, 1) == (0, 0, 0)
    # the next good call, in two halves with the descriptors shuffled (uOff orders the payloads)
    half = len(blocks) // 2
    for part in (blocks[:half], blocks[half:]):
        order = rng.permutation(len(part))
        status, nbad = ctx.text_append_inflated(comp, part[order].copy())
        assert nbad == 0 and not status.any()
    recs = _table(ctx, Z.FASTQ, 1, want, consumed)
    packed, n, staged, _, _ = _pack(ctx, recs)
    assert _device_words(ctx, packed) == _host_words(ctx, [s for _, _, s in want])


def test_errors_and_counts():
    from mashmap_amd import capi
    base = capi.device_bytes()
    c = capi.Context()
    try:
        b2 = np.zeros(64, dtype=np.uint32); nm = np.zeros(64, dtype=np.uint32)
        with pytest.raises(capi.MashmapError, match=r"mm_text_pack failed \(-3\): mm_text_pack: no mm_text_scan"):
            c.text_pack(b2, nm)
        assert b"mm_text_pack" not in c.lib.mm_last_error(c.h)                     # handed out once, then the context's own text again
        c.text_append(b">a\nACGT\n>b\nAC\n")
        with pytest.raises(capi.MashmapError, match=r"mm_text_records failed \(-3\)"):
            c._text_scanned = (1, 1); c.text_records()
        with pytest.raises(capi.MashmapError, match=r"mm_text_scan failed \(-1\): mm_text_scan: unknown format"):
            c.text_scan(2, 1)
        assert c.text_scan(Z.FASTA, 0) == (1, 1, 8)
        c.text_append(b"G\n")                                                      # an append since the scan
        with pytest.raises(capi.MashmapError, match=r"mm_text_pack failed \(-3\)"):
            c.text_pack(b2, nm)
        assert c.text_scan(Z.FASTA, 1) == (2, 2, 16)
        with pytest.raises(capi.MashmapError, match=r"mm_text_pack failed \(-1\): mm_text_pack: the kept records need more than capPackedBases"):
            c.text_pack(b2[:2], nm[:1])                                            # 32 bases of room, 64 needed
        assert c.text_pack(b2, nm) == (64, 1)                                      # the refusal left the buffer and the scan as they were
        with pytest.raises(capi.MashmapError, match=r"mm_text_pack failed \(-3\)"):
            c.text_pack(b2, nm)                                                    # the pack consumed the scan
        assert c.text_scan(Z.FASTA, 1) == (0, 0, 0)                                # and the text
        with pytest.raises(capi.MashmapError, match=r"mm_text_append failed \(-1\): mm_text_append: the text buffer holds at most"):
            c._ck(c.lib.mm_text_append(c.h, capi._ptr(b2), 2 ** 32, 0), "mm_text_append")
        blk = np.array([(0, 10, 65537, 0, 0, 0)], dtype=capi.INFLATE_BLOCK_DT)
        with pytest.raises(capi.MashmapError, match=r"mm_text_append_inflated failed \(-1\): mm_inflate_blocks: a block above MM_INFLATE_MAX_BLOCK"):
            c.text_append_inflated(bytes(16), blk)
        assert c.text_counts() == (3, 3, 24)
        scan_ms, pack_ms = c.text_kernel_ms()
        assert scan_ms >= 0 and pack_ms >= 0
        assert capi.device_bytes() > base
    finally:
        c.close()
    assert capi.device_bytes() == base                                             # the text buffer and its tables are the context's


def test_a_reader_thread_parses_while_the_context_maps(ctx):
    """the thread exception: the mm_text_* calls from another thread while the context's own thread is inside other calls"""
    name, refrec, qrec, _ = {c[0]: c for c in CS.paf_cases()}["default"]
    ctx.index_build([a for _, a in refrec])
    ctx.set_tables_default(0.85)
    reads = [a for _, a in qrec]

    def map_once():
        ctx.reads_upload(reads)
        ctx.map()
        return [x.tobytes() for x in ctx.results()] + [ctx.mappings().tobytes()]

    text = _long_text(Z.FASTQ, 31) * 4
    comp, blocks = _bgzf_blocks(text, np.random.RandomState(3))
    want, consumed = Z.parse(text, Z.FASTQ, 1)
    from mashmap_amd import capi
    hb2, hnm, _, _ = capi.pack_reads(_arrays([s for _, _, s in want]))
    alone_map = map_once()
    assert len(alone_map[-1]) > 0
    rounds, errors = [], []

    def reader():
        try:
            for _ in range(3):
                ctx.text_reset()
                status, nbad = ctx.text_append_inflated(comp, blocks.copy())
                assert nbad == 0
                recs = _table(ctx, Z.FASTQ, 1, want, consumed)
                packed, n, staged, b2, nm = _pack(ctx, recs, slack=0)
                if not staged:
                    assert b2.tobytes() == hb2.tobytes() and nm.tobytes() == hnm.tobytes()
                rounds.append(staged)
        except BaseException as e:                       # noqa: BLE001 -- reported by the assertion below
            errors.append(e)

    t = threading.Thread(target=reader)
    t.start()
    maps = [map_once()]
    while t.is_alive() and len(maps) < 50:
        maps.append(map_once())
    t.join()
    assert not errors, errors
    assert len(rounds) == 3
    assert all(m == alone_map for m in maps)
    ctx.lib.mm_reads_prefetch_drop(ctx.h)
    _whole(ctx, text, Z.FASTQ, 1)                        # and the context's own thread again, with the upload


def _cli(td, name, tag, fastq, device):
    _, refrec, qrec, extra = {c[0]: c for c in CS.paf_cases()}[name]
    rf = os.path.join(td, "%s.%s.ref.fa" % (name, tag))
    open(rf, "wb").write(b"".join(Z.fa(n.encode(), bytes(a), 60) for n, a in refrec))
    text = b"".join(Z.fq(n.encode(), bytes(a)) if fastq else Z.fa(n.encode(), bytes(a), 60) for n, a in qrec)
    qf = os.path.join(td, "%s.%s.q.%s.gz" % (name, tag, "fq" if fastq else "fa"))
    open(qf, "wb").write(IZ.bgzf_bytes(text, 5000))
    out = os.path.join(td, "%s.%s.paf" % (name, tag))
    env = dict(os.environ, MASHMAP_HIP_TIMING="1", MASHMAP_HIP_BATCH_MBP="0.2")       # windows of 200 kB: several per file, tails carried over
    env.pop("MASHMAP_HIP_DEVICE_PARSE", None); env.pop("MASHMAP_HIP_DEVICE_INFLATE", None)
    if device:
        env["MASHMAP_HIP_DEVICE_PARSE"] = "1"
    return subprocess.run([HIP_BIN, "-r", rf, "-q", qf, "-o", out, "-t", "4"] + extra, capture_output=True, text=True, env=env), out, len(qrec), len(text)


@pytest.mark.parametrize("fastq", [False, True])
def test_the_command_line_parses_bgzf_queries_on_the_device(fastq, tmp_path):
    assert os.path.exists(HIP_BIN), "mashmap_hip not built"
    exp = open(os.path.join(PAF_DIR, "default.paf"), "rb").read()
    assert len(exp) > 0
    p, out, nq, nbytes = _cli(str(tmp_path), "default", "dev", fastq, True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(out, "rb").read() == exp
    windows = re.findall(r"reader: device parser: (\d+) blocks, (\d+) records, (\d+) bytes consumed", p.stderr)
    assert len(windows) >= 3 and sum(int(w[1]) for w in windows) == nq and sum(int(w[2]) for w in windows) == nbytes
    m = re.search(r"device parser: (\d+) scans, (\d+) records, (\d+) bytes", p.stderr)
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) == nq and int(m.group(3)) == nbytes
    # without the switch: the same PAF by the host reader, no scan
    p, out, _, _ = _cli(str(tmp_path), "default", "host", fastq, False)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(out, "rb").read() == exp
    assert re.search(r"device parser: 0 scans, 0 records, 0 bytes", p.stderr) and "reader: device parser:" not in p.stderr
