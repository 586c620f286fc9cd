"""mm_inflate_blocks on the GPU (k_inflate_blocks, mashmap_amd/csrc/mm_inflate.hip) against zlib: the zoo of tests/hostlogic/inflate_check.cpp
(the bytes tests/test_inflate_core.py runs through the same decoder under the sanitizers; here a plain build of the program writes them out), more blocks than the grid holds, the named malformed
blocks between good ones, the thread exception, Context.inflate_bgzf, and the command line under MASHMAP_HIP_DEVICE_INFLATE=1."""
import os
import re
import subprocess
import threading
import zlib

import numpy as np
import pytest

import inflatezoo as Z
import mmutil as U
from golden import cases as CS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_BIN = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
PAF_DIR = os.path.join(ROOT, "tests", "golden", "paf")


@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    td = tmp_path_factory.mktemp("inflate_zoo")
    return Z.load_zoo(Z.build_check(td, sanitize=False), td)      # a plain build: the sanitized run of these bytes is the CPU suite's


@pytest.fixture()
def ctx():
    from mashmap_amd import capi
    base = capi.device_bytes()
    c = capi.Context()
    yield c
    c.close()
    assert capi.device_bytes() == base          # the staging buffers are the context's: gone with mm_destroy (0 when no other context lives)


def _layout(items, seed, gaps=True):
    """descriptors for items [(comp, uLen, crc)]: compressed streams end to end in input order, output ranges in shuffled order with gaps"""
    from mashmap_amd import capi
    rng = np.random.RandomState(seed)
    blocks = np.zeros(len(items), dtype=capi.INFLATE_BLOCK_DT)
    comp, at = bytearray(), 0
    for i, (c, ulen, crc) in enumerate(items):
        blocks[i]["cOff"], blocks[i]["cLen"], blocks[i]["uLen"], blocks[i]["crc32"] = len(comp), len(c), ulen, crc
        comp += c
        comp += bytes(int(rng.randint(0, 7)))                      # streams need not be adjacent either
    order = rng.permutation(len(items)) if gaps else np.arange(len(items))
    for i in order:
        at += int(rng.randint(1, 200)) if gaps else 0
        blocks[i]["uOff"] = at
        at += int(blocks[i]["uLen"])
    return bytes(comp), blocks, at + (64 if gaps else 0)


def _check_regions(dst, blocks, payloads, status=None):
    """every OK block's bytes are its payload; every byte outside the regions is still 0xA5"""
    covered = np.zeros(len(dst), dtype=bool)
    for i, b in enumerate(blocks):
        lo, hi = int(b["uOff"]), int(b["uOff"]) + int(b["uLen"])
        covered[lo:hi] = True
        if status is None or status[i] == 0:
            assert dst[lo:hi].tobytes() == payloads[i], i
    assert bool(np.all(dst[~covered] == 0xA5))


def test_the_zoo_in_one_call(zoo, ctx):
    good = [z for z in zoo if z[1] == 0]
    assert len(good) >= 15 + 3 * 7 * 12
    # a payload of 65535 or 65536 bytes that does not compress (random bytes at every level, anything at level 0, the hand-built stored
    # block of 65535) deflates to MORE than MM_INFLATE_MAX_BLOCK bytes: no BGZF block can hold such a stream and the call refuses it
    # (MM_ERR_ARG: test_malformed_blocks_between_good_ones).  The rest go in one call -- both lengths among them, compressed, and a stored
    # block of 65520 bytes behind a header in mid-byte.
    over = [z for z in good if len(z[2]) > 65536]
    assert len(over) <= 19 and all(z[3] >= 65535 for z in over), [z[0] for z in over]
    good = [z for z in good if len(z[2]) <= 65536]
    lens = {z[3] for z in good}
    assert {0, 1, 63, 64, 65, 257, 258, 259, 32768, 32769, 65535, 65536} <= lens
    for z in good:
        assert zlib.decompress(z[2], -15) == z[5] and zlib.crc32(z[5]) == z[4], z[0]          # bytes equal to zlib's, by zlib here
    comp, blocks, n = _layout([(z[2], z[3], z[4]) for z in good], seed=11)
    dst = np.full(n, 0xA5, dtype=np.uint8)
    before = ctx.inflate_counts()
    out, status = ctx.inflate_blocks(comp, blocks, dst)
    assert out is dst
    bad = [(good[i][0], int(s)) for i, s in enumerate(status) if s]
    assert not bad, bad
    assert ctx.inflate_bad == 0
    _check_regions(dst, blocks, [z[5] for z in good])
    after = ctx.inflate_counts()
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, len(good), sum(z[3] for z in good))


def test_more_blocks_than_the_grid_holds(ctx):
    raw = Z.fasta_bytes(6000 * 4096, seed=5)
    items = []
    for i in range(6000):
        chunk = raw[i * 4096:(i + 1) * 4096]
        items.append((Z.raw_deflate(chunk), len(chunk), zlib.crc32(chunk)))
    comp, blocks, n = _layout(items, seed=12, gaps=False)
    out, status = ctx.inflate_blocks(comp, blocks)
    assert not status.any() and out.tobytes() == raw
    assert ctx.inflate_counts() == (1, 6000, len(raw))
    one, st1 = ctx.inflate_blocks(comp, blocks[17:18].copy(), np.zeros(n, dtype=np.uint8))     # then a single block ...
    lo = int(blocks[17]["uOff"])
    assert list(st1) == [0] and one[lo:lo + 4096].tobytes() == raw[lo:lo + 4096] and not one[:lo].any() and not one[lo + 4096:].any()
    none, st0 = ctx.inflate_blocks(comp, blocks[:0])                                            # ... and none
    assert len(none) == 0 and len(st0) == 0
    assert ctx.inflate_counts() == (3, 6001, len(raw) + 4096)


def test_malformed_blocks_between_good_ones(zoo, ctx):
    from mashmap_amd import capi
    bad = [z for z in zoo if z[1] != 0]
    good = [z for z in zoo if z[1] == 0 and 0 < z[3] <= 300][:len(bad) + 1]
    assert len(bad) >= 19 and len(good) == len(bad) + 1
    mixed = [good[0]]
    for b, g in zip(bad, good[1:]):
        mixed += [b, g]
    comp, blocks, n = _layout([(z[2], z[3], z[4]) for z in mixed], seed=13)
    dst = np.full(n, 0xA5, dtype=np.uint8)
    out, status = ctx.inflate_blocks(comp, blocks, dst)                    # MM_OK: the call returns, the status fields say the rest
    got = {z[0]: Z.STATUS[int(s)] for z, s in zip(mixed, status)}
    assert got == {z[0]: Z.STATUS[z[1]] for z in mixed}
    assert ctx.inflate_bad == len(bad)
    _check_regions(dst, blocks, [z[5] for z in mixed], status)
    assert ctx.inflate_counts() == (1, len(mixed), sum(z[3] for z in mixed if z[1] == 0))
    # ranges that leave the buffers, blocks above the bound and overlapping output ranges: MM_ERR_ARG, nothing launched, nothing counted
    g = good[0]
    def one(cOff=0, cLen=len(g[2]), uLen=g[3], uOff=0):
        return np.array([(cOff, cLen, uLen, uOff, g[4], 0)], dtype=capi.INFLATE_BLOCK_DT)
    for blk, ndst in ((one(cOff=1), g[3]), (one(cLen=len(g[2]) + 1), g[3]), (one(uOff=1), g[3]), (one(uLen=g[3] + 1), g[3]), (one(cOff=2 ** 63), g[3]),
                      (one(uOff=2 ** 64 - 1), g[3]), (one(uLen=65537), 70000), (np.concatenate([one(), one(uOff=g[3] - 1)]), 2 * g[3]),
                      (np.concatenate([one(uOff=5), one(uOff=0, uLen=6)]), 2 * g[3] + 5)):
        d = np.full(ndst, 0xA5, dtype=np.uint8)
        with pytest.raises(capi.MashmapError, match=r"mm_inflate_blocks failed \(-1\)"):
            ctx.inflate_blocks(g[2], blk, d)
        assert bool(np.all(d == 0xA5))
    with pytest.raises(capi.MashmapError, match=r"failed \(-1\): mm_inflate_blocks: a block above MM_INFLATE_MAX_BLOCK"):
        ctx.inflate_blocks(g[2] + bytes(70000), one(cLen=65537), np.zeros(g[3], dtype=np.uint8))
    with pytest.raises(capi.MashmapError, match=r"failed \(-1\): mm_inflate_blocks: output ranges overlap"):      # the failed call's own text,
        ctx.inflate_blocks(g[2], np.concatenate([one(), one()]), np.zeros(g[3], dtype=np.uint8))                  # handed out once:
    assert b"mm_inflate_blocks" not in ctx.lib.mm_last_error(ctx.h)                                               # then the context's own again
    assert ctx.inflate_counts() == (1, len(mixed), sum(z[3] for z in mixed if z[1] == 0))
    two, st = ctx.inflate_blocks(g[2], np.concatenate([one(), one(uOff=g[3])]))                # adjacent is not overlapping
    assert not st.any() and two.tobytes() == g[5] * 2


def test_a_reader_thread_inflates_while_the_context_maps(ctx):
    """the thread exception: mm_inflate_blocks from another thread while the context's own thread is inside other calls"""
    name, refrec, qrec, _ = {c[0]: c for c in CS.paf_cases()}["default"]
    ctx.index_build([a for _, a in refrec])
    ctx.set_tables_default(0.85)
    reads = [a for _, a in qrec]

    def map_once():
        ctx.reads_upload(reads)
        ctx.map()
        return [x.tobytes() for x in ctx.results()] + [ctx.mappings().tobytes()]

    raw = Z.fasta_bytes(2000 * 4096, seed=6)
    items = [(Z.raw_deflate(raw[i * 4096:(i + 1) * 4096]), 4096, zlib.crc32(raw[i * 4096:(i + 1) * 4096])) for i in range(2000)]
    comp, blocks, n = _layout(items, seed=14, gaps=False)
    alone_map = map_once()
    alone_out, alone_status = ctx.inflate_blocks(comp, blocks.copy())
    assert alone_out.tobytes() == raw and not alone_status.any() and len(alone_map[-1]) > 0
    got, errors = [], []

    def reader():
        try:
            for _ in range(3):
                out, status = ctx.inflate_blocks(comp, blocks.copy())
                got.append((out.tobytes(), status.tobytes()))
        except Exception as e:                           # noqa: BLE001 -- reported by the assertion below
            errors.append(e)

    t = threading.Thread(target=reader)
    t.start()
    maps = [map_once()]
    while t.is_alive() and len(maps) < 50:
        maps.append(map_once())
    t.join()
    assert not errors, errors
    assert len(got) == 3 and all(g == (raw, alone_status.tobytes()) for g in got)
    assert all(m == alone_map for m in maps)
    assert ctx.inflate_counts() == (4, 8000, 4 * len(raw))


def test_inflate_bgzf(ctx):
    from mashmap_amd import capi
    raw = Z.fasta_bytes(400000, seed=7)
    for block in (60000, 100):
        data = Z.bgzf_bytes(raw[:400000 if block == 60000 else 30000], block)
        assert ctx.inflate_bgzf(data) == raw[:400000 if block == 60000 else 30000]
    data = bytearray(Z.bgzf_bytes(raw, 60000))
    sizes, at = [], 0
    while at < len(data):
        sizes.append((at, data[at + 16] + (data[at + 17] << 8) + 1)); at += sizes[-1][1]
    assert len(sizes) == 8                                    # seven blocks of payload and the end-of-file block
    data[sizes[3][0] + 18 + 1000] ^= 0x20                       # one flipped bit in the deflate stream of block 3
    with pytest.raises(capi.MashmapError, match=r"block 3 \(at byte %d\)" % sizes[3][0]):
        ctx.inflate_bgzf(bytes(data))
    with pytest.raises(capi.MashmapError, match=r"block 7 "):
        ctx.inflate_bgzf(Z.bgzf_bytes(raw, 60000)[:-3])     # a truncated file is caught by the framing


def _fasta_text(records):
    out = bytearray()
    for name, seq in records:
        s = bytes(seq)
        out += b">" + name.encode() + b"\n" + b"\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + b"\n"
    return bytes(out)


def _cli(td, name, tag, device, corrupt=False):
    _, refrec, qrec, extra = {c[0]: c for c in CS.paf_cases()}[name]
    rf = os.path.join(td, "%s.%s.ref.fa.gz" % (name, tag))
    data = bytearray(Z.bgzf_bytes(_fasta_text(refrec), 60000))
    if corrupt:
        data[18 + 2000] ^= 0x01
    open(rf, "wb").write(bytes(data))
    out = os.path.join(td, "%s.%s.paf" % (name, tag))
    args = [HIP_BIN, "-r", rf, "-o", out, "-t", "4"] + extra
    if qrec is not None:
        qf = os.path.join(td, "%s.%s.q.fa.gz" % (name, tag))
        open(qf, "wb").write(Z.bgzf_bytes(_fasta_text(qrec), 60000))
        args += ["-q", qf]
    env = dict(os.environ, MASHMAP_HIP_TIMING="1")
    env.pop("MASHMAP_HIP_DEVICE_INFLATE", None)
    if device:
        env["MASHMAP_HIP_DEVICE_INFLATE"] = "1"
    p = subprocess.run(args, capture_output=True, text=True, env=env)
    return p, out, rf, (qf if qrec is not None else rf)


@pytest.mark.parametrize("name", ["default", "allvsall_Y"])
def test_the_command_line_on_bgzf_input(name, tmp_path):
    assert os.path.exists(HIP_BIN), "mashmap_hip not built"
    exp = open(os.path.join(PAF_DIR, name + ".paf"), "rb").read()
    assert len(exp) > 0
    # with the switch: the golden PAF, the device inflater named for the reference and for the query, blocks counted
    p, out, rf, qf = _cli(str(tmp_path), name, "dev", True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(out, "rb").read() == exp
    lines = re.findall(r"reader: BGZF (device|host) inflater: (\d+) blocks, \d+ bytes of (\S+) in", p.stderr)
    assert lines and all(kind == "device" and int(n) > 0 for kind, n, _ in lines), lines
    assert {path for _, _, path in lines} == {rf, qf}
    m = re.search(r"device inflater: (\d+) calls, (\d+) blocks, (\d+) bytes", p.stderr)
    assert m and int(m.group(1)) >= 2 and int(m.group(2)) == sum(int(n) for _, n, _ in lines) and int(m.group(3)) > 0
    # without it: the same PAF, the host inflater named, mm_inflate_counts not advanced
    p, out, rf, qf = _cli(str(tmp_path), name, "host", False)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(out, "rb").read() == exp
    lines = re.findall(r"reader: BGZF (device|host) inflater: (\d+) blocks, \d+ bytes of (\S+) in", p.stderr)
    assert lines and all(kind == "host" and int(n) > 0 for kind, n, _ in lines), lines
    assert {path for _, _, path in lines} == {rf, qf}
    assert re.search(r"device inflater: 0 calls, 0 blocks, 0 bytes", p.stderr)


def test_the_command_line_refuses_a_corrupt_bgzf_block(tmp_path):
    p, out, rf, _ = _cli(str(tmp_path), "default", "bad", True, corrupt=True)
    assert p.returncode != 0
    assert "corrupt BGZF block in " + rf in p.stderr and "BGZF" in p.stderr
