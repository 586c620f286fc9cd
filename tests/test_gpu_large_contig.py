"""The mashmap_hip command line compiled with -DLARGE_CONTIG (64-bit offset_t on the host, the reference's LARGE_CONTIG index files), end
to end on the device: below 2^31 it writes the PAF of mashmap_hip and of the stock LARGE_CONTIG binary byte for byte, its --saveIndex
files load in the stock LARGE_CONTIG binary and the other way round, and an index file with a position the device's 32-bit index cannot
hold is refused, not truncated."""
import os
import subprocess

import numpy as np
import pytest

import mmutil as U
from golden import cases as CS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mashmap_amd", "host")
LIB = os.path.join(ROOT, "mashmap_amd", "lib")
REF_LARGE_BIN = os.path.join(ROOT, "oracle", "_ref", "large_contig", "mashmap_ref")
PAF_DIR = os.path.join(ROOT, "tests", "golden", "paf")
CASES = {c[0]: c for c in CS.paf_cases()}
MDT = np.dtype([("hash", "<u8"), ("wpos", "<i8"), ("wpos_end", "<i8"), ("seqId", "<i4"), ("strand", "<i2"), ("pad", "<i2")])
PDT = np.dtype([("pos", "<i8"), ("hash", "<u8"), ("seqId", "<i4"), ("side", "i1"), ("pad1", "i1", (3,))])


@pytest.fixture(scope="module")
def large_bin(tmp_path_factory):
    """the recipe of mashmap_amd/host/Makefile's mashmap_hip plus -DLARGE_CONTIG"""
    out = str(tmp_path_factory.mktemp("lc") / "mashmap_hip_lc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-sign-compare", "-DLARGE_CONTIG", "-o", out,
                           os.path.join(HOST, "mashmap_hip_main.cpp"), "-L" + LIB, "-lmashmap_hip", "-Wl,-rpath," + LIB, "-lz", "-lpthread"],
                          timeout=300)
    return out


def _stock_large():
    """the stock LARGE_CONTIG binary: build() makes it beside oracle/_ref/mashmap_ref, so one without the other is a broken build"""
    if os.path.exists(U.REF_BIN):
        assert os.path.exists(REF_LARGE_BIN), "oracle/_ref/mashmap_ref is there but oracle/_ref/large_contig/mashmap_ref is not"
        return REF_LARGE_BIN
    return None


def _run(binary, td, name, extra, tag, expect_ok=True):
    _, refrec, qrec, cext = CASES[name]
    rf = os.path.join(td, name + ".ref.fa")
    if not os.path.exists(rf):
        U.write_fasta(rf, refrec)
    out = os.path.join(td, "%s.%s.paf" % (name, tag))
    args = [binary, "-r", rf, "-o", out, "-t", "4"] + cext + extra
    if qrec is not None:
        qf = os.path.join(td, name + ".q.fa")
        if not os.path.exists(qf):
            U.write_fasta(qf, qrec)
        args += ["-q", qf]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    if not expect_ok:
        return p
    assert p.returncode == 0, p.stderr[-2000:]
    return open(out, "rb").read()


def _read_index_files(prefix):
    raw = open(prefix + ".index", "rb").read()
    n = int(np.frombuffer(raw[:8], dtype="<u8")[0])
    assert len(raw) == 8 + n * MDT.itemsize
    mins = np.frombuffer(raw[8:], dtype=MDT, count=n)
    raw = open(prefix + ".map", "rb").read()
    nk = int(np.frombuffer(raw[:8], dtype="<u8")[0])
    off, keys, lists = 8, [], []
    for _ in range(nk):
        key, cnt = np.frombuffer(raw[off:off + 16], dtype="<u8")
        off += 16
        pts = np.frombuffer(raw[off:off + PDT.itemsize * int(cnt)], dtype=PDT)
        off += PDT.itemsize * int(cnt)
        keys.append(int(key)); lists.append([(int(p["pos"]), int(p["hash"]), int(p["seqId"]), int(p["side"])) for p in pts])
    assert off == len(raw)
    return [tuple(int(m[f]) for f in ("hash", "wpos", "wpos_end", "seqId", "strand")) for m in mins], keys, lists


@pytest.mark.parametrize("name", ["default", "dense_pi80", "asm_one2one", "allvsall_Y", "allvsall_X_lower", "nosplit"])
def test_large_build_writes_the_default_paf(name, tmp_path, large_bin):
    """the golden PAF of tests/golden/paf (the stock default binary's, which mashmap_hip reproduces) and the stock LARGE_CONTIG binary's"""
    got = _run(large_bin, str(tmp_path), name, [], "large")
    exp = open(os.path.join(PAF_DIR, name + ".paf"), "rb").read()
    assert len(exp) > 0 and got == exp
    stock = _stock_large()
    if stock:
        assert _run(stock, str(tmp_path), name, [], "reflarge") == exp


def test_large_index_files_interoperate_with_the_stock_large_binary(tmp_path, large_bin):
    exe, stock = large_bin, _stock_large()
    td = str(tmp_path)
    exp = open(os.path.join(PAF_DIR, "default.paf"), "rb").read()
    assert _run(exe, td, "default", ["--saveIndex", td + "/hipidx"], "hsave") == exp
    mine = _read_index_files(td + "/hipidx")
    assert len(mine[0]) > 1000 and len(mine[1]) > 500
    assert _run(exe, td, "default", ["--loadIndex", td + "/hipidx"], "hload") == exp
    assert _run(exe, td, "default", ["--saveIndex", td + "/hip.tsv"], "htsv") == exp
    assert _run(exe, td, "default", ["--loadIndex", td + "/hip.tsv"], "htsvload") == exp
    if stock:
        assert _run(stock, td, "default", ["--saveIndex", td + "/refidx"], "rsave") == exp
        theirs = _read_index_files(td + "/refidx")
        assert mine[0] == theirs[0], "minmerIndex on disk differs"
        assert mine[1] == theirs[1], "lookup keys (or their order) differ"
        assert mine[2] == theirs[2], "interval point lists differ"
        assert _run(exe, td, "default", ["--loadIndex", td + "/refidx"], "hloadref") == exp
        assert _run(stock, td, "default", ["--loadIndex", td + "/hipidx"], "rloadhip") == exp
    # a record beyond INT32_MAX (a file of a contig the device's 32-bit index cannot hold) is refused with a message, not wrapped
    raw = bytearray(open(td + "/hipidx.index", "rb").read())
    rec = np.frombuffer(raw, dtype=MDT, count=1, offset=8).copy()
    rec["wpos_end"] = (1 << 31) + 7
    raw[8:8 + MDT.itemsize] = rec.tobytes()
    open(td + "/bad.index", "wb").write(bytes(raw))
    open(td + "/bad.map", "wb").write(open(td + "/hipidx.map", "rb").read())
    p = _run(exe, td, "default", ["--loadIndex", td + "/bad"], "bad", expect_ok=False)
    assert p.returncode == 1 and "holds position 2147483655" in p.stderr, p.stderr[-600:]
