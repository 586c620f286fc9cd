"""Shared by tests/test_inflate_core.py and tests/test_gpu_inflate.py: builds tests/hostlogic/inflate_check.cpp (a stand-alone program,
-lz; with -fsanitize=address,undefined for the CPU suite, plain for the GPU module) and reads the zoo it dumps -- the hand-built
streams, the named malformed blocks and generated
blocks at the GPU test's lengths, every one of them run through mm_inflate_core.h under the sanitizers by the program that wrote it."""
import os
import subprocess
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS = ["OK", "BAD_STREAM", "TRUNCATED", "OVERRUN", "SHORT", "BAD_DISTANCE", "BAD_CRC"]


def build_check(tmpdir, sanitize=True):
    """sanitize=True: the CPU suite's build (address and undefined-behaviour sanitizers).  sanitize=False: a plain -O1 build for the GPU
    module, which only needs the program to write the zoo out: no sanitizer runs in a test marked gpu (the bytes it writes do not
    depend on the build, and the sanitized run over them is tests/test_inflate_core.py's)."""
    exe = os.path.join(str(tmpdir), "inflate_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "hostlogic", "inflate_check.cpp"), "-lz"])
    return exe


def load_zoo(exe, tmpdir):
    """[(name, expected status, comp bytes, uLen, crc32, payload bytes)]"""
    path = os.path.join(str(tmpdir), "zoo.bin")
    p = subprocess.run([exe, "--dump", path], capture_output=True, text=True)
    assert p.returncode == 0, "inflate_check --dump failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    data = open(path, "rb").read()
    items, at = [], 0
    while at < len(data):
        nl = data.index(b"\n", at)
        name, expect, ulen, crc, clen, plen = data[at:nl].split()
        at = nl + 1
        comp = data[at:at + int(clen)]; at += int(clen)
        payload = data[at:at + int(plen)]; at += int(plen)
        items.append((name.decode(), int(expect), comp, int(ulen), int(crc), payload))
    return items


def fasta_bytes(n, seed=1, cols=60):
    """n bytes of 60-column random-ACGT FASTA"""
    import numpy as np
    rng = np.random.RandomState(seed)
    rows = n // (cols + 1) + 2
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, size=(rows, cols + 1))].copy()
    a[:, cols] = 10
    return (b">chr1\n" + a.tobytes())[:n]


def raw_deflate(chunk, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(chunk) + c.flush()


def bgzf_bytes(raw, block=60000, eof=True):
    """`raw` as a BGZF file: blocks of `block` bytes and the empty end-of-file block (the writer of tests/test_seq_parse.py)"""
    import struct
    out = bytearray()
    for i in list(range(0, len(raw), block)) + ([None] if eof else []):
        chunk = b"" if i is None else raw[i:i + block]
        data = raw_deflate(chunk)
        bsize = len(data) + 25
        out += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize) + data + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)
