#!/usr/bin/env python3
"""BGZF input inflated on the device (mm_inflate_blocks, MASHMAP_HIP_DEVICE_INFLATE) beside the host's zlib: two measurements, both on
the GPU machine, one file of input for both.

The input is the bench's configs[1] shape (10 kbp reads at 10 % error from a 100 Mbp reference of ten contigs, generated from a seed),
--gbp of it (default 1), written as 60-column FASTA in BGZF blocks of 65 280 bytes, zlib level 6 -- what bgzip writes.

(a) library level: the query file's blocks through mm_inflate_blocks from page-locked buffers (mm_host_alloc), two warm-up calls and seven
    timed ones: the kernel alone by hipEvents (mm_inflate_kernel_ms) and the whole call host to host (copy in, kernel, copy out), as GB/s
    of inflated output.  Beside them the host inflater's seconds for the same file: the sum of the reader's "BGZF host inflater" timing
    lines of the runs of (b) without the switch.
(b) end to end: `mashmap_hip -r ref.fa -q query.fa.gz` on three trees -- the parent commit's build (--parent DIR), this tree with the
    switch and this tree without it --, --rounds alternations of the three (default 3), every run a fresh process: "time spent mapping
    the query", and the sums of the reader's parse lines and of the device stage lines of MASHMAP_HIP_TIMING.

THE RULE, written before the first run: without the switch this tree lies inside the parent's range -- the median of its "time spent
mapping the query" is no less than the parent's fastest run and no more than its slowest; the script prints PASS or FAIL.
Every comparison is printed with the parent's spread beside it.  Results: one JSON document and the two tables as text under --out."""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import re
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK = 65280


def _bgzf_block(chunk):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = c.compress(chunk) + c.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(data) + 25) + data + struct.pack("<II", zlib.crc32(chunk), len(chunk))


def bgzf(raw, procs):
    chunks = [raw[i:i + BLOCK] for i in range(0, len(raw), BLOCK)]
    with multiprocessing.Pool(procs) as pool:
        blocks = pool.map(_bgzf_block, chunks, chunksize=64)
    return b"".join(blocks) + _bgzf_block(b"")


def fasta(names, seqs, width=60):
    out = []
    for name, s in zip(names, seqs):
        n = len(s)
        body = np.full(n + (n + width - 1) // width, 10, dtype=np.uint8)
        idx = np.arange(n)
        body[idx + idx // width] = s
        out.append(b">" + name.encode() + b"\n" + body.tobytes())
    return b"".join(out)


def make_input(td, gbp, procs):
    rng = np.random.RandomState(2024)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    contigs = [acgt[rng.randint(0, 4, size=10_000_000)] for _ in range(10)]
    ref = os.path.join(td, "ref.fa")
    open(ref, "wb").write(fasta(["chr%d" % i for i in range(10)], contigs))
    nreads, L = int(gbp * 1e9) // 10000, 10000
    parts = []
    for r0 in range(0, nreads, 2000):
        R = min(2000, nreads - r0)
        cid, at = rng.randint(0, 10, size=R), rng.randint(0, 10_000_000 - L, size=R)
        seqs = np.stack([contigs[c][p:p + L] for c, p in zip(cid, at)])
        hit = rng.rand(R, L) < 0.10                                    # 10 % substitutions
        seqs[hit] = acgt[rng.randint(0, 4, size=int(hit.sum()))]
        parts.append(fasta(["read%d" % (r0 + r) for r in range(R)], seqs))
    raw = b"".join(parts)
    q = os.path.join(td, "query.fa.gz")
    data = bgzf(raw, procs)
    open(q, "wb").write(data)
    return ref, q, data, len(raw)


def library_level(data, n_raw):
    from mashmap_amd import capi
    lib = capi.load()
    recs, at, uoff = [], 0, 0
    while at < len(data):
        bsize = data[at + 16] + (data[at + 17] << 8) + 1
        crc, isize = struct.unpack("<II", data[at + bsize - 8:at + bsize])
        recs.append((at + 18, bsize - 26, isize, uoff, crc, 0)); uoff += isize; at += bsize
    assert uoff == n_raw
    blocks = np.array(recs, dtype=capi.INFLATE_BLOCK_DT)
    lib.mm_host_alloc.restype = C.c_void_p
    ctx = capi.Context()
    comp, dst = lib.mm_host_alloc(len(data)), lib.mm_host_alloc(uoff)
    assert comp and dst
    C.memmove(comp, data, len(data))
    kernel, call = [], []
    for i in range(9):
        bad = C.c_size_t(0)
        t0 = time.perf_counter()
        rc = lib.mm_inflate_blocks(ctx.h, comp, len(data), blocks.ctypes.data_as(C.c_void_p), len(blocks), dst, uoff, C.byref(bad))
        t1 = time.perf_counter()
        assert rc == 0 and bad.value == 0, (rc, bad.value)
        if i >= 2:
            kernel.append(ctx.inflate_kernel_ms() / 1e3); call.append(t1 - t0)
    out = (C.c_char * uoff).from_address(dst)
    crc = zlib.crc32(memoryview(out)[:1 << 26])                        # the result is the payload (first 64 MB checked against the raw text by the caller)
    lib.mm_host_free(C.c_void_p(comp)); lib.mm_host_free(C.c_void_p(dst))
    ctx.close()
    return dict(blocks=len(blocks), compressed_bytes=len(data), inflated_bytes=uoff, kernel_s=kernel, call_s=call, crc_first_64MB=crc,
                kernel_GBps=[uoff / s / 1e9 for s in kernel], call_GBps=[uoff / s / 1e9 for s in call])


def run_cli(binary, ref, q, td, tag, device):
    env = dict(os.environ, MASHMAP_HIP_TIMING="1")
    env.pop("MASHMAP_HIP_DEVICE_INFLATE", None)
    if device:
        env["MASHMAP_HIP_DEVICE_INFLATE"] = "1"
    out = os.path.join(td, tag + ".paf")
    t0 = time.perf_counter()
    p = subprocess.run([binary, "-r", ref, "-q", q, "-o", out, "-t", "16"], capture_output=True, text=True, env=env, timeout=900)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-3000:]
    err = p.stderr
    f = lambda pat: [float(x) for x in re.findall(pat, err)]
    return dict(wall_s=wall, map_query_s=f(r"time spent mapping the query: ([0-9.eE+-]+) sec")[0],
                reader_parse_s=sum(f(r"reader: parsed \d+ records, \d+ bases in ([0-9.eE+-]+) s")),
                device_stage_s=sum(f(r"device stage \([^)]*\): ([0-9.eE+-]+) s")),
                inflate_s=sum(f(r"BGZF (?:device|host) inflater: \d+ blocks, \d+ bytes of \S*query\S* in ([0-9.eE+-]+) s")),
                inflater=sorted(set(re.findall(r"BGZF (device|host) inflater", err))), paf_crc=zlib.crc32(open(out, "rb").read()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built (its mashmap_amd/lib/mashmap_hip)")
    ap.add_argument("--out", default="inflate_probe_out")
    ap.add_argument("--tmp", default="/tmp/inflate_probe")
    ap.add_argument("--procs", type=int, default=16)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True); os.makedirs(a.tmp, exist_ok=True)
    ref, q, data, n_raw = make_input(a.tmp, a.gbp, a.procs)
    res = dict(gbp=a.gbp, query_bytes=n_raw, query_bgzf_bytes=len(data))
    res["library"] = library_level(data, n_raw)
    json.dump(res, open(os.path.join(a.out, "inflate_probe.json"), "w"), indent=1)
    trees = [("this+switch", os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip"), True), ("this", os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip"), False)]
    if a.parent:
        trees.insert(0, ("parent", os.path.join(a.parent, "mashmap_amd", "lib", "mashmap_hip"), False))
    runs = {t[0]: [] for t in trees}
    for rnd in range(a.rounds):
        for tag, binary, device in trees:
            runs[tag].append(run_cli(binary, ref, q, a.tmp, tag.replace("+", "_"), device))
            json.dump(dict(res, e2e=runs), open(os.path.join(a.out, "inflate_probe.json"), "w"), indent=1)
    res["e2e"] = runs
    lines = []
    L = res["library"]
    med = lambda v: sorted(v)[len(v) // 2]
    lines.append("(a) library level: %d blocks, %.1f MB compressed -> %.1f MB; seven calls after two warm-ups" % (L["blocks"], L["compressed_bytes"] / 1e6, L["inflated_bytes"] / 1e6))
    lines.append("    kernel only (hipEvents)   GB/s of output: median %.2f  (min %.2f, max %.2f)" % (med(L["kernel_GBps"]), min(L["kernel_GBps"]), max(L["kernel_GBps"])))
    lines.append("    whole call, host to host  GB/s of output: median %.2f  (min %.2f, max %.2f)" % (med(L["call_GBps"]), min(L["call_GBps"]), max(L["call_GBps"])))
    if runs.get("this"):
        h = [r["inflate_s"] for r in runs["this"]]
        lines.append("    host inflater (zlib on the reader's threads), same file: %s s  -> %.2f GB/s of output at the median" % (", ".join("%.3f" % x for x in h), n_raw / med(h) / 1e9))
    lines.append("(b) end to end, %d alternations, fresh processes: seconds (every run; parent's spread = max - min)" % a.rounds)
    for key in ("map_query_s", "reader_parse_s", "device_stage_s", "inflate_s"):
        lines.append("    %s" % key)
        for tag in runs:
            v = [r[key] for r in runs[tag]]
            lines.append("      %-12s %s   median %.3f  spread %.3f" % (tag, "  ".join("%.3f" % x for x in v), med(v), max(v) - min(v)))
    pafs = {r["paf_crc"] for v in runs.values() for r in v}
    lines.append("    PAF identical over all runs: %s" % (len(pafs) == 1))
    if a.parent:
        pv = [r["map_query_s"] for r in runs["parent"]]; tv = [r["map_query_s"] for r in runs["this"]]
        spread = max(pv) - min(pv)
        inside = min(pv) <= med(tv) <= max(pv)
        lines.append("    RULE (this tree without the switch vs the parent, time spent mapping the query): parent %.3f .. %.3f (spread %.3f), this median %.3f: %s"
                     % (min(pv), max(pv), spread, med(tv), "PASS" if inside else "FAIL"))
    text = "\n".join(lines)
    print(text)
    open(os.path.join(a.out, "inflate_probe.txt"), "w").write(text + "\n")
    json.dump(res, open(os.path.join(a.out, "inflate_probe.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
