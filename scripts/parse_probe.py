#!/usr/bin/env python3
"""FASTA text parsed on the device (mm_text_*, MASHMAP_HIP_DEVICE_PARSE) beside the host reader: two measurements, both on the GPU
machine, on the file scripts/inflate_probe.py generates (same shape, same seed: 10 kbp reads at 10 % error from a 100 Mbp reference,
--gbp of them, 60-column FASTA in BGZF blocks of 65 280 bytes).

(a) library level, GB/s of text: the scan kernels alone and the pack kernel alone (mm_text_kernel_ms), and the whole chain
    mm_text_append_inflated -> mm_text_scan -> mm_text_records -> mm_text_pack (staged) host to host, two warm-up rounds and seven timed
    ones, the file in windows of --window-mb of text.  Beside them the host reader's rate on the same file: text bytes over the sum of
    its "reader: parsed" timing lines in the runs of (b) without the switch.
(b) end to end: `mashmap_hip -r ref.fa -q query.fa.gz -t 16` on three trees -- the parent commit's build (--parent DIR), this tree with
    the switch and this tree without it --, --rounds alternations of the three (default 3), every run a fresh process: "time spent
    mapping the query", and the process's CPU seconds (user + system, getrusage of the child): host CPU is what the switch is to free.

THE RULE, written before the first run: without the switch this tree lies inside the parent's range -- the median of its "time spent
mapping the query" is no less than the parent's fastest run and no more than its slowest; the script prints PASS or FAIL.  The switch
stays off whatever (b) says.  Results: one JSON document and the tables as text under --out."""
import argparse
import ctypes as C
import json
import os
import re
import resource
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import inflate_probe as IP  # noqa: E402


def library_level(data, n_raw, window):
    from mashmap_amd import capi
    lib = capi.load()
    recs, at, uoff = [], 0, 0
    while at < len(data):
        bsize = data[at + 16] + (data[at + 17] << 8) + 1
        crc, isize = struct.unpack("<II", data[at + bsize - 8:at + bsize])
        recs.append((at + 18, bsize - 26, isize, uoff, crc, 0)); uoff += isize; at += bsize
    assert uoff == n_raw
    blocks = np.array(recs, dtype=capi.INFLATE_BLOCK_DT)
    wins, lo, acc = [], 0, 0                                      # windows of blocks whose payloads sum to `window`
    for i, r in enumerate(recs):
        acc += r[2]
        if acc >= window or i == len(recs) - 1:
            wins.append((lo, i + 1)); lo, acc = i + 1, 0
    lib.mm_host_alloc.restype = C.c_void_p
    ctx = capi.Context()
    comp = lib.mm_host_alloc(len(data))
    assert comp
    C.memmove(comp, data, len(data))
    cap = int(window * 1.2) + (1 << 20)
    b2 = np.zeros(cap // 16, dtype=np.uint32); nm = np.zeros(cap // 32, dtype=np.uint32)
    scan_s, pack_s, chain_s, staged_all, n_records = [], [], [], True, 0
    for rnd in range(9):
        ctx.text_reset()
        t_scan = t_pack = 0.0; n_records = 0
        t0 = time.perf_counter()
        for k, (a, b) in enumerate(wins):
            blk = blocks[a:b].copy()
            bad = C.c_size_t(0)
            rc = lib.mm_text_append_inflated(ctx.h, comp, len(data), blk.ctypes.data_as(C.c_void_p), len(blk), C.byref(bad))
            assert rc == 0 and bad.value == 0, (rc, bad.value)
            n, nb, consumed = ctx.text_scan(capi.MM_TEXT_FASTA, k == len(wins) - 1)
            rec, names = ctx.text_records()
            npk, staged = ctx.text_pack(b2, nm, reserve=cap)
            staged_all &= bool(staged) or npk == 0
            ms = ctx.text_kernel_ms(); t_scan += ms[0] / 1e3; t_pack += ms[1] / 1e3; n_records += n
            lib.mm_reads_prefetch_drop(ctx.h)                    # the piece is not uploaded here: the area starts over
        t1 = time.perf_counter()
        if rnd >= 2:
            scan_s.append(t_scan); pack_s.append(t_pack); chain_s.append(t1 - t0)
    lib.mm_host_free(C.c_void_p(comp))
    ctx.close()
    g = lambda v: [n_raw / s / 1e9 for s in v]
    return dict(windows=len(wins), records=n_records, text_bytes=n_raw, staged=staged_all, scan_s=scan_s, pack_s=pack_s, chain_s=chain_s,
                scan_GBps=g(scan_s), pack_GBps=g(pack_s), chain_GBps=g(chain_s))


def run_cli(binary, ref, q, td, tag, device):
    env = dict(os.environ, MASHMAP_HIP_TIMING="1")
    env.pop("MASHMAP_HIP_DEVICE_INFLATE", None); env.pop("MASHMAP_HIP_DEVICE_PARSE", None)
    if device:
        env["MASHMAP_HIP_DEVICE_PARSE"] = "1"
    out = os.path.join(td, tag + ".paf")
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.perf_counter()
    p = subprocess.run([binary, "-r", ref, "-q", q, "-o", out, "-t", "16"], capture_output=True, text=True, env=env, timeout=900)
    wall = time.perf_counter() - t0
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    assert p.returncode == 0, p.stderr[-3000:]
    err = p.stderr
    f = lambda pat: [float(x) for x in re.findall(pat, err)]
    return dict(wall_s=wall, map_query_s=f(r"time spent mapping the query: ([0-9.eE+-]+) sec")[0],
                cpu_s=(r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime),
                reader_parse_s=sum(f(r"reader: parsed \d+ records, \d+ bases in ([0-9.eE+-]+) s")),
                device_parser_s=sum(f(r"reader: device parser: .* in ([0-9.eE+-]+) s")),
                scans=int((re.findall(r"device parser: (\d+) scans", err) or ["0"])[0]), paf_crc=zlib.crc32(open(out, "rb").read()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built (its mashmap_amd/lib/mashmap_hip)")
    ap.add_argument("--out", default="parse_probe_out")
    ap.add_argument("--tmp", default="/tmp/parse_probe")
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--window-mb", type=float, default=512.0)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True); os.makedirs(a.tmp, exist_ok=True)
    ref, q, data, n_raw = IP.make_input(a.tmp, a.gbp, a.procs)
    res = dict(gbp=a.gbp, query_bytes=n_raw, query_bgzf_bytes=len(data))
    res["library"] = library_level(data, n_raw, int(a.window_mb * 1e6))
    dump = lambda: json.dump(res, open(os.path.join(a.out, "parse_probe.json"), "w"), indent=1)
    dump()
    here = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
    trees = [("this+switch", here, True), ("this", here, False)]
    if a.parent:
        trees.insert(0, ("parent", os.path.join(a.parent, "mashmap_amd", "lib", "mashmap_hip"), False))
    runs = {t[0]: [] for t in trees}
    res["e2e"] = runs
    for rnd in range(a.rounds):
        for tag, binary, device in trees:
            runs[tag].append(run_cli(binary, ref, q, a.tmp, tag.replace("+", "_"), device))
            dump()
    med = lambda v: sorted(v)[len(v) // 2]
    L = res["library"]
    lines = ["(a) library level: %.1f MB of text, %d records, %d windows, staged: %s; seven rounds after two warm-ups, GB/s of text" % (n_raw / 1e6, L["records"], L["windows"], L["staged"])]
    for key, what in (("scan_GBps", "scan kernels only (hipEvents)"), ("pack_GBps", "pack kernel only (hipEvents) "), ("chain_GBps", "whole chain, host to host    ")):
        lines.append("    %s median %.2f  (min %.2f, max %.2f)" % (what, med(L[key]), min(L[key]), max(L[key])))
    if runs.get("this"):
        h = [r["reader_parse_s"] for r in runs["this"]]
        lines.append("    host reader (parse and pack on its threads), same file: %s s  -> %.2f GB/s of text at the median" % (", ".join("%.3f" % x for x in h), n_raw / med(h) / 1e9))
    lines.append("(b) end to end, %d alternations, fresh processes: seconds (every run; spread = max - min)" % a.rounds)
    for key in ("map_query_s", "cpu_s", "reader_parse_s", "device_parser_s"):
        lines.append("    %s" % key)
        for tag in runs:
            v = [r[key] for r in runs[tag]]
            lines.append("      %-12s %s   median %.3f  spread %.3f" % (tag, "  ".join("%.3f" % x for x in v), med(v), max(v) - min(v)))
    lines.append("    scans with the switch: %s; without: %s" % ([r["scans"] for r in runs["this+switch"]], [r["scans"] for r in runs["this"]]))
    lines.append("    PAF identical over all runs: %s" % (len({r["paf_crc"] for v in runs.values() for r in v}) == 1))
    if a.parent:
        pv = [r["map_query_s"] for r in runs["parent"]]; tv = [r["map_query_s"] for r in runs["this"]]
        lines.append("    RULE (this tree without the switch vs the parent, time spent mapping the query): parent %.3f .. %.3f (spread %.3f), this median %.3f: %s"
                     % (min(pv), max(pv), max(pv) - min(pv), med(tv), "PASS" if min(pv) <= med(tv) <= max(pv) else "FAIL"))
    text = "\n".join(lines)
    print(text)
    open(os.path.join(a.out, "parse_probe.txt"), "w").write(text + "\n")
    dump()


if __name__ == "__main__":
    main()
