#!/usr/bin/env python3
"""scripts/paf_probe.py -- what writing a pass's PAF lines on the device (mm_paf_rows) changes, measured against the parent's best
existing path (MASHMAP_HIP_DEVICE_CHAIN=1 alone), in one run.  Modelled on scripts/chain_probe.py, whose helpers it uses.

Part 1, the C ABI stage, one context, the configs[1] shape at bench.py's size (1 M reads of 10 kbp against 100 Mbp; --reads scales it):
the batch is mapped twice (the second pass is a steady-state one) and chained (mm_chain_reads), then three times on the resident rows --
  host    the stage as it is: download the rows (mm_chain_download), mmh_paf_text (MapPost::finishRows + appendReadMappings, one thread:
          the reference for the bytes, not for the time -- the command line runs that code on 16 threads, part 2)
  device  mm_paf_rows bracketed with events on the context's stream (measure, scan, offsets; the one host wait), then the download of
          text and offsets, which waits for k_paf_write: device milliseconds of the call, milliseconds and bytes of the download
-- and whether the device's text is the host's byte for byte.

Part 2, the command line: mashmap_hip FASTA -> PAF, -t 16, on the same workload's files in three alternations of
  chain       MASHMAP_HIP_DEVICE_CHAIN=1
  chain+paf   MASHMAP_HIP_DEVICE_CHAIN=1 MASHMAP_HIP_DEVICE_PAF=1
with, per run: 'time spent mapping the query', the post stage's summed seconds, the process's CPU-seconds (user + system, from the
children's resource usage), the bytes the device stage downloaded (left-over records, rows, text, offsets and flags), and whether the
PAF is byte-identical to the first `chain` run's.  Every run has a time limit (--run-timeout); behind a run that fails or does not end
in time nothing more is started: the probe writes what it has and exits with a non-zero status.

Prints one JSON document (and writes it to --out).  The spread of the `chain` runs is the parent's own spread: the summary says whether
every `chain+paf` figure lies inside it."""
import argparse
import json
import os
import re
import resource
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_workloads import WORKLOADS, contiguous_views, log, make_reads, make_reference, write_fasta  # noqa: E402
from chain_probe import THREADS, StreamEvents, cpu_seconds  # noqa: E402


def part1(torch, dev, W, nreads, out):
    from mashmap_amd import capi
    import pafrows
    K, SEG, S, PI, L = W["k"], W["seg"], W["sketch"], W["pi"], W["read_len"]
    contigs = make_reference(torch, dev, W["ref_contigs"], W["ref_contig_len"])
    ref_np = contiguous_views(torch, contigs)
    ctx = capi.Context(k=K, segLength=SEG, sketchSize=S, flags=capi.MM_FLAG_HG_FILTER)
    ctx.index_build(ref_np, kmerPct=0.001)
    ctx.set_tables_default(PI)
    ctx.set_chain_tables(SEG, 1, 0, 0, True, capi.MM_CHAIN_FILTER_QUERY, 0.0)
    ref_names = ["chr%d" % i for i in range(len(ref_np))]
    clens = [len(a) for a in ref_np]
    ctx.set_paf_tables(ref_names, clens, lenIdThreshold=min(0.7, float(np.float32(PI)) ** 3))
    reads_t = make_reads(torch, dev, contigs, nreads, L, W["err"], seed=4242, chunk=max(64, 8192 * 10000 // L))
    torch.cuda.synchronize()
    offs = np.arange(nreads + 1, dtype=np.int64) * L
    ctx.reads_upload_device(reads_t.data_ptr(), reads_t.numel(), offs)
    del reads_t
    ctx.map(); ctx.map(); ctx.synchronize()
    ctx.chain_reads()
    names = [b"read%07d" % i for i in range(nreads)]
    rl = np.full(nreads, L, dtype=np.int32)
    ev = StreamEvents(ctx.lib.mm_stream(ctx.h))
    forms = {"host": [], "device": []}
    for rep in range(3):
        t0 = time.perf_counter()
        rows = ctx.chain_rows()
        dl = time.perf_counter() - t0
        c0 = cpu_seconds(); t0 = time.perf_counter()
        want, woff, _ = pafrows.host_text(rows, rl, names, ref_names, clens, k=K, s=S, pi=PI)
        forms["host"].append(dict(download_ms=round(dl * 1e3, 3), download_bytes=int(rows.nbytes), host_ms=round((time.perf_counter() - t0) * 1e3, 3),
                                  host_cpu_s=round(cpu_seconds() - c0, 4), text_bytes=len(want), rows=int(len(rows))))
        c0 = cpu_seconds()
        ev.start(); t0 = time.perf_counter()
        ctx.paf_rows(names)
        wall_stage = time.perf_counter() - t0
        dev_ms = ev.elapsed()
        cnt = ctx.paf_counts()
        t0 = time.perf_counter()
        text = ctx.paf_text(); off, handed = ctx.paf_offsets(nreads)
        dl = time.perf_counter() - t0
        forms["device"].append(dict(device_ms_before_the_wait=dev_ms, stage_wall_ms=round(wall_stage * 1e3, 3), download_and_write_ms=round(dl * 1e3, 3),
                                    download_bytes=int(len(text) + off.nbytes + handed.nbytes), host_cpu_s=round(cpu_seconds() - c0, 4), counts=cnt,
                                    same_as_host=bool(text == want and off.tolist() == woff.tolist() and not handed.any())))
        log("[paf_probe] alternation %d: host %r | device %r" % (rep, forms["host"][-1], forms["device"][-1]))
    out["c_abi"] = dict(reads=nreads, read_len=L, forms=forms)
    ctx.close()
    return ref_np, contigs


def part2(torch, dev, W, nreads, ref_np, contigs, out, run_timeout):
    exe = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
    L = W["read_len"]
    td = tempfile.mkdtemp(prefix="mm_paf_probe_")
    try:
        need = nreads * (L + 14) + sum(len(a) for a in ref_np) * 1.02 + (2 << 30)
        free = shutil.disk_usage(td).free
        if free < need:                                             # as bench_e2e.py: fewer reads where the scratch disk is small
            nreads = max(1000, int(nreads * (free - (3 << 30)) / need))
            log("[paf_probe] %.1f GB free under %s: the command line gets %d reads" % (free / 1e9, td, nreads))
        rp, qp = os.path.join(td, "ref.fa"), os.path.join(td, "reads.fa")
        write_fasta(rp, ["chr%d" % i for i in range(len(ref_np))], ref_np)
        with open(qp, "wb") as f:
            for r0 in range(0, nreads, 100_000):
                n = min(100_000, nreads - r0)
                rd = make_reads(torch, dev, contigs, n, L, W["err"], seed=5000 + r0).cpu().numpy().reshape(n, L)
                hdr = np.frombuffer(b"".join(b">read%07d\n" % (r0 + i) for i in range(n)), dtype=np.uint8).reshape(n, 13)
                f.write(np.concatenate([hdr, rd, np.full((n, 1), 10, dtype=np.uint8)], axis=1).tobytes())
        runs = {"chain": [], "chain+paf": []}
        first_paf, stopped = None, None
        for rep, tag in [(rep, tag) for rep in range(3) for tag in ("chain", "chain+paf")]:
            env = {k: v for k, v in os.environ.items() if k not in ("MASHMAP_HIP_DEVICE_CHAIN", "MASHMAP_HIP_DEVICE_PAF")}
            env["MASHMAP_HIP_TIMING"] = "1"; env["MASHMAP_HIP_DEVICE_CHAIN"] = "1"
            if tag == "chain+paf":
                env["MASHMAP_HIP_DEVICE_PAF"] = "1"
            op = os.path.join(td, tag.replace("+", "_") + ".paf")
            r0 = resource.getrusage(resource.RUSAGE_CHILDREN); t0 = time.time()
            try:
                p = subprocess.run([exe, "-r", rp, "-q", qp, "-o", op, "-t", str(THREADS), "-s", str(W["seg"]), "--pi", str(int(round(W["pi"] * 100))), "-J", str(W["sketch"])],
                                   capture_output=True, text=True, env=env, timeout=run_timeout)
            except subprocess.TimeoutExpired:
                stopped = "command line %s, run %d: no end within %d s" % (tag, rep, run_timeout)
                runs[tag].append({"error": stopped})
                break
            wall = time.time() - t0
            r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
            if p.returncode != 0:
                stopped = "command line %s, run %d: status %d" % (tag, rep, p.returncode)
                runs[tag].append({"error": stopped, "stderr": p.stderr[-400:]})
                break
            post = [float(x) for x in re.findall(r"post stage: chain \+ filter \+ format ([0-9.eE+-]+) s", p.stderr)]
            map_s = float(re.search(r"time spent mapping the query\s*:\s*([0-9.eE+-]+)", p.stderr).group(1))
            back = re.findall(r"download of (\d+) left-over candidate mappings and (\d+) chained rows\)", p.stderr)
            text = re.findall(r"\[(\d+) bytes of PAF text of (\d+) chained rows written on the device, (\d+) reads handed over\]", p.stderr)
            left = sum(int(a) for a, _ in back)
            if tag == "chain":
                dl_bytes = left * 48 + sum(int(b) for _, b in back) * 72
            else:                                                    # text + offsets (8 a read and pass) + flags; rows only behind a hand-over
                dl_bytes = left * 48 + sum(int(a) for a, _, _ in text) + 9 * nreads + sum(int(b) * 72 for _, b, h in text if int(h))
            paf = open(op, "rb").read()
            if first_paf is None:
                first_paf = paf
            runs[tag].append(dict(map_s=map_s, wall_s=round(wall, 3), post_s=round(sum(post), 4), gbps=round(nreads * L / map_s / 1e9, 3),
                                  host_cpu_s=round((r1.ru_utime + r1.ru_stime) - (r0.ru_utime + r0.ru_stime), 3), downloaded_bytes=int(dl_bytes),
                                  device_text_bytes=sum(int(a) for a, _, _ in text) if tag == "chain+paf" else None,
                                  handed_reads=sum(int(h) for _, _, h in text) if tag == "chain+paf" else None, paf_identical=bool(paf == first_paf), paf_bytes=len(paf)))
            log("[paf_probe] command line %s, run %d: %r" % (tag, rep, runs[tag][-1]))
        summary = {}
        ok = [r for r in runs["chain"] if "error" not in r]
        new = [r for r in runs["chain+paf"] if "error" not in r]
        for key in ("map_s", "post_s", "host_cpu_s"):
            if ok and new:
                lo, hi = min(r[key] for r in ok), max(r[key] for r in ok)
                summary[key] = dict(parent_spread=[lo, hi], switch=[r[key] for r in new],
                                    inside_parent_spread=bool(all(lo <= r[key] <= hi for r in new)), all_below_parent=bool(all(r[key] < lo for r in new)))
        out["command_line"] = dict(reads=nreads, threads=THREADS, runs=runs, stopped=stopped, summary=summary)
        return stopped
    finally:
        shutil.rmtree(td, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=WORKLOADS["configs1"]["reads"])
    ap.add_argument("--cli-reads", type=int, default=WORKLOADS["configs1"]["reads"])
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--run-timeout", type=int, default=120, help="seconds one mashmap_hip run of part 2 may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    W = WORKLOADS["configs1"]
    out = {"workload": "configs1"}
    ref_np, contigs = part1(torch, dev, W, a.reads, out)
    stopped = None if a.no_cli else part2(torch, dev, W, a.cli_reads, ref_np, contigs, out, a.run_timeout)
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(doc)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
