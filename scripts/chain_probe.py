#!/usr/bin/env python3
"""scripts/chain_probe.py -- what moving the tail of Map::mapModule to the device (mm_chain_reads) changes, measured against the
stage as it was, in one run.

Part 1, one context, the configs[1] shape at bench.py's size (1 M reads of 10 kbp against 100 Mbp; --reads scales it): the batch is
mapped once, then three alternations of two forms on the resident candidate mappings --
  A  the stage as it was: download all records (mm_mappings_download), mmh_post_batch on 16 threads
  B  mm_chain_reads, download rows and left-over records, mmh_post_chained (finishRows / mapModuleFromRecords) on 16 threads
-- and per form: device milliseconds of the stage (events on mm_stream around mm_chain_reads; form A has no device stage), download
milliseconds and bytes, host wall time and CPU-seconds, the share of reads handed over, the reported mappings (both forms must agree).

With --chain-long a third form joins every alternation of part 1 --
  C  form B with MM_OPT_CHAIN_LONG set: reads of 17 .. 512 records are chained on the device by k_chain_reads_long
-- on the same resident records (on configs[1] no read is long: C then costs what the list counter and an empty kernel cost), and
part 1 runs a second time on a long-read workload (key "long_reads"): reads of 100 kbp (--long-read-len) at the same segLength against the
same reference, --long-reads of them, about 20 records a read in one chain, where form B hands every read over.

Part 2, the command line: mashmap_hip FASTA -> PAF on the same workload's files without and with MASHMAP_HIP_DEVICE_CHAIN, three times
alternating, with the stage lines of MASHMAP_HIP_TIMING ('time spent mapping the query', device stage, post stage); the PAFs must be equal.
Every run has a time limit (--run-timeout); behind a run that fails or does not end in time nothing more is started: the probe writes
what it has and exits with a non-zero status.

--groups NAME is a workload of its own, one per invocation (the caller gives every invocation a time limit of its own and starts nothing
behind one that failed): MM_OPT_CHAIN_MODES on a reference of 8 groups -- S0#1#chr .. S7#1#chr, copies of one 12 Mbp sequence with
0 .. 3.5 % substitutions -- at segLength 5000:
  y10k      200 000 reads of 10 kbp under -Y '#' (MM_FLAG_SKIP_PREFIX): a record per fragment and group, about 14 a read
  y50k      40 000 reads of 50 kbp under -Y '#': about 70 a read, the wave-per-read kernel's
  nosplit   100 000 reads of 12 kbp under --noSplit (MM_FLAG_NO_SPLIT)
Three alternations on the same resident records of
  A  the stage as it was: download all records, the host stage (mmh_post_chained_modes without rows) on 16 threads
  C  MM_OPT_CHAIN_LONG and MM_OPT_CHAIN_MODES set: mm_chain_reads, download rows and left-over records, the host stage on both
The reported mappings of the two forms must be byte-identical: the probe stops before it prints a time when they are not.  --scale
shrinks the read counts; --device-only measures form C's device milliseconds alone (the A/B of two builds of the library).

Prints one JSON document (and writes it to --out).  Every figure is read against form A / the run without the switch of the SAME run."""
import argparse
import ctypes as C
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
from bench_workloads import WORKLOADS, contiguous_views, log, make_reads, make_reference, write_fasta  # noqa: E402

THREADS = 16


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


class StreamEvents:
    """hipEvent brackets on the context's own stream, through the HIP runtime the process has loaded (one file: the library's and
    torch's are the same one); elapsed() is None when the process holds two runtimes, and the caller reports wall time alone"""

    def __init__(self, stream):
        paths = sorted({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l})
        self.hip = C.CDLL(paths[0]) if len(paths) == 1 else None
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        if self.hip is not None and (self.hip.hipEventCreate(C.byref(self.a)) != 0 or self.hip.hipEventCreate(C.byref(self.b)) != 0):
            self.hip = None

    def start(self):
        if self.hip is not None:
            self.hip.hipEventRecord(self.a, self.stream)

    def elapsed(self):
        if self.hip is None:
            return None
        ms = C.c_float()
        if self.hip.hipEventRecord(self.b, self.stream) != 0 or self.hip.hipEventSynchronize(self.b) != 0 or self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) != 0:
            return None
        return round(float(ms.value), 3)


def part1(torch, dev, W, nreads, out, chain_long=False, L=None, key="one_context", ref=None):
    from mashmap_amd import capi, shard
    host = shard.host_lib()
    K, SEG, S, PI = W["k"], W["seg"], W["sketch"], W["pi"]
    L = W["read_len"] if L is None else L
    contigs = make_reference(torch, dev, W["ref_contigs"], W["ref_contig_len"]) if ref is None else ref[1]
    ref_np = contiguous_views(torch, contigs) if ref is None else ref[0]
    ctx = capi.Context(k=K, segLength=SEG, sketchSize=S, flags=capi.MM_FLAG_HG_FILTER)
    ctx.index_build(ref_np, kmerPct=0.001)
    ctx.set_tables_default(PI)
    ctx.set_chain_tables(SEG, 1, 0, 0, True, capi.MM_CHAIN_FILTER_QUERY, 0.0)
    reads_t = make_reads(torch, dev, contigs, nreads, L, W["err"], seed=4242, chunk=max(64, 8192 * 10000 // L))      # the same bytes a chunk at any read length
    torch.cuda.synchronize()
    offs = np.arange(nreads + 1, dtype=np.int64) * L
    ctx.reads_upload_device(reads_t.data_ptr(), reads_t.numel(), offs)
    del reads_t
    ctx.map(); ctx.map(); ctx.synchronize()                        # the second pass is a steady-state one: the records of a run in progress
    clens = np.array([len(a) for a in ref_np], dtype=np.int32); rl = np.full(nreads, L, dtype=np.int32)
    ev = StreamEvents(ctx.lib.mm_stream(ctx.h))
    forms = {"A": [], "B": [], "C": []} if chain_long else {"A": [], "B": []}
    for rep in range(3):
        # ---- A
        t0 = time.perf_counter()
        recs = ctx.mappings()
        dl = time.perf_counter() - t0
        sec = C.c_double(); c0 = cpu_seconds(); t0 = time.perf_counter()
        rows_a = np.zeros(len(recs) + 1, dtype=np.dtype([("i", "<i4", 10), ("f", "<f4", 2)]))
        na = host.mmh_post_batch(K, SEG, S, PI, 1, 1, 1, len(clens), clens.ctypes.data, recs.ctypes.data, len(recs), rl.ctypes.data, nreads, 0, THREADS,
                                 C.byref(sec), rows_a.ctypes.data, len(rows_a))
        forms["A"].append(dict(device_ms=0.0, download_ms=round(dl * 1e3, 3), download_bytes=int(recs.nbytes), host_ms=round((time.perf_counter() - t0) * 1e3, 3),
                               host_cpu_s=round(cpu_seconds() - c0, 4), reported=int(na), records=int(len(recs))))
        # ---- B
        ev.start(); t0 = time.perf_counter()
        ctx.chain_reads()
        wall_stage = time.perf_counter() - t0
        dev_ms = ev.elapsed()
        cnt = ctx.chain_counts()
        t0 = time.perf_counter()
        rows = ctx.chain_rows(); left = ctx.chain_leftover()
        dl = time.perf_counter() - t0
        c0 = cpu_seconds(); t0 = time.perf_counter()
        rows_b = np.zeros(len(recs) + 1, dtype=rows_a.dtype)
        nb = host.mmh_post_chained(K, SEG, S, PI, 1, 1, 1, 1, SEG, SEG, len(clens), clens.ctypes.data, rows.ctypes.data if len(rows) else None, len(rows),
                                   left.ctypes.data if len(left) else None, len(left), rl.ctypes.data, nreads, 0, THREADS, None, rows_b.ctypes.data, None, None, len(rows_b))
        forms["B"].append(dict(device_ms=dev_ms, stage_wall_ms=round(wall_stage * 1e3, 3), download_ms=round(dl * 1e3, 3),
                               download_bytes=int(rows.nbytes + left.nbytes), host_ms=round((time.perf_counter() - t0) * 1e3, 3), host_cpu_s=round(cpu_seconds() - c0, 4),
                               reported=int(nb), rows=int(len(rows)), leftover_records=int(len(left)), offered=cnt["offered"], finished=cnt["finished"],
                               handed_over_share=round(1 - cnt["finished"] / max(1, cnt["offered"]), 6), same_as_A=bool(na == nb and rows_a[:na].tobytes() == rows_b[:nb].tobytes())))
        log("[chain_probe] alternation %d: A %r | B %r" % (rep, forms["A"][-1], forms["B"][-1]))
        if chain_long:
            # ---- C
            ctx.chain_long(True)
            ev.start(); t0 = time.perf_counter()
            ctx.chain_reads()
            wall_stage = time.perf_counter() - t0
            dev_ms = ev.elapsed()
            cnt, lcnt = ctx.chain_counts(), ctx.chain_long_counts()
            t0 = time.perf_counter()
            rows = ctx.chain_rows(); left = ctx.chain_leftover()
            dl = time.perf_counter() - t0
            ctx.chain_long(False)
            c0 = cpu_seconds(); t0 = time.perf_counter()
            rows_c = np.zeros(len(recs) + 1, dtype=rows_a.dtype)
            nc = host.mmh_post_chained(K, SEG, S, PI, 1, 1, 1, 1, SEG, SEG, len(clens), clens.ctypes.data, rows.ctypes.data if len(rows) else None, len(rows),
                                       left.ctypes.data if len(left) else None, len(left), rl.ctypes.data, nreads, 0, THREADS, None, rows_c.ctypes.data, None, None, len(rows_c))
            forms["C"].append(dict(device_ms=dev_ms, stage_wall_ms=round(wall_stage * 1e3, 3), download_ms=round(dl * 1e3, 3),
                                   download_bytes=int(rows.nbytes + left.nbytes), host_ms=round((time.perf_counter() - t0) * 1e3, 3), host_cpu_s=round(cpu_seconds() - c0, 4),
                                   reported=int(nc), rows=int(len(rows)), leftover_records=int(len(left)), offered=cnt["offered"], finished=cnt["finished"],
                                   long_offered=lcnt["offered"], long_finished=lcnt["finished"],
                                   handed_over_share=round(1 - cnt["finished"] / max(1, cnt["offered"]), 6), same_as_A=bool(na == nc and rows_a[:na].tobytes() == rows_c[:nc].tobytes())))
            log("[chain_probe] alternation %d: C %r" % (rep, forms["C"][-1]))
    nrec = np.bincount(recs["querySeqId"], minlength=nreads)
    out[key] = dict(reads=nreads, read_len=L, host_threads=THREADS, forms=forms,
                              records_per_read={"mean": round(float(nrec.mean()), 3), "max": int(nrec.max()), "reads_above_16": int((nrec > 16).sum()),
                                                "histogram_0_to_17plus": np.bincount(np.minimum(nrec, 17), minlength=18).tolist()})
    ctx.close()
    return ref_np, contigs


def part2(torch, dev, W, nreads, ref_np, contigs, out, run_timeout):
    exe = os.path.join(ROOT, "mashmap_amd", "lib", "mashmap_hip")
    L = W["read_len"]
    td = tempfile.mkdtemp(prefix="mm_chain_probe_")
    try:
        need = nreads * (L + 14) + sum(len(a) for a in ref_np) * 1.02 + (2 << 30)
        free = shutil.disk_usage(td).free
        if free < need:                                             # as bench_e2e.py: fewer reads where the scratch disk is small
            nreads = max(1000, int(nreads * (free - (3 << 30)) / need))
            log("[chain_probe] %.1f GB free under %s: the command line gets %d reads" % (free / 1e9, td, nreads))
        rp, qp = os.path.join(td, "ref.fa"), os.path.join(td, "reads.fa")
        write_fasta(rp, ["chr%d" % i for i in range(len(ref_np))], ref_np)
        with open(qp, "wb") as f:
            for r0 in range(0, nreads, 100_000):
                n = min(100_000, nreads - r0)
                rd = make_reads(torch, dev, contigs, n, L, W["err"], seed=5000 + r0).cpu().numpy().reshape(n, L)
                hdr = np.frombuffer(b"".join(b">read%07d\n" % (r0 + i) for i in range(n)), dtype=np.uint8).reshape(n, 13)
                f.write(np.concatenate([hdr, rd, np.full((n, 1), 10, dtype=np.uint8)], axis=1).tobytes())
        runs = {"off": [], "on": []}
        pafs = {}
        stopped = None
        for rep, tag in [(rep, tag) for rep in range(3) for tag in ("off", "on")]:
            # every run under a time limit of its own; nothing more is started on the card behind a run that failed, was killed by a
            # signal or did not end in time: what was collected so far is written, and the probe ends with a non-zero status
            env = {k: v for k, v in os.environ.items() if k != "MASHMAP_HIP_DEVICE_CHAIN"}
            env["MASHMAP_HIP_TIMING"] = "1"
            if tag == "on":
                env["MASHMAP_HIP_DEVICE_CHAIN"] = "1"
            op = os.path.join(td, tag + ".paf")
            t0 = time.time()
            try:
                p = subprocess.run([exe, "-r", rp, "-q", qp, "-o", op, "-t", str(THREADS), "-s", str(W["seg"]), "--pi", str(int(round(W["pi"] * 100))), "-J", str(W["sketch"])],
                                   capture_output=True, text=True, env=env, timeout=run_timeout)
            except subprocess.TimeoutExpired:
                stopped = "command line %s, run %d: no end within %d s" % (tag, rep, run_timeout)
                runs[tag].append({"error": stopped})
                break
            wall = time.time() - t0
            if p.returncode != 0:
                stopped = "command line %s, run %d: status %d" % (tag, rep, p.returncode)
                runs[tag].append({"error": stopped, "stderr": p.stderr[-400:]})
                break
            dev_s = re.findall(r"device stage \(.*?\): ([0-9.eE+-]+) s \(upload ([0-9.eE+-]+), kernels ([0-9.eE+-]+), download ([0-9.eE+-]+)\)", p.stderr)
            post = [float(x) for x in re.findall(r"post stage: chain \+ filter \+ format ([0-9.eE+-]+) s", p.stderr)]
            map_s = float(re.search(r"time spent mapping the query\s*:\s*([0-9.eE+-]+)", p.stderr).group(1))
            runs[tag].append(dict(map_s=map_s, wall_s=round(wall, 3),
                                  device_stage_s=round(sum(float(r[0]) for r in dev_s), 4), device_kernels_s=round(sum(float(r[2]) for r in dev_s), 4),
                                  device_download_s=round(sum(float(r[3]) for r in dev_s), 4), device_passes=len(dev_s), post_s=round(sum(post), 4),
                                  gbps=round(nreads * L / map_s / 1e9, 3),
                                  chained_rows=sum(int(x) for x in re.findall(r"and (\d+) chained rows\)", p.stderr)) if tag == "on" else None))
            pafs[tag] = open(op, "rb").read()
            log("[chain_probe] command line %s, run %d: %r" % (tag, rep, runs[tag][-1]))
        out["command_line"] = dict(reads=nreads, threads=THREADS, runs=runs, stopped=stopped,
                                   paf_identical=bool(pafs.get("on") is not None and pafs.get("on") == pafs.get("off")), paf_bytes=len(pafs.get("off", b"")))
        return stopped
    finally:
        shutil.rmtree(td, ignore_errors=True)


GROUP_WORKLOADS = {"y10k": dict(reads=200_000, read_len=10_000, nosplit=False), "y50k": dict(reads=40_000, read_len=50_000, nosplit=False),
                   "nosplit": dict(reads=100_000, read_len=12_000, nosplit=True)}


def groups_part(torch, dev, name, out, scale=1.0, device_only=False):
    from mashmap_amd import capi, shard
    host = shard.host_lib()
    W, G = WORKLOADS["configs1"], GROUP_WORKLOADS[name]
    K, SEG, S, PI, L = W["k"], W["seg"], W["sketch"], W["pi"], G["read_len"]
    nreads = max(1000, int(G["reads"] * scale))
    base = make_reference(torch, dev, 1, 12_000_000, seed=7)[0]
    gen = torch.Generator(device=dev); gen.manual_seed(77)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    contigs = []
    for g in range(8):                                              # group g: i.i.d. substitutions at 0.5 % x g
        c = base.clone()
        if g:
            hit = torch.rand(len(c), generator=gen, device=dev) < 0.005 * g
            c[hit] = lut[torch.randint(0, 4, (int(hit.sum()),), generator=gen, device=dev)]
        contigs.append(c)
    ref_np = contiguous_views(torch, contigs)
    grouped = not G["nosplit"]
    ref_group = np.arange(8, dtype=np.int32) if grouped else None   # S0#1#chr .. S7#1#chr: a group a contig
    ctx = capi.Context(k=K, segLength=SEG, sketchSize=S, flags=capi.MM_FLAG_HG_FILTER | (capi.MM_FLAG_SKIP_PREFIX if grouped else capi.MM_FLAG_NO_SPLIT))
    ctx.index_build(ref_np, ref_group, 0.001)
    ctx.set_tables_default(PI)
    ctx.set_chain_tables(SEG, 1, 0, 0, True, capi.MM_CHAIN_FILTER_QUERY, 0.0)
    reads_t = make_reads(torch, dev, contigs, nreads, L, W["err"], seed=4343, chunk=max(64, 8192 * 10000 // L))
    torch.cuda.synchronize()
    offs = np.arange(nreads + 1, dtype=np.int64) * L
    ctx.reads_upload_device(reads_t.data_ptr(), reads_t.numel(), offs, np.full(nreads, -1, dtype=np.int32), np.full(nreads, -1, dtype=np.int32))
    del reads_t
    ctx.map(); ctx.synchronize()
    clens = np.array([len(a) for a in ref_np], dtype=np.int32); rl = np.full(nreads, L, dtype=np.int32)
    rg_ptr = ref_group.ctypes.data if grouped else None
    split = 0 if G["nosplit"] else 1
    ev = StreamEvents(ctx.lib.mm_stream(ctx.h))
    ctx.chain_long(True); ctx.chain_modes(True)
    row_dt = np.dtype([("i", "<i4", 10), ("f", "<f4", 2)])

    def host_stage(rows, recs, cap):
        res = np.zeros(cap, dtype=row_dt)
        c0 = cpu_seconds(); t0 = time.perf_counter()
        n = host.mmh_post_chained_modes(K, SEG, S, PI, 1, 1, 1, 1, SEG, SEG, len(clens), clens.ctypes.data, rows.ctypes.data if rows is not None and len(rows) else None,
                                        0 if rows is None else len(rows), recs.ctypes.data if len(recs) else None, len(recs), rl.ctypes.data, nreads, 0, THREADS, None,
                                        res.ctypes.data, None, None, cap, rg_ptr, split)
        return res[:n], round((time.perf_counter() - t0) * 1e3, 3), round(cpu_seconds() - c0, 4)

    forms = {"C": []} if device_only else {"A": [], "C": []}
    recs = None
    for rep in range(3):
        if not device_only:
            t0 = time.perf_counter()
            recs = ctx.mappings()
            dl = time.perf_counter() - t0
            rep_a, host_ms, cpu_s = host_stage(None, recs, len(recs) + 1)
            a = dict(device_ms=0.0, download_ms=round(dl * 1e3, 3), download_bytes=int(recs.nbytes), host_ms=host_ms, host_cpu_s=cpu_s, reported=int(len(rep_a)), records=int(len(recs)))
        ev.start(); t0 = time.perf_counter()
        ctx.chain_reads()
        wall_stage = time.perf_counter() - t0
        dev_ms = ev.elapsed()
        cnt, lcnt, gcnt = ctx.chain_counts(), ctx.chain_long_counts(), ctx.chain_group_counts()
        c = dict(device_ms=dev_ms, stage_wall_ms=round(wall_stage * 1e3, 3), offered=cnt["offered"], finished=cnt["finished"], rows=cnt["rows"], leftover_records=cnt["leftover"],
                 long_offered=lcnt["offered"], long_finished=lcnt["finished"], group_reads=gcnt["reads"], group_runs=gcnt["runs"])
        if not device_only:
            t0 = time.perf_counter()
            rows = ctx.chain_rows(); left = ctx.chain_leftover()
            dl = time.perf_counter() - t0
            rep_c, host_ms, cpu_s = host_stage(rows, left, len(recs) + 1)
            if rep_a.tobytes() != rep_c.tobytes():                  # before any time is printed
                raise SystemExit("chain_probe.py --groups %s: the reported mappings of form C differ from form A's (%d against %d)" % (name, len(rep_c), len(rep_a)))
            c.update(download_ms=round(dl * 1e3, 3), download_bytes=int(rows.nbytes + left.nbytes), host_ms=host_ms, host_cpu_s=cpu_s, reported=int(len(rep_c)), same_as_A=True)
            forms["A"].append(a)
            log("[chain_probe] %s, alternation %d: A %r" % (name, rep, a))
        forms["C"].append(c)
        log("[chain_probe] %s, alternation %d: C %r" % (name, rep, c))
    res = dict(reads=nreads, read_len=L, flags="-Y '#'" if grouped else "--noSplit", host_threads=THREADS, forms=forms)
    if recs is not None:
        nrec = np.bincount(recs["querySeqId"], minlength=nreads)
        res["records_per_read"] = {"mean": round(float(nrec.mean()), 3), "max": int(nrec.max()), "reads_above_16": int((nrec > 16).sum()), "reads_above_512": int((nrec > 512).sum())}
    out["groups_" + name] = res
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=WORKLOADS["configs1"]["reads"])
    ap.add_argument("--cli-reads", type=int, default=WORKLOADS["configs1"]["reads"])
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--run-timeout", type=int, default=120, help="seconds one mashmap_hip run of part 2 may take (it takes about 2.5 at the default size)")
    ap.add_argument("--chain-long", action="store_true", help="form C (MM_OPT_CHAIN_LONG) in part 1, and part 1 again on the long-read workload")
    ap.add_argument("--long-reads", type=int, default=20000, help="reads of the long-read workload (20 000 x 100 kbp: about 400 000 records)")
    ap.add_argument("--long-read-len", type=int, default=100000)
    ap.add_argument("--groups", choices=sorted(GROUP_WORKLOADS), default=None, help="the MM_OPT_CHAIN_MODES workload of that name alone (8 reference groups)")
    ap.add_argument("--scale", type=float, default=1.0, help="--groups: share of the workload's reads")
    ap.add_argument("--device-only", action="store_true", help="--groups: form C's device milliseconds alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chain_probe.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev).cpu()
    W = WORKLOADS["configs1"]
    out = {"workload": W["label"]}
    if a.groups:
        groups_part(torch, dev, a.groups, out, a.scale, a.device_only)
        text = json.dumps(out, indent=1)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    ref_np, contigs = part1(torch, dev, W, a.reads, out, chain_long=a.chain_long)
    if a.chain_long:
        part1(torch, dev, W, a.long_reads, out, chain_long=True, L=a.long_read_len, key="long_reads", ref=(ref_np, contigs))
    stopped = None
    if not a.no_cli:
        stopped = part2(torch, dev, W, a.cli_reads, ref_np, contigs, out, a.run_timeout)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if stopped:
        sys.exit("chain_probe.py: stopped behind " + stopped)


if __name__ == "__main__":
    main()
