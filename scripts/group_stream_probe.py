"""-Y reference groups at library level: what the L1 stage of a pass costs with and without MM_OPT_L1_GROUP_STREAM.

Index: H haplotype-like copies of one random genome (hap<i>#1#chr<j>, --div substitutions each), built on the device.  Reads: the same
contigs, every read with its contig's reference group (all against all: a read's own haplotype is dropped), cut to segments by the
library.  One context, one process: --warmup passes, then --reps timed ones with the kernel timers on.  Prints one JSON line: the
medians of MM_K_SORT (gather + sort of the point path), MM_K_L1 (the L1 kernels) and the whole pass in ms, and (queued, literal) of
mm_pass_l1_literal.  --option 1 sets MM_OPT_L1_GROUP_STREAM (a library without it answers MM_ERR_ARG: run those with --option 0).

Not part of the test suite; scripts/ab_libs.sh describes how to put another build's library beside this one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mashmap_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--haps", type=int, default=8)
ap.add_argument("--chrs", type=int, default=6)
ap.add_argument("--chr-len", type=int, default=2000000)
ap.add_argument("--div", type=float, default=0.01)
ap.add_argument("--pi", type=float, default=0.95)
ap.add_argument("--sketch", type=int, default=200)
ap.add_argument("--option", type=int, default=0)
ap.add_argument("--hg", type=int, default=1)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tag", default="")
a = ap.parse_args()

K, L = 19, 5000
rng = np.random.default_rng(7)
acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
genome = [acgt[rng.integers(0, 4, a.chr_len)] for _ in range(a.chrs)]
contigs, groups = [], []
for h in range(a.haps):
    for j in range(a.chrs):
        c = genome[j].copy()
        hit = rng.random(a.chr_len) < a.div * 4.0 / 3.0
        c[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
        contigs.append(c); groups.append(h)                      # hap<h>#1#chr<j>: one group per haplotype, its contigs adjacent

ctx = capi.Context(k=K, segLength=L, sketchSize=a.sketch, flags=capi.MM_FLAG_SKIP_PREFIX | (capi.MM_FLAG_HG_FILTER if a.hg else 0))
if a.option: ctx.l1_group_stream(True)
t0 = time.perf_counter()
ctx.index_build(contigs, groups)
ctx.set_tables_default(a.pi)
ctx.set_replay_tables(*capi.stat_replay_tables(a.sketch, K, a.pi, 0.0, True))
nF = ctx.reads_upload(contigs, groups, list(range(len(contigs))), 0)
ctx.synchronize()
t_setup = time.perf_counter() - t0
ctx.profile(True)
rows = []
for it in range(a.warmup + a.reps):
    ctx.profile_read(True)
    t1 = time.perf_counter()
    ctx.map(); ctx.synchronize()
    ms = (time.perf_counter() - t1) * 1e3
    pr = ctx.profile_read(True)
    if it >= a.warmup: rows.append((pr["sort"][0], pr["l1"][0], pr["lookup"][0], pr["l2"][0] + pr["l2_locate"][0], ms))
queued, literal = ctx.pass_l1_literal()
nL1, nL2 = ctx.result_counts()
med = [float(np.median([r[i] for r in rows])) for i in range(5)]
print(json.dumps(dict(tag=a.tag, option=a.option, hg=a.hg, index_mbp=a.haps * a.chrs * a.chr_len / 1e6, fragments=nF, queued=queued, literal=literal,
                      nL1=nL1, nL2=nL2, k_sort_ms=round(med[0], 3), k_l1_ms=round(med[1], 3), k_lookup_ms=round(med[2], 3), k_l2_ms=round(med[3], 3),
                      pass_ms=round(med[4], 3), pass_ms_min=round(min(r[4] for r in rows), 3), k_l1_ms_all=[round(r[1], 3) for r in rows],
                      steady=ctx.pass_stats()[1], setup_s=round(t_setup, 2))))
ctx.close()
