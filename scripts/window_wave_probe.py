"""--noSplit with reads longer than a segment at library level: what the stages of a pass cost with and without MM_OPT_L2_WINDOW_WAVE.

The shape of profiles/r13f_nosplit_30kbp_reads_both_command_lines.txt: --reads reads of --read-len bases (substitutions at --err) against
an index of --index-mbp Mbp of random sequence built on the device, k 19, segLength 5000, s 130, pi 0.85, MM_FLAG_NO_SPLIT with the HG
filter.  One context, one process: --warmup passes, then --reps timed ones with the kernel timers on.  Prints one JSON line: the medians
of MM_K_SORT and MM_K_LOOKUP (the point path), MM_K_L1 (k_l1_window), MM_K_L2_LOCATE (k_l2_window_extents and its scans), MM_K_L2 (the L2
sweeps) and the whole pass in ms, and (candidates, literal) of mm_pass_l2_window.

--option 1 sets MM_OPT_L2_WINDOW_WAVE.  --tree DIR takes the package and its built library from another checkout (the parent commit's,
which knows neither the option nor mm_pass_l2_window: run it with --option 0).  Not part of the test suite."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--index-mbp", type=float, default=40.0)
ap.add_argument("--contigs", type=int, default=8)
ap.add_argument("--reads", type=int, default=2000)
ap.add_argument("--read-len", type=int, default=30000)
ap.add_argument("--err", type=float, default=0.03)
ap.add_argument("--sketch", type=int, default=130)
ap.add_argument("--option", type=int, default=0)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tag", default="")
a = ap.parse_args()
sys.path.insert(0, a.tree)
from mashmap_amd import capi  # noqa: E402

K, L, PI = 19, 5000, 0.85
rng = np.random.default_rng(11)
acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
clen = int(a.index_mbp * 1e6 / a.contigs)
contigs = [acgt[rng.integers(0, 4, clen)] for _ in range(a.contigs)]
reads = []
for i in range(a.reads):
    c = contigs[int(rng.integers(0, a.contigs))]
    st = int(rng.integers(0, clen - a.read_len))
    r = c[st:st + a.read_len].copy()
    hit = rng.random(a.read_len) < a.err * 4.0 / 3.0
    r[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
    reads.append(r)

ctx = capi.Context(k=K, segLength=L, sketchSize=a.sketch, flags=capi.MM_FLAG_NO_SPLIT | capi.MM_FLAG_HG_FILTER)
if a.option: ctx.l2_window_wave(True)
t0 = time.perf_counter()
ctx.index_build(contigs)
ctx.set_tables_default(PI)
ctx.set_replay_tables(*capi.stat_replay_tables(a.sketch, K, PI, 0.0, True))
nF = ctx.reads_upload(reads, None, [-1] * len(reads), 0)
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
    if it >= a.warmup: rows.append((pr["sort"][0], pr["lookup"][0], pr["l1"][0], pr["l2_locate"][0], pr["l2"][0], ms))
cands, literal = ctx.pass_l2_window() if hasattr(ctx, "pass_l2_window") else (None, None)
nL1, nL2 = ctx.result_counts()
med = [float(np.median([r[i] for r in rows])) for i in range(6)]
print(json.dumps(dict(tag=a.tag, option=a.option, index_mbp=a.index_mbp, fragments=nF, candidates=cands, literal=literal, nL1=nL1, nL2=nL2,
                      k_sort_ms=round(med[0], 3), k_lookup_ms=round(med[1], 3), k_l1_ms=round(med[2], 3), k_l2_locate_ms=round(med[3], 3),
                      k_l2_ms=round(med[4], 3), pass_ms=round(med[5], 3), pass_ms_min=round(min(r[5] for r in rows), 3),
                      k_l2_ms_all=[round(r[4], 3) for r in rows], steady=ctx.pass_stats()[1], setup_s=round(t_setup, 2))))
ctx.close()
