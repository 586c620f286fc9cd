"""Sketch sizes beyond 8190 at library level: how a pass splits into stages, with and without MM_OPT_L2_LARGE_WAVE.

The shape of scripts/large_sketch_paf.py: a 3.2 Mbp random reference in three contigs, index built on the device, k 19, pi 0.80, no HG
filter; --reads reads of --read-len bases (substitutions at --err).  Two rows: --seg 200000 / --sketch 19998 (what --dense --pi 80
-s 200000 derives) and --seg 100000 / --sketch 9998.  One context, one process: --warmup passes, then --reps timed ones with the kernel
timers on.  Prints one JSON line: the medians of MM_K_SKETCH (+ MM_K_SKETCH_HARD), MM_K_LOOKUP + MM_K_SORT, MM_K_L1, MM_K_L2_LOCATE, MM_K_L2
and the whole pass in ms, and (candidates, literal) of mm_pass_l2_large.

--option 1 sets MM_OPT_L2_LARGE_WAVE.  --tree DIR takes the package and its built library from another checkout (the parent commit's,
which knows neither the option nor mm_pass_l2_large: run it with --option 0).  Not part of the test suite.

The decision rule, stated before the first run.  Three rounds of (parent, this tree with the option, this tree without), each run a fresh
process; "spread" is the parent's largest minus smallest figure over its three runs.
  1. With the option, MM_K_L2 + MM_K_L2_LOCATE is below the parent's by more than the parent's spread of that sum, in every pair.
  2. With the option, the whole pass is not slower than the parent's by more than the parent's spread of the whole pass, in every pair.
  3. Without the option this tree equals the parent within the spread, compared on the medians over the three rounds.
skch::Sketch sets the option for sketchSize > 8190 if 1 and 2 hold on both rows; 3 is reported either way.

--sketch-large sets MM_OPT_SKETCH_LARGE (k_sketch_large instead of the global-memory sketch kernel); the line then carries (fragments,
uncut) of mm_sketch_large_counts as well.  Its rule, stated before the first run, on the same two rows and the same three rounds of
(parent, this tree with --sketch-large, this tree without), MM_OPT_L2_LARGE_WAVE = 1 (--option 1) in all three:
  1. With the option, MM_K_SKETCH + MM_K_SKETCH_HARD (k_sketch_ms) is below the parent's in every pair, by more than the parent's spread.
  2. With the option, the whole pass is below the parent's by more than the parent's spread of the whole pass, in every pair.
  3. Without the option, both figures equal the parent's within its spread (medians over the three rounds).
skch::Sketch sets MM_OPT_SKETCH_LARGE for sketchSize > 8190 if 1 and 2 hold on both rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--seg", type=int, default=200000)
ap.add_argument("--sketch", type=int, default=19998)
ap.add_argument("--reads", type=int, default=40)
ap.add_argument("--read-len", type=int, default=450000)
ap.add_argument("--err", type=float, default=0.03)
ap.add_argument("--option", type=int, default=0)
ap.add_argument("--sketch-large", action="store_true")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tag", default="")
a = ap.parse_args()
sys.path.insert(0, a.tree)
from mashmap_amd import capi  # noqa: E402

K, PI = 19, 0.80
rng = np.random.default_rng(13)
acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
contigs = [acgt[rng.integers(0, 4, n)] for n in (1500000, 1100000, 600000)]
reads = []
for i in range(a.reads):
    c = contigs[i % 3]
    st = int(rng.integers(0, len(c) - a.read_len))
    r = c[st:st + a.read_len].copy()
    hit = rng.random(a.read_len) < a.err * 4.0 / 3.0
    r[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
    reads.append(r)

ctx = capi.Context(k=K, segLength=a.seg, sketchSize=a.sketch, flags=0)
if a.option: ctx.l2_large_wave(a.option)
if a.sketch_large: ctx.sketch_large()
t0 = time.perf_counter()
ctx.index_build(contigs)
lib = capi.load()
min_hits = np.array([0] + [lib.mm_stat_min_hits_relaxed(q, K, PI) for q in range(1, a.sketch + 1)], dtype=np.int32)
ctx.set_tables(min_hits, capi.stat_sketch_cutoffs(a.sketch, K, False))     # (no replay tables: (s + 1)^2 entries; the pass stops at the loci)
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
    if it >= a.warmup: rows.append((pr["sketch"][0] + pr["sketch_hard"][0], pr["lookup"][0] + pr["sort"][0], pr["l1"][0], pr["l2_locate"][0], pr["l2"][0], ms))
cands, literal = ctx.pass_l2_large() if hasattr(ctx, "pass_l2_large") else (None, None)
sk_large = ctx.sketch_large_counts() if hasattr(ctx, "sketch_large_counts") else None
nL1, nL2 = ctx.result_counts()
med = [float(np.median([r[i] for r in rows])) for i in range(6)]
print(json.dumps(dict(tag=a.tag, option=a.option, sketch_large=bool(a.sketch_large), sketch_large_counts=sk_large, seg=a.seg, sketch=a.sketch, fragments=nF, candidates=cands, literal=literal, nL1=nL1, nL2=nL2,
                      k_sketch_ms=round(med[0], 3), k_lookup_sort_ms=round(med[1], 3), k_l1_ms=round(med[2], 3), k_l2_locate_ms=round(med[3], 3),
                      k_l2_ms=round(med[4], 3), pass_ms=round(med[5], 3), pass_ms_min=round(min(r[5] for r in rows), 3),
                      k_l2_ms_all=[round(r[4], 3) for r in rows], k_sketch_ms_all=[round(r[0], 3) for r in rows], setup_s=round(t_setup, 2))))
ctx.close()
