"""-Y reference groups at library level: what the lookup .. L1 stages of a pass cost with and without MM_OPT_L1_GROUP_FUSED.

The workload of scripts/group_stream_probe.py: H haplotype-like copies of one random genome (hap<i>#1#chr<j>, --div substitutions each),
built on the device, mapped all against all (every read with its contig's reference group), MM_OPT_L1_GROUP_STREAM on everywhere.  One
run = one context in one process: --warmup passes, then --reps timed ones with the kernel timers on; it prints one JSON line with the
medians of MM_K_LOOKUP, MM_K_SORT (where k_lookup_groups is timed, as k_lookup_mid is), MM_K_L1, the L2 kernels and the whole pass in
ms, and (offered, fused) of mm_pass_l1_group_fused.

--fused 1 sets MM_OPT_L1_GROUP_FUSED.  --tree DIR takes the package and its built library from another checkout (the parent commit's,
which knows neither the option nor the call: run it with --fused 0).

--rounds N --parent-tree DIR is the comparison that decides whether the command line sets the option: parent, this tree with the
option, this tree without it, N times in that order, every run a fresh process; then the table and the rule
  * with the option, lookup + sort + L1 lies below the parent's in every round by more than the parent's own spread (max - min over
    its N runs) of that sum;
  * the whole pass is not slower than the parent's in any round by more than the parent's spread of the whole pass;
  * without the option, this tree equals the parent within those spreads (sum and whole pass, every round).
Not part of the test suite."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=HERE)
ap.add_argument("--haps", type=int, default=8)
ap.add_argument("--chrs", type=int, default=6)
ap.add_argument("--chr-len", type=int, default=2000000)
ap.add_argument("--div", type=float, default=0.01)
ap.add_argument("--pi", type=float, default=0.95)
ap.add_argument("--sketch", type=int, default=200)
ap.add_argument("--fused", type=int, default=0)
ap.add_argument("--hg", type=int, default=1)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tag", default="")
ap.add_argument("--rounds", type=int, default=0)
ap.add_argument("--parent-tree", default="")
ap.add_argument("--run-timeout", type=int, default=240)
a = ap.parse_args()


def compare():
    variants = (("parent", a.parent_tree, 0), ("fused", HERE, 1), ("off", HERE, 0))
    rows = {v[0]: [] for v in variants}
    for rnd in range(a.rounds):
        for name, tree, fused in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--fused", str(fused), "--tag", "%s%d" % (name, rnd), "--haps", str(a.haps),
                   "--chrs", str(a.chrs), "--chr-len", str(a.chr_len), "--div", str(a.div), "--pi", str(a.pi), "--sketch", str(a.sketch), "--hg", str(a.hg),
                   "--reps", str(a.reps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.run_timeout)
            if p.returncode != 0:                                  # nothing more is started behind a run that failed
                sys.stderr.write(p.stderr[-3000:]); sys.exit("run %s of round %d ended with status %d" % (name, rnd, p.returncode))
            r = json.loads(p.stdout.strip().splitlines()[-1])
            r["sum3"] = round(r["k_lookup_ms"] + r["k_sort_ms"] + r["k_l1_ms"], 3)
            rows[name].append(r); print(json.dumps(r), flush=True)
    spread = {k: max(r[k] for r in rows["parent"]) - min(r[k] for r in rows["parent"]) for k in ("sum3", "pass_ms")}
    print("| run | MM_K_LOOKUP | MM_K_SORT | MM_K_L1 | sum of the three | L2 | whole pass | offered | fused |")
    print("|---|---|---|---|---|---|---|---|---|")
    for rnd in range(a.rounds):
        for name, _, _ in variants:
            r = rows[name][rnd]
            print("| %s, round %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %s | %s |" % (name, rnd + 1, r["k_lookup_ms"], r["k_sort_ms"], r["k_l1_ms"], r["sum3"],
                                                                                        r["k_l2_ms"], r["pass_ms"], r["offered"], r["fused"]))
    rule1 = all(rows["parent"][i]["sum3"] - rows["fused"][i]["sum3"] > spread["sum3"] for i in range(a.rounds))
    rule2 = all(rows["fused"][i]["pass_ms"] - rows["parent"][i]["pass_ms"] <= spread["pass_ms"] for i in range(a.rounds))
    rule3 = all(abs(rows["off"][i]["sum3"] - rows["parent"][i]["sum3"]) <= spread["sum3"] and
                abs(rows["off"][i]["pass_ms"] - rows["parent"][i]["pass_ms"]) <= spread["pass_ms"] for i in range(a.rounds))
    print("parent's spread: sum of the three %.3f ms, whole pass %.3f ms" % (spread["sum3"], spread["pass_ms"]))
    print("fused == offered: %r" % [r["fused"] == r["offered"] for r in rows["fused"]])
    print("rule 1 (sum below the parent's by more than its spread, every round): %s" % rule1)
    print("rule 2 (whole pass not slower than the parent's by more than its spread): %s" % rule2)
    print("rule 3 (without the option equal to the parent within the spreads): %s" % rule3)
    print("decision: the command line %s MM_OPT_L1_GROUP_FUSED under -Y" % ("SETS" if rule1 and rule2 and rule3 else "leaves off"))


if a.rounds:
    if not a.parent_tree: sys.exit("--rounds needs --parent-tree")
    compare(); sys.exit(0)

import numpy as np  # noqa: E402
sys.path.insert(0, a.tree)
from mashmap_amd import capi  # noqa: E402

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
ctx.l1_group_stream(True)
if a.fused: ctx.l1_group_fused(True)
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
    if it >= a.warmup: rows.append((pr["lookup"][0], pr["sort"][0], pr["l1"][0], pr["l2"][0] + pr["l2_locate"][0], ms))
offered, fused = ctx.pass_l1_group_fused() if hasattr(ctx, "pass_l1_group_fused") else (None, None)
queued, literal = ctx.pass_l1_literal()
nL1, nL2 = ctx.result_counts()
med = [float(np.median([r[i] for r in rows])) for i in range(5)]
print(json.dumps(dict(tag=a.tag, fused_option=a.fused, hg=a.hg, index_mbp=a.haps * a.chrs * a.chr_len / 1e6, fragments=nF, offered=offered, fused=fused,
                      queued=queued, literal=literal, nL1=nL1, nL2=nL2, k_lookup_ms=round(med[0], 3), k_sort_ms=round(med[1], 3), k_l1_ms=round(med[2], 3),
                      k_l2_ms=round(med[3], 3), pass_ms=round(med[4], 3), pass_ms_min=round(min(r[4] for r in rows), 3), steady=ctx.pass_stats()[1],
                      setup_s=round(t_setup, 2))))
ctx.close()
