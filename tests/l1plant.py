"""A planted index and a model of the path a fragment takes through the default L1 kernels (mashmap_amd/csrc/mm_map.hip: k_lookup_l1,
k_lookup_mid, mm_l1_fused) -- test infrastructure for tests/test_gpu_l1_edges.py.

Planted index.  The reads are random DNA unrelated to the contigs, so a fragment of theirs has no hit of its own; a Plan lists, per fragment,
the minmer records that give it hits -- (seed rank in the fragment's sketch, seqId, wpos, wpos_end, strand) -- and `Plan.mutate` is the
`mutate_index` function of Oracle.session: it merges those records, under the hashes of the fragments' sketches, into the contigs' own
records in (seqId, wpos) order.  Every record of a hash becomes one interval [wpos, wpos_end) = two interval points (Sketch::index joins a
record to the one before it under the same hash when its wpos equals that one's wpos_end: `Plan.mutate` refuses such a plan).  The sketch
hashes come from Oracle.sketch_sequence, the function an oracle session sketches a fragment with.

Route model.  `route` restates the kernels' capacities over the oracle's per-fragment data (`view`) and names where a fragment ends:
  ("fused", None)        finished by k_lookup_l1
  ("mid", None)          passed to k_lookup_mid and finished there
  ("mid>HBM", reason)    passed to k_lookup_mid and handed to the HBM point path: seeds, span, contigs, kept, mixed, runs
  ("HBM", reason)        queued by k_lookup_l1 for the HBM point path: minHits, sketch, points, mixed, runs
  ("none", None)         no point and no usable sketch: nothing to do"""
import numpy as np

import l1filter
import mmutil as U

# mm_map.hip
FUSE_MAXRUNS = 64                                                # MM_FUSE_MAXRUNS
MID_MAXSKETCH, MID_MAXSEEDS, MID_MAXKEEP, MID_MAXPTS = 512, 256, 1024, 16384
FILT_SLOTS, FILT_MAXSPAN, FILT_CONTIGS = 2048, 64, 128
SORT_WAVECAP, SORT_LDSCAP = 512, 4096


def fused_cap(s):
    """pass_lookup: the MAXPTS of the k_lookup_l1 instance a sketch size gets"""
    return 512 if s > 256 else 256 if s > 160 else 128


def hbm_slots(P):
    """the slots a queued list of P points gets: a power of two, at least 128, above 64 points"""
    if P <= 64: return P
    n = 128
    while n < P: n <<= 1
    return n


class Plan:
    def __init__(self, oracle, reads, k, s):
        """reads: [(name, uint8 array)], each one fragment"""
        self.hashes = [[x[0] for x in oracle.sketch_sequence(a, k, s, i)] for i, (_, a) in enumerate(reads)]
        self.recs = []                                           # (hash, wpos, wpos_end, seqId, strand)
        self.per = [[] for _ in reads]

    def add(self, f, rank, seq, o, c, strand=1):
        self.recs.append((self.hashes[f][rank], o, c, seq, strand))
        self.per[f].append((rank, seq, o, c, strand))

    def cluster(self, f, ranks, seq, at, step=3, width=200):
        """one interval per rank, each `step` behind the one before: len(ranks) of them overlap"""
        for j, r in enumerate(ranks): self.add(f, r, seq, at + j * step, at + j * step + width)

    def singles(self, f, ranks, seq, at, n, stride, width=2):
        """n intervals `stride` apart, dealt to the ranks in turn"""
        for i in range(n): self.add(f, ranks[i % len(ranks)], seq, at + i * stride, at + i * stride + width)

    def merged(self, natural):
        add = np.zeros(len(self.recs), dtype=U.MINMER_DT)
        for i, (h, o, c, q, st) in enumerate(self.recs):
            add[i] = (h, o, c, q, st, 0)
        out = np.concatenate([natural, add])
        out = out[np.lexsort((out["wpos"], out["seqId"]))]       # stable: a contig's own record stays before a planted one at its wpos
        mine, last = {r[0] for r in self.recs}, {}
        for h, o, c in zip(out["hash"].tolist(), out["wpos"].tolist(), out["wpos_end"].tolist()):
            if h not in mine: continue                           # (the contigs' own windows of one hash do follow each other like this)
            assert last.get(h) != o, "Sketch::index would join a planted record to the one before it under its hash"
            last[h] = c
        return out

    def mutate(self, natural):
        return self.merged(natural)

    def keys_after(self, natural):
        """distinct hashes of the merged index: what the frequency filter's percentage is taken of"""
        return int(np.unique(self.merged(natural)["hash"]).size)


def view(oracle, contigs, reads, k, L, s, pi, flags, kmerPct, plan, base=0):
    """per fragment (= read), from one oracle session over the planted index: raw and final sketch size, P (the interval points of its
    seeds before the seqId filters), the seeds with points, the intervals that pass the seqId filters, the sorted points, L1; and the
    session's cutoffs and frequency threshold"""
    h = oracle.session(contigs, k, L, s, pi, U.FILTER_MAP, flags, b"\0", kmerPct, mutate_index=plan.mutate if plan else None)
    names = [n for n, _ in contigs]
    ix = oracle.export_index(h)
    by_key = {int(kk): (int(ix["offsets"][i]), int(ix["offsets"][i + 1])) for i, kk in enumerate(ix["keys"])}
    out = []
    for ri, (name, a) in enumerate(reads):
        e = oracle.map_fragment(h, a, base + ri, name.encode(), len(a), s)
        self_id = names.index(name) if name in names else -1
        P, seeds, iv = 0, 0, []
        for x in e["sketch"]:
            lo, hi = by_key.get(x[0], (0, 0))
            if hi == lo: continue
            P += hi - lo; seeds += 1
            seq, pos = ix["points"]["seqId"][lo:hi].tolist(), ix["points"]["pos"][lo:hi].tolist()
            for j in range(0, hi - lo - 1, 2):
                q = seq[j]
                if (flags & U.FLAG_SKIP_SELF) and q == self_id: continue
                if (flags & U.FLAG_LOWER_TRI) and not (base + ri > q): continue
                iv.append((q, pos[j], pos[j + 1], seq[j + 1]))
        out.append(dict(raw=e["rawSketchSize"], q=e["sketchSize"], P=P, seeds=seeds, iv=iv, points=[p[:3] for p in e["points"]], l1=e["l1"],
                        sketch=[x[0] for x in e["sketch"]]))
        assert len(out[-1]["points"]) == 2 * len(iv)
    cut, thr = oracle.cutoffs(h), oracle.f("session_freq_threshold")(h)
    oracle.free(h)
    return out, cut, thr


def fused_sweep(pts, q, mh, cut, hg, s):
    """mm_l1_fused over a sorted point list [(seqId, pos, side)]: ("mixed" | "runs" | None, candidate runs before they are joined)"""
    if any(a[1] == b[1] and a[0] != b[0] for a, b in zip(pts, pts[1:])): return "mixed", 0
    groups, run = [], 0
    for i, p in enumerate(pts):
        run += 1 if p[2] == 1 else -1
        if i + 1 == len(pts) or pts[i + 1][1] != p[1]: groups.append((p[0], run))
    if not groups: return None, 0
    best = max(0, max(c for _, c in groups))
    if hg:
        if best < mh: return None, 0
        ci = min(int(min(best, q) / max(s / 1000.0, 1.0)), len(cut) - 1)
        mh = max(cut[ci], mh)
    flag = [i < len(groups) - 1 and c >= mh for i, (_, c) in enumerate(groups)]
    runs = sum(1 for i in range(len(groups)) if flag[i] and not (i > 0 and flag[i - 1] and groups[i - 1][0] == groups[i][0]))
    return ("runs" if runs > FUSE_MAXRUNS else None), runs


def kept_points(fr, mh):
    """k_lookup_mid's two sweeps: (reason it gives up | None, the sorted points its filter keeps)"""
    iv = fr["iv"]
    if any(c <= o or ((c - 1) >> l1filter.BIN_SHIFT) - (o >> l1filter.BIN_SHIFT) >= FILT_MAXSPAN or qc != q for q, o, c, qc in iv): return "span", None
    if len({q for q, _, _, _ in iv}) > FILT_CONTIGS: return "contigs", None
    keep = l1filter.keep_mask([x[0] for x in iv], [x[1] for x in iv], [x[2] for x in iv], mh, table_slots=FILT_SLOTS) if iv else []
    out = []
    for (q, o, c, _), k in zip(iv, keep):
        if k: out += [(q, o, 1), (q, c, -1)]
    return None, sorted(out)


def route(fr, s, mh_tab, cut, hg):
    """where the default sized pass finishes the fragment, and the figures behind it"""
    q, P = fr["q"], fr["P"]
    mh = int(mh_tab[q]) if q > 0 else 0
    info = dict(P=P, seeds=fr["seeds"], minHits=mh, valid=len(fr["points"]), kept=None, runs=None)
    if P <= fused_cap(s):
        if mh <= 0: return (("HBM", "minHits") if P > 0 else ("none", None)), info
        if P == 0: return ("fused", None), info
        why, info["runs"] = fused_sweep(fr["points"], q, mh, cut, hg, s)
        return (("HBM", why) if why else ("fused", None)), info
    if mh <= 1: return ("HBM", "minHits"), info
    if s > MID_MAXSKETCH: return ("HBM", "sketch"), info
    if P > MID_MAXPTS: return ("HBM", "points"), info
    if fr["seeds"] > MID_MAXSEEDS: return ("mid>HBM", "seeds"), info
    why, kept = kept_points(fr, mh)
    if why: return ("mid>HBM", why), info
    info["kept"] = len(kept)
    if len(kept) > MID_MAXKEEP: return ("mid>HBM", "kept"), info
    why, info["runs"] = fused_sweep(kept, q, mh, cut, hg, s)
    return (("mid>HBM", why) if why else ("mid", None)), info


def counts(routes):
    """(pass_l1_mid(), pass_l1_literal()[0]) of a batch with these routes"""
    mid = sum(1 for (r, _), _ in routes if r in ("mid", "mid>HBM"))
    queued = sum(1 for (r, _), i in routes if r == "mid>HBM" or (r == "HBM" and i["P"] > 0))
    return mid, queued
