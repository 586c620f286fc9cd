"""Planted inputs for k_l2_select (mashmap_amd/csrc/mm_select.hip, mm_select_core.h, mm_heap.h), doL2Mapping's best-first walk -- test
infrastructure for tests/test_select_walk.py (CPU) and tests/test_gpu_select_edges.py.

Inputs.  Reads of random DNA, one fragment each, over random contigs: a fragment's L1 candidates are exactly the clusters a Batch plants
through l1plant.Plan -- m overlapping intervals under the fragment's sketch ranks 0 .. m-1 give one candidate of intersectionSize m with
one L2 locus sharing m.  The clusters lie 1 500 bases apart, further than segLength, so none is joined to its neighbour, and a fragment's
candidates are emitted in slot order (seqId, position).  `shared=j` lowers the locus of a candidate to j shared hashes without moving its
L1 range: s reference-only hashes between the fragment's hashes of ranks j-1 and j, open over the whole cluster, fill the window's
smallest s hashes behind rank j-1 (reference-only hashes make no interval point, as in tests/l2plant.py).

Walkers.  hl_select_walk (tests/hostlogic/hostlogic.cpp) walks one fragment's integers twice: (a) MapPost::doL2MappingReplay -- libstdc++'s
std::make_heap / std::pop_heap and the reference's float expressions, once per reference group --, the reference of both test files; (b)
mm_select_fragment over mmhost::replayTables, the code the kernel compiles.

Cases.  CASES[name]() builds a batch once per process, from ONE oracle session over the planted index: per fragment the oracle's
candidates, loci and mappings, and the push sequences of both walkers.  The facts a case is named for are asserted by
tests/test_select_walk.py from those; a case holds what the test needs for that under "expect"."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import l1plant
import l2plant
import mmutil as U

K, L, S, PI = 16, 1000, 130, 0.85
HG = U.FLAG_HG
SLOT0, SLOT_STEP, CONTIG_LEN = 500, 1500, 40000
SLOTS_PER_CONTIG = (CONTIG_LEN - SLOT0 - 600) // SLOT_STEP + 1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HL_DIR = os.path.join(ROOT, "tests", "hostlogic")


@functools.lru_cache(maxsize=None)
def hostlogic():
    so, src = os.path.join(HL_DIR, "libhostlogic.so"), os.path.join(HL_DIR, "hostlogic.cpp")
    hdrs = [os.path.join(ROOT, "mashmap_amd", "host", f) for f in ("skch_map_post.hpp", "skch_types.hpp", "mm_stats.hpp")]
    hdrs += [os.path.join(ROOT, "mashmap_amd", "csrc", f) for f in ("mm_select_core.h", "mm_heap.h")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in [src] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wno-sign-compare", "-o", so, src])
    lib = C.CDLL(so)
    lib.hl_select_walk.restype = C.c_int
    return lib


@functools.lru_cache(maxsize=None)
def tables(s=S, k=K, pi=PI, keep_low=True):
    """(accept, minIsz) of mmhost::replayTables, as [Qs][x] arrays"""
    acc = np.zeros((s + 1, s + 1), dtype=np.uint8); mi = np.zeros((s + 1, s + 1), dtype=np.int16)
    vp = C.c_void_p
    hostlogic().hl_replay_tables(C.c_int(s), C.c_int(k), C.c_float(pi), C.c_int(1 if keep_low else 0), acc.ctypes.data_as(vp), mi.ctypes.data_as(vp))
    return acc, mi


def first_accepted(qs, s=S, k=K, pi=PI, keep_low=True):
    """the smallest shared count a fragment of sketch size qs has reported"""
    return int(np.argmax(tables(s, k, pi, keep_low)[0][qs, :qs + 1]))


def walk(k, s, pi, flags, qs, l1, l2, groups, ncontigs):
    """l1: [(seqId, rangeStart, rangeEnd, intersectionSize)], l2: [(candidate, seqId, meanOptimalPos, optimalStart, optimalEnd, shared, strand)]
    in candidate order (a fragment of Oracle.map_fragment).  Returns the push sequences (a, b), each [(candidate, index into l2)]"""
    nC = len(l1)
    seq = np.array([c[0] for c in l1], dtype=np.int32); isz = np.array([c[3] for c in l1], dtype=np.int32)
    off = np.zeros(nC + 1, dtype=np.int32)
    for x in l2: off[x[0] + 1] += 1
    off = np.cumsum(off, dtype=np.int32)
    assert [x[0] for x in l2] == sorted(x[0] for x in l2)
    shared = np.array([x[5] for x in l2], dtype=np.int32)
    grp = np.array(groups, dtype=np.int32) if groups is not None else None
    cap = len(l2) + 1
    oa, ob = np.zeros(2 * cap, dtype=np.int32), np.zeros(2 * cap, dtype=np.int32)
    na, nb = C.c_int32(), C.c_int32()
    vp = C.c_void_p
    hflags = (1 if flags & U.FLAG_HG else 0) | (4 if flags & U.FLAG_SKIP_PREFIX else 0) | (64 if flags & U.FLAG_DROP_LOW_ID else 0)
    rc = hostlogic().hl_select_walk(C.c_int(k), C.c_int(s), C.c_float(pi), C.c_int(hflags), C.c_int(qs), C.c_int(nC), seq.ctypes.data_as(vp), isz.ctypes.data_as(vp),
                                    off.ctypes.data_as(vp), shared.ctypes.data_as(vp), C.c_int(ncontigs), grp.ctypes.data_as(vp) if grp is not None else None,
                                    oa.ctypes.data_as(vp), C.byref(na), ob.ctypes.data_as(vp), C.byref(nb), C.c_int(cap))
    assert rc == 0
    return [tuple(p) for p in oa[:2 * na.value].reshape(-1, 2).tolist()], [tuple(p) for p in ob[:2 * nb.value].reshape(-1, 2).tolist()]


def record_key(l2row):
    """what identifies a pushed locus in a device record: (refSeqId, refStartPos, conservedSketches, strand)"""
    return (l2row[1], l2row[2], l2row[5], l2row[6])


class Batch:
    def __init__(self, name, nreads, ncontigs, seed, s=S, pi=PI, flags=HG, contig_names=None, read_names=None, delim="\0"):
        self.oracle = U.Oracle()
        self.name, self.s, self.pi, self.flags, self.delim, self.kmerPct = name, s, pi, flags, delim, 0.0
        self.reads = [((read_names or {}).get(i, "r%d" % i), U.random_dna(seed + i, L)) for i in range(nreads)]
        self.contigs = [((contig_names or {}).get(i, "c%d" % i), U.random_dna(seed + 100000 + i, CONTIG_LEN)) for i in range(ncontigs)]
        self.plan = l1plant.Plan(self.oracle, self.reads, K, s)
        self.piles, self.slot, self.planted = [], 0, [[] for _ in range(nreads)]

    def skip_to_contig(self, q):
        assert self.slot <= q * SLOTS_PER_CONTIG
        self.slot = q * SLOTS_PER_CONTIG

    def cand(self, f, m, shared=None):
        """the next slot gets a candidate of fragment f with intersectionSize m and one locus sharing `shared` (default m).  Returns its
        index among the fragment's candidates"""
        q, at = self.slot // SLOTS_PER_CONTIG, SLOT0 + (self.slot % SLOTS_PER_CONTIG) * SLOT_STEP
        assert q < len(self.contigs), "out of slots"
        self.slot += 1
        self.plan.cluster(f, list(range(m)), q, at, step=3, width=200)
        if shared is not None and shared != m:
            assert 1 <= shared < m
            h = self.plan.hashes[f]
            lo = h[shared - 1]
            assert h[shared] - lo > self.s + 1
            self.piles.append((lo, q, at - 150, at + 3 * m + 300))
        self.planted[f].append((q, m, m if shared is None else shared))
        return len(self.planted[f]) - 1

    def tie(self, f, n, m, shared=None):
        return [self.cand(f, m, shared) for _ in range(n)]

    def frequent(self, f, rank, q, at):
        """40 records under the fragment's hash of that rank, 2 bases long, 300 apart: the one frequent seed of the batch"""
        self.plan.singles(f, [rank], q, at, 40, 300, 2)

    def mutate(self, natural):
        out = self.plan.merged(natural)
        if not self.piles: return out
        add = np.zeros(len(self.piles) * self.s, dtype=U.MINMER_DT)
        for i, (lo, q, w0, end) in enumerate(self.piles):
            for j in range(self.s): add[i * self.s + j] = (lo + 1 + j, w0 + j, end, q, 1, 0)
        sketch_hashes = {x for hs in self.plan.hashes for x in hs}
        assert not set(add["hash"].tolist()) & (set(out["hash"].tolist()) | sketch_hashes)
        return l2plant.resort(np.concatenate([out, add]))

    def groups(self):
        if not self.flags & U.FLAG_SKIP_PREFIX: return None
        import gpucheck
        return gpucheck.prefix_groups([n for n, _ in self.contigs], self.delim)[1]

    def finish(self, expect=None):
        o = self.oracle
        if self.kmerPct == "one":                                 # the share of one and a half hashes: the threshold falls on the most frequent hash
            nat = np.concatenate([o.add_minmers(a, K, L, self.s, i) for i, (_, a) in enumerate(self.contigs)])
            self.kmerPct = 100.0 * 1.5 / int(np.unique(self.mutate(nat)["hash"]).size)
        h = o.session(self.contigs, K, L, self.s, self.pi, U.FILTER_MAP, self.flags, self.delim.encode() if self.delim != "\0" else b"\0", self.kmerPct,
                      mutate_index=self.mutate)
        frs = [o.map_fragment(h, a, i, n.encode(), len(a), self.s) for i, (n, a) in enumerate(self.reads)]
        o.free(h)
        grp = self.groups()
        per = []
        for f, e in enumerate(frs):
            a, b = walk(K, self.s, self.pi, self.flags, e["sketchSize"], e["l1"], e["l2"], grp, len(self.contigs))
            per.append(dict(qs=e["sketchSize"], l1=e["l1"], l2=e["l2"], maps_i=e["maps_i"], a=a, b=b, planted=self.planted[f]))
        return dict(name=self.name, contigs=self.contigs, reads=self.reads, mutate=self.mutate, s=self.s, pi=self.pi, flags=self.flags, delim=self.delim,
                    kmerPct=self.kmerPct, per=per, expect=expect or {})


def pushed_records(fr, which="a"):
    """the record keys of a walker's push sequence"""
    return [record_key(fr["l2"][i]) for _, i in fr[which]]


# ----------------------------------------------------------------------------- cases
TIE_N = (2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 31, 32, 33, 64)
T_CUT, T_KEPT = 9, 8                                             # minIsz[130][9] == 10: a tie at 9 is cut to one; minIsz[130][8] == 8: a tie at 8 is kept


def contigs_for(ncand):
    return (ncand + SLOTS_PER_CONTIG - 1) // SLOTS_PER_CONTIG


def shuffled(items, seed):
    """a fixed permutation: the levels of a fragment do not arrive sorted"""
    r = U.splitmix64(seed, len(items)).tolist()
    return [x for _, _, x in sorted(zip(r, range(len(items)), items))]


def plant_mixed(b, f, spec, seed):
    """spec: [(n, intersectionSize, shared | None)]; the candidates in a fixed shuffled order.  Returns per candidate (intersectionSize, shared)"""
    order = shuffled([(m, sh) for n, m, sh in spec for _ in range(n)], seed)
    for m, sh in order: b.cand(f, m, sh)
    return [(m, m if sh is None else sh) for m, sh in order]


@functools.lru_cache(maxsize=None)
def ties(t):
    """one fragment per n of TIE_N: n candidates of intersectionSize t, each with one locus sharing t"""
    b = Batch("ties t=%d" % t, len(TIE_N), contigs_for(sum(TIE_N)), 9100 + t)
    for f, n in enumerate(TIE_N): b.tie(f, n, t)
    return b.finish(dict(t=t, n=TIE_N))


@functools.lru_cache(maxsize=None)
def levels():
    """fragment 0: three candidates at 12 among five at 9 -- both levels are cut to one, so one 12 is all; fragment 1: three at 8 over five at
    5 -- the 8s are kept, their best cuts the 5s; fragment 2: the same with the 8s' loci lowered to 5 -- best stays 5 and all eight are
    reported; fragment 3: three levels, 11, 7 and 4, every locus at 4 -- minIsz[130][4] == 4 keeps all of them and cuts the two at 3"""
    b = Batch("levels", 4, contigs_for(8 + 8 + 8 + 13), 9200)
    spec = {0: [(3, 12, None), (5, 9, None)], 1: [(3, 8, None), (5, 5, None)], 2: [(3, 8, 5), (5, 5, None)], 3: [(2, 11, 4), (4, 7, 4), (5, 4, None), (2, 3, None)]}
    planted = {f: plant_mixed(b, f, sp, 9210 + f) for f, sp in spec.items()}
    return b.finish(dict(planted=planted, reported={0: [12], 1: [8] * 3, 2: [5] * 8, 3: [4] * 11}))


@functools.lru_cache(maxsize=None)
def cut_between():
    """fragment 0: a candidate at 12 whose locus shares 7: best = 7, minIsz[130][7] == 7 -- the two candidates at 7 are walked, the two at 6
    are cut.  Fragment 1: a candidate at 14 whose locus shares 9: best = 9, minIsz[130][9] == 10 -- the two at 10 (loci lowered to 9, so
    that best stays) are walked, the two at 9 are cut although they equal best"""
    b = Batch("cut_between", 2, 1, 9300)
    for m, sh in ((6, None), (7, None), (12, 7), (7, None), (6, None)): b.cand(0, m, sh)
    for m, sh in ((9, None), (10, 9), (14, 9), (10, 9), (9, None)): b.cand(1, m, sh)
    return b.finish(dict(best={0: 7, 1: 9}, walked={0: [1, 2, 3], 1: [1, 2, 3]}, cut={0: [0, 4], 1: [0, 4]}))


@functools.lru_cache(maxsize=None)
def acceptance(drop_low):
    """a = the first accepted shared count of row 130 (3; 6 with FLAG_DROP_LOW_ID).  The candidate with the largest intersectionSize is walked
    first and its locus shares a - 1: refused, best stays 0.  Two candidates at a with loci sharing a are reported (minIsz[130][a] == a for both
    values of a); a candidate at a whose locus is lowered to a - 1 is walked and refused; with FLAG_DROP_LOW_ID a candidate at a - 1 (a refusal as
    it occurs by itself) lies below the cut"""
    a = first_accepted(S, keep_low=not drop_low)
    b = Batch("acceptance drop_low=%d" % drop_low, 1, 1, 9400 + drop_low, flags=HG | (U.FLAG_DROP_LOW_ID if drop_low else 0))
    spec = [(a, None), (a + 2, a - 1), (a, a - 1), (a, None)] + ([(a - 1, None)] if drop_low else [])
    for m, sh in spec: b.cand(0, m, sh)
    return b.finish(dict(a=a, spec=[(m, m if sh is None else sh) for m, sh in spec]))


@functools.lru_cache(maxsize=None)
def rows():
    """fragment 0: its seed of rank 100 is the batch's one frequent seed, Qs = 129; fragment 1: Qs = 130.  Both hold a six-way tie at 9:
    minIsz[130][9] == 10 cuts it to one, minIsz[129][9] == 9 keeps all six"""
    b = Batch("rows", 2, 2, 9500)
    b.tie(0, 6, T_CUT); b.tie(1, 6, T_CUT)
    b.frequent(0, 100, 1, 1000)
    b.kmerPct = "one"
    return b.finish()


@functools.lru_cache(maxsize=None)
def hg_off():
    """flags 0: no heap and no cut -- every accepted locus in candidate order; the locus lowered to 2 is refused"""
    b = Batch("hg_off", 1, 1, 9600, flags=0)
    spec = [(9, None), (5, 2), (12, None), (9, None), (3, None), (12, 7), (4, None)]
    for m, sh in spec: b.cand(0, m, sh)
    return b.finish(dict(spec=[(m, m if sh is None else sh) for m, sh in spec]))


@functools.lru_cache(maxsize=None)
def skip_prefix():
    """contigs A_0, B_0, C_0, one reference group each (delimiter _).  Read 0 has one candidate at 12 on A_0, a six-way tie at 9 on B_0 and
    one candidate at 5 on C_0: best starts again in every group, so the tie is cut to one by its own first member (not to none by A_0's
    12), and the 5 -- below the cut a best of 9 sets -- is reported.  Read 1 is named B_r: its own group is skipped, the same plan leaves it
    the candidates on A_0 and C_0"""
    b = Batch("skip_prefix", 2, 3, 9700, flags=HG | U.FLAG_SKIP_PREFIX, contig_names={0: "A_0", 1: "B_0", 2: "C_0"}, read_names={0: "q_0", 1: "B_r"}, delim="_")
    for f in (0, 1): b.cand(f, 12)
    b.skip_to_contig(1)
    for f in (0, 1): b.tie(f, 6, T_CUT)
    b.skip_to_contig(2)
    for f in (0, 1): b.cand(f, 5)
    return b.finish()


@functools.lru_cache(maxsize=None)
def placement():
    """fragment 0: a tie; 1: no candidate; 2: a read of N, Qs = 0; 3: a tie; 4: no candidate; 5: a kept tie"""
    b = Batch("placement", 6, 1, 9800)
    b.reads[2] = ("r2", np.full(L, ord("N"), dtype=np.uint8))
    b.plan = l1plant.Plan(b.oracle, b.reads, K, b.s)
    b.tie(0, 6, T_CUT); b.tie(3, 5, T_CUT); b.tie(5, 4, T_KEPT)
    return b.finish()


@functools.lru_cache(maxsize=None)
def seam():
    """257 fragments, one thread each in workgroups of 256: fragments 255 and 256 carry ties (and fragment 0, so that the first workgroup has
    records before its last thread's)"""
    b = Batch("seam", 257, 1, 9900)
    b.tie(0, 3, T_CUT); b.tie(255, 6, T_CUT); b.tie(256, 5, T_KEPT)
    return b.finish()


MANY = 1000                                                      # candidates of the one fragment of `many`: what Oracle.map_fragment's buffer of 1 024 candidates
                                                                 # takes; the case's oracle session runs 1.4 s at this count (0.45 s at 200, 1.0 s at 500)


@functools.lru_cache(maxsize=None)
def many():
    """MANY candidates of one fragment, levels 12, 9, 8, 5 and 4 in a fixed shuffled order, every locus of the levels above 5 lowered to 5: best
    stays 5, minIsz[130][5] == 5, so the walk pops four fifths of the candidates off the heap and reports each; the fifth at 4 is cut"""
    n = MANY
    b = Batch("many", 1, contigs_for(n), 10000)
    spec = [(n * 3 // 20, 12, 5), (n // 5, 9, 5), (n // 4, 8, 5), (n // 5, 5, None)]
    reported = sum(x[0] for x in spec)
    spec.append((n - reported, 4, None))
    planted = plant_mixed(b, 0, spec, 10001)
    return b.finish(dict(planted=planted, reported=reported))


CASES = {"ties_cut": lambda: ties(T_CUT), "ties_kept": lambda: ties(T_KEPT), "levels": levels, "cut_between": cut_between,
         "acceptance": lambda: acceptance(False), "acceptance_drop_low_id": lambda: acceptance(True), "rows": rows, "hg_off": hg_off,
         "skip_prefix": skip_prefix, "placement": placement, "seam": seam, "many": many}
