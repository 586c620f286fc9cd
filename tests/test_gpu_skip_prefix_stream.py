"""mm_pass_l1_literal: which L1 kernel took the fragments of the HBM point path in the last sized pass.

One batch -- eight contigs with four loci planted in each, 43 fragments cut from them with 5-8 % substitutions, one of them placed so
that its last interval point in one contig and its first in the next share a position (the one place where a position group can span
two contigs, which k_l1_stream leaves to the literal k_l1_sweep) -- is mapped two ways, each on a fresh context:

* plain, every fragment's points kept in HBM (MM_OPT_KEEP_POINTS, so that every fragment with a point is queued): `literal` is the
  length of the list k_l1_stream left, read back from the device; it must equal the number of fragments for which the oracle's sorted
  points hold such a group, and lie strictly between 0 and `queued`;
* under -Y reference groups (MM_FLAG_SKIP_PREFIX): every queued fragment is the literal kernel's, `literal == queued`.

Then both again in a fresh child process with MM_L1_LITERAL set (the library reads its environment once per context): `literal ==
queued` there, and stats / L1 / L2 / candidate mappings byte-identical to the first run.

k = 16, segLength 500, s = 32.  Reads are named r<i>: they belong to no reference group, so none of their points is dropped and the
oracle's point list is the device's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpucheck
import mmutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, L, S, PI = 16, 500, 32, 0.90
YFLAGS = U.FLAG_SKIP_PREFIX


# ----------------------------------------------------------------------------- inputs
def subst(a, seed, rate):
    """substitutions only, i.i.d. at `rate`"""
    r = U.splitmix64(seed, len(a))
    hit = (r >> np.uint64(11)).astype(np.float64) / float(1 << 53) < rate
    out = a.copy()
    idx = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), a[hit])
    out[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[(idx + 1 + ((r[hit] >> np.uint64(5)) % np.uint64(3)).astype(np.int64)) % 4]
    return out


def genome(seed, names, n=20000):
    return [(nm, U.random_dna(seed * 1000 + i, n)) for i, nm in enumerate(names)]


def plant(contigs, name, at, block):
    a = dict(contigs)[name]
    assert 0 <= at and at + len(block) <= len(a)
    a[at:at + len(block)] = block


def reads_from(block, seed, n, length, rate, first=0):
    """n reads of `length` bases cut from the block at spread offsets, substitutions at `rate`"""
    out = []
    for i in range(n):
        at = (i * 97) % max(1, len(block) - length + 1)
        out.append(("r%d" % (first + i), np.ascontiguousarray(subst(block[at:at + length], seed * 131 + i, rate))))
    return out


GROUP_NAMES = ["A#1#x", "A#1#y", "B#1#x", "B#1#y", "C#1#x", "C#1#y", "A#1#z", "A#2#x"]   # A#1 comes back behind C#1: a group of its own


def close_boundary(oracle, build, read, a, b, pi=None):
    """build(shift) -> contigs, with a locus in contig a and, moved by `shift`, in contig b (a + 1 == b): the shift at which the last
    interval point of `read`'s fragment in a and its first in b share a position -- in the sorted list the two are neighbours, the one
    place where a position group can span two contigs"""
    shift = 0
    for _ in range(4):
        cs = build(shift)
        pts = oracle_points(oracle, cs, [read], YFLAGS, pi=pi or PI)[0][0][0]
        pa = [x for x in pts if x[0] == a]; pb = [x for x in pts if x[0] == b]
        assert pa and pb
        if pa[-1][1] == pb[0][1]: return cs
        shift += pa[-1][1] - pb[0][1]
    raise AssertionError("the boundary does not close")


def case_groups(oracle):
    """three groups of two contigs, A#1 again behind them (Map::setRefGroups numbers it anew) and A#2; four loci, each in every contig,
    at offsets more than a read apart; one small locus in both contigs of B#1, placed so that its fragment's last point in B#1#x and
    first in B#1#y share a position: a position group across two contigs"""
    src = U.random_dna(77, 4 * 3000)
    small = U.random_dna(78, L + 600)
    small_read = ("r12", subst(small[300:300 + L], 9, 0.05))

    def build(shift):
        cs = genome(11, GROUP_NAMES, 26000)
        for li in range(4):
            for ci, (nm, _) in enumerate(cs):                    # contig ci holds locus li in slot (li + ci) % 4
                plant(cs, nm, 500 + ((li + ci) % 4) * 5500 + ci * 100, subst(src[li * 3000:(li + 1) * 3000], 500 + li * 16 + ci, 0.01))
        plant(cs, "B#1#x", 23300, small); plant(cs, "B#1#y", 23300 + shift, small)
        return cs
    cs = close_boundary(oracle, build, small_read, 2, 3)
    reads = []
    for li in range(4):
        reads += reads_from(src[li * 3000:(li + 1) * 3000], 40 + li, 3, 2 * L + 123, 0.05 + 0.01 * li, first=len(reads))
    assert small_read[0] == "r%d" % len(reads)
    reads.append(small_read)
    for ci in (0, 3, 7):                                         # unique sequence: points in one contig only
        reads.append(("r%d" % len(reads), subst(cs[ci][1][300:300 + L + 77].copy(), 60 + ci, 0.07)))
    return cs, reads


# ----------------------------------------------------------------------------- the oracle's view of a batch
def fragments_of(a):
    """Map::mapModule's split of a read: full segments and the overlapping tail"""
    n = len(a)
    if n < L: return []
    out = [(i * L, L) for i in range(n // L)]
    if n % L: out.append((n - L, L))
    return out


def oracle_points(oracle, contigs, reads, flags, pi=PI, kmerPct=0.001):
    """per fragment, in the device's fragment order: (sorted interval points as (seqId, pos, side), Q.sketchSize)"""
    h = oracle.session(contigs, K, L, S, pi, U.FILTER_MAP, flags, b"#", kmerPct)
    out = []
    for ri, (name, a) in enumerate(reads):
        for at, ln in fragments_of(a):
            e = oracle.map_fragment(h, a[at:at + ln], ri, name.encode(), len(a), S)
            out.append(([p[:3] for p in e["points"]], e["sketchSize"], e["l1"]))
    cut = oracle.cutoffs(h)
    oracle.free(h)
    return out, cut


def takes_literal(points, q_sketch, min_hits_tab, cutoffs, hg):
    """k_l1_stream's two rules on a fragment's sorted points: a position group spans two contigs, or minimumHits (after the
    sketchCutoffs step under hg) is <= 0"""
    if any(points[i][1] == points[i - 1][1] and points[i][0] != points[i - 1][0] for i in range(1, len(points))): return True
    min_hits = int(min_hits_tab[q_sketch])
    if hg:
        run, best = 0, 0
        for i, p in enumerate(points):
            run += 1 if p[2] == 1 else -1
            if i + 1 == len(points) or points[i + 1][1] != p[1]: best = max(best, run)
        if best >= min_hits:
            min_hits = max(min_hits, int(cutoffs[min(int(min(best, q_sketch) / max(S / 1000.0, 1.0)), len(cutoffs) - 1)]))
    return min_hits <= 0


def run_batch(oracle, contigs, reads, flags):
    """one sized pass over the batch on a fresh context: (queued, literal) of mm_pass_l1_literal, the pass's host waits, and everything
    it leaves as bytes.  Without FLAG_SKIP_PREFIX every fragment's points are kept in HBM: every fragment with a point is queued"""
    from mashmap_amd import capi
    grouped = bool(flags & U.FLAG_SKIP_PREFIX)
    h = oracle.session(contigs, K, L, S, PI, U.FILTER_MAP, flags, b"#" if grouped else b"\0", 0.001)
    ix = oracle.export_index(h)
    cflags = (capi.MM_FLAG_SKIP_PREFIX if grouped else 0) | (capi.MM_FLAG_HG_FILTER if flags & U.FLAG_HG else 0)
    ctx = capi.Context(k=K, segLength=L, sketchSize=S, flags=cflags)
    rg = gpucheck.prefix_groups([n for n, _ in contigs], "#")[1] if grouped else None
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"], rg)
    ctx.set_tables(oracle.min_hits_table(S, K, PI), oracle.cutoffs(h))
    ctx.set_replay_tables(*capi.stat_replay_tables(S, K, PI, 0.0, True))
    ctx.reads_upload([a for _, a in reads], [-1] * len(reads) if grouped else None, [-1] * len(reads), 0)
    if not grouped: ctx.keep_points(True)
    ctx.map()
    queued, literal = ctx.pass_l1_literal()
    stats, l1, l2 = ctx.results()
    out = dict(queued=queued, literal=literal, waits=ctx.pass_stats()[0], stats=stats.tobytes().hex(), l1=l1.tobytes().hex(), l2=l2.tobytes().hex(),
               mappings=ctx.mappings().tobytes().hex())
    ctx.close(); oracle.free(h)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("hg", [True, False], ids=["hg", "nohg"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "reference_groups"])
def test_literal_count_and_the_forced_literal_run(oracle, hg, grouped):
    cs, reads = case_groups(oracle)
    flags = (U.FLAG_SKIP_PREFIX if grouped else 0) | (U.FLAG_HG if hg else 0)
    per, cut = oracle_points(oracle, cs, reads, flags)
    with_points = [(p, q) for p, q, _ in per if p]
    here = run_batch(oracle, cs, reads, flags)
    print("queued %d, literal %d, host waits %d" % (here["queued"], here["literal"], here["waits"]))
    assert here["queued"] == len(with_points) == 43
    if grouped:
        assert here["literal"] == here["queued"]
    else:
        mh = oracle.min_hits_table(S, K, PI)
        expected = [i for i, (p, q) in enumerate(with_points) if takes_literal(p, q, mh, cut, hg)]
        assert here["literal"] == len(expected), (here["literal"], expected)
        assert 0 < here["literal"] < here["queued"]
    # the same batch with every queued fragment forced through the literal kernel, in a fresh process
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(flags)], capture_output=True, text=True, timeout=300, env=dict(os.environ, MM_L1_LITERAL="1"))
    assert p.returncode == 0, p.stderr[-3000:]
    there = json.loads(p.stdout.strip().splitlines()[-1])
    assert there["literal"] == there["queued"] == here["queued"]
    for what in ("stats", "l1", "l2", "mappings"):
        assert len(here[what]) > 0 and there[what] == here[what], "the forced literal run disagrees on " + what


def test_the_new_call_is_exported_and_declared():
    """CPU: libmashmap_hip.so exports mm_pass_l1_literal, the header declares it and the binding lists and types it"""
    import ctypes
    from mashmap_amd import capi
    assert "mm_pass_l1_literal" in capi.EXPORTS
    assert "mm_pass_l1_literal(const mm_ctx* ctx, uint64_t* queued, uint64_t* literal);" in open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "mm_pass_l1_literal")
    fn = capi.load().mm_pass_l1_literal
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 3
    assert callable(getattr(capi.Context, "pass_l1_literal"))
    assert capi.load().mm_abi_version() == 2                    # additive: the ABI version stays


if __name__ == "__main__":                                       # the child of the test above: the batch, flags = argv[1]
    sys.path.insert(0, ROOT)
    orc_ = U.Oracle()
    cs_, reads_ = case_groups(orc_)
    print(json.dumps(run_batch(orc_, cs_, reads_, int(sys.argv[1]))))
