"""A model of what the L2 stream kernels branch on, and planters that put an index on those branches -- test infrastructure for
tests/test_l2_plant_model.py (CPU) and tests/test_gpu_l2_edges.py (mashmap_amd/csrc/mm_l2.hip: k_l2_extents, k_l2_locate,
k_l2_sweep<narrow|wide>, k_l2_sweep_exact).

Slice model.  `slice_model` restates the slice arithmetic from the COMMENTS of k_l2_extents, k_l2_locate and k_l2_sweep -- not from
their code --, over the exported minmerIndex (as tests/mmutil.py restates the capacities a sized pass leaves):
  * every record is two events of its contig, an insert with key wpos * 2 + 1 and an eviction with key wpos_end * 2, in key order
    (record order among equals);
  * the slide of a candidate (seqId, rangeStart, rangeEnd) is [lower_bound(rangeStart * 2 + 1), lower_bound(rangeEnd * 2 + 2));
  * the pre-load takes the records with wpos >= target = rangeStart - segLength - 1 that are still open at rangeStart; the kernel
    reads them from the list of records open at the block boundary B = rangeStart rounded down to 2^10 (wpos < B < wpos_end) and
    from the events in [max(B, target), rangeStart): those two counts together are what the pre-load limit (4000) is held against;
  * a stream position is the wpos of an insert minus the wpos of the insert before it (rangeStart at first); a difference beyond the
    entry's delta field (MAXDELTA: 8191 for the 11-bit sketch-position field, 2047 for the 13-bit one) takes a skip entry.  The end
    marker carries the wpos of the contig's next insert behind the slide's last one, or that one's own;
  * a cell counts 1 (its query hash) + the open reference-only hashes h with q[p-1] < h < q[p]; hashes above the largest query hash
    have no cell.  The narrow sweep holds a count of 31 (5 bits), the wide one 4095 (12 bits): an insert that would raise a cell
    beyond that sends the candidate on (narrow -> wide -> exact), and so does a pre-load state with a cell beyond 31 (-> wide).

Planters.  Each returns a `mutate_index` callable for Oracle.session.  Reference-only hashes create no interval points, so a planter
that adds or rewrites only those leaves the L1 candidates where they were: the cases run the oracle once on the plain index for the
ranges and the sketches, plant against those, and assert afterwards that the ranges did not move (`hole` drops records of any hash and
is planted blind: its cases take the ranges from the holed index).

Cases.  `CASES` names the inputs of both test files; CASES[name]() returns one with the model's facts per candidate, computed once per
process."""
import bisect
import functools

import numpy as np

import mmutil as U

OPEN_BLOCK_SHIFT = 10                                            # mm_internal.h: MM_OPEN_BLOCK_SHIFT
MAXDELTA = {11: 8191, 13: 2047}                                  # mm_l2.hip: EF<JB>::MAXDELTA
NARROW_MAX, WIDE_MAX = 31, 4095                                  # the largest count a 5-bit / a 12-bit cell holds
PRE_LIMIT = 4000                                                 # mm_internal.h: l2PreLimit
U64 = (1 << 64) - 1


def jb_of(s):
    """width of the stream entries' sketch-position field (mm_l2_plan.h: 11 for sketches of up to 2046 entries)"""
    return 11 if s <= 2046 else 13


class Stream:
    """the contigs' event streams of an exported minmerIndex"""

    def __init__(self, recs):
        self.recs, self.by = recs, {}
        seq = recs["seqId"]
        for q in np.unique(seq).tolist():
            r = recs[seq == q]
            key = np.empty(2 * len(r), dtype=np.int64)
            key[0::2] = r["wpos"].astype(np.int64) * 2 + 1
            key[1::2] = r["wpos_end"].astype(np.int64) * 2
            o = np.argsort(key, kind="stable")
            ins = (o & 1) == 0
            self.by[q] = dict(key=key[o], ins=ins, insAt=np.nonzero(ins)[0], hash=r["hash"][o >> 1], r=r)


def slice_model(index_records, candidate, maxdelta, seg_length, sketch=None):
    """index_records: the exported minmerIndex (or a Stream over it); candidate: (seqId, rangeStart, rangeEnd, ...); sketch: the
    fragment's sketch hashes in ascending order, for the cell counts.  See the module's docstring for what is restated here."""
    st = index_records if isinstance(index_records, Stream) else Stream(index_records)
    q, rs, re = int(candidate[0]), int(candidate[1]), int(candidate[2])
    ev = st.by[q]
    key, ins, ins_at, r = ev["key"], ev["ins"], ev["insAt"], ev["r"]
    target = rs - seg_length - 1
    B = (rs >> OPEN_BLOCK_SHIFT) << OPEN_BLOCK_SHIFT
    lb = lambda k: int(np.searchsorted(key, k, side="left"))
    e0 = lb(2 * max(target, B))
    e_mid, ub = lb(2 * rs + 1), lb(2 * re + 2)
    n_open = int(np.count_nonzero((r["wpos"] < B) & (r["wpos_end"] > B)))
    a, b = int(np.searchsorted(ins_at, e_mid)), int(np.searchsorted(ins_at, ub))      # the slide's inserts: ins_at[a:b]
    w = (key[ins_at[a:b]] >> 1).tolist()
    out = dict(n_slide=ub - e_mid, n_inserts=b - a, no_insert=b == a, preload_records=n_open + (e_mid - e0),
               last_of_contig=b == len(ins_at), behind_evictions=(int(ins_at[b]) if b < len(ins_at) else len(key)) - ub)
    if b == a:
        out.update(gap_in=False, first_gap=False, end_skip=False, tail_evictions=ub - e_mid)
    else:
        next_w = int(key[ins_at[b]] >> 1) if b < len(ins_at) else w[-1]
        out.update(gap_in=any(y - x > maxdelta for x, y in zip(w, w[1:])), first_gap=w[0] - rs > maxdelta, end_skip=next_w - w[-1] > maxdelta,
                   tail_evictions=ub - 1 - int(ins_at[b - 1]), first_delta=w[0] - rs, next_w=next_w, max_gap=max([y - x for x, y in zip(w, w[1:])] + [0]), end_gap=next_w - w[-1])
    if sketch is not None:
        qs = [int(x) for x in sketch]
        assert qs == sorted(qs) and len(set(qs)) == len(qs)
        qmax, inq = qs[-1], set(qs)
        cnt = {}
        keep = (r["wpos"] >= target) & (r["wpos"] < rs) & (r["wpos_end"] > rs)
        for h in r["hash"][keep].tolist():
            if h <= qmax and h not in inq:
                j = bisect.bisect_left(qs, h); cnt[j] = cnt.get(j, 1) + 1
        out["cell_preload"] = max(cnt.values(), default=1)
        top = 0
        end = int(ins_at[b - 1]) + 1 if b > a else e_mid                                # nothing behind the last insert is streamed
        for isin, h in zip(ins[e_mid:end].tolist(), ev["hash"][e_mid:end].tolist()):
            if h > qmax or h in inq: continue
            j = bisect.bisect_left(qs, h)
            if isin:
                cnt[j] = cnt.get(j, 1) + 1
                top = max(top, cnt[j])
            else:
                cnt[j] = cnt.get(j, 1) - 1
                assert cnt[j] >= 1, "an eviction of a record that was neither pre-loaded nor inserted"
        out["cell_slide"] = top
        out["slide_hashes"] = set(ev["hash"][e_mid:end][ins[e_mid:end]].tolist())
    return out


def route(m):
    """the sweep kernels a candidate with these facts goes through, and hence what it adds to the "l2" launch count of a sized pass"""
    if m["preload_records"] >= PRE_LIMIT: return ("narrow", "wide", "exact")
    if m["cell_preload"] > NARROW_MAX or m["cell_slide"] > NARROW_MAX:
        return ("narrow", "wide", "exact") if max(m["cell_slide"], m["cell_preload"]) > WIDE_MAX else ("narrow", "wide")
    return ("narrow",)


# ----------------------------------------------------------------------------- planters
def resort(recs):
    """(seqId, wpos), originals first among equals"""
    return recs[np.lexsort((np.arange(len(recs)), recs["wpos"], recs["seqId"]))]


def hole(seqId, a, b=None):
    """drops the records of the contig with a <= wpos < b (b None: to its end)"""
    def f(recs):
        m = (recs["seqId"] == seqId) & (recs["wpos"] >= a)
        if b is not None: m &= recs["wpos"] < b
        return recs[~m]
    return f


def neighbour_values(sketch_hashes):
    """q[p] - 1 and q[p] + 1 of every p (qmax + 1 among them), 0 and 2^64 - 1; each once"""
    qs = [int(x) for x in sketch_hashes]
    out = []
    for x in qs + [1, U64 - 1]: out += [x - 1, x + 1]
    return [v for v in dict.fromkeys(out) if 0 <= v <= U64 and v != 2 and v != U64 - 2]


def neighbours(sketch_hashes, seqId, lo, hi):
    """rewrites the hashes of the contig's records with lo <= wpos < hi that the sketch does not hold, cycling over q[p] - 1 and q[p] + 1
    of every p, then 0, qmax + 1 and 2^64 - 1; a value that is in the sketch or in the index is left out"""
    inq = set(int(x) for x in sketch_hashes)
    def f(recs):
        have = set(recs["hash"].tolist())
        vals = [v for v in neighbour_values(sketch_hashes) if 0 <= v <= U64 and v not in inq and v not in have]
        out = recs.copy()
        at = [i for i in np.nonzero((recs["seqId"] == seqId) & (recs["wpos"] >= lo) & (recs["wpos"] < hi))[0].tolist() if int(recs["hash"][i]) not in inq]
        for n, i in enumerate(at): out["hash"][i] = vals[n % len(vals)]
        f.placed = min(len(at), len(vals)); f.values = vals
        return out
    return f


def pile(hash_lo, n, seqId, wpos0, span, step=1):
    """adds n records with the hashes hash_lo + 1 .. hash_lo + n at wpos0, wpos0 + step, .., each open for `span`"""
    def f(recs):
        add = np.zeros(n, dtype=U.MINMER_DT)
        for i in range(n): add[i] = (hash_lo + 1 + i, wpos0 + i * step, wpos0 + i * step + span, seqId, 1, 0)
        assert not set(add["hash"].tolist()) & set(recs["hash"].tolist())
        return resort(np.concatenate([recs, add]))
    return f


def chain(*fs):
    def f(recs):
        for g in fs: recs = g(recs)
        return recs
    return f


# ----------------------------------------------------------------------------- cases
K, PI = 19, 0.85


def read_at(g, x, L, seed, err):
    """one fragment: exactly L bases of the contig from x on, with ONT-like errors"""
    return U.mutate(g[x:x + L + L // 8], seed, err)[:L].copy()


def view(oracle, c, mutate):
    """(minmerIndex, the oracle's per-fragment data) of the case's batch over the index `mutate` leaves"""
    h = oracle.session(c["contigs"], c["k"], c["L"], c["s"], c["pi"], U.FILTER_MAP, c["flags"], b"\0", 0.0, mutate_index=mutate)
    recs = oracle.index_array(h)
    frs = [oracle.map_fragment(h, a, i, n.encode(), len(a), c["s"]) for i, (n, a) in enumerate(c["reads"])]
    oracle.free(h)
    return recs, frs


def facts(recs, frs, L, s):
    """slice_model of every L1 candidate of every fragment"""
    st, out = Stream(recs), []
    for f, e in enumerate(frs):
        qs = [x[0] for x in e["sketch"]]
        for c in e["l1"]:
            m = slice_model(st, c, MAXDELTA[jb_of(s)], L, qs)
            m.update(frag=f, cand=c, route=route(m))
            out.append(m)
    return out


def case(name, contigs, reads, L, s, flags=U.FLAG_HG):
    assert all(len(a) == L for _, a in reads)                    # one fragment per read
    return dict(name=name, contigs=contigs, reads=reads, k=K, L=L, s=s, pi=PI, flags=flags, mutate=None)


def finish(oracle, c, mutate, plain=None):
    """the facts of the case over the planted index; plain: the fragments' data over the plain index -- the L1 candidates must not have moved"""
    c["mutate"] = mutate
    recs, frs = view(oracle, c, mutate)
    if plain is not None:
        assert [e["l1"] for e in frs] == [e["l1"] for e in plain], "planting moved an L1 candidate"
    c["facts"] = facts(recs, frs, c["L"], c["s"])
    c["l2"] = [e["l2"] for e in frs]                              # per fragment: (candidate, seqId, meanOptimalPos, optimalStart, optimalEnd, shared, strand)
    c["launches"] = len(set(x for m in c["facts"] for x in m["route"]))
    assert c["facts"], c["name"] + ": no L1 candidate"
    return c


def summary(c):
    return "\n".join("%s frag %d %r: %r" % (c["name"], m["frag"], m["cand"], {k: v for k, v in m.items() if k not in ("slide_hashes", "frag", "cand")}) for m in c["facts"])


@functools.lru_cache(maxsize=None)
def skip_jb11(s):
    """a sketch of 3 or 5 per 30 kbp: the index holds a record every few thousand bases"""
    oracle, L = U.Oracle(), 30000
    g = U.random_dna(7101, 600000)
    reads = [("r%d" % i, read_at(g, 20000 + 47000 * i, L, 7200 + i, 0.02)) for i in range(12)]
    return finish(oracle, case("skip_jb11 s=%d" % s, [("c0", g), ("decoy", U.random_dna(7102, 100000))], reads, L, s), None)


@functools.lru_cache(maxsize=None)
def skip_jb13():
    """the 13-bit position field (MAXDELTA 2047) and a hole of 2 500 bases: two ranges that end inside the hole, two that span it -- one of
    a read before the hole, one of a read behind it, whose best position then lies behind the skip.  A second hole begins inside the best
    run of the last read: that run ends with the end marker, 21 911 bases behind the last insert, and with 2 047 evictions between them.
    Without the HG filter, whose table the oracle takes half a minute to build at this sketch size"""
    oracle, L, s = U.Oracle(), 21000, 2100
    g = U.random_dna(7301, 200000)
    reads = [("r%d" % i, read_at(g, x, L, 7400 + i, 0.02)) for i, x in enumerate((80150, 80300, 92000, 103000, 140150))]
    return finish(oracle, case("skip_jb13", [("c0", g)], reads, L, s, flags=0), chain(hole(0, 100000, 102500), hole(0, 140100, 162000)))


def closers(n, seqId, wpos0, end0):
    """adds n records that open every 5 bases from wpos0 and close every 3 bases from end0; hashes from 2^63 up: above any sketch's range"""
    def f(recs):
        add = np.zeros(n, dtype=U.MINMER_DT)
        for i in range(n): add[i] = ((1 << 63) + i, wpos0 + 5 * i, end0 + 3 * i, seqId, 1, 0)
        assert not set(add["hash"].tolist()) & set(recs["hash"].tolist())
        return resort(np.concatenate([recs, add]))
    return f


@functools.lru_cache(maxsize=None)
def tail_and_behind():
    """a hole of 4 000 bases.  About s records are open where it begins, so a range that ends inside it has at most about 130 evictions
    behind its last insert whatever the hole's width: 100 records more that open before the hole and close inside it bring the ranges
    that end there beyond 128"""
    oracle, L, s = U.Oracle(), 5000, 130
    g = U.random_dna(7501, 100000)
    reads = [("r%d" % i, read_at(g, x, L, 7600 + i, 0.02)) for i, x in enumerate(range(42000, 56001, 500))]
    return finish(oracle, case("tail_and_behind", [("c0", g)], reads, L, s), chain(hole(0, 50000, 54000), closers(100, 0, 49000, 50300)))


@functools.lru_cache(maxsize=None)
def last_of_contig():
    """the contig's records end at 95 000, inside the ranges of the reads that reach that far"""
    oracle, L, s = U.Oracle(), 5000, 130
    g = U.random_dna(7901, 110000)
    reads = [("r%d" % i, read_at(g, x, L, 8000 + i, 0.02)) for i, x in enumerate(range(92000, 99501, 500))]
    return finish(oracle, case("last_of_contig", [("c0", g)], reads, L, s), hole(0, 95000, None))


def one_read(name, L, s, err, seed):
    """a contig of 12 segments and one read out of its middle, without the HG filter: the L1 range is about two segments long"""
    g = U.random_dna(seed, 12 * L)
    return case(name, [("c0", g)], [("r0", read_at(g, 5 * L, L, seed + 1, err))], L, s, flags=0)


def only_candidate(frs):
    assert len(frs) == 1 and len(frs[0]["l1"]) == 1, [e["l1"] for e in frs]
    return frs[0]["l1"][0], [x[0] for x in frs[0]["sketch"]]


@functools.lru_cache(maxsize=None)
def hash_neighbours(L, s):
    """8 % error: fewer of the contig's records carry a hash of the read's sketch, which leaves more records to rewrite than there are values"""
    oracle = U.Oracle()
    c = one_read("hash_neighbours s=%d" % s, L, s, 0.08, 8101)
    _, plain = view(oracle, c, None)
    (q, rs, re, _), qs = only_candidate(plain)
    mut = neighbours(qs, q, rs, re + 1)
    finish(oracle, c, mut, plain)
    c["values"], c["placed"], c["sketch"] = mut.values, mut.placed, qs
    return c


def widest_cell(qs):
    """the query hash with the most room up to the next one, away from the sketch's ends"""
    p = max(range(len(qs) // 4, 3 * len(qs) // 4), key=lambda i: qs[i + 1] - qs[i])
    assert qs[p + 1] - qs[p] > 10000
    return p


def tuned(oracle, c, plain, fact, want, planter):
    """plants planter(n) with the n that brings the only candidate's `fact` to exactly `want` (the contig's own records count as well)"""
    n = want - 1
    for _ in range(6):
        finish(oracle, c, planter(n), plain)
        got = c["facts"][0][fact]
        if got == want: break
        n += want - got
    assert c["facts"][0][fact] == want, (c["name"], fact, want, c["facts"][0][fact])
    c["planted"] = n
    return c


@functools.lru_cache(maxsize=None)
def cell_slide(want):
    """a pile of reference-only hashes inside the slide, all open at once under one query cell: the cell's count reaches `want`"""
    oracle = U.Oracle()
    L, s = (5000, 130) if want < 100 else (10000, 200)
    c = one_read("cell_slide %d" % want, L, s, 0.02, 8201)
    _, plain = view(oracle, c, None)
    (q, rs, re, _), qs = only_candidate(plain)
    p = widest_cell(qs)
    assert re - rs > 2 * want + 400 and want + 200 < L
    return tuned(oracle, c, plain, "cell_slide", want, lambda n: pile(qs[p], n, q, rs + 100, n + 100))


@functools.lru_cache(maxsize=None)
def cell_preload(want):
    """the same pile before rangeStart, open across it"""
    oracle = U.Oracle()
    c = one_read("cell_preload %d" % want, 5000, 130, 0.02, 8301)
    _, plain = view(oracle, c, None)
    (q, rs, re, _), qs = only_candidate(plain)
    p = widest_cell(qs)
    return tuned(oracle, c, plain, "cell_preload", want, lambda n: pile(qs[p], n, q, rs - n - 10, n + 12))


def pads(n, seqId, rs, L):
    """n units of pre-load that is closed at rangeStart.  A record open over the block boundary B before rangeStart and evicted at
    rangeStart is on the block's open list and has its eviction among the events in [B, rangeStart): two units; a record evicted at B itself
    is an event only: one unit.  Hashes from 2^63 up: above any sketch's range"""
    B = (rs >> OPEN_BLOCK_SHIFT) << OPEN_BLOCK_SHIFT
    assert rs > B and n // 2 + 2 < L - 1100
    def f(recs):
        add = np.zeros(n // 2 + n % 2, dtype=U.MINMER_DT)
        for i in range(n // 2): add[i] = ((1 << 63) + i, B - 1 - i, rs, seqId, 1, 0)
        if n % 2: add[n // 2] = ((1 << 63) + n, B - 2 - n // 2, B, seqId, 1, 0)
        assert not set(add["hash"].tolist()) & set(recs["hash"].tolist()) and int(add["wpos"].min()) >= rs - L - 1
        return resort(np.concatenate([recs, add]))
    return f


@functools.lru_cache(maxsize=None)
def preload_records(want):
    oracle = U.Oracle()
    c = one_read("preload_records %d" % want, 5000, 130, 0.02, 8401)
    recs, plain = view(oracle, c, None)
    (q, rs, re, _), qs = only_candidate(plain)
    have = slice_model(recs, (q, rs, re), MAXDELTA[11], c["L"], qs)["preload_records"]
    finish(oracle, c, pads(want - have, q, rs, c["L"]), plain)
    assert c["facts"][0]["preload_records"] == want
    return c


CASES = {"skip_jb11_s3": lambda: skip_jb11(3), "skip_jb11_s5": lambda: skip_jb11(5), "skip_jb13": skip_jb13, "tail_and_behind": tail_and_behind,
         "last_of_contig": last_of_contig, "hash_neighbours_s130": lambda: hash_neighbours(5000, 130), "hash_neighbours_s2100": lambda: hash_neighbours(21000, 2100),
         "cell_31": lambda: cell_slide(31), "cell_32": lambda: cell_slide(32), "cell_4095": lambda: cell_slide(4095), "cell_4096": lambda: cell_slide(4096),
         "preload_cell_31": lambda: cell_preload(31), "preload_cell_32": lambda: cell_preload(32),
         "preload_3999": lambda: preload_records(3999), "preload_4000": lambda: preload_records(4000)}
