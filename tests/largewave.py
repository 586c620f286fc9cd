"""Helpers of tests/test_gpu_large_wave.py: the oracle per fragment with buffers large enough for long segments, the figures of a
candidate's slice of the index as k_l2_extents cuts it, one mapping run of a batch on a fresh context with a value of
MM_OPT_L2_LARGE_WAVE, and the "loci8" batch that outgrows the locus buffer behind either wave kernel (tests/test_gpu_window_wave.py
uses it too)."""
import ctypes as C

import numpy as np

import mmutil as U

LOCAP0 = 8                             # mm_l2.hip: MM_LOCAP0
LW_MAX_SKETCH = 20460                  # mm_l2.hip: MM_LW_MAX_SKETCH


def fragments_of(read_len, L):
    """Map::mapModule's cut (computeMap.hpp:587-671): full segments + one overlapping tail"""
    if read_len <= L:
        return [(0, read_len)]
    fr = [(i * L, L) for i in range(read_len // L)]
    if read_len % L:
        fr.append((read_len - L, L))
    return fr


arrayed = U.arrayed                    # a tandem array of the unit between random flanks of 3 kbp; div 0: exact copies, which tie in L2


# ---- the locus buffer behind a wave kernel: tests/test_gpu_map.py's eight-copy "loci8" index (k 16, segLength 1 000, pi 0.95) at its s = 32
LOCI8_K, LOCI8_L, LOCI8_PI = 16, 1000, 0.95


def loci8_reads(n):
    return U.unit_reads(U.random_dna(9052, 1300), 9056, n, rl=LOCI8_L)


def loci8_pass(reads, flags, set_option, s=32):
    """the batch on a fresh context with the kernel timers on, the option set by set_option(ctx), mapped TWICE: everything the first pass
    leaves, (L1, L2) counts, loci per candidate, the context's two (candidates, literal) queries -- and `l2_brackets`, the MM_K_L2 timer
    brackets of the first and of the second pass.  mm_launch_l2_window closes one bracket per kernel launch of an attempt and keeps the
    grown l2Cap in the context, so the first pass has more of them than the second exactly when it had to repeat an attempt"""
    import gpucheck
    from mashmap_amd import capi
    ua, ub = U.random_dna(9051, 1100), U.random_dna(9052, 1300)
    ctx = capi.Context(k=LOCI8_K, segLength=LOCI8_L, sketchSize=s, flags=capi.MM_FLAG_HG_FILTER | flags)
    ctx.index_build([U.random_dna(9001, 500000)[:200000], arrayed(9053, ua, 6, 0.03), arrayed(9054, ub, 8, 0)], kmerPct=0.0); ctx.set_tables_default(LOCI8_PI)
    set_option(ctx)
    ctx.reads_upload(reads); ctx.synchronize(); ctx.profile(True); ctx.profile_read(True)
    ctx.map(); ctx.synchronize()
    first = ctx.profile_read(True)["l2"][1]
    l2 = ctx.results()[2]
    out = dict(bytes=gpucheck.pass_bytes(ctx), counts=ctx.result_counts(), per=np.bincount(l2["cand"]) if len(l2) else np.zeros(1, dtype=np.int64),
               large=ctx.pass_l2_large(), window=ctx.pass_l2_window())
    ctx.map(); ctx.synchronize()
    out["l2_brackets"] = (first, ctx.profile_read(True)["l2"][1])
    assert ctx.result_counts() == out["counts"]
    ctx.close()
    return out


def map_fragment(orc, h, seq, seqCounter, name, fullLen, s, npts=1 << 19):
    """mmutil.Oracle.map_fragment with room for `npts` interval points (a tandem array at a long segment has some 200 000)"""
    b = bytes(seq)
    qsk = (U.Minmer * (s + 1))(); pts = (U.Point * npts)(); l1 = (U.L1 * 1024)(); l2 = (U.L2 * 4096)()
    l2c = (C.c_int * 4096)(); maps = (U.Mapping * 1024)(); counts = (C.c_int64 * 8)(); kc = C.c_double(0)
    orc.f("session_map_fragment")(h, b, len(b), fullLen, seqCounter, name, qsk, s + 1, pts, npts, l1, 1024, l2, l2c, 4096, maps, 1024, counts, C.byref(kc))
    c = list(counts)
    assert c[1] <= npts and c[2] <= 1024 and c[3] <= 4096 and c[4] <= 1024
    loci = [[] for _ in range(c[2])]
    for i in range(c[3]): loci[l2c[i]].append(l2[i].key())
    return dict(sketch=[qsk[i].key() for i in range(c[0])], nPoints=c[1], l1=[l1[i].key() for i in range(c[2])], l2=loci, sketchSize=c[6])


def slice_figures(by_contig, cand, L, qhashes=None):
    """a candidate's slice of the index, as k_l2_extents cuts it out of the contig's stream of insert and eviction events:
    before = index records in front of rangeStart from the target rangeStart - segLength - 1 on (the pre-load is taken from them),
    slide = events from the insert at rangeStart to the last insert at or before rangeEnd (inserts, and the evictions between them),
    last_is_contig_last = that insert is the contig's last record; doubly_open (qhashes given) = two overlapping windows of one hash
    of the query sketch among the records the candidate takes"""
    seq, rs, re_ = cand[0], cand[1], cand[2]
    r = by_contig[seq]
    wpos, wend = r["wpos"], r["wpos_end"]
    ins = (wpos >= rs) & (wpos <= re_)
    fig = dict(before=int(((wpos >= rs - L - 1) & (wpos < rs)).sum()), slide=0, last_is_contig_last=False, doubly_open=False)
    if ins.any():
        last = int(wpos[ins].max())
        fig["slide"] = int(ins.sum()) + int(((wend > rs) & (wend <= last)).sum())
        fig["last_is_contig_last"] = last == int(wpos.max())
    if qhashes is not None:
        t = r[(wpos >= rs - L - 1) & (wpos <= re_) & np.isin(r["hash"], np.array(sorted(qhashes), dtype=np.uint64))]
        t = t[np.lexsort((t["wpos"], t["hash"]))]
        same = t["hash"][1:] == t["hash"][:-1]
        fig["doubly_open"] = bool((same & (t["wpos_end"][:-1] > t["wpos"][1:])).any())
    return fig


def oracle_batch(orc, contigs, reads, k, L, s, pi, flags=0, mutate_index=None, figures=True, with_sketch_hashes=False):
    """the batch on the CPU: per fragment (in the order Map::mapModule cuts them) the oracle's L1, its loci per candidate and the slice
    figures per candidate; the oracle's session stays open (the caller frees it)"""
    h = orc.session(contigs, k, L, s, pi, U.FILTER_MAP, flags, b"\0", 0.0, mutate_index=mutate_index)
    by_contig = None
    if figures:
        idx = orc.index_array(h)
        by_contig = [idx[idx["seqId"] == i] for i in range(len(contigs))]
    per = []
    for ri, (name, a) in enumerate(reads):
        if len(a) < k: continue                          # computeMap.hpp:325: shorter reads are skipped
        for off, ln in fragments_of(len(a), L):
            e = map_fragment(orc, h, a[off:off + ln], ri, name.encode(), len(a), s)
            qh = {x[0] for x in e["sketch"]} if with_sketch_hashes else None
            per.append(dict(read=ri, off=off, len=ln, l1=e["l1"], l2=e["l2"], sketchSize=e["sketchSize"],
                            fig=[slice_figures(by_contig, c, L, qh) for c in e["l1"]] if figures else None))
    return h, per


_REPLAY = {}


def replay_tables(s, k, pi):
    """mm_stat_replay_tables, computed once per (s, k, pi) and shared, unchanged ((s + 1)^2 entries: 200 MB at s = 8 200)"""
    from mashmap_amd import capi
    if (s, k, pi) not in _REPLAY:
        _REPLAY.clear()
        _REPLAY[(s, k, pi)] = capi.stat_replay_tables(s, k, pi, 0.0, True)
    return _REPLAY[(s, k, pi)]


def run(orc, h, reads, k, L, s, pi, flags, value, min_hits=None, replay=True):
    """one map() of the batch on a fresh context with MM_OPT_L2_LARGE_WAVE = value, on the oracle session's index: pass_l2_large(), what
    the pass leaves as bytes, and L1 / L2 per fragment"""
    from mashmap_amd import capi
    ix = orc.export_index(h)
    ctx = capi.Context(k=k, segLength=L, sketchSize=s, flags=capi.MM_FLAG_HG_FILTER if flags & U.FLAG_HG else 0)
    if value: ctx.l2_large_wave(value)
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"])
    ctx.set_tables(min_hits if min_hits is not None else orc.min_hits_table(s, k, pi), orc.cutoffs(h))
    if replay: ctx.set_replay_tables(*replay_tables(s, k, pi))
    ctx.reads_upload([a for _, a in reads], None, [-1] * len(reads), 0)
    ctx.map()
    large = ctx.pass_l2_large()
    stats, l1, l2 = ctx.results()
    frs = [(int(f["readId"]), int(f["fragStart"]), int(f["len"])) for f in ctx.fragments()]
    l2_by_c = {}
    for x in l2:
        l2_by_c.setdefault(int(x["cand"]), []).append((int(x["seqId"]), int(x["meanOptimalPos"]), int(x["optimalStart"]), int(x["optimalEnd"]),
                                                                        int(x["sharedSketchSize"]), int(x["strand"])))
    per = [dict(l1=[], l2=[]) for _ in range(len(stats))]
    for gi, c in enumerate(l1):                          # (a downloaded locus names its candidate by the candidate's index in l1)
        f = per[int(c["frag"])]
        f["l2"].append(l2_by_c.get(gi, []))
        f["l1"].append((int(c["seqId"]), int(c["rangeStartPos"]), int(c["rangeEndPos"]), int(c["intersectionSize"])))
    out = dict(large=large, stats=stats.tobytes(), l1=l1.tobytes(), l2=l2.tobytes(), mappings=ctx.mappings().tobytes() if replay else b"", frags=frs, per=per,
               pass_stats=ctx.pass_stats())
    ctx.close()
    return out


def check_values(orc, h, reads, per, k, L, s, pi, flags, expect, min_hits=None, replay=True, empty_ok=False):
    """maps the batch on a fresh context per value of `expect` = {value: (candidates, literal)}: pass_l2_large() as expected, stats, L1, L2
    and candidate mappings byte-identical between the contexts, L1 and L2 equal to the oracle's per fragment and candidate"""
    outs = {v: run(orc, h, reads, k, L, s, pi, flags, v, min_hits, replay) for v in expect}
    print({v: o["large"] for v, o in outs.items()}, "expected", expect)
    for v, o in outs.items():
        assert o["large"] == expect[v], "pass_l2_large() at value %d: %r, expected %r" % (v, o["large"], expect[v])
        assert o["pass_stats"][1] is False
    first = outs[next(iter(expect))]
    for v, o in outs.items():
        for what in ("stats", "l1", "l2", "mappings"):
            assert empty_ok or what == "mappings" or len(o[what]) > 0, what
            assert o[what] == first[what], "value %d disagrees on %s" % (v, what)
    assert first["frags"] == [(p["read"], p["off"], p["len"]) for p in per]
    for f, (g, p) in enumerate(zip(first["per"], per)):
        assert g["l1"] == p["l1"], ("fragment %d" % f, g["l1"][:4], p["l1"][:4])
        assert g["l2"] == p["l2"], ("fragment %d" % f, [x[:3] for x in g["l2"]][:3], [x[:3] for x in p["l2"]][:3])
    return outs
