"""Fuzzed interval-point lists for the CPU checks of L1 (test_l1_point_filter.py, test_l1_literal_core.py) and the oracle's literal
computeL1CandidateRegions over them -- test infrastructure.  The scenario kinds: clusters that reach minimumHits (dense), few scattered hits
(sparse), long merged intervals (long), contigs whose last and first points share a position (seam, seam2: the reference groups by `pos` alone)."""
import ctypes as C

import numpy as np

import mmutil as U

L1_DT = np.dtype([("seqId", "<i4"), ("rangeStartPos", "<i4"), ("rangeEndPos", "<i4"), ("intersectionSize", "<i4")])


def points(seq, o, c, hashes=None):
    """the intervals' OPEN / CLOSE points in the reference's order (seqId, pos, CLOSE first); hashes: one per interval (hash_to_freq's key)"""
    pts = np.zeros(2 * len(seq), dtype=U.POINT_DT)
    if hashes is not None:
        pts["hash"][0::2] = hashes; pts["hash"][1::2] = hashes
    pts["seqId"][0::2] = seq; pts["pos"][0::2] = o; pts["side"][0::2] = 1
    pts["seqId"][1::2] = seq; pts["pos"][1::2] = c; pts["side"][1::2] = -1
    order = np.lexsort((pts["side"], pts["pos"], pts["seqId"]))
    return np.ascontiguousarray(pts[order])


def l1_of_points(orc, h, pts, qs, min_hits, frag_len=5000):
    """the oracle's computeL1CandidateRegions over a sorted point list; windowLen = max(0, frag_len - the session's segLength)"""
    out = np.zeros(4096, dtype=L1_DT)
    fn = orc.lib.orc_session_l1_from_points
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    n = fn(h, pts.ctypes.data, len(pts), qs, frag_len, min_hits, out.ctypes.data, len(out))
    assert 0 <= n <= len(out)
    return out[:n].tobytes(), n


def l1(orc, h, seq, o, c, qs, min_hits):
    return l1_of_points(orc, h, points(seq, o, c), qs, min_hits)


KINDS = ("dense", "sparse", "long", "seam", "seam2")


def scenario(rng, kind):
    ncontig = int(rng.integers(1, 6))
    clen = int(rng.choice([9000, 40000, 400000]))
    seq, o, c = [], [], []

    def add(q, a, ln):
        seq.append(q); o.append(int(a)); c.append(int(a + ln))
    for _ in range(int(rng.integers(0, 5))):                       # loci where many intervals overlap
        q = int(rng.integers(0, ncontig)); at = int(rng.integers(0, clen))
        for _ in range(int(rng.integers(2, 40))):
            add(q, at + int(rng.integers(-3000, 3000)) if at > 3000 else at + int(rng.integers(0, 3000)), int(rng.integers(1, 5000)))
    for _ in range(int(rng.integers(0, 300 if kind != "sparse" else 30))):   # scattered single hits
        add(int(rng.integers(0, ncontig)), int(rng.integers(0, clen)), int(rng.integers(1, 5000)))
    if kind == "long":                                             # merged windows of one hash: several segment lengths
        for _ in range(int(rng.integers(1, 4))):
            add(int(rng.integers(0, ncontig)), int(rng.integers(0, clen)), int(rng.integers(5000, 60000)))
    if kind == "seam":                                             # last point of a contig at the position of the next one's first
        p = int(rng.integers(100, 5000))
        for q in range(ncontig):
            add(q, p, int(rng.integers(1, 3000)))                  # many contigs open at p ...
            add(q, max(0, p - int(rng.integers(1, 3000))), 0 + int(rng.integers(1, 50)))
        m = max(c) + int(rng.integers(0, 3))
        for q in range(ncontig):
            add(q, m - int(rng.integers(1, 2000)), 0)              # ... and close at one position m (length fixed below)
            c[-1] = m
            for _ in range(int(rng.integers(0, 4))):
                add(q, p, int(rng.integers(1, 4000)))
    if kind == "seam2":
        # the case the boundary rule exists for: contig A's last point is the CLOSE of a lone interval at p, contig A + 1's first points are
        # a cluster opening at p -- the reference's sweep groups them together and reports the candidate under contig A; a filter that
        # drops the lone interval (it reaches no count) would move it to contig A + 1
        seq, o, c = [], [], []
        p = int(rng.integers(200, 9000)); A = int(rng.integers(0, 3)); k = int(rng.integers(2, 10))
        for _ in range(int(rng.integers(0, 10))):
            a = int(rng.integers(0, max(1, p - 150))); add(A, a, 1); c[-1] = min(p - 1, a + int(rng.integers(1, 120)))
        add(A, p - int(rng.integers(1, 150)), 1); c[-1] = p
        for _ in range(k):
            add(A + 1, p, int(rng.integers(50, 4000)))
        for _ in range(int(rng.integers(0, 20))):
            add(A + 1, p + int(rng.integers(1, 20000)), int(rng.integers(1, 4000)))
    seq = np.array(seq, dtype=np.int64); o = np.maximum(0, np.array(o, dtype=np.int64)); c = np.array(c, dtype=np.int64)
    c = np.maximum(c, o + 1)
    return seq, o, c
