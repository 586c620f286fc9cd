"""Helpers of tests/test_gpu_paf_rows.py: planted rows for mm_paf_format -- reads of 1, 2 and 16 rows with reads without rows between
them, names of every length around k_paf_write's 4-byte words and 64-lane wave, rows the length filter drops, rows the boundary check
clamps, identities of exactly 0 and 1, a complexity in exponent form, a row that is not formattable -- and what the host writes for
given rows (mmh_paf_text of libmashmap_host.so: MapPost::finishRows + appendReadMappings), with the counts derived from it.

k 16, sketch 80, pi 0.85; seven contigs whose names are 0, 1, 3, 63, 64, 65 and 300 bytes long."""
import numpy as np

K, S, PI = 16, 80, 0.85
NAME_LENGTHS = [0, 1, 3, 63, 64, 65, 300]
CONTIG_LENS = [60000, 40000, 1, 5000, 77777, 1000, 123456]
READ_LEN = 5000
# (legacy, aniPercentage, merge, filterLengthMismatches)
MODES = {"default": (False, False, True, False), "legacy": (True, False, True, False), "ani_percentage": (False, True, True, False),
         "merge_off": (False, False, False, False), "length_filter": (False, False, True, True)}


def name_of(kind, i, n):
    base = ("%s%d_" % (kind, i)).encode()
    return (base * (n // len(base) + 1))[:n]


def contigs():
    return [name_of("c", i, n) for i, n in enumerate(NAME_LENGTHS)], list(CONTIG_LENS)


def len_id_threshold():
    return min(0.7, float(np.float32(PI)) ** 3)                       # std::min(0.7, std::pow(percentageIdentity, 3)) of a float pi


def planted(n_rows, specials=True):
    """(rows CHAIN_ROW_DT, read_lens, read_names, handed: the reads that hold a row which is not formattable).  Reads take 1, 2, 16 rows in
    turn (and one read three), with a read without rows at the front, after every third read and at the end; the last read with rows takes what is left.
    With `specials` (and enough rows) single reads are made the cases of the module docstring."""
    from mashmap_amd import capi
    per_read, left, turn, three = [0], n_rows, 0, None
    while left > 0:
        if specials and turn == 6 and three is None and left >= 3:     # one read of three rows: its middle row is made not formattable
            three = len(per_read)
            per_read.append(3); left -= 3
            continue
        take = min(left, (1, 2, 16)[turn % 3])
        per_read.append(take); left -= take; turn += 1
        if turn % 3 == 0:
            per_read.append(0)
    per_read.append(0)
    rows = np.zeros(n_rows, dtype=capi.CHAIN_ROW_DT)
    i = 0
    for r, n in enumerate(per_read):
        for j in range(n):
            x = rows[i]
            ref = (r + j) % len(CONTIG_LENS)
            span = 1000
            qs = (j * 200) % (READ_LEN - span)
            rs = min(100 * j, max(0, CONTIG_LENS[ref] - span - 1))
            x["querySeqId"], x["queryLen"], x["queryStartPos"], x["queryEndPos"] = r, READ_LEN, qs, qs + span
            x["refSeqId"], x["refStartPos"], x["refEndPos"], x["strand"] = ref, rs, rs + span - 1 + (j % 5), 1 if (i % 3) else -1
            sk = 1 + (i * 7) % S
            x["sketchSize"], x["conservedSketches"] = sk, (i * 5) % (sk + 1)
            x["blockLength"], x["approxMatches"], x["n_merged"], x["splitMappingId"] = span + j, 900, 1 + j, j
            x["nucIdentity"] = np.float32(1.0) - np.float32((i % 23) / 64.0)
            x["kmerComplexity"] = 0.25 + (i % 17) / 8.0
            i += 1
    handed = []
    if specials:
        first = np.concatenate([[0], np.cumsum(per_read)])
        by_rows = {n: [r for r, m in enumerate(per_read) if m == n] for n in (1, 2, 16)}

        def far(x):                                                    # the length filter drops it: the reference span is three times the query's
            x["refEndPos"] = x["refStartPos"] + 3 * (x["queryEndPos"] - x["queryStartPos"])
        if len(by_rows[16]) >= 3:
            a, b, c = by_rows[16][:3]
            far(rows[first[a]])                                        # the first row of a read dropped
            far(rows[first[b] + 15])                                   # the last
            for j in range(16):                                        # every clamp of the boundary check, on both axes
                x = rows[first[c] + j]
                clen = CONTIG_LENS[int(x["refSeqId"])]
                if j == 0: x["queryStartPos"] = -5
                if j == 1: x["queryStartPos"], x["queryEndPos"] = READ_LEN + 3, READ_LEN + 9
                if j == 2: x["queryEndPos"] = x["queryStartPos"] - 7
                if j == 3: x["queryEndPos"] = READ_LEN + 40
                if j == 4: x["refStartPos"] = -9
                if j == 5: x["refStartPos"], x["refEndPos"] = clen + 2, clen + 11
                if j == 6: x["refEndPos"] = x["refStartPos"] - 3
                if j == 7: x["refEndPos"] = clen + 17
                if j == 8: x["nucIdentity"] = 0.0                      # mapQ text -0
                if j == 9: x["nucIdentity"], x["conservedSketches"] = 1.0, x["sketchSize"]          # 255
                if j == 10: x["kmerComplexity"] = 1e-7                 # 1e-07
                if j == 11: x["kmerComplexity"] = 0.0
                if j == 12: x["kmerComplexity"] = 999999.5             # 1e+06
                if j == 13: x["queryEndPos"], x["refEndPos"] = x["queryStartPos"], x["refStartPos"] - 1   # q_l == 0, delta == 0: kept
                if j == 14: x["queryEndPos"] = x["queryStartPos"]      # q_l == 0, delta > 0: dropped
        if len(by_rows[2]) >= 2:
            a = by_rows[2][1]
            far(rows[first[a]]); far(rows[first[a] + 1])               # every row of a read dropped
        if three is not None:
            rows[first[three] + 1]["kmerComplexity"] = 2.0 ** -70         # below the formattable range (legacy output has no such field:
            rows[first[three] + 1]["nucIdentity"] = 1.5                   # there the identity outside [0, 1] is what hands the read over)
            handed.append(three)
    names = [name_of("q", r, NAME_LENGTHS[(r * 3 + 1) % len(NAME_LENGTHS)]) for r in range(len(per_read))]
    return rows, np.full(len(per_read), READ_LEN, dtype=np.int32), names, handed


def host_text(rows, read_lens, read_names, ref_names, ref_lens, mode=(False, False, True, False), first=0, k=K, s=S, pi=PI):
    """mmh_paf_text: (text bytes, off int64[nReads + 1], reported int64[nReads]) -- the host's own lines of the rows, read by read"""
    from mashmap_amd import capi, shard
    lib = shard.host_lib()
    rows = np.ascontiguousarray(rows, dtype=capi.CHAIN_ROW_DT); rl = np.ascontiguousarray(read_lens, dtype=np.int32)
    cl = np.ascontiguousarray(ref_lens, dtype=np.int32)
    qn, qo = capi.pack_names(read_names); rn, ro = capi.pack_names(ref_names)
    off = np.zeros(len(rl) + 1, dtype=np.int64); rep = np.zeros(max(len(rl), 1), dtype=np.int64)
    args = [k, s, pi, int(mode[0]), int(mode[1]), int(mode[2]), int(mode[3]), len(cl), cl.ctypes.data, rn.ctypes.data, ro.ctypes.data,
            rows.ctypes.data if len(rows) else None, len(rows), rl.ctypes.data if len(rl) else None, len(rl), first, qn.ctypes.data, qo.ctypes.data]
    n = lib.mmh_paf_text(*(args + [None, 0, off.ctypes.data, rep.ctypes.data]))
    assert n >= 0, "mmh_paf_text refused the rows"
    text = np.zeros(n + 1, dtype=np.uint8)
    assert lib.mmh_paf_text(*(args + [text.ctypes.data, n, off.ctypes.data, rep.ctypes.data])) == n
    return text[:n].tobytes(), off, rep[:len(rl)]


def expected(rows, read_lens, read_names, ref_names, ref_lens, mode, handed, first=0):
    """what the device must leave: (text, off, handed flags, counts) -- the host's text without the spans of the handed-over reads"""
    text, off, rep = host_text(rows, read_lens, read_names, ref_names, ref_lens, mode, first)
    n = len(read_lens)
    keep = [r for r in range(n) if r not in handed]
    spans = [text[off[r]:off[r + 1]] if r in keep else b"" for r in range(n)]
    eoff = np.concatenate([[0], np.cumsum([len(x) for x in spans])]).astype(np.int64)
    flags = np.zeros(n, dtype=np.uint8)
    flags[list(handed)] = 1
    counts = dict(readsWithText=sum(1 for x in spans if x), lines=int(sum(rep[r] for r in keep)), bytes=int(eoff[-1]),
                  dropped=int(len(rows) - rep.sum()), handedReads=len(handed))
    return b"".join(spans), eoff, flags, counts
