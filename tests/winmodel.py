"""What the windowLen != 0 L2 tests share (test_l2_window_core.py on the CPU, test_gpu_window_wave.py on the GPU): the tandem-repeat cases,
the oracle's view of a read, and a Python model of computeL2MappedRegions' window bookkeeping (computeMap.hpp:1323-1371) over
orc.index_array -- which records the gate lets in, by the reference's counter + heap (gate_literal) and by the presence rule of
mm_l2_window_core.h (gate_expiry) --, with the figures the cases assert: records walked / entering / skipped / re-entered after an expiry,
the largest heap, and where a record's insert event lies on k_l2_window_wave's grid of 64 events per step."""
import heapq

import numpy as np

import mmutil as U

K, L, S, PI = 16, 1000, 80, 0.85
WW_HEAP = 2048                                                   # mm_l2.hip: MM_WW_HEAP
LOCAP0 = 8                                                       # mm_l2.hip: MM_LOCAP0 (k_l2_window_wave holds LOCAP0 closed loci and the pending one)
# seed -> (period, copies, err, read length): a 90 kbp contig random_dna(4101 + seed) with a unit random_dna(4100 + seed, period) planted
# `copies` times in tandem from position 5000, copy j = mutate(unit, 50 + j, err) cut to the period; the read is the contig's [5100, 5100 + len)
TANDEM = {1: (1800, 14, 0.0, 3000), 2: (700, 30, 0.01, 2500), 3: (300, 60, 0.02, 1400), 4: (1800, 6, 0.03, 21000), 5: (150, 100, 0.0, 5000)}


def planted_contig(contig_seed, unit_seed, period, copies, err):
    c = U.random_dna(contig_seed, 90000)
    unit = U.random_dna(unit_seed, period)
    for j in range(copies):
        m = U.mutate(unit, 50 + j, err)[:period]
        c[5000 + j * period:5000 + j * period + len(m)] = m
    return c


def tandem_contig(seed):
    period, copies, err, _ = TANDEM[seed]
    return planted_contig(4101 + seed, 4100 + seed, period, copies, err)


def tandem_read(seed, contig, length=None):
    return contig[5100:5100 + (length or TANDEM[seed][3])].copy()


def mixed_strand_read(seed, contig, piece=410):
    """the seed's read cut into pieces of `piece` bases, every second one reverse-complemented: the strand votes change sign along the
    candidate, so a locus's strand depends on WHEN the votes are sampled (computeMap.hpp:1342: before the record's own evictions, behind
    those of the slide records before it)"""
    r = tandem_read(seed, contig)
    parts = [r[i:i + piece] for i in range(0, len(r), piece)]
    return np.concatenate([U.revcomp(x) if j % 2 else x for j, x in enumerate(parts)])


def session(orc, contigs, hg):
    return orc.session(contigs, K, L, S, PI, U.FILTER_MAP, U.FLAG_NOSPLIT | (U.FLAG_HG if hg else 0), b"\0", 0.0)


def first_record(idx, seq, wpos):
    """std::lower_bound(minmerIndex, (seqId, wpos)) (computeMap.hpp:1290-1293)"""
    key = (idx["seqId"].astype(np.int64) << 32) | idx["wpos"].astype(np.int64)
    return int(np.searchsorted(key, (int(seq) << 32) | max(int(wpos), 0), "left"))      # (every wpos is >= 0)


def event_index(idx, seq):
    """{record -> index of its insert event in the contig's event stream} (mm_index_dev.hip: key = pos * 2 + isInsert, inserts of one
    wpos in index order), and the sorted keys"""
    r = np.nonzero(idx["seqId"] == seq)[0]
    ins = idx["wpos"][r].astype(np.int64) * 2 + 1
    keys = np.sort(np.concatenate([ins, idx["wpos_end"][r].astype(np.int64) * 2]), kind="stable")
    at = np.searchsorted(keys, ins, "left")
    rank = np.zeros(len(r), dtype=np.int64)
    for i in range(1, len(r)):
        if ins[i] == ins[i - 1]: rank[i] = rank[i - 1] + 1
    return dict(zip(r.tolist(), (at + rank).tolist())), keys


def walked(idx, cand, W):
    """the records the two loops look at, as (record, in the set-up loop): wpos from rangeStart - segLength - 1; before rangeStart only those
    still open there (:1323-1338), then up to rangeEnd + windowLen (:1340)"""
    seq, rs, re_ = cand[:3]
    i, n, out = first_record(idx, seq, rs - L - 1), len(idx), []
    while i < n and idx["seqId"][i] == seq and idx["wpos"][i] < rs:
        if idx["wpos_end"][i] > rs: out.append((i, True))
        i += 1
    while i < n and idx["seqId"][i] == seq and idx["wpos"][i] <= re_ + W:
        out.append((i, False)); i += 1
    return out


def gate_literal(idx, recs, W):
    """hash_to_freq and the heap of open records, as the reference keeps them: per walked record whether it enters; the largest heap"""
    freq, heap, out, largest = {}, [], [], 0
    for n_, (i, setup) in enumerate(recs):
        h, wpos, wend = int(idx["hash"][i]), int(idx["wpos"][i]), int(idx["wpos_end"][i])
        if not setup:
            while heap and heap[0][0] <= wpos - W:
                fh = heap[0][2]
                if W > 0: freq[fh] -= 1
                if W == 0 or freq[fh] == 0: heapq.heappop(heap)
        if W > 0: freq[h] = freq.get(h, 0) + 1
        enters = W == 0 or freq[h] == 1
        if enters:
            heapq.heappush(heap, (wend, n_, h)); largest = max(largest, len(heap))
        out.append(enters)
    return out, largest


def gate_expiry(idx, recs, W):
    """the presence rule: a hash is absent, or present with the record that is in (its wpos_end); per walked record whether it enters, and
    whether it re-enters after an expiry"""
    entry, out, again = {}, [], []
    for i, setup in recs:
        h, wpos, wend = int(idx["hash"][i]), int(idx["wpos"][i]), int(idx["wpos_end"][i])
        present = W > 0 and h in entry and (setup or entry[h] > wpos - W)
        again.append(W > 0 and not present and h in entry)
        if not present: entry[h] = wend
        out.append(not present)
    return out, again


def figures(idx, cand, W):
    """everything a case asserts about one candidate, with both gates held against each other"""
    recs = walked(idx, cand, W)
    lit, largest = gate_literal(idx, recs, W)
    exp, again = gate_expiry(idx, recs, W)
    assert lit == exp, "the literal gate and the expiry gate disagree on candidate %r" % (cand,)
    ev, keys = event_index(idx, cand[0])
    e0 = int(np.searchsorted(keys, max(cand[1] - L - 1, 0) * 2, "left"))
    step = [(ev[i] - e0) // 64 for i, _ in recs]                 # the step of 64 events a record's insert falls into
    assert all(s >= 0 for s in step)
    first_slide = next((ev[i] - e0 for i, setup in recs if not setup), None)
    same_step = False
    seen = {}
    for (i, _), st in zip(recs, step):
        key = (int(idx["hash"][i]), st)
        same_step |= key in seen; seen[key] = True
    # entering slide records behind a skipped slide record (whose evictions they make first), and those of them whose skipped
    # predecessor lies in an earlier step of 64 events (its wpos reaches the entering record through the kernel's carry)
    behind_skipped = behind_skipped_earlier_step = 0
    for n_ in range(1, len(recs)):
        if lit[n_] and not recs[n_][1] and not recs[n_ - 1][1] and not lit[n_ - 1]:
            behind_skipped += 1; behind_skipped_earlier_step += step[n_ - 1] < step[n_]
    return dict(walked=len(recs), entering=sum(lit), skipped=len(lit) - sum(lit), reentered=sum(again), largest_heap=largest,
                behind_skipped=behind_skipped, behind_skipped_earlier_step=behind_skipped_earlier_step,
                setup=sum(1 for _, s_ in recs if s_), first_slide_event=first_slide, steps=(max(step) + 1) if step else 0, same_hash_in_a_step=same_step)


def oracle_read(orc, h, read):
    """the oracle on the whole read as one fragment: its result, and the loci per L1 candidate"""
    e = orc.map_fragment(h, read, 0, b"q", len(read), S)
    per = [[] for _ in e["l1"]]
    for x in e["l2"]:
        per[x[0]].append(x[1:])
    return e, per


def takes_literal(fig, n_loci):
    """k_l2_window_wave's hand-over rule: a heap beyond MM_WW_HEAP, or more tied loci than MM_LOCAP0 closed ones and the pending one (the
    oracle's count of the candidate's loci: the best count's, which is where the kernel's list ends)"""
    return fig["largest_heap"] > WW_HEAP or n_loci > LOCAP0 + 1
