"""Shared by tests/test_text_core.py and tests/test_gpu_text.py: builds tests/hostlogic/text_check.cpp (a stand-alone program; with
-fsanitize=address,undefined for the CPU suite, plain for a module marked gpu), a Python restatement of the record rules of
mashmap_amd/csrc/mm_text_core.h (the reference of the GPU tests), and the edge texts at a tile size T."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTA, FASTQ = 0, 1


def build_check(tmpdir, sanitize=True):
    exe = os.path.join(str(tmpdir), "text_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "hostlogic", "text_check.cpp"), "-lz", "-lpthread"])
    return exe


def lines_of(text):
    """[(offset, line without its '\\n', terminated)]: lines end at '\\n', the last one may be unterminated"""
    out, pos, n = [], 0, len(text)
    while pos < n:
        nl = text.find(b"\n", pos)
        end = n if nl < 0 else nl
        out.append((pos, text[pos:end], nl >= 0))
        pos = end + 1
    return out


def name_of(header):
    """the header line without its first byte, cut at the first ' ' only"""
    return header[1:].split(b" ", 1)[0]


def parse(text, fmt, final):
    """([(hdrOff, name, sequence bytes)], consumed) by the rules"""
    lines = lines_of(text)
    recs = []
    if fmt == FASTA:
        for i, (off, ln, _) in enumerate(lines):
            if i == 0 or ln[:1] == b">":
                recs.append([off, name_of(ln), bytearray()])
            else:
                recs[-1][2] += ln
        if final:
            return [(o, n, bytes(s)) for o, n, s in recs], len(text)
        consumed = recs[-1][0] if recs else 0
        return [(o, n, bytes(s)) for o, n, s in recs[:-1]], consumed
    complete = sum(1 for _, _, t in lines if t) // 4
    groups = (len(lines) + 3) // 4 if final else complete
    for g in range(groups):
        off, hdr, _ = lines[4 * g]
        seq = lines[4 * g + 1][1] if 4 * g + 1 < len(lines) else b""
        recs.append((off, name_of(hdr), bytes(seq)))
    if final:
        return recs, len(text)
    consumed = lines[4 * complete - 1][0] + len(lines[4 * complete - 1][1]) + 1 if complete else 0
    return recs, consumed


def has_n(seq):
    return int(any(ch not in b"ACGTacgt" for ch in seq))


def bases(rng, n, alpha=b"ACGT"):
    return np.frombuffer(alpha, dtype=np.uint8)[rng.randint(0, len(alpha), size=max(0, n))].tobytes()


def fa(name, seq, width=0):
    if not width:
        return b">" + name + b"\n" + seq + b"\n"
    return b">" + name + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def fq(name, seq, qual=None):
    return b"@" + name + b"\n" + seq + b"\n+\n" + (qual if qual is not None else b"I" * len(seq)) + b"\n"


def edge_texts(T, seed=3):
    """[(name, format, text)]: the cases at exact multiples of the tile T and one byte either side"""
    rng = np.random.RandomState(seed)
    B = lambda n, a=b"ACGT": bases(rng, n, a)
    out = []
    for d in (-1, 0, 1):
        tag = "%+d" % d
        head = fa(b"a", B(T - 4 + d))                                 # its '\n' is byte T - 1 + d
        out.append(("newline_ends_a_tile_gt_starts_the_next" + tag, FASTA, head + fa(b"b", B(9))))
        head = fa(b"a", B(T - 5 + d))                                 # the next line's first byte is byte T - 1 + d
        out.append(("gt_ends_a_tile" + tag, FASTA, head + fa(b"", B(5)) + fa(b"c", B(3))))
        out.append(("header_crosses_a_boundary" + tag, FASTA, fa(b"r1", B(T - 20 + d)) + fa(b"name_that_crosses_the_tile_boundary extra", B(40))))
        out.append(("header_crosses_a_boundary_fq" + tag, FASTQ, fq(b"r1", B((T - 30 + d) // 2)) + fq(b"name_that_crosses_the_tile_boundary extra", B(40))))
        out.append(("long_header_space_in_tile_2" + tag, FASTA, fa(b"h" * (T + 10 + d) + b" " + b"k" * (T + 9), B(33)) + fa(b"z", B(3))))
        out.append(("long_header_no_space" + tag, FASTA, fa(b"h" * (2 * T + 9 + d), B(33)) + fa(b"z", B(3))))
        out.append(("long_header_no_space_fq" + tag, FASTQ, fq(b"h" * (2 * T + 9 + d), B(33)) + fq(b"z", B(3))))
        out.append(("long_line_no_newline" + tag, FASTA, b">long\n" + B(3 * T + 5 + d)))
        out.append(("long_line" + tag, FASTA, fa(b"x", B(3 * T + 5 + d)) + fa(b"y", B(2))))
        out.append(("long_line_fq" + tag, FASTQ, fq(b"x", B(3 * T + 5 + d)) + fq(b"y", B(2))))
        out.append(("length_16T" + tag, FASTA, fa(b"w", B(16 * T + d), 60) + fa(b"v", B(7))))
        out.append(("length_16T_fq" + tag, FASTQ, fq(b"w", B(16 * T + d), B(16 * T + d, b"@+>I"))))
        out.append(("exact_multiple" + tag, FASTA, (fa(b"e", B(50), 60) * (3 * T // 54 + 2))[:3 * T + d]))
    out.append(("one_line_pair", FASTA, fa(b"only", B(100))))
    out.append(("one_line_pair_fq", FASTQ, fq(b"only", B(100))))
    out.append(("forty_tiny_records", FASTA, b"".join(fa(b"r%d" % i, B(i % 4)) for i in range(40))))
    out.append(("forty_tiny_records_fq", FASTQ, b"".join(fq(b"r%d" % i, B(i % 4)) for i in range(40))))
    out.append(("consecutive_headers", FASTA, b">a\n>b\n>c\nAC\n>d\n>e\n"))
    out.append(("empty_lines", FASTA, b">a\n\nAC\n\n\nGT\n\n>b\n\n\n>\n\nA\n"))
    out.append(("crlf", FASTA, b">a x\r\nACGT\r\nAC\r\n>b\r\nGG\r\n"))
    out.append(("crlf_fq", FASTQ, b"@a x\r\nACGT\r\n+\r\nIIII\r\n@b\r\nGG\r\n+\r\nII\r\n"))
    out.append(("marks_in_mid_line", FASTA, b">a>b @c\td e\nAC>GT@A\n>b\nA>\n"))
    out.append(("marks_in_mid_line_fq", FASTQ, b"@a>b @c\nAC>GT@A\n+\n@@@@@@@\n@b@\nA@\n+\nI>\n"))
    out.append(("lower_case_and_iupac", FASTA, fa(b"iupac", b"acgtnRYKMSWBDHVNacguACGT" * 5, 17)))
    for L in (31, 32, 33, 63, 64, 65):
        out.append(("length_%d" % L, FASTA, fa(b"l", B(L, b"ACGTNacgt")) + fa(b"m", B(L), 7) + fa(b"n", B(L))))
        out.append(("length_%d_fq" % L, FASTQ, fq(b"l", B(L, b"ACGTNacgt")) + fq(b"m", B(L))))
    out.append(("no_final_newline", FASTA, b">nolf\nACGT\n>x\nACGTA"))
    out.append(("line_0_is_a_header", FASTA, b"ACGT\nAC\n>x\tY z\nGG\n"))
    out.append(("quality_lines_with_marks_fq", FASTQ, b"@q\nACGT\n+\n@III\n@r\nAC\n+\n+I\n@s\nGG\n+\n>I\n"))
    for k, tail in enumerate((b"@r", b"@r\nAC", b"@r\nAC\n+", b"@r\nAC\n+\n")):
        out.append(("final_group_%d_fq" % k, FASTQ, b"@q\nACGT\n+\nIIII\n" + tail))
    return out
