"""mm_paf_rows and the calls around it: declared in the header, exported by the built library, bound in capi with the header's struct
layout; the host entry points beside them exported by libmashmap_host.so.  CPU only."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mm_set_paf_tables", "mm_paf_rows", "mm_paf_format", "mm_paf_counts", "mm_paf_download", "mm_paf_offsets_download", "mm_paf_device"]
C_TYPES = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64}


def test_the_parameter_block_has_the_headers_layout():
    """size and every field's offset of mm_paf_params, from the header's own declaration laid out by ctypes, against capi.PafParams"""
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} mm_paf_params;", hdr)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), C_TYPES[ctype]) for n in names.split(",")]
    assert [n for n, _ in fields] == ["legacy", "aniPercentage", "merge", "filterLengthMismatches", "lenIdThreshold", "sparsityThreshold"]

    class FromHeader(ctypes.Structure):
        _fields_ = fields
    assert ctypes.sizeof(FromHeader) == ctypes.sizeof(capi.PafParams) == 32
    for name, _ in fields:
        assert getattr(FromHeader, name).offset == getattr(capi.PafParams, name).offset, name
        assert getattr(FromHeader, name).size == getattr(capi.PafParams, name).size, name
    assert (capi.PafParams.lenIdThreshold.offset, capi.PafParams.sparsityThreshold.offset) == (16, 24)
    assert "#define MM_PAF_MAPQ_TEXT 8" in hdr and "#define MM_PAF_MAX_MAPQ 128" in hdr
    assert (capi.MM_PAF_MAPQ_TEXT, capi.MM_PAF_MAX_MAPQ) == (8, 128)


def test_the_calls_are_declared_exported_and_bound():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    for decl in ("int mm_paf_rows(mm_ctx* ctx, const char* queryNames, const uint64_t* queryNameOff, size_t nReads);",
                 "int mm_paf_counts(const mm_ctx* ctx, uint64_t* readsWithText, uint64_t* lines, uint64_t* bytes, uint64_t* dropped, uint64_t* handedReads);",
                 "int mm_paf_download(mm_ctx* ctx, char* text, size_t cap, size_t* n);",
                 "int mm_paf_offsets_download(mm_ctx* ctx, int64_t* off, uint8_t* handed);",
                 "int mm_paf_device(const mm_ctx* ctx, const char** dText, size_t* n, const int64_t** dOff);"):
        assert decl in hdr, decl
    assert re.search(r"int mm_set_paf_tables\(mm_ctx\* ctx, const mm_paf_params\* params, const float\* mapqThresholds, const char\* mapqText, size_t nMapq,\s+"
                     r"const char\* refNames, const uint64_t\* refNameOff, const int32_t\* refLens, size_t nContigs\);", hdr)
    assert re.search(r"int mm_paf_format\(mm_ctx\* ctx, const mm_chain_row\* rows, size_t nRows, const int32_t\* readLens, int32_t firstSeqId,\s+"
                     r"const char\* queryNames, const uint64_t\* queryNameOff, size_t nReads\);", hdr)
    assert "#define MM_ABI_VERSION 2" in hdr
    lib = ctypes.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(lib, n), n
        assert getattr(capi.load(), n).restype is ctypes.c_int
    assert capi.load().mm_abi_version() == 2                                                        # additive: the ABI version stays
    assert len(capi.load().mm_set_paf_tables.argtypes) == 9 and len(capi.load().mm_paf_format.argtypes) == 8 and len(capi.load().mm_paf_counts.argtypes) == 6
    for m in ("set_paf_tables", "paf_rows", "paf_format", "paf_counts", "paf_text", "paf_offsets", "paf_device"):
        assert callable(getattr(capi.Context, m)), m


def test_the_host_library_builds_the_mapq_table_and_the_text():
    """mmh_paf_mapq_table: thresholds from 0 to 1, `-0` for an identity of exactly 0 and `255` for exactly 1; mmh_paf_text on two rows"""
    from mashmap_amd import capi, shard
    import pafrows as P
    lib = shard.host_lib()
    assert hasattr(lib, "mmh_paf_mapq_table") and hasattr(lib, "mmh_paf_text") and len(lib.mmh_paf_text.argtypes) == 22
    thr, txt = capi.paf_mapq_table()
    texts = [bytes(txt[i * 8:i * 8 + 8]).rstrip(b"\0") for i in range(len(thr))]
    assert thr[0] == 0 and thr[-1] == 1 and (np.diff(thr) > 0).all() and 60 <= len(thr) <= capi.MM_PAF_MAX_MAPQ
    assert texts[0] == b"-0" and texts[1] == b"0" and texts[2] == b"1" and texts[-1] == b"255" and all(0 < len(t) < 8 for t in texts)
    assert [int(t) for t in texts[1:-1]] == sorted(set(int(t) for t in texts[1:-1]))             # ascending, none twice
    rows, read_lens, names, handed = P.planted(3, specials=False)
    cn, cl = P.contigs()
    text, off, rep = P.host_text(rows, read_lens, names, cn, cl)
    assert rep.tolist() == [0, 1, 2, 0] and off.tolist()[0] == 0 and off[-1] == len(text) and text.count(b"\n") == 3
    assert text.startswith(names[1] + b"\t5000\t0\t1000\t")
    assert capi.pack_names([b"ab", "c", b""])[1].tolist() == [0, 2, 3, 3]
