"""mm_text_*: declared in the header, exported by the built library, bound in capi; the record's size and field offsets, the constants,
and what the addition leaves as it was.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mm_text_reset", "mm_text_append", "mm_text_append_inflated", "mm_text_scan", "mm_text_records", "mm_text_pack", "mm_text_counts", "mm_text_kernel_ms")


def _hdr():
    return open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()


def test_the_record():
    from mashmap_amd import capi
    assert "typedef struct { uint64_t hdrOff; int64_t seqLen; uint32_t nameLen, hasN; } mm_text_record;" in _hdr()
    dt = capi.TEXT_RECORD_DT
    assert dt.itemsize == 24
    assert {n: dt.fields[n][1] for n in dt.names} == {"hdrOff": 0, "seqLen": 8, "nameLen": 16, "hasN": 20}
    assert [dt.fields[n][0].itemsize for n in dt.names] == [8, 8, 4, 4] and dt.fields["seqLen"][0].kind == "i"

    class Record(ctypes.Structure):                      # the C layout of the declaration, laid out by the C rules
        _fields_ = [("hdrOff", ctypes.c_uint64), ("seqLen", ctypes.c_int64), ("nameLen", ctypes.c_uint32), ("hasN", ctypes.c_uint32)]
    assert ctypes.sizeof(Record) == 24 and [getattr(Record, n).offset for n in dt.names] == [dt.fields[n][1] for n in dt.names]


def test_the_constants():
    from mashmap_amd import capi
    hdr = _hdr()
    assert "enum { MM_TEXT_FASTA = 0, MM_TEXT_FASTQ = 1 };" in hdr and (capi.MM_TEXT_FASTA, capi.MM_TEXT_FASTQ) == (0, 1)
    m = re.search(r"^#define MM_TEXT_TILE (\d+)\b", hdr, re.M)
    assert m and int(m.group(1)) == capi.MM_TEXT_TILE == 4096
    core = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_text_core.h")).read()
    assert "enum { MMT_FASTA = 0, MMT_FASTQ = 1 };" in core and "mashmap_hip.h\"" not in core


def test_the_exported_symbols():
    from mashmap_amd import capi
    hdr = _hdr()
    for decl in ("int mm_text_reset(mm_ctx* ctx);",
                 "int mm_text_append(mm_ctx* ctx, const void* bytes, size_t n, int onDevice);",
                 "int mm_text_append_inflated(mm_ctx* ctx, const void* comp, size_t nComp, mm_inflate_block* blocks, size_t nBlocks, size_t* nBad);",
                 "int mm_text_scan(mm_ctx* ctx, int format, int final, size_t* nRecords, size_t* nNameBytes, size_t* consumed);",
                 "int mm_text_records(mm_ctx* ctx, mm_text_record* recs, char* names);",
                 "int mm_text_counts(const mm_ctx* ctx, uint64_t* scans, uint64_t* records, uint64_t* bytes);",
                 "int mm_text_kernel_ms(const mm_ctx* ctx, double* scanMs, double* packMs);"):
        assert decl in hdr, decl
    assert re.search(r"int mm_text_pack\(mm_ctx\* ctx, const uint8_t\* keep, uint32_t\* bases2, uint32_t\* nmask, size_t capPackedBases,\s+"
                     r"size_t reservePackedBases, size_t\* nPackedBases, int\* staged\);", hdr)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name), name
    for name in capi.EXPORTS:
        assert hasattr(lib, name), name
    bound = capi.load()
    assert [len(getattr(bound, n).argtypes) for n in NAMES] == [1, 4, 6, 6, 3, 8, 4, 3]
    assert all(getattr(bound, n).restype is ctypes.c_int for n in NAMES)
    for m in ("text_reset", "text_append", "text_append_inflated", "text_scan", "text_records", "text_pack", "text_counts", "text_kernel_ms"):
        assert callable(getattr(capi.Context, m)), m


def test_what_stays_as_it_was():
    from mashmap_amd import capi
    hdr = _hdr()
    assert "#define MM_ABI_VERSION 2" in hdr and capi.load().mm_abi_version() == 2
    assert "MM_K_SELECT, MM_K_COUNT };" in hdr and len(capi.KERNELS) == 11
    assert "MM_OPT_CHAIN_MODES = 10 };" in hdr
    assert "int mm_inflate_kernel_ms(const mm_ctx* ctx, double* ms);" in hdr and "size_t mm_device_bytes(void);" in hdr
    mk = open(os.path.join(ROOT, "mashmap_amd", "csrc", "Makefile")).read()
    assert "mm_text.hip" in mk and "mm_text_core.h" in mk
