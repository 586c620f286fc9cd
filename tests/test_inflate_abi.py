"""mm_inflate_blocks / mm_inflate_counts / mm_inflate_kernel_ms: declared in the header, exported by the built library, bound in capi; the
descriptor's size and field offsets, the constants, and what the addition leaves as it was.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hdr():
    return open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()


def test_the_descriptor():
    from mashmap_amd import capi
    hdr = _hdr()
    assert "typedef struct { uint64_t cOff; uint32_t cLen, uLen; uint64_t uOff; uint32_t crc32, status; } mm_inflate_block;" in hdr
    dt = capi.INFLATE_BLOCK_DT
    assert dt.itemsize == 32
    assert {n: dt.fields[n][1] for n in dt.names} == {"cOff": 0, "cLen": 8, "uLen": 12, "uOff": 16, "crc32": 24, "status": 28}
    assert [dt.fields[n][0].itemsize for n in dt.names] == [8, 4, 4, 8, 4, 4]

    class Block(ctypes.Structure):                       # the C layout of the declaration, laid out by the C rules
        _fields_ = [("cOff", ctypes.c_uint64), ("cLen", ctypes.c_uint32), ("uLen", ctypes.c_uint32), ("uOff", ctypes.c_uint64),
                    ("crc32", ctypes.c_uint32), ("status", ctypes.c_uint32)]
    assert ctypes.sizeof(Block) == 32 and [getattr(Block, n).offset for n in dt.names] == [dt.fields[n][1] for n in dt.names]


def test_the_constants():
    from mashmap_amd import capi
    hdr = _hdr()
    assert re.search(r"^#define MM_INFLATE_MAX_BLOCK 65536\b", hdr, re.M) and capi.MM_INFLATE_MAX_BLOCK == 65536
    assert re.search(r"enum \{ MM_INFLATE_OK = 0, MM_INFLATE_BAD_STREAM, MM_INFLATE_TRUNCATED, MM_INFLATE_OVERRUN,\s+MM_INFLATE_SHORT, MM_INFLATE_BAD_DISTANCE, MM_INFLATE_BAD_CRC \};", hdr)
    assert (capi.MM_INFLATE_OK, capi.MM_INFLATE_BAD_STREAM, capi.MM_INFLATE_TRUNCATED, capi.MM_INFLATE_OVERRUN, capi.MM_INFLATE_SHORT,
            capi.MM_INFLATE_BAD_DISTANCE, capi.MM_INFLATE_BAD_CRC) == (0, 1, 2, 3, 4, 5, 6)
    assert capi.INFLATE_STATUS == ["OK", "BAD_STREAM", "TRUNCATED", "OVERRUN", "SHORT", "BAD_DISTANCE", "BAD_CRC"]
    core = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_inflate_core.h")).read()
    assert "enum { MMI_OK = 0, MMI_BAD_STREAM = 1, MMI_TRUNCATED = 2, MMI_OVERRUN = 3, MMI_SHORT = 4, MMI_BAD_DISTANCE = 5, MMI_BAD_CRC = 6 };" in core


def test_the_exported_symbols():
    from mashmap_amd import capi
    hdr = _hdr()
    assert re.search(r"int mm_inflate_blocks\(mm_ctx\*( ctx)?, const void\* comp, size_t nComp, mm_inflate_block\* blocks, size_t nBlocks,\s+void\* dst, size_t nDst, size_t\* nBad\);", hdr)
    assert "int mm_inflate_counts(const mm_ctx* ctx, uint64_t* calls, uint64_t* blocks, uint64_t* bytesOut);" in hdr
    assert "int mm_inflate_kernel_ms(const mm_ctx* ctx, double* ms);" in hdr
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("mm_inflate_blocks", "mm_inflate_counts", "mm_inflate_kernel_ms"):
        assert name in capi.EXPORTS and hasattr(lib, name), name
    for name in capi.EXPORTS:
        assert hasattr(lib, name), name
    bound = capi.load()
    assert len(bound.mm_inflate_blocks.argtypes) == 8 and len(bound.mm_inflate_counts.argtypes) == 4 and bound.mm_inflate_blocks.restype is ctypes.c_int
    for m in ("inflate_blocks", "inflate_bgzf", "inflate_counts"):
        assert callable(getattr(capi.Context, m)), m


def test_what_stays_as_it_was():
    from mashmap_amd import capi
    hdr = _hdr()
    assert "#define MM_ABI_VERSION 2" in hdr and capi.load().mm_abi_version() == 2
    assert "MM_K_SELECT, MM_K_COUNT };" in hdr and len(capi.KERNELS) == 11
    assert "MM_OPT_CHAIN_MODES = 10 };" in hdr
    assert "int mm_reads_prefetch(mm_ctx* ctx, const char* bases, size_t nBytes);" in hdr and "size_t mm_device_bytes(void);" in hdr


def test_the_reader_stays_free_of_the_c_abi():
    """seq_parse.hpp restates the descriptor; skch_sketch.hpp, which binds the hook to mm_inflate_blocks, asserts that the two agree"""
    sp = open(os.path.join(ROOT, "mashmap_amd", "host", "seq_parse.hpp")).read()
    assert "#include \"../../include/mashmap_hip.h\"" not in sp and "mm_inflate_blocks(" not in sp and "mm_ctx" not in sp
    assert "struct InflateBlock { uint64_t cOff; uint32_t cLen, uLen; uint64_t uOff; uint32_t crc32, status; };" in sp
    sk = open(os.path.join(ROOT, "mashmap_amd", "host", "skch_sketch.hpp")).read()
    assert "sizeof(mmhost::InflateBlock) == sizeof(mm_inflate_block)" in sk and 'getenv("MASHMAP_HIP_DEVICE_INFLATE")' in sk
