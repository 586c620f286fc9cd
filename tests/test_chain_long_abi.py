"""MM_OPT_CHAIN_LONG and mm_chain_long_counts: declared in the header, exported by the built library, bound in capi -- and what the
option leaves as it was: the ABI version, the 16-record limit of the one-thread kernel, the parameter block.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_option_the_limit_and_the_count_call():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert re.search(r"^#define MM_CHAIN_LONG_MAX_RECORDS 512\b", hdr, re.M)
    assert re.search(r"enum \{[^}]*MM_OPT_KEEP_POINTS = 1,[^}]*MM_OPT_CHAIN_LONG = 8[^}]*\};", hdr)
    assert "int mm_chain_long_counts(const mm_ctx* ctx, uint64_t* offered, uint64_t* finished);" in hdr
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert "mm_chain_long_counts" in capi.EXPORTS and hasattr(lib, "mm_chain_long_counts")
    assert capi.load().mm_chain_long_counts.restype is ctypes.c_int and len(capi.load().mm_chain_long_counts.argtypes) == 3
    assert capi.MM_OPT_CHAIN_LONG == 8 and capi.MM_CHAIN_LONG_MAX_RECORDS == 512
    for m in ("chain_long", "chain_long_counts"):
        assert callable(getattr(capi.Context, m)), m


def test_what_stays_as_it_was():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert "#define MM_ABI_VERSION 2" in hdr and capi.load().mm_abi_version() == 2
    assert re.search(r"^#define MM_CHAIN_MAX_RECORDS 16\b", hdr, re.M) and capi.MM_CHAIN_MAX_RECORDS == 16
    assert ctypes.sizeof(capi.ChainParams) == 32 and capi.CHAIN_ROW_DT.itemsize == 72
    assert "int mm_chain_counts(const mm_ctx* ctx, size_t* offered, size_t* finished, size_t* rows, size_t* leftover);" in hdr
