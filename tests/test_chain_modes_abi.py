"""MM_OPT_CHAIN_MODES and mm_chain_group_counts: declared in the header, exported by the built library, bound in capi; the checker entry
mmh_chain_rows_modes of the host library -- and what the option leaves as it was: the ABI version, the other options' values, the two
record limits, the parameter block and the row.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_option_and_the_count_call():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert re.search(r"enum \{[^}]*MM_OPT_KEEP_POINTS = 1,[^}]*MM_OPT_CHAIN_LONG = 8,[^}]*MM_OPT_SKETCH_LARGE = 9,[^}]*MM_OPT_CHAIN_MODES = 10[^}]*\};", hdr)
    assert "int mm_chain_group_counts(const mm_ctx* ctx, uint64_t* reads, uint64_t* runs);" in hdr
    assert re.search(r"MM_OPT_CHAIN_MODES \(default 0\)", hdr) and "A RUN is" in hdr
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert "mm_chain_group_counts" in capi.EXPORTS and hasattr(lib, "mm_chain_group_counts")
    for name in capi.EXPORTS:
        assert hasattr(lib, name), name
    assert capi.load().mm_chain_group_counts.restype is ctypes.c_int and len(capi.load().mm_chain_group_counts.argtypes) == 3
    assert capi.MM_OPT_CHAIN_MODES == 10
    for m in ("chain_modes", "chain_group_counts"):
        assert callable(getattr(capi.Context, m)), m


def test_the_checker_entry_of_the_host_library():
    from mashmap_amd import shard
    lib = shard.host_lib()
    assert hasattr(lib, "mmh_chain_rows_modes") and len(lib.mmh_chain_rows_modes.argtypes) == len(lib.mmh_chain_rows.argtypes) + 2
    for name in ("mmh_chain_rows", "mmh_post_chained", "mmh_post_batch"):
        assert hasattr(lib, name), name


def test_what_stays_as_it_was():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert "#define MM_ABI_VERSION 2" in hdr and capi.load().mm_abi_version() == 2
    assert re.search(r"^#define MM_CHAIN_MAX_RECORDS 16\b", hdr, re.M) and re.search(r"^#define MM_CHAIN_LONG_MAX_RECORDS 512\b", hdr, re.M)
    assert capi.MM_OPT_CHAIN_LONG == 8 and capi.MM_OPT_SKETCH_LARGE == 9
    assert ctypes.sizeof(capi.ChainParams) == 32 and capi.CHAIN_ROW_DT.itemsize == 72
    assert "int mm_chain_counts(const mm_ctx* ctx, size_t* offered, size_t* finished, size_t* rows, size_t* leftover);" in hdr
    assert "int mm_chain_long_counts(const mm_ctx* ctx, uint64_t* offered, uint64_t* finished);" in hdr
