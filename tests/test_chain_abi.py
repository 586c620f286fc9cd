"""mm_chain_reads and the calls around it: declared in the header, exported by the built library, bound in capi; the host entry points
beside mmh_post_batch exported by libmashmap_host.so.  CPU only."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mm_stat_identity_table", "mm_set_chain_tables", "mm_chain_reads", "mm_chain_counts", "mm_chain_download", "mm_chain_leftover_download",
         "mm_chain_device"]


def test_the_calls_are_declared_exported_and_bound():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    for decl in ("int mm_set_chain_tables(mm_ctx* ctx, const mm_chain_params* params, const float* identity, size_t stride);",
                 "int mm_chain_reads(mm_ctx* ctx);",
                 "int mm_chain_counts(const mm_ctx* ctx, size_t* offered, size_t* finished, size_t* rows, size_t* leftover);",
                 "int mm_chain_download(mm_ctx* ctx, mm_chain_row* out, size_t cap, size_t* n);",
                 "int mm_chain_leftover_download(mm_ctx* ctx, mm_mapping* out, size_t cap, size_t* n);",
                 "#define MM_CHAIN_MAX_RECORDS 16", "#define MM_CHAIN_MAX_SKETCH 2048", "#define MM_CHAIN_MAX_GAP (1 << 25)"):
        assert decl in hdr, decl
    assert "#define MM_ABI_VERSION 2" in hdr
    assert re.search(r"enum \{ MM_K_PACK = 0,[^}]*MM_K_SELECT, MM_K_COUNT \};", hdr)                 # the kernel enum is as it was
    lib = ctypes.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(lib, n), n
        assert getattr(capi.load(), n).restype is ctypes.c_int
    assert capi.load().mm_abi_version() == 2                                                        # additive: the ABI version stays
    assert ctypes.sizeof(capi.ChainParams) == 32 and capi.CHAIN_ROW_DT.itemsize == 72
    assert (capi.MM_CHAIN_MAX_RECORDS, capi.MM_CHAIN_MAX_SKETCH, capi.MM_CHAIN_MAX_GAP) == (16, 2048, 1 << 25)
    for m in ("set_chain_tables", "chain_reads", "chain_counts", "chain_rows", "chain_leftover", "chain_device"):
        assert callable(getattr(capi.Context, m)), m


def test_the_identity_table_is_the_hosts_expression():
    """identity[Qs * stride + shared] = 1 - j2md(1.0 * shared / Qs, k) in floats, the expression of MapPost::identityOf"""
    from mashmap_amd import capi
    s, k = 80, 16
    t = capi.stat_identity_table(s, k).reshape(s + 1, s + 1)
    lib = capi.load()
    for qs, sh in ((80, 80), (80, 40), (80, 0), (64, 33), (1, 1), (77, 76)):
        want = np.float32(1) - np.float32(lib.mm_stat_j2md(ctypes.c_float(np.float32(1.0 * sh / qs)), k))
        assert t[qs, sh].tobytes() == np.float32(want).tobytes(), (qs, sh, t[qs, sh], want)
    assert t[80, 80] == 1.0 and t[80, 0] == 0.0


def test_the_host_library_exports_the_stage_behind_the_rows():
    from mashmap_amd import shard
    lib = shard.host_lib()
    assert hasattr(lib, "mmh_post_chained") and hasattr(lib, "mmh_chain_rows") and hasattr(lib, "mmh_post_batch")
    assert len(lib.mmh_post_batch.argtypes) == 18                                                    # its signature is as it was
    assert len(lib.mmh_post_chained.argtypes) == 25 and len(lib.mmh_chain_rows.argtypes) == 19
