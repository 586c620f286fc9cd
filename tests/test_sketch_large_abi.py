"""MM_OPT_SKETCH_LARGE and mm_sketch_large_counts: declared in the header, exported by the built library, bound in capi.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_option_and_the_query_are_declared_exported_and_bound():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert re.search(r"enum \{[^}]*MM_OPT_KEEP_POINTS = 1,[^}]*MM_OPT_CHAIN_LONG = 8,[^}]*MM_OPT_SKETCH_LARGE = 9[^}]*\};", hdr)
    assert "int mm_sketch_large_counts(mm_ctx* ctx, uint64_t* fragments, uint64_t* uncut);" in hdr
    assert "#define MM_ABI_VERSION 2" in hdr or re.search(r"MM_ABI_VERSION\s*=?\s*2\b", hdr)
    assert capi.MM_OPT_SKETCH_LARGE == 9
    assert "mm_sketch_large_counts" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "mm_sketch_large_counts")
    fn = capi.load().mm_sketch_large_counts
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 3
    assert callable(getattr(capi.Context, "sketch_large")) and callable(getattr(capi.Context, "sketch_large_counts"))
    assert capi.load().mm_abi_version() == 2                     # additive: the ABI version stays


def test_the_tile_and_the_count_words_are_what_the_gpu_test_and_the_kernel_use():
    import test_gpu_sketch_large as G
    plan = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_sketch_large_plan.h")).read()
    m = re.search(r"#define MM_SKL_TILE (\d+)\b", plan)
    assert m and int(m.group(1)) == G.SKL_TILE
    # the two counts have names among the sketch launcher's words, inside the block it resets, and the kernel counts in them by name
    internal = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_internal.h")).read()
    assert re.search(r"\bMM_SKW_LARGE_FRAGS\s*=\s*1\b", internal) and re.search(r"\bMM_SKW_LARGE_UNCUT\s*=\s*2\b", internal)
    src = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_sketch_large.hip")).read()
    assert "atomicAdd(&sketchWords[MM_SKW_LARGE_FRAGS], 1ull)" in src and "atomicAdd(&sketchWords[MM_SKW_LARGE_UNCUT], 1ull)" in src
    # no timer entry of its own: the kernel is bracketed as the global-memory sketch kernel is
    assert "KernelTimer t(c, MM_K_SKETCH_HARD);" in src
