"""MM_OPT_L1_GROUP_FUSED and mm_pass_l1_group_fused: declared in the header, exported by the built library, bound in capi.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_option_and_the_call_are_declared_exported_and_bound():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert re.search(r"enum \{[^}]*MM_OPT_L1_GROUP_FUSED = 6[^}]*\};", hdr)
    assert "int mm_pass_l1_group_fused(const mm_ctx* ctx, uint64_t* offered, uint64_t* fused);" in hdr
    assert "#define MM_ABI_VERSION 2" in hdr or re.search(r"MM_ABI_VERSION\s*=?\s*2\b", hdr)
    assert capi.MM_OPT_L1_GROUP_FUSED == 6
    assert "mm_pass_l1_group_fused" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "mm_pass_l1_group_fused")
    fn = capi.load().mm_pass_l1_group_fused
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 3
    assert callable(getattr(capi.Context, "l1_group_fused")) and callable(getattr(capi.Context, "pass_l1_group_fused"))
    assert capi.load().mm_abi_version() == 2                     # additive: the ABI version stays


def test_the_counter_word_is_named_beside_the_others():
    """the hand-over count of k_lookup_groups has a name under MM_PC_* and the kernel counts in it by that name"""
    internal = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_internal.h")).read()
    assert re.search(r"\bMM_PC_GRP_LEN\s*=\s*MM_PC_MID_LEN\b", internal)
    mapsrc = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_map.hip")).read()
    assert "atomicAdd(&counters[MM_PC_GRP_LEN], 1ull)" in mapsrc
