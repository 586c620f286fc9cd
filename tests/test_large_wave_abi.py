"""MM_OPT_L2_LARGE_WAVE and mm_pass_l2_large: declared in the header, exported by the built library, bound in capi.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_option_and_the_call_are_declared_exported_and_bound():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert re.search(r"enum \{[^}]*MM_OPT_L2_LARGE_WAVE = 7[^}]*\};", hdr)
    assert "int mm_pass_l2_large(const mm_ctx* ctx, uint64_t* candidates, uint64_t* literal);" in hdr
    assert "#define MM_ABI_VERSION 2" in hdr or re.search(r"MM_ABI_VERSION\s*=?\s*2\b", hdr)
    assert capi.MM_OPT_L2_LARGE_WAVE == 7
    assert "mm_pass_l2_large" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "mm_pass_l2_large")
    fn = capi.load().mm_pass_l2_large
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 3
    assert callable(getattr(capi.Context, "l2_large_wave")) and callable(getattr(capi.Context, "pass_l2_large"))
    assert capi.load().mm_abi_version() == 2                     # additive: the ABI version stays


def test_the_hand_over_word_is_named_beside_the_others():
    """the hand-over count of k_l2_large_wave has a name under MM_PC_*, the kernel counts in it by that name, and the largest sketch the
    kernel's LDS layout holds includes the reference's 19 998"""
    internal = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_internal.h")).read()
    assert re.search(r"\bMM_PC_L2_LARGE_LEN\s*=\s*7\b", internal) and re.search(r"\bMM_PC_L2_WIDE_LEN\s*=\s*7\b", internal)
    src = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_l2.hip")).read()
    assert "atomicAdd(&counters[MM_PC_L2_LARGE_LEN], 1ull)" in src
    m = re.search(r"#define MM_LW_MAX_SKETCH (\d+)\b", src)
    assert m and 19998 <= int(m.group(1)) and (int(m.group(1)) + 2) * 8 + 8 * 16 <= 160 * 1024
