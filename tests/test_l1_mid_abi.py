"""mm_pass_l1_mid: declared in the header, exported by the built library, bound in capi.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_call_is_declared_exported_and_bound():
    from mashmap_amd import capi
    hdr = open(os.path.join(ROOT, "include", "mashmap_hip.h")).read()
    assert re.search(r"/\*[^\n]*\*/\nint mm_pass_l1_mid\(const mm_ctx\* ctx, uint64_t\* mid\);", hdr)       # with its one-line comment
    assert "mm_pass_l1_mid" in capi.EXPORTS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "mm_pass_l1_mid")
    fn = capi.load().mm_pass_l1_mid
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 2
    assert callable(getattr(capi.Context, "pass_l1_mid"))
    assert capi.load().mm_abi_version() == 2                     # additive: the ABI version stays


def test_it_reads_the_count_the_sized_pass_already_keeps():
    """no kernel, no counter word: the accessor returns SizedPass::Seen::prevMid, which map_pass fills from the word k_lookup_mid's list
    length has always been read back into"""
    api = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_api.hip")).read()
    assert re.search(r"int mm_pass_l1_mid\(const mm_ctx\* c, uint64_t\* mid\) \{\s*if \(mid\) \*mid = c->sized\.seen\.prevMid;\s*return MM_OK;\s*\}", api)
    mapsrc = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_map.hip")).read()
    assert "seen.prevMid = (size_t)p.hMid" in mapsrc
