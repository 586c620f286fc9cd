"""The device counter block mm_ctx::dCounters is described once, in mashmap_amd/csrc/mm_internal.h (MM_CW_* and the names under it), and
every file that writes it or reads it back addresses it by those names: under mashmap_amd/csrc/ no subscript or pointer offset applied to
the block, to a pointer derived from it, or to one of its host copies is an integer literal, and no flag is OR-ed into it as a bare
number.  (A new counter, or a reset that is eight bytes longer, then has to say which word it means.)  CPU only: reads the sources."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mashmap_amd", "csrc")

# everywhere: the kernels' views of the block (the sketch tables' LDS words of the same name have named slots too), its host copies, the
# block itself
EVERYWHERE = {
    "counters[N]": r"\bcounters\s*\)?\s*\[\s*\d+\s*\]",
    "passCnt[N]": r"\bpassCnt\s*\[\s*\d+\s*\]",
    "hc[N]": r"\bhc\s*\[\s*\d+\s*\]",
    "hPass[N]": r"\bhPass\s*\[\s*\d+\s*\]",
    "dCounters.as<T>() + N": r"\bdCounters\s*\.\s*as\s*<[^>]*>\s*\(\s*\)\s*\+\s*\d+",
    "atomicOr(&counters[..], Null)": r"\batomicOr\s*\(\s*&\s*counters\s*\[[^\]]*\]\s*,\s*\d+ull\s*\)",
}
# the mapping pass's launchers and kernels: `cnt` / `cnt2` are its pointers into the block
PASS_FILES = ("mm_map.hip", "mm_l2.hip", "mm_select.hip")
IN_PASS_FILES = {
    "cnt[N]": r"\bcnt\s*\[\s*\d+\s*\]",
    "cnt + N": r"\bcnt\s*\+\s*\d+",
    "cnt2 + N": r"\bcnt2\s*\+\s*\d+",
}


def _strip_comments(text):
    """C++ source without its comments (string and character literals are kept as they are)"""
    pat = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', re.S)
    return pat.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", text)


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
                yield f, _strip_comments(fh.read())


def _hits(patterns, name, code):
    out = []
    for what, pat in patterns.items():
        for m in re.finditer(pat, code):
            out.append("%s:%d: %s (%s)" % (name, code.count("\n", 0, m.start()) + 1, m.group(0), what))
    return out


def test_the_patterns_see_what_they_are_meant_to_see():
    bad = """atomicOr(&counters[6], 32ull); x = counters[ 2 ]; if (passCnt[1] | passCnt[3]) y = hc[7] + c->hPass[16];
             p = c->dCounters.as<unsigned long long>() + 48; q = cnt + 4; r = cnt2 + 1; s = cnt[16]; ((volatile uint32_t*)counters)[1];"""
    assert len(_hits(EVERYWHERE, "bad", bad)) == 9 and len(_hits(IN_PASS_FILES, "bad", bad)) == 3
    good = """atomicOr(&counters[MM_PC_L2_FLAGS], MM_L2F_CANDS); binCnt[3] = 0; cnt[c] = 0; n = cnt + MM_PC_L1_CAND; // counters[6]
              /* hc[5] */ s = "a // b"; t = hc[MM_PC_L2_LOCI]; c->dCounters.as<unsigned long long>() + MM_CW_MAP; tab.counters[tid] = 0; h = hc[MM_PC_READ - 1];"""
    code = _strip_comments(good)
    assert "hc[MM_PC_L2_LOCI]" in code and not _hits(EVERYWHERE, "good", code) and not _hits(IN_PASS_FILES, "good", code)


def test_no_counter_word_is_addressed_by_a_bare_number():
    seen, hits = [], []
    for name, code in _sources():
        seen.append(name)
        hits += _hits(EVERYWHERE, name, code)
        if name in PASS_FILES:
            hits += _hits(IN_PASS_FILES, name, code)
    assert set(PASS_FILES) <= set(seen) and "mm_internal.h" in seen and "mm_sketch.hip" in seen and "mm_index_dev.hip" in seen, seen
    assert not hits, "\n" + "\n".join(hits)


def test_the_block_has_one_length_and_the_redo_test_has_no_mask_that_masks_nothing():
    for name, code in _sources():
        assert not re.search(r"\bdCounters\s*\.\s*ensure\s*\(\s*\d+", code), "%s: dCounters.ensure(<number>): MM_COUNTER_BYTES is its length" % name
        assert "&~0ull" not in code.replace(" ", ""), "%s: a mask of all ones" % name
