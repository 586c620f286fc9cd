"""The host side compiled with -DLARGE_CONTIG (64-bit offset_t, as the reference's build of that name: base_types.hpp:18-22), checked
without a GPU: it compiles standalone and as a drop-in with the reference's records of that build (the layout of its index files), the
command line built that way refuses to run without a device, and the stock LARGE_CONTIG binary -- the yardstick of that build -- writes
the same PAF and the same index contents as the stock default binary where positions fit in 32 bits."""
import os
import subprocess

import numpy as np
import pytest

import mmutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
HOST = os.path.join(ROOT, "mashmap_amd", "host")
LIB = os.path.join(ROOT, "mashmap_amd", "lib")
REF_LARGE_BIN = os.path.join(ROOT, "oracle", "_ref", "large_contig", "mashmap_ref")
HAVE_REF = os.path.exists(os.path.join(REF, "src", "map", "mash_map.cpp"))


# the reference's LARGE_CONTIG records (MinmerInfo / IntervalPoint with int64 offset_t), as its --saveIndex files hold them
MINMER64_DT = np.dtype([("hash", "<u8"), ("wpos", "<i8"), ("wpos_end", "<i8"), ("seqId", "<i4"), ("strand", "<i2"), ("pad", "<i2")])
POINT64_DT = np.dtype([("pos", "<i8"), ("hash", "<u8"), ("seqId", "<i4"), ("side", "i1"), ("pad1", "i1", (3,))])


def _built():
    if not os.path.exists(os.path.join(LIB, "libmashmap_hip.so")):
        import __graft_entry__ as g
        g.build()


def large_cli(out):
    """the mashmap_hip command line compiled with -DLARGE_CONTIG (the recipe of mashmap_amd/host/Makefile plus that macro)"""
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-sign-compare", "-DLARGE_CONTIG", "-o", out,
                           os.path.join(HOST, "mashmap_hip_main.cpp"), "-L" + LIB, "-lmashmap_hip", "-Wl,-rpath," + LIB, "-lz", "-lpthread"],
                          timeout=300)
    return out


LAYOUT_SRC = r"""
#include <cstddef>
#include <cstdio>
#include "skch_sketch.hpp"
static_assert(sizeof(skch::offset_t) == 8, "offset_t");
int main() {
  printf("%zu %zu %zu %zu %zu\n", sizeof(skch::MinmerInfo), offsetof(skch::MinmerInfo, wpos_end), offsetof(skch::MinmerInfo, seqId),
         offsetof(skch::MinmerInfo, strand), sizeof(skch::offset_t));
  printf("%zu %zu %zu %zu\n", sizeof(skch::IntervalPoint), offsetof(skch::IntervalPoint, hash), offsetof(skch::IntervalPoint, seqId),
         offsetof(skch::IntervalPoint, side));
  return 0;
}
"""


def test_standalone_host_compiles_with_large_contig(tmp_path):
    """skch_types.hpp with -DLARGE_CONTIG: 64-bit offset_t, MinmerInfo / IntervalPoint byte for byte the reference's records of that build"""
    _built()
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_SRC)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-DLARGE_CONTIG", "-I" + HOST, "-o", exe, str(src), "-L" + LIB, "-lmashmap_hip",
                           "-Wl,-rpath," + LIB, "-lz", "-lpthread"], timeout=300)
    a, b = [list(map(int, l.split())) for l in subprocess.check_output([exe], text=True, timeout=60).splitlines()]
    m, p = MINMER64_DT, POINT64_DT
    assert a == [m.itemsize, m.fields["wpos_end"][1], m.fields["seqId"][1], m.fields["strand"][1], 8]
    assert b == [p.itemsize, p.fields["hash"][1], p.fields["seqId"][1], p.fields["side"][1]]


@pytest.mark.skipif(not HAVE_REF, reason="reference tree not present")
def test_reference_main_compiles_with_large_contig(tmp_path):
    """the drop-in boundary of INTEGRATION.md in the reference's LARGE_CONTIG build: its unmodified mash_map.cpp against this
    repository's skch::Sketch / skch::Map, with the reference's own base_types.hpp making offset_t 64-bit"""
    _built()
    exe = str(tmp_path / "dropin_large")
    inc = ["-I" + os.path.join(HOST, "reference_tree"), "-I" + HOST, "-I" + os.path.join(REF, "src"), "-I" + os.path.join(REF, "src", "common"),
           "-I" + os.path.join(ROOT, "oracle", "gsl_shim")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-DLARGE_CONTIG", "-DMASHMAP_HIP_REFERENCE_TREE"] + inc +
                          ["-o", exe, os.path.join(REF, "src", "map", "mash_map.cpp"), "-L" + LIB, "-lmashmap_hip", "-Wl,-rpath," + LIB,
                           "-lz", "-lpthread"], timeout=300)
    chk = tmp_path / "offset.cpp"
    chk.write_text('#include "map/include/base_types.hpp"\n#include "skch_sketch.hpp"\n'
                   'static_assert(sizeof(skch::offset_t) == 8, "offset_t");\n'
                   'static_assert(sizeof(skch::MinmerInfo) == 32 && sizeof(skch::IntervalPoint) == 24, "records");\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-DLARGE_CONTIG", "-DMASHMAP_HIP_REFERENCE_TREE"] + inc + [str(chk)], timeout=300)
    p = subprocess.run([exe, "-v"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "3.1.3" in p.stderr


def test_large_contig_cli_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _built()
    exe = large_cli(str(tmp_path / "mashmap_hip_lc"))
    fa = tmp_path / "t.fa"
    fa.write_text(">a\n" + "ACGT" * 2000 + "\n")
    p = subprocess.run([exe, "-r", str(fa), "-q", str(fa), "-o", "/dev/null"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "no usable HIP device" in p.stderr


def _yardstick_case():
    cs = [U.random_dna(611, 150000), U.random_dna(612, 90000)]
    blk = U.mutate(cs[0][20000:45000], 81, 0.03)
    cs[1][10000:10000 + len(blk)] = blk
    ref = [("c1", cs[0]), ("c2", cs[1])]
    reads = [(n, a) for n, a, _ in U.sample_reads(cs, 21, 24, 10000, 0.08)]
    return ref, reads


@pytest.mark.skipif(not (HAVE_REF or os.path.exists(REF_LARGE_BIN)), reason="reference tree not present")
def test_stock_large_binary_matches_stock_default(tmp_path):
    """the yardstick itself: below 2^31 the reference's LARGE_CONTIG build writes the PAF of its default build, and its --saveIndex
    files hold the 64-bit records MINMER64_DT / POINT64_DT describe, with the positions of the default build's files"""
    _built()
    assert os.path.exists(REF_LARGE_BIN) and os.path.exists(U.REF_BIN)
    ref, reads = _yardstick_case()
    rf, qf = str(tmp_path / "r.fa"), str(tmp_path / "q.fa")
    U.write_fasta(rf, ref)
    U.write_fasta(qf, reads)
    outs = {}
    for tag, exe in (("default", U.REF_BIN), ("large", REF_LARGE_BIN)):
        o = str(tmp_path / (tag + ".paf"))
        subprocess.check_call([exe, "-r", rf, "-q", qf, "-o", o, "-t", "4", "--saveIndex", str(tmp_path / tag)], stderr=subprocess.DEVNULL, timeout=600)
        outs[tag] = open(o, "rb").read()
    assert outs["default"].count(b"\n") > 20
    assert outs["large"] == outs["default"]
    from mashmap_amd import capi
    idx = {}
    for tag, mdt, pdt in (("default", capi.MINMER_DT, capi.POINT_DT), ("large", MINMER64_DT, POINT64_DT)):
        raw = open(str(tmp_path / tag) + ".index", "rb").read()
        n = int(np.frombuffer(raw[:8], dtype="<u8")[0])
        assert len(raw) == 8 + n * mdt.itemsize
        mins = np.frombuffer(raw[8:], dtype=mdt, count=n)
        raw = open(str(tmp_path / tag) + ".map", "rb").read()
        nk, off, pts = int(np.frombuffer(raw[:8], dtype="<u8")[0]), 8, []
        for _ in range(nk):
            key, cnt = (int(x) for x in np.frombuffer(raw[off:off + 16], dtype="<u8"))
            p = np.frombuffer(raw[off + 16:off + 16 + pdt.itemsize * cnt], dtype=pdt)
            pts.append((key, [(int(x["pos"]), int(x["hash"]), int(x["seqId"]), int(x["side"])) for x in p]))
            off += 16 + pdt.itemsize * cnt
        assert off == len(raw)
        idx[tag] = ([tuple(int(m[f]) for f in ("hash", "wpos", "wpos_end", "seqId", "strand")) for m in mins], pts)
    assert len(idx["large"][0]) > 100 and idx["large"] == idx["default"]
