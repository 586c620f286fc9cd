"""mashmap_amd/csrc/mm_text_core.h -- the record rules of FASTA / FASTQ text as a decomposition over tiles (summarise, combine, resolve),
which the kernels of mashmap_amd/csrc/mm_text.hip run on the device -- against the serial functions of mashmap_amd/host/seq_parse.hpp:
tests/hostlogic/text_check.cpp, a stand-alone program with its own main, built with -fsanitize=address,undefined.  Tiles of 1, 7, 64 and
4096 bytes, both formats, final 0 and 1; the edge texts, their mutations and 6000 random strings over {>, @, +, \\n, \\r, ' ', A, c, N, x}.
Also: the Python reference of the GPU tests (tests/textzoo.py) against the same specification.  Runs without a GPU."""
import re
import subprocess

import pytest

import textzoo as Z


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return Z.build_check(tmp_path_factory.mktemp("text_check"))


@pytest.fixture(scope="module")
def out(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "text_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def _num(out, pattern):
    m = re.search(pattern, out, re.M)
    assert m, pattern
    return int(m.group(1))


def test_no_difference_from_the_serial_reader_and_nothing_for_the_sanitizers(out):
    assert re.search(r"^differences 0$", out, re.M)


def test_what_was_run(out):
    texts = _num(out, r"^texts (\d+)$")
    assert _num(out, r"^random texts (\d+)$") >= 6000 and texts >= 6900
    assert _num(out, r"^runs (\d+)$") == texts * 2 * 2 * 4               # formats x final x tile sizes
    assert _num(out, r"^records (\d+)$") > 100000
    assert _num(out, r"^plain tiles (\d+)$") > 100000
    assert _num(out, r"^scan orders (\d+)$") == texts * 16
    assert _num(out, r"^associativity checks (\d+)$") == 40000


def test_the_python_reference_of_the_gpu_tests(exe, tmp_path):
    """tests/textzoo.py's parse(), the reference of tests/test_gpu_text.py, against the specification on every edge text, cut in places"""
    path = str(tmp_path / "text.bin")
    n = 0
    for name, fmt, text in Z.edge_texts(256):
        for cut in (len(text), len(text) // 2, len(text) - 1):
            t = text[:cut]
            open(path, "wb").write(t)
            for final in (0, 1):
                p = subprocess.run([exe, "--parse", path, "fasta" if fmt == Z.FASTA else "fastq", str(final)], capture_output=True, text=True)
                assert p.returncode == 0, p.stderr[-2000:]
                recs, consumed = Z.parse(t, fmt, final)
                want = ["%d %s. %d %d" % (o, nm.hex(), len(s), Z.has_n(s)) for o, nm, s in recs] + ["consumed %d" % consumed]
                assert p.stdout.split("\n")[:-1] == want, (name, cut, final)
                n += 1
    assert n > 400


def test_the_plain_build(exe, tmp_path):
    """a module marked gpu may use the plain build only: the same verdict"""
    p = subprocess.run([Z.build_check(tmp_path, sanitize=False)], capture_output=True, text=True)
    assert p.returncode == 0 and re.search(r"^differences 0$", p.stdout, re.M)
