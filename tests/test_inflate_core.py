"""mashmap_amd/csrc/mm_inflate_core.h -- the raw-deflate decoder and the CRC-32 (bytewise, and the combine step) that k_inflate_blocks
runs on the device -- against zlib on the host: tests/hostlogic/inflate_check.cpp, a stand-alone program with its own main, built with
-fsanitize=address,undefined and linked with -lz.  Corpora of 60-column ACGT FASTA, FASTQ and random bytes at levels 0, 1, 6, 9 and with
Z_FIXED, Z_RLE and Z_HUFFMAN_ONLY, every payload length 0 .. 600 and 32767, 32768, 32769, 65280, 65535, 65536; the hand-built streams
(a bit writer inside the check); the named malformed blocks, each with its status; more than 200 000 mutated streams (bit flips,
truncations, descriptors that lie about cLen, uLen or the CRC), all on heap blocks of exactly cLen / uLen bytes.  The rules: what zlib's
inflate(.., -15) accepts with total_out == uLen and the descriptor's CRC decodes to the same bytes with status OK; status OK implies uLen
bytes with the descriptor's CRC-32; no run takes more iterations than 8 cLen + uLen.

HCLEN 4: a stream zlib accepts cannot have it -- it names the lengths of the code-length symbols 16, 17, 18 and 0 only, so every
literal/length code is 0 bits long and the end-of-block code is missing.  The check holds that stream among the malformed ones (zlib
refuses it too) and HCLEN 5, the least an accepted stream can have, among the hand-built ones.  Runs without a GPU."""
import re
import subprocess

import pytest

import inflatezoo as Z


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return Z.build_check(tmp_path_factory.mktemp("inflate_check"))


@pytest.fixture(scope="module")
def out(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "inflate_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def _num(out, pattern):
    m = re.search(pattern, out, re.M)
    assert m, pattern
    return [int(x) for x in m.groups()]


def test_no_difference_from_zlib_and_nothing_for_the_sanitizers(out):
    assert re.search(r"^differences 0$", out, re.M)


def test_the_corpora_and_the_hand_built_streams(out):
    assert _num(out, r"^corpus streams (\d+)$")[0] == 3 * 7 * (601 + 6)
    assert _num(out, r"^hand-built streams (\d+)$")[0] >= 16
    assert _num(out, r"^malformed blocks (\d+)$")[0] >= 19


def test_the_mutations(out):
    assert _num(out, r"^mutated streams (\d+)$")[0] >= 200000
    runs, accepted, here_only, over = _num(out, r"^runs (\d+) accepted by zlib (\d+) accepted here only (\d+) over the step bound (\d+)$")
    assert over == 0 and here_only == 0 and accepted > 10000 and runs > 210000
    counts = _num(out, r"^status counts ok (\d+) bad_stream (\d+) truncated (\d+) overrun (\d+) short (\d+) bad_distance (\d+) bad_crc (\d+)$")
    assert all(c > 100 for c in counts), counts           # every status is reached by the mutations


def test_crc32_and_the_combine_step(out):
    assert _num(out, r"^crc checks (\d+)$")[0] == 301 * 302 // 2 + 9


def test_the_zoo_for_the_gpu_test(exe, tmp_path):
    """what tests/test_gpu_inflate.py takes from the check: every named case, each with its expected status"""
    zoo = Z.load_zoo(exe, tmp_path)
    names = [z[0] for z in zoo]
    assert len(set(names)) == len(names)
    for n in ("one_bit_distance_code", "no_distance_code", "fifteen_bit_codes", "hclen_5", "zero_repeat_across_the_boundary",
              "copied_length_across_the_boundary", "length_258_at_distances_1_to_8", "distance_32768", "match_ends_at_ulen", "match_reaches_byte_0",
              "stored_len_0", "stored_65535_behind_a_header_in_mid_byte", "stored_65520_behind_a_header_in_mid_byte", "end_of_block_on_the_last_bit", "empty_stored_block_in_mid_stream"):
        assert any(z[0] == n and z[1] == 0 for z in zoo), n
    want = {"block_type_3": 1, "stored_len_is_not_the_complement": 1, "hlit_above_286": 1, "hdist_above_30": 1, "repeat_with_nothing_to_repeat": 1,
            "repeat_past_the_end": 1, "over_subscribed_set": 1, "missing_end_of_block_code": 1, "hclen_4": 1, "length_symbol_286": 1, "length_symbol_287": 1,
            "distance_symbol_30": 1, "distance_symbol_31": 1, "distance_one_before_byte_0": 5, "input_exhausted": 2, "output_past_ulen": 3,
            "match_past_ulen": 3, "stream_ends_before_ulen": 4, "crc_mismatch": 6}
    assert {z[0]: z[1] for z in zoo if z[1]} == want
    assert sum(1 for z in zoo if z[1] == 0 and re.match(r"(fasta|fastq|random)_", z[0])) == 3 * 7 * 12


def test_the_plain_build_writes_the_same_zoo(exe, tmp_path):
    """tests/test_gpu_inflate.py builds the program without the sanitizers (none runs in a test marked gpu) to have the zoo written out:
    byte for byte the file the sanitized build writes, and has run"""
    a, b = tmp_path / "san", tmp_path / "plain"
    a.mkdir(); b.mkdir()
    Z.load_zoo(exe, a)
    Z.load_zoo(Z.build_check(b, sanitize=False), b)
    assert open(a / "zoo.bin", "rb").read() == open(b / "zoo.bin", "rb").read()
