"""mashmap_amd/csrc/mm_devbuf.h -- DevBuf, the owner of every device allocation of the library: tests/hostlogic/devbuf_check.cpp, a
stand-alone program built with -fsanitize=address,undefined, includes the header with hipMalloc / hipFree / hipGetLastError of its own
(counting fakes over malloc / free that fail the allocations they are told to) and checks that ensure() keeps the pointer when the size
fits, grows new-before-old with an eighth plus 256 of head room, gives the old buffer up and retries (then at the exact size, then leaves
the buffer empty with the error) when allocations fail; move construction, move assignment onto a full buffer, self-move, std::swap,
release twice, structs of buffers swapped; after every step the live-byte counter behind mm_device_bytes equals the sum of `bytes`, and
at exit it is zero with every pointer freed exactly once.  The same program, with fakes for the stream, event and page-locked calls,
checks the other owners of that header: DevStream and DevEvent (ensure() twice creates once, a failed creation leaves the handle null and a
later one succeeds, the moves, a half-made context gives back what it made) and PinnedBuf (fits keeps the pointer, growth frees and then
allocates exactly what is asked, a failure leaves it empty with the sticky error cleared); every handle is destroyed exactly once.
Runs without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def devbuf_out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devbuf_check") / "devbuf_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "hostlogic", "devbuf_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, "devbuf_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-4000:])
    return p.stdout


def test_every_case_ran_without_a_mismatch(devbuf_out):
    assert re.search(r"^cases 6$", devbuf_out, re.M)
    assert sorted(re.findall(r"^ok (\w+)$", devbuf_out, re.M)) == ["failure_paths", "fits_and_grows", "handles", "moves", "pinned", "structs"]
    assert re.search(r"^mismatches 0$", devbuf_out, re.M) and "FAIL" not in devbuf_out


def test_every_allocation_was_freed_once(devbuf_out):
    m = re.search(r"^allocations (\d+) frees (\d+)$", devbuf_out, re.M)
    assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) >= 15


def test_every_stream_event_and_pinned_block_was_given_back_once(devbuf_out):
    for kind, gone, least in (("streams", "destroyed", 3), ("events", "destroyed", 5), ("pinned", "freed", 5)):
        m = re.search(r"^%s (\d+) %s (\d+)$" % (kind, gone), devbuf_out, re.M)
        assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) >= least, (kind, m and m.groups())
