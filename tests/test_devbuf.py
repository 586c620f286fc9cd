"""mashmap_amd/csrc/mm_devbuf.h -- DevBuf, the owner of every device allocation of the library: tests/hostlogic/devbuf_check.cpp, a
stand-alone program built with -fsanitize=address,undefined, includes the header with hipMalloc / hipFree / hipGetLastError of its own
(counting fakes over malloc / free that fail the allocations they are told to) and checks that ensure() keeps the pointer when the size
fits, grows new-before-old with an eighth plus 256 of head room, gives the old buffer up and retries (then at the exact size, then leaves
the buffer empty with the error) when allocations fail; move construction, move assignment onto a full buffer, self-move, std::swap,
release twice, structs of buffers swapped; after every step the live-byte counter behind mm_device_bytes equals the sum of `bytes`, and
at exit it is zero with every pointer freed exactly once.  Runs without a GPU."""
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
    assert re.search(r"^cases 4$", devbuf_out, re.M)
    assert sorted(re.findall(r"^ok (\w+)$", devbuf_out, re.M)) == ["failure_paths", "fits_and_grows", "moves", "structs"]
    assert re.search(r"^mismatches 0$", devbuf_out, re.M) and "FAIL" not in devbuf_out


def test_every_allocation_was_freed_once(devbuf_out):
    m = re.search(r"^allocations (\d+) frees (\d+)$", devbuf_out, re.M)
    assert m and int(m.group(1)) == int(m.group(2)) and int(m.group(1)) >= 15
