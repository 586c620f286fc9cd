"""mashmap_amd/csrc/mm_pass_state.h -- what mm_ctx keeps about a mapping pass (PassReport, SizedPass, PassTotals), the steady-state decisions
of mm_launch_map, the sizing rules of a sized pass and the route predicates -- on the CPU: tests/hostlogic/pass_state_check.cpp, a
stand-alone program built with -fsanitize=address,undefined.  The program prints every sizing rule at a fixed list of inputs; the GPU
tests compute their expectations from the restatement of those rules in tests/mmutil.py, and this module is what ties the two together
without a GPU: where they disagree the header is wrong (it was copied from code the GPU tests have checked against mmutil.py)."""
import os
import subprocess

import pytest

import mmutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = [0, 1, 7, 8, 63, 64, 1000, 10 ** 6, 2 ** 31 + 5, 3072, 3073]       # (3072: the locus buffer a pass without candidates starts with)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pass_state_check") / "pass_state_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "pass_state_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "FAIL" not in p.stdout, "pass_state_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    return p.stdout.splitlines()


@pytest.fixture(scope="module")
def rules(report):
    """{rule: {input: value}} as the header computes them"""
    out = {}
    for l in report:
        if l.startswith("rule "):
            _, name, n, v = l.split()
            out.setdefault(name, {})[int(n)] = int(v)
    assert all(sorted(d) == sorted(INPUTS) for d in out.values()) and len(out) == 11, {k: sorted(d) for k, d in out.items()}
    return out


def ensure_arg(monkeypatch, fn, *args):
    """the byte count fn hands to DevBuf::ensure: what mmutil.devbuf is called with"""
    seen = []
    with monkeypatch.context() as m:
        m.setattr(U, "devbuf", lambda need: seen.append(need) or need)
        fn(*args)
    assert len(seen) == 1
    return seen[0]


@pytest.mark.parametrize("what", ["structs", "steady_state", "grid_guesses", "sizing_rules", "predicates"])
def test_the_host_program_passed(report, what):
    assert "ok " + what in report and "mismatches 0" in report, report[-8:]


def test_the_sizing_rules_are_the_ones_the_gpu_tests_restate(rules):
    for n in INPUTS:
        assert rules["pts_cap"][n] == U.pts_cap(n), n
        assert rules["region_cap"][n] == U.region_cap(n), n
        assert rules["cand_cap"][n] == U.cand_cap(n), n
        assert rules["loci_cap0"][n] == U.loci_cap(n, 0), n
        # a pass without candidates starts with loci_cap0[0] loci; demand beyond that grows the buffer by the other rule
        start = rules["loci_cap0"][0]
        assert U.loci_cap(0, n) == (start if n <= start else rules["loci_cap_grown"][n]), n
    assert any(n > rules["loci_cap0"][0] for n in INPUTS) and any(0 < n <= rules["loci_cap0"][0] for n in INPUTS)


def test_the_byte_counts_of_the_wrapped_rules(rules, monkeypatch):
    for n in INPUTS:
        assert rules["dense_bytes"][n] == ensure_arg(monkeypatch, U.dense_cap, n), n
        assert rules["map_bytes"][n] == ensure_arg(monkeypatch, U.map_cap, n), n
        assert rules["ops_bytes"][n] == ensure_arg(monkeypatch, U.ops_cap, n), n
    assert U.devbuf(1000) == 1000 + 125 + 256                                     # (the patch is gone)
