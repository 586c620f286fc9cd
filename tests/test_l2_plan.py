"""mashmap_amd/csrc/mm_l2_plan.h -- the LDS geometry of the split L2 route (k_l2_locate, k_l2_sweep) for every sketch size the route sees,
and the cut of a batch's candidates into chunks of located streams -- on the CPU: tests/hostlogic/l2_plan_check.cpp, a stand-alone program
built with -fsanitize=address,undefined.  It sweeps s = 1..8190 (every size fits the 160 KiB of a CU, which is why mm_launch_l2 and
mm_check_params carry no run-time check of it) and runs the planner on random offset vectors against a linear planner."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("l2_plan_check") / "l2_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "l2_plan_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "FAIL" not in p.stdout, "l2_plan_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    return p.stdout.splitlines()


def test_the_geometry_fits_a_cu_at_every_sketch_size(report):
    assert any(l.startswith("ok geometry ") for l in report), report[-5:]
    steps = {int(l.split()[1]): dict(zip(l.split()[2::2], map(int, l.split()[3::2]))) for l in report if l.startswith("step ")}
    # the sizes at which a field changes are the ones mm_l2_plan.h asserts at compile time, on both sides
    assert sorted(steps) == [1, 257, 513, 1025, 1279, 2047, 2049, 2182, 4097, 4367, 5119], sorted(steps)
    assert (steps[2182]["wpb"], steps[4367]["wpb"]) == (2, 1)
    assert steps[1279]["lpwW"] == 32 and steps[2047]["JB"] == 13 and (steps[5119]["lpwN"], steps[5119]["lpwW"]) == (16, 8)
    top = [l for l in report if l.startswith("top 8190 ")]
    assert top and all(int(x) <= 163840 for x in top[0].split()[3::2])


def test_the_chunk_planner_is_the_greedy_rule(report):
    assert any(l.startswith("ok planner ") for l in report), report[-5:]
