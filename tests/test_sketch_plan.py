"""mashmap_amd/csrc/mm_sketch_plan.h -- the LDS layouts of k_sketch_fast and k_sketch_hard, the fast kernel's geometry and the route a
batch takes (fast / all-hard / spilled / non-power-of-two table / stream / refused) -- on the CPU: tests/hostlogic/sketch_plan_check.cpp, a
stand-alone program built with -fsanitize=address,undefined.  Its plan rows are compared with tests/golden/sketch_plan_rows.txt, recorded from
the planner as it stood inside mm_sketch.hip with its hand-written LDS formulas; the layouts are swept over every fragment length."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sketch_plan_check") / "sketch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostlogic", "sketch_plan_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "FAIL" not in p.stdout, "sketch_plan_check (sanitized) failed with status %d:\n%s\n%s" % (p.returncode, p.stdout[-4000:], p.stderr[-4000:])
    return p.stdout.splitlines()


def test_the_plans_are_the_recorded_rows(report):
    got = [l for l in report if " | " in l]
    want = open(os.path.join(ROOT, "tests", "golden", "sketch_plan_rows.txt")).read().splitlines()
    assert len(want) == 1320
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # the grid reaches every route: refused, stream, spilled with the fast kernel and without, all-hard in LDS, and strips of 20
    flags = {tuple(l.split(" | ")[1].split()[:4]) for l in want}
    assert flags == {("0", "0", "1", "1"), ("1", "0", "0", "0"), ("1", "0", "1", "0"), ("1", "0", "1", "1"), ("1", "1", "0", "0"), ("1", "1", "1", "0")}
    assert sum(l.split(" | ")[1].split()[4] == "20" for l in want) == 60


def test_the_layouts_hold_at_every_fragment_length(report):
    assert any(l.startswith("ok layouts ") for l in report), report[-5:]


def test_the_parameter_classes_and_the_fast_cut(report):
    assert any(l == "ok params" for l in report), report[-5:]
    assert any(l == "ok fast cut" for l in report), report[-5:]


def test_the_kernels_carve_by_the_layouts():
    """the kernels take their pointers from the layout structs and the launchers size with them: no second statement of the carve is left"""
    src = open(os.path.join(ROOT, "mashmap_amd", "csrc", "mm_sketch.hip")).read()
    assert "off +=" not in src
    for gone in ("sketch_fast_lds", "sketch_hard_lds", "sketch_hard_lds_spill"):
        assert gone not in src
    assert "sketch_fast_layout(" in src and "sketch_hard_layout(" in src
