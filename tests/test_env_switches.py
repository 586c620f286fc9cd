"""The environment switches: the names the code under mashmap_amd/ reads with getenv are exactly the rows of the table "Environment
switches" in INTEGRATION.md -- a switch is not added, kept or retired without the table saying so.  CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = (".hip", ".h", ".hpp", ".cpp", ".py")


def _read_in_code():
    names = set()
    for d, _, files in os.walk(os.path.join(ROOT, "mashmap_amd")):
        for f in files:
            if f.endswith(SOURCES):
                with open(os.path.join(d, f), encoding="utf-8", errors="replace") as fh:
                    names.update(re.findall(r'getenv\("([A-Za-z0-9_]+)"\)', fh.read()))
    return names


def _in_table():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        text = fh.read()
    section = re.search(r"^## \d+\. Environment switches\n(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert section, "INTEGRATION.md has no section 'Environment switches'"
    return re.findall(r"^\| `([A-Za-z0-9_]+)` \|", section.group(1), re.M)


def test_every_switch_read_is_in_the_table_and_nothing_else():
    code, rows = _read_in_code(), _in_table()
    assert len(rows) == len(set(rows)), "a switch is listed twice"
    assert code, "no getenv call found under mashmap_amd/"
    assert set(rows) == code, "read but not listed: %s; listed but not read: %s" % (sorted(code - set(rows)), sorted(set(rows) - code))


def test_the_device_library_reads_the_environment_in_one_place():
    """mm_read_env (mm_api.hip) is the only function of the device library that calls getenv: the launchers read the context's copy"""
    where = []
    csrc = os.path.join(ROOT, "mashmap_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(csrc, f), encoding="utf-8") as fh:
                where += [(f, i) for i, line in enumerate(fh, 1) if "getenv" in line]
    with open(os.path.join(csrc, "mm_api.hip"), encoding="utf-8") as fh:
        lines = fh.read().splitlines()
    start = next(i for i, l in enumerate(lines, 1) if l.startswith("mm_env mm_read_env()"))
    end = next(i for i, l in enumerate(lines, 1) if i > start and l.startswith("}"))
    outside = [(f, i) for f, i in where if not (f == "mm_api.hip" and start < i < end)]
    assert where and not outside, outside
