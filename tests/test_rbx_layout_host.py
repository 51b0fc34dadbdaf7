"""The LDS layout of the split-bf16 residual blocks, enumerated on the host: tests/rbx_layout_check.cpp walks the layout
functions of csrc/resnet_plan.h (the ones RbxCfg and resblock_x3_kernel take their cells, tap offsets and zero cells from)
over every compiled (block, input height) and checks every fragment address; see its header comment for the list.  It is
host C++ with no GPU code, built here once plain and once with the address and undefined-behaviour sanitizers."""
import functools
import os
import re
import shutil
import subprocess

import pytest

from cough_detector_amd import build as cbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cough_detector_amd", "csrc")
BLOCK0_ROWS, BLOCK1_ROWS = (16, 17, 22, 23, 24, 26, 27), (8, 9, 11, 12, 13, 14)


@functools.lru_cache(maxsize=None)
def _run(tmp, sanitize):
    exe = os.path.join(tmp, "rbx_layout_check" + ("_san" if sanitize else ""))
    cxx = [shutil.which("c++")] if shutil.which("c++") else [cbuild._hipcc(), "-x", "c++"]
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.run([*cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "rbx_layout_check.cpp"),
                    "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rbx_layout"))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_fragment_address_of_every_instantiation(tmp, sanitize):
    r = _run(tmp, sanitize)
    print(r.stdout)
    assert r.returncode == 0, r.stderr
    assert r.stderr == ""
    lines = r.stdout.splitlines()
    assert lines[-1] == f"ok {len(BLOCK0_ROWS) + len(BLOCK1_ROWS)} instantiations"
    seen = [(int(m[1]), int(m[2])) for m in (re.match(r"block (\d) +(\d+)x", ln) for ln in lines[:-1])]
    assert seen == [(0, r) for r in BLOCK0_ROWS] + [(1, r) for r in BLOCK1_ROWS]


def test_which_instantiations_are_bordered_and_what_they_cost(tmp):
    """Bordered x planes where the workgroups-per-CU bound leaves room (block 0 at 16, 17, 22 and 26 rows), selects
    elsewhere; the shipped block 0 stays under 80 KB (two workgroups per CU), block 1 is what it was."""
    rows = {}
    for ln in _run(tmp, False).stdout.splitlines()[:-1]:
        m = re.match(r"block (\d) +(\d+)x\d+ G(\d) (\S+) x=(\S+) lds=(\d+) \(un-bordered (\d+), bound (\d+)\)", ln)
        rows[int(m[1]), int(m[2])] = (m[4], m[5], int(m[6]), int(m[7]), int(m[8]))
    assert {k for k, v in rows.items() if v[1] == "bordered"} == {(0, 16), (0, 17), (0, 22), (0, 26)}
    assert rows[0, 22] == ("16x16x32", "bordered", 78368, 74784, 80 * 1024)
    assert rows[0, 27][0] == "32x32" and rows[1, 11] == ("16x16x32", "select", 81440, 81440, 80 * 1024)
    for (blk, xh), (_, kind, lds, before, bound) in rows.items():
        assert before <= lds <= bound and (kind == "bordered" or lds == before), (blk, xh)
