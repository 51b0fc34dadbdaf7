"""The compile-time lane masks of the residual blocks' border selects, checked on the host: tests/rbx_tap_mask_check.cpp
compares csrc/rbx_taps.h (rbx_tap_mask, the mask resblock_x3_kernel hands to v_cndmask_b32; rbx_zero_x / rbx_zero_h, the
zero cell a masked lane reads) with the image geometry, for every (tile, tap, lane) of conv1, the projection and conv2 of
all 13 instantiations; see its header comment for the list.  Host C++ with no GPU code, built once plain and once with
the address and undefined-behaviour sanitizers; with --shifted (every mask moved by one lane) it must fail."""
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
def _build(tmp, sanitize):
    exe = os.path.join(tmp, "rbx_tap_mask_check" + ("_san" if sanitize else ""))
    cxx = [shutil.which("c++")] if shutil.which("c++") else [cbuild._hipcc(), "-x", "c++"]
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.run([*cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "rbx_tap_mask_check.cpp"),
                    "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rbx_tap_masks"))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_mask_bit_and_zero_cell_of_every_instantiation(tmp, sanitize):
    r = subprocess.run([_build(tmp, sanitize)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr
    assert r.stderr == ""
    lines = r.stdout.splitlines()
    assert lines[-1] == f"ok {len(BLOCK0_ROWS) + len(BLOCK1_ROWS)} instantiations"
    seen = [(int(m[1]), int(m[2])) for m in (re.match(r"block (\d) +(\d+)x", ln) for ln in lines[:-1])]
    assert seen == [(0, r) for r in BLOCK0_ROWS] + [(1, r) for r in BLOCK1_ROWS]
    # two operands x tiles x nine taps x 64 lanes each: the shipped block 0 has 9 tiles, block 1 (two clips) 6
    bits = {(int(m[1]), int(m[2])): int(m[3]) for m in (re.match(r"block (\d) +(\d+)x.* mask bits=(\d+)", ln) for ln in lines[:-1])}
    assert bits[0, 22] == 2 * 9 * 9 * 64 and bits[1, 11] == 2 * 6 * 9 * 64


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_a_shifted_mask_is_caught(tmp, sanitize):
    r = subprocess.run([_build(tmp, sanitize), "--shifted"], capture_output=True, text=True)
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    assert "mask bit" in r.stderr and "checks failed" in r.stderr
    assert not r.stdout.splitlines()[-1].startswith("ok ")
