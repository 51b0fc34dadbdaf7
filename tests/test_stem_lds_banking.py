"""The fused stem's A-fragment reads against the LDS banking of gfx950, modelled on the CPU from the constants of
``csrc/featurize.hip``.

Banking of ``ds_read_b32`` (and of each dword of ``ds_read2_b32``): a wave's 64 lanes are served in two groups of 32 lanes,
{0..31} and {32..63}, one LDS cycle per group when conflict-free; the bank of a dword is ``dword index mod 32``; lanes of one
group that read the same dword share one access, and every further distinct dword on a bank that is already busy costs the group
one more cycle.

A fragment of the stem is four dwords at ``(2 (2 ph + dy) + sh) * pitch + 2 (2 pw + dx)`` bf16 (+ plane, + two image rows per
k-step), lane = (sr, sh), sr = (pool window q, dy, dx), pooled position P = 8 tile + q.  At the narrow pitch of 106 bf16 the
dy = 1 half of a group lands 10 banks behind the dy = 0 half and every read takes two passes (ratio 2.000); the wide pitch of
112 bf16 puts it 16 banks behind and leaves only the tiles that cross a pooled-row boundary conflicted (1.275).
"""
import os
import re

import pytest

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cough_detector_amd", "csrc", "featurize.hip")
LDS_THREE_WORKGROUPS = 53760     # the largest workgroup of which a CU still holds three (1280-byte granules of 160 KB)
BANKS, GROUP = 32, 32


@pytest.fixture(scope="module")
def consts():
    text = open(SRC).read()

    def const(name):
        m = re.search(r"\b" + name + r"\s*=\s*(\d+)\b", text)
        assert m, f"{name} not found in featurize.hip"
        return int(m.group(1))

    c = {n: const(n) for n in ("NFRAMES", "NMEL", "NMFCC", "THREADS", "FPW", "XROW", "ST_P1H", "ST_P1W", "ST_ROWS",
                               "ST_PITCH_NARROW", "ST_PITCH_WIDE", "LDS_WG3_MAX", "TL_HALF", "TL_ROWS")}
    # the pitch rule itself: shipped instantiations wide, full-band ones narrow
    assert re.search(r"st_pitch\(bool full\)\s*\{\s*return full \? ST_PITCH_NARROW : ST_PITCH_WIDE;", text)
    return c


def _group_cycles(dwords):
    """LDS cycles of one 32-lane group reading these dword indices."""
    per_bank = {}
    for d in set(dwords):
        per_bank[d % BANKS] = per_bank.get(d % BANKS, 0) + 1
    return max(per_bank.values())


def _clip_cycles(c, pitch, p1h, rows):
    """(cycles, conflict-free cycles) of all fragment reads of one image: every tile, both operand planes, four k-steps, four
    dwords.  ``p1h`` pooled rows out of a ``rows``-row image (the 103-row stem runs two such halves)."""
    assert pitch % 2 == 0
    per, plane = p1h * c["ST_P1W"], rows * pitch // 2
    tiles = (per + 7) // 8
    cycles = ideal = 0
    for tile in range(tiles):
        base = []
        for lane in range(64):
            sr, sh = lane & 31, lane >> 5
            q, dy, dx = sr >> 2, (sr >> 1) & 1, sr & 1
            p = min(tile * 8 + q, per - 1)
            ph, pw = divmod(p, c["ST_P1W"])
            row, col = 2 * (2 * ph + dy) + sh, 2 * (2 * pw + dx)
            assert row + 6 < rows and col + 7 < pitch          # the last k-step and the fourth dword stay inside the image
            base.append((row * pitch + col) // 2)
        for pl in range(2):
            for st in range(4):
                for k in range(4):
                    off = pl * plane + st * pitch + k              # + 2 image rows per k-step = `pitch` dwords
                    for g in range(0, 64, GROUP):
                        cycles += _group_cycles([b + off for b in base[g:g + GROUP]])
                        ideal += 1
    return cycles, ideal


def test_wide_pitch_keeps_the_stem_fragment_reads_within_1_3x_of_conflict_free(consts):
    c = consts
    wide, narrow = c["ST_PITCH_WIDE"], c["ST_PITCH_NARROW"]
    assert (2 * (wide // 2)) % 32 == 16                            # dy (two image rows) moves a fragment 16 banks on
    assert wide >= c["NFRAMES"] + 3 + 2 and narrow >= c["NFRAMES"] + 3 + 2
    # every widened instantiation: the 90-row stem (shipped, pre-emphasis, PCEN rows) and a half of the 103-row stem
    shapes = {"90-row stem": (c["ST_P1H"], c["ST_ROWS"]), "103-row stem, one half": (c["TL_HALF"], c["TL_ROWS"])}
    for name, (p1h, rows) in shapes.items():
        cyc, ideal = _clip_cycles(c, wide, p1h, rows)
        print(f"{name}: pitch {wide}: {cyc} cycles / {ideal} conflict-free = {cyc / ideal:.3f}")
        assert cyc <= 1.3 * ideal
    cyc, ideal = _clip_cycles(c, wide, c["ST_P1H"], c["ST_ROWS"])
    assert ideal == 69 * 2 * 4 * 4 * 2 == 4416 and abs(cyc / ideal - 1.275) < 5e-4
    # the narrow pitch the full-band instantiations keep: every read takes two passes
    cyc_n, ideal_n = _clip_cycles(c, narrow, c["ST_P1H"], c["ST_ROWS"])
    print(f"90-row stem: pitch {narrow}: {cyc_n} cycles / {ideal_n} conflict-free = {cyc_n / ideal_n:.3f}")
    assert cyc_n == 2 * ideal_n == 8832


def test_widened_stem_workgroups_still_share_a_cu_three_ways(consts):
    c = consts
    assert c["LDS_WG3_MAX"] == LDS_THREE_WORKGROUPS
    nmf = c["NMFCC"] * c["NFRAMES"]
    lds_total = (c["THREADS"] // 64 * c["FPW"] * 16 * c["XROW"] * 4 + c["NMEL"] * c["NFRAMES"] * 4 + 16 * 4 + 16 * c["XROW"] * 8)
    assert lds_total == 45504
    # 90-row split-bf16 stem: MFCC rows | hi image | lo image
    x3_off = (nmf * 4 + 15) & ~15
    img = c["ST_ROWS"] * c["ST_PITCH_WIDE"] * 2
    wide_total = x3_off + 2 * img
    print(f"split-bf16 stem at pitch {c['ST_PITCH_WIDE']}: {wide_total} B of LDS per workgroup")
    assert lds_total <= wide_total <= LDS_THREE_WORKGROUPS and wide_total == 47376
    # single-bf16 stem: its one image lies over the dB buffer
    assert img <= c["NMEL"] * c["NFRAMES"] * 4
    # 103-row stem: MFCC + delta rows | hi + lo partial images of 58 rows | the 15 mel rows of the second half
    tl_img_off = (2 * nmf * 4 + 15) & ~15
    tl_end = tl_img_off + 2 * c["TL_ROWS"] * c["ST_PITCH_WIDE"] * 2 + 15 * c["NFRAMES"] * 4
    assert tl_end <= lds_total <= LDS_THREE_WORKGROUPS
