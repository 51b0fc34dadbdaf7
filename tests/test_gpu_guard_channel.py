"""The three entry points of libcough_amd_channel.so between the guard zones of tests/guarded.py: the rows flush against
a trailing guard, the bank at exactly ``cough_channel_bank_bytes`` under every fill, every output at exactly its promised
size, at every 4-byte phase of the source and of the output.  In range, the guarded run must equal the unguarded one bit
for bit.  With garbage in the device-side plans and lengths the result is what the header says it is (the entries are
made harmless), the guards stay intact and no guard word reaches an output."""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import channel as cch
import guarded as G
import channel_ref as R

pytestmark = pytest.mark.gpu
BIG, NEG = 2**31 - 1, -(2**31)
LENGTHS = [1, 63, 65, 16385, 20000]
WIDTH = 20000
PLANS = [(0, 0.5), (4, 1.0), (-1, 0.25), (3, 0.0), (1, float("nan"))]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _prepare(sos, n_sections, ptr, nbytes):
    sos, n_sections = np.ascontiguousarray(sos, dtype=np.float64), np.ascontiguousarray(n_sections, dtype=np.int32)
    _lib.check_channel(_lib.load_channel().cough_channel_prepare(
        sos.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double)), n_sections.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int)),
        n_sections.size, ptr, nbytes, _st()), "cough_channel_prepare")


def _rows(src_ptr, offs, lens, plans, bank_ptr, n_bank, out_ptr, width):
    _lib.check_channel(_lib.load_channel().cough_channel_rows(src_ptr, offs.data_ptr(), lens.data_ptr(), lens.numel(), plans.data_ptr(),
                                                              bank_ptr, n_bank, out_ptr, width, _st()), "cough_channel_rows")


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(6)
    rows = [(0.4 * rng.standard_normal(n)).astype(np.float32) for n in LENGTHS]
    bank = cda.ChannelBank.from_sos(R.bank_sos())
    data = torch.from_numpy(np.concatenate(rows)).cuda()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(LENGTHS)[:-1]]).astype(np.int64)).cuda()
    lens = torch.tensor(LENGTHS, dtype=torch.int32).cuda()
    plans = cch.plans_to_device(cch.plan_array(PLANS, len(bank)), data.device)
    plain = cch.channel_rows(data, offs, lens, plans, WIDTH, bank)
    unclipped = cch.channel_rows(data, offs, lens, cch.plans_to_device(cch.plan_array([(f, 1.0) for f, _ in PLANS], len(bank)), data.device),
                                 WIDTH, bank).cpu().numpy()
    refs = R.recurrence([bank.sos[f] if f >= 0 else None for f, _ in PLANS], rows, np.longdouble)
    for r, (x, (f, ratio)) in enumerate(zip(rows, PLANS)):                 # the unguarded run is itself inside the contract
        y = unclipped[r, :x.size]
        if f >= 0:
            assert (np.abs(y.astype(np.longdouble) - refs[r]) <= R.bound(refs[r], R.gain(bank.sos[f]), float(np.abs(x).max()))).all(), r
        assert np.array_equal(plain[r, :x.size].cpu().numpy().view(np.uint32), R.clip_ref(y, ratio).view(np.uint32)), r
        assert not plain[r, x.size:].any()
    return dict(bank=bank, rows=rows, data=data, offs=offs, lens=lens, plans=plans, plain=plain)


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_prepare_and_rows_between_guards_under_every_bank_fill(case, phase):
    bank = case["bank"]
    src = G.Guarded.holding(case["data"], align=16, phase=phase, name="rows")
    nbytes = cch.bank_bytes(len(bank))
    assert nbytes == 1280 * len(bank)
    sos, n_sections = np.concatenate(bank.sos), bank.n_sections
    other = np.concatenate([R.bank_sos()[4], R.bank_sos()[1]])              # a different bank, of two entries

    def leave_stale(ws):
        return G.run_other(ws, cch.bank_bytes(2), lambda ptr, size: _prepare(other, [4, 1], ptr, size))

    for fill, ws, more in G.workspaces(nbytes, leave_stale):
        _prepare(sos, n_sections, ws.ptr, nbytes)
        out = G.output((len(LENGTHS), WIDTH), torch.float32, align=16, phase=(phase + 8) % 16, name="out")
        _rows(src.ptr, case["offs"], case["lens"], case["plans"], ws.ptr, len(bank), out.ptr, WIDTH)
        G.check([src, ws, out] + more, {"out": out.view(torch.float32, len(LENGTHS), WIDTH), "bank": ws.float64},
                {"out": case["plain"], "bank": bank.blob(case["data"].device).view(torch.float64)},
                f"cough_channel_prepare + cough_channel_rows, bank fill {fill}")


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_garbage_plans_and_lengths_between_guards(case, phase):
    bank = case["bank"]
    src = G.Guarded.holding(case["data"], align=16, phase=phase, name="rows")
    blob = bank.blob(case["data"].device)
    nan_bits = np.array([np.nan], dtype=np.float32).view(np.int32)[0]
    # (filter, the ratio's bits): filters the bank does not have, every kind of ratio word
    garbage = [[(BIG, BIG), (NEG, NEG), (len(bank), 0), (-2, nan_bits), (5, np.array([0.5], dtype=np.float32).view(np.int32)[0])],
               [(BIG, np.array([0.25], dtype=np.float32).view(np.int32)[0]), (NEG, 0), (-1, NEG), (99, -1),
                (7, np.array([0.75], dtype=np.float32).view(np.int32)[0])]]
    for k, wild in enumerate(garbage):
        plans = torch.tensor([list(p) for p in wild], dtype=torch.int32).cuda()
        ratios = plans[:, 1].cpu().numpy().view(np.float32)
        tame = np.zeros(len(wild), dtype=cch.PLAN_DTYPE)                  # what the header makes of them: no filter
        tame["filter"], tame["clip_ratio"] = -1, ratios
        out = G.output((len(LENGTHS), WIDTH), torch.float32, align=16, phase=(phase + 12) % 16, name="out")
        _rows(src.ptr, case["offs"], case["lens"], plans, blob.data_ptr(), len(bank), out.ptr, WIDTH)
        want = cch.channel_rows(case["data"], case["offs"], case["lens"], tame, WIDTH, bank)
        for r, x in enumerate(case["rows"]):
            assert np.array_equal(want[r, :x.size].cpu().numpy().view(np.uint32), R.clip_ref(x, ratios[r]).view(np.uint32)), (k, r)
        G.check([src, out], {"out": out.view(torch.float32, len(LENGTHS), WIDTH)}, {"out": want}, f"cough_channel_rows, garbage plans {k}")
    # lengths the device cannot take: negative ones are empty rows, and a row longer than the matrix is cut to its width
    # (the one row for which that is tried ends the packed buffer, so its width is all it may read)
    lens = torch.tensor([NEG, -1, 0, 16385, 20000], dtype=torch.int32).cuda()
    narrow = 1000
    out = G.output((len(LENGTHS), narrow), torch.float32, align=16, phase=phase, name="out")
    _rows(src.ptr, case["offs"], lens, case["plans"], blob.data_ptr(), len(bank), out.ptr, narrow)
    want = cch.channel_rows(case["data"], case["offs"], torch.tensor([0, 0, 0, narrow, narrow], dtype=torch.int32).cuda(), case["plans"],
                            narrow, bank)
    assert not want[:3].any()
    G.check([src, out], {"out": out.view(torch.float32, len(LENGTHS), narrow)}, {"out": want}, "cough_channel_rows, garbage lengths")


@pytest.mark.parametrize("b", [1, 64, 65])
def test_draw_channel_between_guards(b):
    for phase in (0, 4, 8, 12):
        out = G.output((b, 2), torch.int32, align=16, phase=phase, name="plans")
        _lib.check_channel(_lib.load_channel().cough_draw_channel(2**63 + 5, b, 0.5, 100, 0.5, 0.25, 1.0, out.ptr, _st()),
                           "cough_draw_channel")
        want = torch.from_numpy(R.draw_channel_ref(2**63 + 5, b, 0.5, 100, 0.5, 0.25, 1.0).view(np.int32).reshape(b, 2))
        G.check([out], {"plans": out.view(torch.int32, b, 2)}, {"plans": want}, "cough_draw_channel")
