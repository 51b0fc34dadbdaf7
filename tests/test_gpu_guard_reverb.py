"""The three entry points of libcough_amd_reverb.so between the guard zones of tests/guarded.py: the taps and the rows
flush against a trailing guard, the workspace at exactly ``cough_reverb_bank_bytes`` under every fill, every output at
exactly its promised size, at every 4-byte phase of the source and of the output.  In range, the guarded run must equal
the unguarded one bit for bit.  With garbage in the device-side plans the result is what the header says it is (the
entries are made harmless), the guards stay intact and no guard word reaches an output."""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import reverb as crev
import guarded as G
import reverb_ref as R

pytestmark = pytest.mark.gpu
BIG, NEG = 2**31 - 1, -(2**31)
TAPS = [1, 300, 8193]
LENGTHS = [1, 255, 8193, 16385, 20000]
WIDTH = 20000 + 8192                                   # two spans, the second one ragged
PLANS = [(0, 0, 1), (-3, 1, 554), (100, 2, 16385), (0, -1, 16000), (-4000, 2, WIDTH)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _prepare(taps_ptr, offsets, lengths, ws_ptr, ws_bytes):
    offsets, lengths = np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(lengths, dtype=np.int32)
    _lib.check_reverb(_lib.load_reverb().cough_reverb_prepare(
        taps_ptr, offsets.ctypes.data_as(_lib.C.POINTER(_lib.C.c_longlong)), lengths.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int)),
        lengths.size, ws_ptr, ws_bytes, _st()), "cough_reverb_prepare")


def _rows(src_ptr, offs, lens, plans, ws_ptr, n_rirs, out_ptr, width):
    _lib.check_reverb(_lib.load_reverb().cough_reverb_rows(src_ptr, offs.data_ptr(), lens.data_ptr(), lens.numel(), plans.data_ptr(),
                                                           ws_ptr, n_rirs, out_ptr, width, _st()), "cough_reverb_rows")


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(6)
    taps = [(rng.standard_normal(n) / np.sqrt(n)).astype(np.float32) for n in TAPS]
    rows = [rng.standard_normal(n).astype(np.float32) for n in LENGTHS]
    bank = cda.RirBank(taps)
    data = torch.from_numpy(np.concatenate(rows)).cuda()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(LENGTHS)[:-1]]).astype(np.int64)).cuda()
    lens = torch.tensor(LENGTHS, dtype=torch.int32).cuda()
    plans = torch.from_numpy(crev.plan_array(PLANS, len(TAPS), WIDTH)).cuda()
    plain = crev.reverb_rows(data, offs, lens, plans, WIDTH, bank)
    for r, (x, (shift, rir, out_len)) in enumerate(zip(rows, PLANS)):           # the unguarded run is itself inside the contract
        h = taps[rir] if rir >= 0 else None
        row = dict(name=str(r), x=x, shift=shift, rir=rir, out_len=out_len, twin=None)
        e = dict(ref=R.reverb_ref(x, shift, h, out_len), emu=R.emulate(x, shift, h, out_len))
        if h is not None:
            e.update(bound=R.bound(x, shift, h, out_len), bad=R.bad_spans(x, shift, out_len), silent=R.silent_spans(x, shift, out_len))
        R.check_row(plain[r].cpu().numpy(), row, e, WIDTH)
    return dict(bank=bank, data=data, offs=offs, lens=lens, plans=plans, plain=plain)


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_prepare_and_rows_between_guards_under_every_workspace_fill(case, phase):
    bank = case["bank"]
    taps = G.Guarded.holding(bank.device_taps(case["data"].device), align=16, phase=(phase + 4) % 16, name="taps")
    src = G.Guarded.holding(case["data"], align=16, phase=phase, name="rows")
    nbytes = crev.bank_bytes(len(bank))
    assert nbytes == 131072 * (len(bank) + 1)
    other = torch.from_numpy(np.linspace(-1, 1, 700).astype(np.float32)).cuda()

    def leave_stale(ws):                                   # a different bank, of two responses, prepared into the same bytes
        return G.run_other(ws, crev.bank_bytes(2), lambda ptr, size: _prepare(other.data_ptr(), [0, 200], [200, 500], ptr, size))

    for fill, ws, more in G.workspaces(nbytes, leave_stale):
        _prepare(taps.ptr, bank.offsets, bank.lengths, ws.ptr, nbytes)
        out = G.output((len(LENGTHS), WIDTH), torch.float32, align=16, phase=(phase + 8) % 16, name="out")
        _rows(src.ptr, case["offs"], case["lens"], case["plans"], ws.ptr, len(bank), out.ptr, WIDTH)
        G.check([taps, src, ws, out] + more, {"out": out.view(torch.float32, len(LENGTHS), WIDTH),
                                               "workspace": ws.float32},
                {"out": case["plain"], "workspace": bank.workspace(case["data"].device).view(torch.float32)},
                f"cough_reverb_prepare + cough_reverb_rows, workspace fill {fill}")


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_garbage_plans_between_guards(case, phase):
    bank = case["bank"]
    src = G.Guarded.holding(case["data"], align=16, phase=phase, name="rows")
    ws = bank.workspace(case["data"].device)
    garbage = [[(BIG, BIG, BIG), (NEG, NEG, NEG), (0, len(TAPS), WIDTH + 1), (BIG, 2, -1), (NEG, 1, BIG)],
               [(-1, 2, BIG), (1, 2, WIDTH), (NEG, 2, WIDTH), (BIG, 0, 5), (7, -2, 7)]]
    # what the header makes of them: a response that does not exist copies the row, out_len is clamped to 0 .. width
    tame = [[(BIG, -1, WIDTH), (NEG, -1, 0), (0, -1, WIDTH), (BIG, 2, 0), (NEG, 1, WIDTH)],
            [(-1, 2, WIDTH), (1, 2, WIDTH), (NEG, 2, WIDTH), (BIG, 0, 5), (7, -1, 7)]]
    for k, (wild, want_plans) in enumerate(zip(garbage, tame)):
        plans = torch.tensor([list(p) + [NEG] for p in wild], dtype=torch.int32).cuda()
        out = G.output((len(LENGTHS), WIDTH), torch.float32, align=16, phase=(phase + 12) % 16, name="out")
        _rows(src.ptr, case["offs"], case["lens"], plans, ws.data_ptr(), len(bank), out.ptr, WIDTH)
        want = crev.reverb_rows(case["data"], case["offs"], case["lens"], crev.plan_array(want_plans, len(TAPS), WIDTH), WIDTH, bank)
        G.check([src, out], {"out": out.view(torch.float32, len(LENGTHS), WIDTH)}, {"out": want}, f"cough_reverb_rows, garbage {k}")


@pytest.mark.parametrize("b", [1, 64, 65])
def test_draw_reverb_between_guards(b):
    lengths = [(977 * i) % 40000 for i in range(b)]
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    for phase in (0, 4, 8, 12):
        out = G.output((b, 4), torch.int32, align=16, phase=phase, name="plans")
        _lib.check_reverb(_lib.load_reverb().cough_draw_reverb(2**63 + 5, b, lens.data_ptr(), 0.5, 100, out.ptr, _st()),
                          "cough_draw_reverb")
        G.check([out], {"plans": out.view(torch.int32, b, 4)}, {"plans": torch.from_numpy(R.draw_reverb_ref(2**63 + 5, lengths, 0.5, 100))},
                "cough_draw_reverb")
