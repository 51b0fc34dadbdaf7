"""``tests/guarded.py`` on CPU tensors: the checker the GPU guard suites end with does fail when it should.

A "kernel" here is a numpy function that gets what a HIP kernel gets -- the process's flat memory and addresses into it
(the whole allocation of each buffer as a float32 array plus the word index its region starts at) -- so it can reach
outside its buffers exactly as a kernel can.  The operation: ``ws[i] = 2 * x[i]`` into the workspace, then
``out[i] = ws[i] + 1``.  One kernel is correct; four carry the defects the guards exist for.  Planted defects live in this
file and nowhere else."""
import numpy as np
import pytest
import torch

import guarded as G
from guarded import Guarded

N = 37


def _mem(g: Guarded):
    return g.raw.numpy().view(np.float32), g.first


def k_correct(x, ws, out, n):
    (xm, x0), (wm, w0), (om, o0) = x, ws, out
    wm[w0:w0 + n] = 2 * xm[x0:x0 + n]
    om[o0:o0 + n] = wm[w0:w0 + n] + 1


def k_writes_before(x, ws, out, n):
    k_correct(x, ws, out, n)
    out[0][out[1] - 1] = 0.0


def k_writes_after(x, ws, out, n):
    k_correct(x, ws, out, n)
    out[0][out[1] + n] = 0.0


def k_reads_past_input(x, ws, out, n):
    """The last element comes from x[n] (an off-by-one of the tail)."""
    k_correct(x, ws, out, n)
    (xm, x0), (wm, w0), (om, o0) = x, ws, out
    om[o0 + n - 1] = xm[x0 + n]


def k_reads_workspace_first(x, ws, out, n):
    """The last workspace element is never written, but read."""
    (xm, x0), (wm, w0), (om, o0) = x, ws, out
    wm[w0:w0 + n - 1] = 2 * xm[x0:x0 + n - 1]
    om[o0:o0 + n] = wm[w0:w0 + n] + 1


X = torch.arange(1, N + 1, dtype=torch.float32) / 8
WANT = {"out": 2 * X + 1}


def run(kernel, fill="ones_bits", phase=0, stale_from=None):
    """One guarded run of ``kernel``; returns (guards, outputs)."""
    x = Guarded.holding(X, align=16, phase=phase, name="x")
    out = Guarded(4 * N, align=16, phase=phase, device="cpu", name="out")
    ws = Guarded(4 * N, align=256, device="cpu", name="ws")
    if fill == "stale":
        ws.fill("ones_bits")
        k_correct(_mem(Guarded.holding(-X, name="other x")), _mem(ws), _mem(Guarded(4 * N, 16, device="cpu")), N - 5)
    ws.fill(fill)
    with np.errstate(invalid="ignore"):
        kernel(_mem(x), _mem(ws), _mem(out), N)
    return [x, out, ws], {"out": out.float32.clone()}


def test_layout_alignment_and_views():
    for align, phase in ((4, 0), (16, 0), (16, 4), (16, 8), (16, 12), (256, 0), (8, 4)):
        g = Guarded(40, align, phase, device="cpu")
        assert (g.ptr - phase) % align == 0 and (g.ptr - phase) % (2 * align) == align      # align, and no more
        assert g.first * 4 >= G.GUARD_BYTES and (g.raw.numel() - g.first - g.words) * 4 >= G.GUARD_BYTES
        assert g.region.data_ptr() == g.ptr and g.region.numel() * 4 == 40
        assert g.raw[g.first + g.words:].data_ptr() == g.ptr + 40       # the trailing guard begins at the next byte
        assert g.intact() is None
    g = Guarded(48, 8, 0, device="cpu")
    assert g.float32.numel() == g.int32.numel() == 12 and g.int64.numel() == g.float64.numel() == 6
    assert g.int64.data_ptr() == g.ptr and g.view("float32", 3, 4).shape == (3, 4)
    g.fill("ones_bits")
    assert bool(torch.isnan(g.float32).all()) and bool(torch.isnan(g.float64).all())
    assert bool((g.int32 == -1).all()) and bool((g.int64 == -1).all())
    assert bool(torch.isnan(g.region.view(torch.bfloat16)).all()) and g.intact() is None
    g.fill("zeros")
    assert not g.float32.any() and g.intact() is None
    assert np.isnan(np.array([G.GUARD_WORD], np.uint32).view(np.float32)[0])
    with pytest.raises(ValueError):
        Guarded(6, 16, device="cpu")
    with pytest.raises(ValueError):
        Guarded.holding(torch.zeros(4, dtype=torch.int64))


def test_holding_puts_the_last_element_against_the_guard():
    x = Guarded.holding(X.view(1, N), align=16, phase=4)
    mem, first = _mem(x)
    assert np.array_equal(mem[first:first + N], X.numpy())
    assert mem[first + N:first + N + 1].view(np.uint32)[0] == G.GUARD_WORD
    assert mem[first - 1:first].view(np.uint32)[0] == G.GUARD_WORD
    e = Guarded.holding(torch.arange(5, dtype=torch.float64), align=8)
    assert e.float64.tolist() == [0, 1, 2, 3, 4] and e.nbytes == 40


@pytest.mark.parametrize("fill", G.FILLS)
@pytest.mark.parametrize("phase", (0, 4, 8, 12))
def test_the_correct_kernel_passes(fill, phase):
    guards, got = run(k_correct, fill, phase)
    G.check(guards, got, WANT, "correct")


def test_a_write_one_element_before_the_region_is_reported():
    guards, got = run(k_writes_before)
    with pytest.raises(AssertionError, match=r"out: leading guard changed at byte offset -4 \(4 bytes before the region"):
        G.check(guards, got, WANT)


def test_a_write_one_element_after_the_region_is_reported():
    guards, got = run(k_writes_after)
    with pytest.raises(AssertionError, match=rf"out: trailing guard changed at byte offset {4 * N} \(0 bytes past"):
        G.check(guards, got, WANT)


def test_a_read_one_element_past_a_flush_input_is_reported():
    guards, got = run(k_reads_past_input)
    with pytest.raises(AssertionError, match=rf"output 'out' holds GUARD_WORD at word {N - 1} "):
        G.check(guards, got, WANT)


@pytest.mark.parametrize("fill", G.FILLS)
def test_a_workspace_read_before_it_is_written_is_reported(fill):
    """Under every fill the element fed by the unwritten word differs from the normal run's (zeros: 1, ones_bits: NaN,
    stale: what the other call left)."""
    guards, got = run(k_reads_workspace_first, fill)
    with pytest.raises(AssertionError, match=rf"output 'out' differs in 1 of {N} elements, first at element {N - 1}:"):
        G.check(guards, got, WANT)


def test_a_run_that_launched_nothing_is_reported():
    guards, got = run(lambda *a: None)
    with pytest.raises(AssertionError, match="output 'out' holds GUARD_WORD at word 0"):
        G.check(guards, got, WANT)
    with pytest.raises(AssertionError, match="outputs"):
        G.check(guards, {}, WANT)
