"""What the restatements of the Small and Standard training steps share for max-pool windows (TEST INFRASTRUCTURE, not
product): a 2x2 floor max-pool whose backward winner can be overridden per window, the resolver that takes the choices a
float32 step cannot make reliably (ReLU inputs within rounding of 0, pool windows whose top two values lie within
rounding of each other) from that step's side, and the census of such windows that the tie tests assert on.

Why.  The input grid of the step tests makes the first pool's windows exact; every later pool sees values that float32
rounds, and a window whose top two values differ by less than that rounding routes its gradient to another pixel in
float64.  One such window moves a whole tensor's gradient by 1e-2 of its scale, exactly as a ReLU input at 1e-7 does.
Exact ties are never touched: first of equal values in scan order (dy * 2 + dx) is the rule under test.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

KINK = 1e-6             # the project's threshold: |ReLU input| < KINK, 0 < gap < KINK * max of a pool window
MAX_KEPT = 8            # a step that needs more changes than this is not a rounding matter
NOISE = 1e-12           # two float64 sums of the same terms in another order differ by 1e-16 .. 4e-13 of their value
GREY = 4e-6             # gaps of KINK .. GREY of the maximum: past the resolver, within float32's reach (grey_windows)


def windows(v: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) -> (B, C, H // 2, W // 2, 4): the 2x2 windows of a floor max-pool, in scan order dy * 2 + dx"""
    b, c, h, w = v.shape
    oh, ow = h // 2, w // 2
    return v[:, :, :oh * 2, :ow * 2].reshape(b, c, oh, 2, ow, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, oh, ow, 4)


def first_largest(win: torch.Tensor) -> torch.Tensor:
    """index (0..3) of the first largest value of every window, spelled out: no reliance on an argmax's tie rule"""
    eq = win == win.amax(dim=-1, keepdim=True)
    return ((eq.cumsum(dim=-1) == 1) & eq).to(torch.int64).argmax(dim=-1)


class MaxPool2(torch.autograd.Function):
    """F.max_pool2d(v, 2) whose backward routes each window's gradient to ``pick`` (B, C, H // 2, W // 2; int64) where
    that is >= 0 and to the first largest value in scan order elsewhere.  ``pick`` is read when backward runs, so an
    override set after the forward takes effect on the next backward of the same graph (as _Relu's ``flip``)."""

    @staticmethod
    def forward(ctx, v, pick):
        if v.shape[2] < 2 or v.shape[3] < 2:
            raise RuntimeError(f"max-pool of {tuple(v.shape)}: output size is too small")        # as F.max_pool2d
        win = windows(v)
        ctx.save_for_backward(first_largest(win))
        ctx.pick, ctx.shape = pick, v.shape
        return win.amax(dim=-1)

    @staticmethod
    def backward(ctx, g):
        first, = ctx.saved_tensors
        idx = torch.where(ctx.pick >= 0, ctx.pick, first)
        b, c, h, w = ctx.shape
        oh, ow = h // 2, w // 2
        gw = torch.zeros(b, c, oh, ow, 4, dtype=g.dtype).scatter_(-1, idx.unsqueeze(-1), g.unsqueeze(-1))
        out = torch.zeros(ctx.shape, dtype=g.dtype)
        out[:, :, :oh * 2, :ow * 2] = gw.reshape(b, c, oh, ow, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, oh * 2,
                                                                                                     ow * 2)
        return out, None


def pool(ref, v: torch.Tensor, name: str, relu: str = None) -> torch.Tensor:
    """``RefStep``'s max-pool: records the input as ``ref.pool_in[name]`` and a fresh ``ref.pick[name]`` (all -1).
    ``relu``: the name of the ReLU whose output ``v`` is, where the pool follows one directly (``ref.pool_of``)."""
    ref.pool_in[name] = v.detach()
    ref.pick[name] = torch.full((v.shape[0], v.shape[1], v.shape[2] // 2, v.shape[3] // 2), -1, dtype=torch.int64)
    if relu is not None:
        ref.pool_of[relu] = name
    return MaxPool2.apply(v, ref.pick[name])


def top_two(win: torch.Tensor):
    """(max, runner-up value, index of the first runner-up) of every window; the runner-up is the largest value at
    another position than the first largest (equal to the max in an exact tie)"""
    first = first_largest(win)
    rest = win.scatter(-1, first.unsqueeze(-1), float("-inf"))
    return win.amax(dim=-1), rest.amax(dim=-1), first_largest(rest)


def _gaps(v: torch.Tensor):
    top, second, where = top_two(windows(v))
    return top, top - second, where


def near_ties(v: torch.Tensor, kink: float = KINK) -> List[Tuple[float, tuple, int]]:
    """the windows of pool input ``v`` that a float32 step may decide the other way: positive maximum and
    NOISE * max <= max - runner-up < kink * max (below NOISE the two are one value: ``equal_up_to_rounding``).
    [(relative gap, window index, runner-up's position)]"""
    top, gap, where = _gaps(v)
    sel = (top > 0) & (gap >= NOISE * top) & (gap > 0) & (gap < kink * top)
    return [((gap[i] / top[i]).item(), i, int(where[i])) for i in map(tuple, sel.nonzero().tolist())]


def tie_census(v: torch.Tensor, kink: float = KINK) -> Dict[str, int]:
    """of the windows of pool input ``v`` with a positive maximum, by the gap between the top two values as a fraction
    of the maximum: ``exact`` 0, ``rounding`` (0, NOISE), ``near`` [NOISE, kink), ``grey`` [kink, GREY); ``positive`` is
    all of them"""
    top, gap, _ = _gaps(v)
    pos = top > 0
    band = lambda lo, hi: int((pos & (gap >= lo * top) & (gap < hi * top)).sum())
    return {"positive": int(pos.sum()), "exact": int((pos & (gap == 0)).sum()),
            "rounding": int((pos & (gap > 0) & (gap < NOISE * top)).sum()), "near": band(NOISE, kink),
            "grey": band(kink, GREY)}


def equal_up_to_rounding(ref) -> int:
    """Windows whose top values agree to NOISE of the maximum hold one value: the same sum, accumulated in another order
    at another pixel (a GEMM's edge tiles; which pixels differ depends on the CPU's vector width).  Float64 then routes
    by its own rounding, not by the rule.  This hands each such window of ``ref`` (after ``grads``) to the first of its
    equal values; returns how many windows that changed.  ``ref.regrad()`` gives the gradients."""
    changed = 0
    for name, v in ref.pool_in.items():
        win = windows(v)
        top = win.amax(dim=-1, keepdim=True)
        eq = win >= top * (1 - NOISE)
        first = ((eq.cumsum(dim=-1) == 1) & eq).to(torch.int64).argmax(dim=-1)
        move = (top.squeeze(-1) > 0) & (first != first_largest(win))
        ref.pick[name][move] = first[move]
        changed += int(move.sum())
    return changed


def grey_windows(ref) -> int:
    """How many windows of ``ref``'s pools past the first (after a forward) have a positive maximum and top two values
    KINK .. GREY of it apart.  The resolver does not touch them, yet float32 may decide them the other way where the
    pool input is a K-term dot product: its rounding is about sqrt(K) 2^-24 of the value, 2e-6 at Standard's last conv
    (K = 9 * 128 = 1152; 5e-7 at the Small net's widest, K = 9 + 64, which therefore needs no such rule), and GREY is
    two of those.  Measured on Standard batches of 12 to 21 clips: single windows of the last two pools 1.3e-6, 1.7e-6
    and 3.7e-6 apart each moved conv 0's weight gradient by 5e-4 .. 8e-3 of its scale, in the HIP step and (two of the
    three) in torch's own float32 step alike; with that one window taken the other way every tensor was within 2e-6.
    An input with such a window cannot tell a right kernel from a wrong one, so the Standard step tests draw another
    one (a rule on the restatement alone: nothing of the kernel's enters it).  A wider band is not practical: a draw of
    8 x 90 x 101 has about 0.3 such windows per 1e-6 of band, which is also why those tests keep B F T below 80,000.
    The first pool is not counted: the step tests make conv 0's outputs exact, the BatchNorm and ReLU after it are
    non-decreasing per channel in any arithmetic, so float32 cannot invert two of its inputs."""
    return sum(tie_census(v)["grey"] for v in list(ref.pool_in.values())[1:])


def choices_that_differ(a, b) -> set:
    """the discrete choices two ``RefStep`` runs of the same step (after ``grads``) took differently: ReLU inputs of
    different sign (``(name, index)``) and pool windows with different winners"""
    out = set()
    for name in a.pre:
        for idx in ((a.pre[name] > 0) != (b.pre[name] > 0)).nonzero().tolist():
            out.add((name, tuple(idx)))
    for name in a.pool_in:
        wa, wb = first_largest(windows(a.pool_in[name])), first_largest(windows(b.pool_in[name]))
        for idx in (wa != wb).nonzero().tolist():
            out.add((name, tuple(idx)))
    return out


def resolve(g, ref, rgrads, worst, kink=KINK, limit=64, rtol=1e-4, ties=False):
    """The resolver behind both nets' ``resolve_kinks``.  ``worst(g, rgrads)`` is the net's largest gradient error as a
    fraction of its tensor's scale.  Within ``rtol`` already: returns ``(rgrads, [])``, the same object.  Otherwise the
    candidates (ReLU inputs with |v| < kink and, with ``ties``, the ``near_ties`` of every pool) are tried on ``ref``
    (after ``grads``) one at a time in order of margin (|v|, relative gap) and kept where that lowers the worst error; a
    ReLU candidate flips the derivative, a pool candidate hands the window to its runner-up.  A ReLU input <= 0 whose
    output goes straight into a pool, in a window whose four outputs are all 0, is one choice with that window: taken
    as positive it is the window's largest, so the window goes to it with the flip (float64 gives such a window to its
    first pixel, where the flipped derivative would never be read).  Then every kept change is undone in turn and
    stays undone unless that makes the worst error larger: a change that only happened to lower the maximum while the
    real one was still missing does not survive.  Only the backward pass is touched.  Returns (gradients, kept changes
    as (name, index, ReLU input or relative gap))."""
    best = worst(g, rgrads)
    if best <= rtol:
        return rgrads, []
    # a candidate is (margin, what to report, [(table, name, index, value when on, value when off)])
    cand = []
    for name, v in ref.pre.items():
        for idx in map(tuple, (v.abs() < kink).nonzero().tolist()):
            acts = [(ref.flip, name, idx, True, False)]
            pn = ref.pool_of.get(name)
            if pn is not None and v[idx] <= 0:
                b, c, i, j = idx
                widx = (b, c, i // 2, j // 2)
                inside = widx[2] < ref.pick[pn].shape[2] and widx[3] < ref.pick[pn].shape[3]
                # taken as positive, this value is the largest of a window whose other ReLU outputs are all 0
                if inside and windows(ref.pool_in[pn])[widx].max() == 0:
                    acts.append((ref.pick, pn, widx, (i % 2) * 2 + j % 2, -1))
            cand.append((abs(v[idx].item()), (name, idx, v[idx].item()), acts))
    if ties:
        for name, v in ref.pool_in.items():
            for rel, idx, runner in near_ties(v, kink):
                cand.append((rel, (name, idx, rel), [(ref.pick, name, idx, runner, -1)]))
    cand.sort(key=lambda c: c[0])

    def put(acts, on):
        for table, name, idx, yes, no in acts:
            table[name][idx] = yes if on else no

    kept = []
    for _, what, acts in cand[:limit]:
        put(acts, True)
        trial = ref.regrad()
        w = worst(g, trial)
        if w < best:
            best, rgrads = w, trial
            kept.append((what, acts))
            if best <= rtol:
                break
        else:
            put(acts, False)
    for change in list(kept) if len(kept) > 1 else []:
        put(change[1], False)
        trial = ref.regrad()
        w = worst(g, trial)
        if w <= best:
            best, rgrads = w, trial
            kept.remove(change)
        else:
            put(change[1], True)
    return rgrads, [what for what, _ in kept]
