"""Guard zones and poisoned workspaces for calls into the C ABI.

``torch.empty`` rounds every request up and carves it from large segments, so a store a few floats past an output, a load
past an input's last element or a workspace region that runs past ``*_workspace_bytes`` lands in slack or in a neighbour
and no parity test sees it.  Here every buffer a call receives lies inside one flat allocation the test owns::

    [ guard >= 64 KiB | region (exactly nbytes) | guard >= 64 KiB ]

both guards filled with ``GUARD_WORD``, a NaN bit pattern no kernel produces.  A stray store changes a guard word; a stray
load returns NaN, which shows in what it feeds.  The helper is device-agnostic (``"cuda"`` and ``"cpu"`` tensors):
``tests/test_guarded_host.py`` runs it on the CPU against small numpy "kernels" with planted defects, the GPU suites run the
HIP kernels between the same zones and through the same ``check``.

64 KiB per side is a condition, not a measurement: it is more than any single tile or row these kernels store, so a stray
access of one tile or row stays inside memory the test owns.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional

import torch

GUARD_WORD = 0x7FA5A5A5           # a NaN as float32 (tests/test_gpu_adamw.py uses the same pattern)
GUARD_BYTES = 64 * 1024           # on each side, at least
FILLS = ("zeros", "ones_bits", "stale")

_VIEWS = {"float32": torch.float32, "int32": torch.int32, "int64": torch.int64, "float64": torch.float64}


class Guarded:
    """``nbytes`` bytes between two guard zones, in one flat allocation.  The region starts at an address that is a
    multiple of ``align`` -- an odd multiple, so it is aligned to ``align`` and to nothing larger -- plus ``phase`` bytes,
    and the trailing guard begins at the very next byte after it.  ``nbytes``, ``align`` and ``phase`` are multiples
    of 4: everything guarded here is made of 4- and 8-byte elements, and the guards are compared word by word."""

    def __init__(self, nbytes: int, align: int = 256, phase: int = 0, device="cuda", name: str = ""):
        nbytes, align, phase = int(nbytes), int(align), int(phase)
        if nbytes < 0 or nbytes % 4 or align < 4 or align & (align - 1) or phase % 4 or not 0 <= phase < align:
            raise ValueError(f"Guarded: nbytes={nbytes}, align={align}, phase={phase}")
        self.nbytes, self.align, self.phase, self.name = nbytes, align, phase, name
        total = GUARD_BYTES + 4 * align + nbytes + GUARD_BYTES
        self.raw = torch.full((total // 4,), GUARD_WORD, dtype=torch.int32, device=device)
        base = self.raw.data_ptr()
        assert base % 4 == 0
        start = -(-(base + GUARD_BYTES) // (2 * align)) * (2 * align) + align + phase
        self.first = (start - base) // 4                      # word index of the region in raw
        self.words = nbytes // 4
        assert self.first * 4 >= GUARD_BYTES and (self.raw.numel() - self.first - self.words) * 4 >= GUARD_BYTES
        assert (self.ptr - phase) % align == 0 and (self.ptr - phase) % (2 * align) == align

    # ------------------------------------------------------------------ the region
    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + 4 * self.first

    @property
    def region(self) -> torch.Tensor:
        """The region as int32 words (a view)."""
        return self.raw[self.first:self.first + self.words]

    def view(self, dtype, *shape) -> torch.Tensor:
        """The region as ``dtype`` (``torch.float32`` / ``int32`` / ``int64`` / ``float64`` or their names), reshaped."""
        dtype = _VIEWS[dtype] if isinstance(dtype, str) else dtype
        if dtype not in _VIEWS.values():
            raise ValueError(f"Guarded.view: {dtype}")
        t = self.region.view(dtype)
        return t.view(*shape) if shape else t

    float32 = property(lambda self: self.view(torch.float32))
    int32 = property(lambda self: self.view(torch.int32))
    int64 = property(lambda self: self.view(torch.int64))
    float64 = property(lambda self: self.view(torch.float64))

    # ------------------------------------------------------------------ fills (of the region only)
    def fill(self, kind: str) -> "Guarded":
        """``zeros``; ``ones_bits``: every byte 0xFF -- a NaN as f32, bf16 and f64 and -1 at every integer width, so an
        index read before it is written points just in front of its base, into the leading guard, not far away;
        ``stale``: left as it is (whatever an earlier call wrote)."""
        if kind == "zeros":
            self.region.zero_()
        elif kind == "ones_bits":
            self.region.fill_(-1)
        elif kind != "stale":
            raise ValueError(f"Guarded.fill: {kind!r}")
        return self

    @classmethod
    def holding(cls, tensor: torch.Tensor, align: int = 16, phase: int = 0, name: str = "") -> "Guarded":
        """A copy of an INPUT (float data only: waveforms, images, banks, probabilities, energies) whose last element is
        flush against the trailing guard: a load past its end returns NaN.  Index, length, offset and record arrays stay
        in ordinary tensors -- a stray read of a huge integer would send a later access far away."""
        if not tensor.dtype.is_floating_point or tensor.dtype not in _VIEWS.values():
            raise ValueError(f"Guarded.holding takes float32 / float64 data, got {tensor.dtype}")
        t = tensor.detach().contiguous()
        g = cls(t.numel() * t.element_size(), align, phase, device=t.device, name=name)
        g.view(t.dtype).copy_(t.reshape(-1))
        return g

    # ------------------------------------------------------------------ the guards
    def intact(self) -> Optional[str]:
        """None while both guard zones hold ``GUARD_WORD`` in every word; otherwise a description of the first changed
        word: its byte offset relative to the region's start (negative: in front of it) and what it holds."""
        lo, hi = self.raw[:self.first], self.raw[self.first + self.words:]
        for zone, words, origin in (("leading", lo, -4 * self.first), ("trailing", hi, self.nbytes)):
            bad = torch.nonzero(words != GUARD_WORD)
            if bad.numel():
                k = int(bad[0])
                at = origin + 4 * k
                rel = f"{-at} bytes before the region" if at < 0 else f"{at - self.nbytes} bytes past the region's end"
                return (f"{self.name or 'buffer'}: {zone} guard changed at byte offset {at} ({rel}; {int(bad.numel())} "
                        f"words changed in that zone), it holds 0x{int(words[k]) & 0xFFFFFFFF:08X}")
        return None


def output(shape, dtype=torch.float32, align: Optional[int] = None, phase: int = 0, device="cuda", name: str = "") -> Guarded:
    """A guarded OUTPUT of ``shape`` elements of ``dtype``; ``align`` defaults to the element size (no more than the
    type itself needs).  It starts out holding ``GUARD_WORD`` everywhere, so an output nothing wrote fails ``check``."""
    size = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)):
        n *= int(s)
    return Guarded(n * size, max(size, 4) if align is None else align, phase, device=device, name=name)


def workspaces(nbytes: int, leave_stale: Callable[[Guarded], List[Guarded]], device="cuda"):
    """One guarded 256-byte aligned workspace of exactly ``nbytes`` per fill: yields ``(fill, workspace, more guards)``.
    For ``stale``, ``leave_stale(workspace)`` runs a DIFFERENT earlier call on it (``run_other``) and returns the guards
    that call used besides."""
    for fill in FILLS:
        ws = Guarded(nbytes, 256, device=device, name=f"workspace ({fill})")
        more = []
        if fill == "stale":
            ws.fill("ones_bits")
            more = leave_stale(ws)
        else:
            ws.fill(fill)
        yield fill, ws, more


def run_other(ws: Guarded, other_bytes: int, call: Callable[[int, int], None]) -> List[Guarded]:
    """Leave in ``ws`` what ``call(workspace pointer, workspace bytes)`` -- a call of another batch size that needs
    ``other_bytes`` -- leaves behind.  A call that fits runs through ``ws`` itself; a larger one runs in a guarded
    workspace of its own size whose leading ``ws.nbytes`` bytes are then copied over (same stream): either way ``ws`` holds
    another call's values at the addresses the call under test is about to use."""
    if other_bytes <= ws.nbytes:
        call(ws.ptr, other_bytes)
        return []
    tmp = Guarded(other_bytes, 256, device=ws.raw.device, name="the other call's workspace").fill("ones_bits")
    call(tmp.ptr, other_bytes)
    ws.region.copy_(tmp.region[:ws.words])
    return [tmp]


def _words(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous().reshape(-1)
    if t.element_size() not in (4, 8):
        raise ValueError(f"check: {t.dtype} outputs are not compared here")
    return t.view(torch.int32)


def _elements(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def check(guards: Iterable[Guarded], got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], what: str = "") -> None:
    """The one assertion every guarded run ends with: every guard zone of ``guards`` is intact, no output of ``got`` holds
    ``GUARD_WORD``, and every output of ``got`` is bit-equal to the one of the same name in ``want`` (compared through
    ``view(torch.int32)`` / ``view(torch.int64)``; no tolerance).  ``got`` and ``want`` must name the same outputs."""
    tag = f"{what}: " if what else ""
    for g in guards:
        msg = g.intact()
        assert msg is None, f"{tag}{msg}"
    assert set(got) == set(want) and got, f"{tag}outputs {sorted(got)} against {sorted(want)}"
    for name, t in got.items():
        w = _words(t)
        hit = torch.nonzero(w == GUARD_WORD)
        assert hit.numel() == 0, (f"{tag}output {name!r} holds GUARD_WORD at word {int(hit[0]) if hit.numel() else -1} "
                                  f"({int(hit.numel())} words): something read a guard zone")
    for name, t in got.items():
        r = want[name]
        assert tuple(t.shape) == tuple(r.shape) and t.dtype == r.dtype, \
            f"{tag}output {name!r}: {tuple(t.shape)} {t.dtype} against {tuple(r.shape)} {r.dtype}"
        a, b = _elements(t), _elements(r).to(t.device)
        diff = torch.nonzero(a != b)
        if diff.numel():
            k = int(diff[0])
            raise AssertionError(f"{tag}output {name!r} differs in {int(diff.numel())} of {a.numel()} elements, first at "
                                 f"element {k}: 0x{int(a[k]) & (2 ** (8 * a.element_size()) - 1):X} against "
                                 f"0x{int(b[k]) & (2 ** (8 * b.element_size()) - 1):X}")
