"""What the launches of the waveform chain read and wrote during one run, for ``chain_ref.check_trace``.

``recording()`` wraps the Python entry points of the chain's launches for the duration of a block -- ``warp.warp_rows``,
``pitch.stretch_rows``, ``reverb.reverb_rows``, ``AudioAugmentor._run`` and ``draws.augment_rows_drawn`` -- the way
``tests/test_gpu_reverb.py`` wraps ``reverb_rows``.  ``recording(channel=True)`` also wraps ``channel.channel_rows``, the
launch behind the augmentation kernel, as a link of kind ``channel``; it is off by default, so ``check_trace``'s callers
see the links in front of it and no other.  ``pitch_shift_rows`` stays as it is: its two launches appear as
``stretch`` and ``back``.  For every call it keeps host copies of the rows the call was given (cut out of ``src`` by its
offsets and lengths), the lengths, the plans read back from the device after the call, the records of the augmentation
link, and the output matrix -- a link in the form ``tests/chain_ref.py`` describes.  A plain helper, not a fixture.
"""
import contextlib

import numpy as np
import torch

from cough_detector_amd import channel as cch
from cough_detector_amd import draws as cdraws
from cough_detector_amd import pitch as cpitch
from cough_detector_amd import reverb as crev
from cough_detector_amd import warp as cwarp
from cough_detector_amd.augmentation import AudioAugmentor
import draws_ref as D

_STRETCH = np.dtype([("shift", np.int32), ("reserved", np.int32), ("rate", np.float64)])


def _host(t):
    return t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.array(t)


def _cut(src, offsets, lengths):
    flat = src.detach().reshape(-1)
    return [flat[o:o + max(n, 0)].cpu().numpy().copy() for o, n in zip(_host(offsets).tolist(), _host(lengths).tolist())]


def _bank(aug):
    host = aug._bank_host.numpy()
    return [host[o:o + n].copy() for o, n in zip(aug._bank_offsets, aug._bank_lengths)]


@contextlib.contextmanager
def recording(channel=False):
    """-> the list that receives one link per launch, in order, while the block runs.  ``channel``: record
    ``channel_rows`` too (its rows are cut out before the call: it may write in place)."""
    trace = []
    real = dict(warp=cwarp.warp_rows, stretch=cpitch.stretch_rows, reverb=crev.reverb_rows, run=AudioAugmentor._run,
                drawn=cdraws.augment_rows_drawn)

    def warp_rows(src, offsets, lengths, plans, n_samples, return_lengths=False):
        res = real["warp"](src, offsets, lengths, plans, n_samples, return_lengths)
        p = _host(plans).reshape(-1, 3)
        trace.append(dict(kind="back" if trace and trace[-1]["kind"] == "stretch" else "warp", rows=_cut(src, offsets, lengths),
                          lengths=_host(lengths).astype(np.int64), shift=p[:, 0].astype(np.int64),
                          param=[(int(o), int(m)) for _, o, m in p], out=_host(res[0] if return_lengths else res)))
        return res

    def stretch_rows(src, offsets, lengths, plans, n_samples, return_lengths=False):
        res = real["stretch"](src, offsets, lengths, plans, n_samples, return_lengths)
        p = np.frombuffer(_host(plans).tobytes(), dtype=_STRETCH)
        trace.append(dict(kind="stretch", rows=_cut(src, offsets, lengths), lengths=_host(lengths).astype(np.int64),
                          shift=p["shift"].astype(np.int64), param=[(float(r), int(m)) for r, m in zip(p["rate"], p["reserved"])],
                          out=_host(res[0] if return_lengths else res)))
        return res

    def reverb_rows(src, offsets, lengths, plans, width, bank):
        res = real["reverb"](src, offsets, lengths, plans, width, bank)
        p = _host(plans).reshape(-1, 4)
        trace.append(dict(kind="reverb", rows=_cut(src, offsets, lengths), lengths=_host(lengths).astype(np.int64),
                          shift=p[:, 0].astype(np.int64), param=[(int(k), int(m)) for _, k, m, _ in p], out=_host(res)))
        return res

    def run(self, x, clips, lengths, gaussian, seed):
        res = real["run"](self, x, clips, lengths, gaussian, seed)
        b, n = x.shape
        lens = np.asarray([int(v) for v in lengths] if lengths is not None else [n] * b, dtype=np.int64)
        xs = _host(x)
        records = np.frombuffer(b"".join(bytes(c) for c in clips), dtype=D.CLIP_DTYPE).copy()
        trace.append(dict(kind="augment", rows=[xs[r, :lens[r]].astype(np.float32) for r in range(b)], lengths=lens,
                          shift=records["shift"].astype(np.int64), param=[None] * b, out=_host(res), records=records,
                          gaussian=None if gaussian is None else _host(gaussian), bank=_bank(self)))
        return res

    def augment_rows_drawn(bank_data, offsets, lengths, n_samples, clips, aug, seed):
        res = real["drawn"](bank_data, offsets, lengths, n_samples, clips, aug, seed)
        records = np.frombuffer(_host(clips).tobytes(), dtype=D.CLIP_DTYPE).copy()
        trace.append(dict(kind="augment", rows=_cut(bank_data, offsets, lengths), lengths=_host(lengths).astype(np.int64),
                          shift=records["shift"].astype(np.int64), param=[None] * len(records), out=_host(res), records=records,
                          gaussian=None, bank=_bank(aug)))
        return res

    def channel_rows(packed, offsets, lengths, plans, width, bank, out=None):
        rows = _cut(packed, offsets, lengths)
        res = real["channel"](packed, offsets, lengths, plans, width, bank, out=out)
        p = np.ascontiguousarray(_host(plans)).view(np.int32).reshape(-1, 2)
        trace.append(dict(kind="channel", rows=rows, lengths=_host(lengths).astype(np.int64), shift=np.zeros(len(p), np.int64),
                          param=[(int(f), float(r)) for f, r in zip(p[:, 0], p[:, 1].copy().view(np.float32))], out=_host(res)))
        return res

    cwarp.warp_rows, cpitch.stretch_rows, crev.reverb_rows = warp_rows, stretch_rows, reverb_rows
    if channel:
        real["channel"], cch.channel_rows = cch.channel_rows, channel_rows
    AudioAugmentor._run, cdraws.augment_rows_drawn = run, augment_rows_drawn
    try:
        yield trace
    finally:
        cwarp.warp_rows, cpitch.stretch_rows, crev.reverb_rows = real["warp"], real["stretch"], real["reverb"]
        AudioAugmentor._run, cdraws.augment_rows_drawn = real["run"], real["drawn"]
        if channel:
            cch.channel_rows = real["channel"]
