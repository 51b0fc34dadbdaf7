"""The data-side entry points between guard zones (``tests/guarded.py``): waveform augmentation (host and device
records), the row kernels that align float4 stores on the destination with a scalar head and tail (``cough_gather_rows``,
``cough_prepare_rows``, ``cough_copy_segments``, ``cough_mask_images``), the frame energies and the segment picker, and the
short scalar-store kernels around them.

Float inputs are held flush against a trailing guard at 4-byte alignment (these headers ask for no more; float64 and
int64 arrays 8), outputs are guarded regions -- at all four 4-byte phases of a 16-byte line where the header promises
alignment independence -- and workspaces are guarded regions of exactly ``*_workspace_bytes`` under the three fills.  Index,
length, offset and record arrays stay in ordinary tensors.  Every output must be bit-equal to the normal path: the Python
wrapper where there is one that makes the same call, otherwise the same call on ordinary ``torch.empty`` tensors; the
copy kernels are also held to the copy they stand for, written with torch indexing."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as G
from cough_detector_amd import _lib, draws, segments
from cough_detector_amd.augmentation import AudioAugmentor
from cough_detector_amd.data import DeviceClipBank
from guarded import Guarded

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
LENS = (1, 3, 4, 5, 1023, 16001)
PHASES = (0, 4, 8, 12)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.4


def _dev(values, dtype):
    return torch.tensor(list(values), dtype=dtype, device="cuda")


def _packed(lengths, first=3, gap=1, seed=0):
    """Rows of ``lengths`` packed into one float32 buffer with rows at odd element offsets (4-byte alignment only),
    the last row ending on the buffer's last element; -> (buffer, offsets)."""
    offs, at = [], first
    for n in lengths:
        offs.append(at)
        at += n + gap
    return _rand(at - gap, seed=seed), offs


# ------------------------------------------------------------------ waveform augmentation
def _bank():
    g = torch.Generator().manual_seed(11)
    return [torch.randn((1, 700), generator=g) * 0.3, torch.randn((1, 9000), generator=g)]


def _augmentor():
    aug = AudioAugmentor(p_augment=1.0)
    aug.noise_samples = _bank()
    aug._pack_bank()
    return aug


def _record(kind: int, length: int, entry: int) -> _lib.CoughAugClip:
    """kind 0: gauss only, 1: bank only, 2: both, 3: neither -- each with a shift and a gain where the row allows one"""
    c = _lib.CoughAugClip(shift=0, gain=1.0, gaussian=0, bank_index=-1, gaussian_snr_db=0.0, bank_snr_db=0.0, bank_start=0)
    c.shift = (length // 7) * (1 if kind % 2 else -1)
    c.gain = 0.8 + 0.1 * kind
    if kind in (0, 2):
        c.gaussian, c.gaussian_snr_db = 1, 12.5 + kind
    if kind in (1, 2):
        bl = (700, 9000)[entry]
        rep = bl if bl >= length else (length // bl + 1) * bl
        c.bank_index, c.bank_snr_db, c.bank_start = entry, 7.0 + kind, rep - length     # the last admissible start: wraps
    return c


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("n", [4000, 16257], ids=["staged_4000", "multi_pass_16257"])
def test_augment_waveforms(n, noise):
    aug = _augmentor()
    lib = _lib.load()
    lengths = [n, 1, 701]
    b = len(lengths)
    x = _rand(b, n, seed=n)
    z = _rand(b, n, seed=n + 1) if noise == "host" else None
    bank_dev = aug._bank_device(torch.device("cuda", torch.cuda.current_device()))
    nb = len(aug._bank_lengths)
    offs, blen = (C.c_longlong * nb)(*aug._bank_offsets), (C.c_int * nb)(*aug._bank_lengths)
    need = lib.cough_augment_workspace_bytes(b)
    other_need = lib.cough_augment_workspace_bytes(1)
    assert need > 0 and other_need > 0
    other_x = _rand(1, n, seed=5)
    other_x[0, n // 2] = float("nan")
    other_x, other_out = Guarded.holding(other_x.cuda(), 4), torch.empty((1, n), device="cuda")

    def call(src, bb, out_ptr, lens, recs, zz, p, nbytes):
        _lib.check(lib.cough_augment_waveforms(
            src.ptr, n, out_ptr, bb, n, (C.c_int * bb)(*lens), (_lib.CoughAugClip * bb)(*recs), bank.ptr, bank_dev.numel(), offs,
            blen, nb, None if zz is None else zz.ptr, 99, p, nbytes, _stream()), "cough_augment_waveforms")

    for rot in range(4):                       # every row takes every kind: gauss only, bank only, both, neither
        recs = [_record((i + rot) % 4, lengths[i], (i + rot) % 2) for i in range(b)]
        want = {"out": aug._run(x.cuda(), recs, lengths, None if z is None else z.cuda(), 99)}
        bank = Guarded.holding(bank_dev, 4, name="d_bank")

        def stale(ws):
            return G.run_other(ws, other_need, lambda p, nbytes: call(other_x, 1, other_out.data_ptr(), [n], [_record(2, n, 0)],
                                                                      None, p, nbytes))
        for fill, ws, more in G.workspaces(need, stale):
            src = Guarded.holding(x.cuda(), 4, name="d_in")
            zz = None if z is None else Guarded.holding(z.cuda(), 4, name="d_gaussian")
            out = G.output((b, n), name="d_out")
            call(src, b, out.ptr, lengths, recs, zz, ws.ptr, need)
            torch.cuda.synchronize()
            G.check([src, out, bank, ws] + more + ([zz] if zz else []), {"out": out.float32.view(b, n)}, want,
                    f"cough_augment_waveforms n={n} rotation {rot} workspace {fill}")


@pytest.mark.parametrize("n", [4000, 16257], ids=["staged_4000", "multi_pass_16257"])
def test_augment_rows_drawn(n):
    aug = _augmentor()
    lib = _lib.load_draws()
    dev = torch.device("cuda", torch.cuda.current_device())
    lengths = [n, 1, 701]
    b = len(lengths)
    data, row_offs = _packed(lengths, seed=n)
    data = data.cuda()
    offs_dev, lens_dev = _dev(row_offs, I64), _dev(lengths, I32)
    bank_dev = aug._bank_device(dev)
    boffs, blens = aug._bank_tables_device(dev)
    nb = len(aug._bank_lengths)
    need = lib.cough_augment_rows_drawn_workspace_bytes(b)
    other_need = lib.cough_augment_rows_drawn_workspace_bytes(1)
    assert need > 0 and other_need > 0 and draws.CLIP_BYTES == C.sizeof(_lib.CoughAugClip)
    other = torch.full((n,), float("nan"))
    other[1:] = _rand(n - 1, seed=8)
    other, other_out = Guarded.holding(other.cuda(), 4), torch.empty((1, n), device="cuda")

    def records(recs):
        raw = bytes((_lib.CoughAugClip * len(recs))(*recs))
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()

    def call(src, offs, lens, bb, recs_dev, out_ptr, p, nbytes):
        _lib.check_draws(lib.cough_augment_rows_drawn(
            src.ptr, offs.data_ptr(), lens.data_ptr(), bb, n, recs_dev.data_ptr(), bank.ptr, bank_dev.numel(), boffs.data_ptr(),
            blens.data_ptr(), nb, 2027, out_ptr, p, nbytes, _stream()), "cough_augment_rows_drawn")

    other_recs, other_offs, other_lens = records([_record(2, n, 1)]), _dev([0], I64), _dev([n], I32)
    for rot in range(4):
        recs_dev = records([_record((i + rot) % 4, lengths[i], (i + rot) % 2) for i in range(b)])
        want = {"out": draws.augment_rows_drawn(data, offs_dev, lens_dev, n, recs_dev, aug, 2027)}
        bank = Guarded.holding(bank_dev, 4, name="d_bank")

        def stale(ws):
            return G.run_other(ws, other_need, lambda p, nbytes: call(other, other_offs, other_lens, 1, other_recs,
                                                                      other_out.data_ptr(), p, nbytes))
        for fill, ws, more in G.workspaces(need, stale):
            src = Guarded.holding(data, 4, name="d_src")
            out = G.output((b, n), name="d_out")
            call(src, offs_dev, lens_dev, b, recs_dev, out.ptr, ws.ptr, need)
            torch.cuda.synchronize()
            G.check([src, out, bank, ws] + more, {"out": out.float32.view(b, n)}, want,
                    f"cough_augment_rows_drawn n={n} rotation {rot} workspace {fill}")


# ------------------------------------------------------------------ float4 stores aligned on the destination
@pytest.mark.parametrize("row_len", LENS)
def test_gather_rows_every_output_phase(row_len):
    lib = _lib.load_data()
    lengths = [n for n in LENS if n <= row_len] + [row_len]
    b = len(lengths)
    data, offs = _packed(lengths, seed=row_len)
    offs_dev, lens_dev = _dev(offs, I64), _dev(lengths, I32)
    exact = torch.zeros(b, row_len)
    for r, (o, n) in enumerate(zip(offs, lengths)):
        exact[r, :n] = data[o:o + n]

    def call(src_ptr, out_ptr):
        _lib.check_data(lib.cough_gather_rows(src_ptr, offs_dev.data_ptr(), lens_dev.data_ptr(), b, out_ptr, row_len, row_len,
                                              _stream()), "cough_gather_rows")
    plain_src, plain = data.cuda(), torch.empty((b, row_len), device="cuda")
    call(plain_src.data_ptr(), plain.data_ptr())
    assert torch.equal(plain.cpu(), exact)
    for phase in PHASES:
        src, out = Guarded.holding(data.cuda(), 4, name="d_src"), G.output((b, row_len), align=16, phase=phase, name="d_out")
        call(src.ptr, out.ptr)
        torch.cuda.synchronize()
        G.check([src, out], {"out": out.float32.view(b, row_len)}, {"out": plain}, f"cough_gather_rows phase {phase}")


@pytest.mark.parametrize("out_len", LENS)
def test_prepare_rows_every_output_phase(out_len):
    lib = _lib.load_data()
    lengths = list(LENS)                       # shorter rows are padded, longer ones centre-trimmed
    b = len(lengths)
    data, offs = _packed(lengths, seed=out_len + 1)
    offs_dev, lens_dev = _dev(offs, I64), _dev(lengths, I32)

    def call(src_ptr, out_ptr, flags):
        _lib.check_data(lib.cough_prepare_rows(src_ptr, offs_dev.data_ptr(), lens_dev.data_ptr(), b, out_ptr, out_len, flags,
                                               _stream()), "cough_prepare_rows")
    for flags in (_lib.PREP_NORMALIZE, 0):
        plain_src, plain = data.cuda(), torch.empty((b, out_len), device="cuda")
        call(plain_src.data_ptr(), plain.data_ptr(), flags)
        if not flags:                          # without the division: a centre trim / symmetric pad, exactly
            exact = torch.zeros(b, out_len)
            for r, (o, n) in enumerate(zip(offs, lengths)):
                if n >= out_len:
                    s = (n - out_len) // 2
                    exact[r] = data[o + s:o + s + out_len]
                else:
                    left = (out_len - n) // 2
                    exact[r, left:left + n] = data[o:o + n]
            assert torch.equal(plain.cpu(), exact)
        for phase in PHASES:
            src = Guarded.holding(data.cuda(), 4, name="d_src")
            out = G.output((b, out_len), align=16, phase=phase, name="d_out")
            call(src.ptr, out.ptr, flags)
            torch.cuda.synchronize()
            G.check([src, out], {"out": out.float32.view(b, out_len)}, {"out": plain},
                    f"cough_prepare_rows flags {flags} phase {phase}")


def test_copy_segments_every_output_phase():
    lib = _lib.load_segments()
    lengths = list(LENS)
    b = len(lengths)
    starts = [0, 2, 1, 0, 5, 3]                                     # a row is read at its clip's offset + start
    data, offs = _packed([n + s for n, s in zip(lengths, starts)], seed=17)
    dst_offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()        # packed: the rows of dst start anywhere
    total = sum(lengths)
    src_offs_dev, dst_offs_dev = _dev(offs, I64), _dev(dst_offs, I64)
    starts_dev, lens_dev = _dev(starts, I32), _dev(lengths, I32)
    exact = torch.cat([data[o + s:o + s + n] for o, s, n in zip(offs, starts, lengths)])

    def call(src_ptr, dst_ptr, max_len):
        _lib.check_segments(lib.cough_copy_segments(src_ptr, src_offs_dev.data_ptr(), starts_dev.data_ptr(), lens_dev.data_ptr(),
                                                    dst_offs_dev.data_ptr(), b, max_len, dst_ptr, _stream()),
                            "cough_copy_segments")
    for max_len in (max(lengths), 1023):       # 1023: the grid is sized for less than the longest row, which is still whole
        plain_src, plain = data.cuda(), torch.empty(total, device="cuda")
        call(plain_src.data_ptr(), plain.data_ptr(), max_len)
        assert torch.equal(plain.cpu(), exact)
        for phase in PHASES:
            src, dst = Guarded.holding(data.cuda(), 4, name="d_src"), G.output((total,), align=16, phase=phase, name="d_dst")
            call(src.ptr, dst.ptr, max_len)
            torch.cuda.synchronize()
            G.check([src, dst], {"dst": dst.float32}, {"dst": plain}, f"cough_copy_segments max_len {max_len} phase {phase}")


@pytest.mark.parametrize("width", LENS)
def test_mask_images_every_output_phase(width):
    lib = _lib.load_data()
    height = 3
    for n_img in (1, 3):
        x = _rand(n_img, height, width, seed=width + n_img)
        # per image: a frequency mask (row 1), a time mask over the row's tail, an empty one and one of no usable axis
        axis = _dev([0, 1, 1, 7] * n_img, I32)
        start = _dev([1, max(width - 3, 0), 2, 0] * n_img, I32)
        end = _dev([2, width, 2, 1] * n_img, I32)
        exact = x.clone()
        exact[:, 1, :] = 0
        exact[:, :, max(width - 3, 0):] = 0

        def call(in_ptr, out_ptr):
            _lib.check_data(lib.cough_mask_images(in_ptr, out_ptr, n_img, height, width, 4, axis.data_ptr(), start.data_ptr(),
                                                  end.data_ptr(), _stream()), "cough_mask_images")
        plain_in, plain = x.cuda(), torch.empty((n_img, height, width), device="cuda")
        call(plain_in.data_ptr(), plain.data_ptr())
        assert torch.equal(plain.cpu(), exact)
        for phase in PHASES:
            src = Guarded.holding(x.cuda(), 16, phase, name="d_in")
            out = G.output(x.shape, align=16, phase=phase, name="d_out")
            call(src.ptr, out.ptr)
            torch.cuda.synchronize()
            G.check([src, out], {"out": out.float32.view(x.shape)}, {"out": plain}, f"cough_mask_images phase {phase}")
            call(src.ptr, src.ptr)             # in place
            torch.cuda.synchronize()
            G.check([src], {"out": src.float32.view(x.shape)}, {"out": plain}, f"cough_mask_images in place, phase {phase}")


# ------------------------------------------------------------------ frame energies and the segment picker
CLIP_LENGTHS = (1, 399, 400, 561)


def _tiles(lengths, frame_length, hop_length):
    """The frame offsets and (clip, first frame) tiles ``segments._frame_energy`` builds."""
    frames = segments.frame_counts(np.asarray(lengths), frame_length, hop_length)
    frame_offsets = np.concatenate([[0], np.cumsum(frames, dtype=np.int64)]).astype(np.int64)
    tile_frames = _lib.load_segments().cough_frame_energy_tile_frames(frame_length, hop_length)
    assert tile_frames >= 1
    tiles = [(k, f) for k, nf in enumerate(frames) for f in range(0, int(nf), tile_frames)]
    return frame_offsets, np.asarray(tiles, dtype=np.int32)


@pytest.mark.parametrize("frame_length,hop_length", [(400, 160), (7, 3)])
def test_frame_energy_and_pick_segments(frame_length, hop_length):
    lib = _lib.load_segments()
    clips = [_rand(n, seed=n) * (1.0 + torch.sin(torch.arange(n) / 40.0) ** 2) for n in CLIP_LENGTHS]
    bank = DeviceClipBank(clips, [0] * len(clips))
    n = len(clips)
    want_energy, host_offsets = segments.frame_energy(bank, frame_length, hop_length)
    frame_offsets, tiles = _tiles(CLIP_LENGTHS, frame_length, hop_length)
    assert np.array_equal(frame_offsets, host_offsets.numpy())
    offs_dev, tiles_dev = torch.from_numpy(frame_offsets).cuda(), torch.from_numpy(tiles.reshape(-1)).cuda()
    n_frames = int(frame_offsets[-1])
    for phase in (0, 8):                       # float64: both 8-byte phases of a 16-byte line
        data = Guarded.holding(bank.data, 4, name="d_bank")       # the last clip ends on the bank's last element
        energy = G.output((n_frames,), F64, align=16, phase=phase, name="d_energy")
        _lib.check_segments(lib.cough_frame_energy(data.ptr, bank.offsets_dev.data_ptr(), bank.lengths_dev.data_ptr(),
                                                   offs_dev.data_ptr(), n, tiles_dev.data_ptr(), len(tiles), frame_length,
                                                   hop_length, energy.ptr, _stream()), "cough_frame_energy")
        torch.cuda.synchronize()
        G.check([data, energy], {"energy": energy.float64}, {"energy": want_energy}, f"cough_frame_energy phase {phase}")

    for max_segments in (1, 16):
        args = (frame_length, hop_length, 2 * frame_length, 1, max_segments, 0.25, 1e-9)

        def call(e_ptr, counts, starts, lens, peak):
            _lib.check_segments(lib.cough_pick_segments(e_ptr, offs_dev.data_ptr(), bank.lengths_dev.data_ptr(), n, *args, counts,
                                                        starts, lens, peak, _stream()), "cough_pick_segments")
        shapes = {"counts": ((n,), I32), "starts": ((n, max_segments), I32), "lengths": ((n, max_segments), I32),
                  "peak_db": ((n, max_segments), F32)}
        want = {k: torch.empty(s, dtype=d, device="cuda") for k, (s, d) in shapes.items()}
        call(want_energy.data_ptr(), *(want[k].data_ptr() for k in shapes))
        torch.cuda.synchronize()
        assert int(want["counts"].sum()) >= 1
        for phase in PHASES:
            e = Guarded.holding(want_energy, 8, name="d_energy")
            outs = {k: G.output(s, d, align=16, phase=phase, name="d_" + k) for k, (s, d) in shapes.items()}
            call(e.ptr, *(outs[k].ptr for k in shapes))
            torch.cuda.synchronize()
            got = {k: o.view(shapes[k][1]).view(shapes[k][0]) for k, o in outs.items()}
            G.check([e] + list(outs.values()), got, want, f"cough_pick_segments max_segments {max_segments} phase {phase}")


# ------------------------------------------------------------------ the short scalar-store kernels
def _both(call, ins, outs, what, phases=(0,)):
    """``call(pointers)`` once on ordinary tensors and once per phase between guards, the two compared.  ``ins``:
    name -> float tensor (held flush against a guard, float64 8-byte aligned, float32 4); ``outs``: name -> (shape, dtype,
    initial contents or None).  Returns the ordinary run's outputs."""
    plain_in = {k: t.cuda() for k, t in ins.items()}
    want = {k: (torch.empty(s, dtype=d, device="cuda") if init is None else init.clone().cuda().view(d).view(s))
            for k, (s, d, init) in outs.items()}
    call({**{k: t.data_ptr() for k, t in plain_in.items()}, **{k: t.data_ptr() for k, t in want.items()}})
    torch.cuda.synchronize()
    for phase in phases:
        gin = {k: Guarded.holding(t.cuda(), t.element_size(), name=k) for k, t in ins.items()}
        gout = {}
        for k, (s, d, init) in outs.items():
            size = torch.empty((), dtype=d).element_size()
            gout[k] = G.output(s, d, align=16, phase=phase - phase % size, name=k)
            if init is not None:
                gout[k].view(d).copy_(init.cuda().view(d).reshape(-1))
        call({**{k: g.ptr for k, g in gin.items()}, **{k: g.ptr for k, g in gout.items()}})
        torch.cuda.synchronize()
        got = {k: g.view(outs[k][1]).view(outs[k][0]) for k, g in gout.items()}
        G.check(list(gin.values()) + list(gout.values()), got, want, f"{what} phase {phase}")
    return want


def _shipped_pre(**kw):
    import cough_detector_amd as cda
    from parity import SHIPPED
    return cda.AudioPreprocessor(device="cuda", **{**SHIPPED, **kw})


@pytest.mark.parametrize("orig_sr", [44100, 8000])
def test_resample(orig_sr):
    pre = _shipped_pre()
    for rows, n in ((1, 1), (3, 1), (1, 1000), (3, 1000)):
        x = _rand(rows, n, seed=n + rows)
        normal = pre.resample(x.cuda(), orig_sr)
        kern, width, orig, new = pre._resamplers[orig_sr]
        out_len = normal.shape[1]
        want = _both(lambda p: _lib.check(_lib.load().cough_resample(p["in"], n, rows, n, p["kernel"], orig, new, width, p["out"],
                                                                     out_len, out_len, _stream()), "cough_resample"),
                     {"in": x, "kernel": kern}, {"out": ((rows, out_len), F32, None)}, f"cough_resample {orig_sr} {rows}x{n}",
                     PHASES)
        assert torch.equal(want["out"], normal)


def test_prepare_clip():
    pre = _shipped_pre()
    for channels, n, out_len in ((1, 1000, 16000), (3, 20001, 16000), (2, 5, 5), (1, 1, 4)):
        x = _rand(channels, n, seed=n)
        for normalize in (True, False):
            normal = pre._prepare(x.cuda(), out_len, normalize)
            want = _both(lambda p: _lib.check(_lib.load().cough_prepare_clip(p["in"], n, channels, n, p["out"], out_len,
                                                                             _lib.PREP_NORMALIZE if normalize else 0, _stream()),
                                              "cough_prepare_clip"),
                         {"in": x}, {"out": ((1, out_len), F32, None)}, f"cough_prepare_clip {channels}x{n}", PHASES)
            assert torch.equal(want["out"], normal)


def test_pre_emphasis_deltas_pcen():
    lib = _lib.load()
    pre = _shipped_pre(use_pre_emphasis=True)
    for rows, n in ((1, 1), (3, 1001), (2, 4)):
        x = _rand(rows, n, seed=n)
        want = _both(lambda p: _lib.check(lib.cough_pre_emphasis(p["in"], n, p["out"], n, rows, n, float(pre.pre_emphasis_coef),
                                                                 _stream()), "cough_pre_emphasis"),
                     {"in": x}, {"out": ((rows, n), F32, None)}, f"cough_pre_emphasis {rows}x{n}", PHASES)
        assert torch.equal(want["out"], pre.apply_pre_emphasis(x.cuda()))
    for shape in ((1, 1, 1), (1, 3, 2), (3, 13, 101)):
        x, t = _rand(*shape, seed=shape[-1]), shape[-1]
        rows = x.numel() // t
        want = _both(lambda p: _lib.check(lib.cough_compute_deltas(p["in"], p["out"], rows, t, _stream()), "cough_compute_deltas"),
                     {"in": x}, {"out": (shape, F32, None)}, f"cough_compute_deltas {shape}", PHASES)
        assert torch.equal(want["out"], pre.compute_deltas(x.cuda()))
    for shape in ((1, 1, 1), (1, 64, 101), (3, 5, 7)):
        x, t = _rand(*shape, seed=shape[-1] + 1).abs() + 1e-3, shape[-1]
        rows = x.numel() // t
        want = _both(lambda p: _lib.check(lib.cough_pcen(p["in"], p["out"], rows, t, 0.98, 2.0, 0.5, 1e-6, _stream()),
                                          "cough_pcen"),
                     {"in": x}, {"out": (shape, F32, None)}, f"cough_pcen {shape}", PHASES)
        assert torch.equal(want["out"], pre.apply_pcen(x.cuda()))


def test_mask_axes_and_mix_rows():
    lib = _lib.load()
    for n_img, h, w in ((1, 3, 1), (3, 5, 7), (2, 90, 101)):
        x = _rand(n_img, h, w, seed=w)
        axis, start, end = (0, 1, 1), (1, max(w - 2, 0), 0), (2, w, 0)
        arr = lambda v: (C.c_int * 3)(*v)                            # noqa: E731
        want = _both(lambda p: _lib.check(lib.cough_mask_axes(p["in"], p["out"], n_img, h, w, 3, arr(axis), arr(start), arr(end),
                                                              _stream()), "cough_mask_axes"),
                     {"in": x}, {"out": ((n_img, h, w), F32, None)}, f"cough_mask_axes {(n_img, h, w)}", PHASES)
        exact = x.clone()
        exact[:, 1, :] = 0
        exact[:, :, max(w - 2, 0):] = 0
        assert torch.equal(want["out"].cpu(), exact)
    for rows, n in ((1, 1), (3, 5), (3, 1023)):
        x1, x2 = _rand(rows, n, seed=n), _rand(rows, n, seed=n + 1)
        coef = torch.tensor([[0.25, 0.75], [0.9, 0.1], [0.5, 0.5]])[:rows].contiguous()
        for index in (None, _dev(list(range(rows))[::-1], I32)):
            _both(lambda p: _lib.check(lib.cough_mix_rows(p["x1"], p["x2"], None if index is None else index.data_ptr(), p["out"],
                                                          rows, n, p["coef"], _stream()), "cough_mix_rows"),
                  {"x1": x1, "x2": x2, "coef": coef}, {"out": ((rows, n), F32, None)}, f"cough_mix_rows {rows}x{n}", PHASES)


def test_synth_clips():
    from cough_detector_amd import synth
    for count in (1, 3):
        want = _both(lambda p: _lib.check(_lib.load().cough_synth_clips(p["out"], 16000, count, 41, 7, _stream()),
                                          "cough_synth_clips"),
                     {}, {"out": ((count, 16000), F32, None)}, f"cough_synth_clips {count}", PHASES)
        assert torch.equal(want["out"], synth.device_clips(41, count, seed_stride=7))


def test_ring_write_and_window_gather_positions_that_wrap():
    lib = _lib.load()
    streams, ring_len, chunk_len, window = 3, 100, 30, 64
    rings = _rand(streams, ring_len, seed=1)
    chunks = _rand(2, chunk_len, seed=2)
    ids, pos = _dev([2, 0], I32), _dev([90, 100 * 7 + 85], I64)          # both chunks wrap round the ring's end
    want = _both(lambda p: _lib.check(lib.cough_ring_write(p["rings"], ring_len, p["chunks"], chunk_len, ids.data_ptr(),
                                                           pos.data_ptr(), 2, _stream()), "cough_ring_write"),
                 {"chunks": chunks}, {"rings": ((streams, ring_len), F32, rings)}, "cough_ring_write", PHASES)
    exact = rings.clone()
    for c, (s, p0) in enumerate(((2, 90), (0, 785))):
        for i in range(chunk_len):
            exact[s, (p0 + i) % ring_len] = chunks[c, i]
    assert torch.equal(want["rings"].cpu(), exact)
    wid, wpos = _dev([0, 2, 1], I32), _dev([70, 299, 0], I64)            # two windows wrap, one does not
    want = _both(lambda p: _lib.check(lib.cough_window_gather(p["rings"], ring_len, wid.data_ptr(), wpos.data_ptr(), 3, window,
                                                              p["out"], _stream()), "cough_window_gather"),
                 {"rings": exact}, {"out": ((3, window), F32, None)}, "cough_window_gather", PHASES)
    for r, (s, p0) in enumerate(((0, 70), (2, 299), (1, 0))):
        assert torch.equal(want["out"][r].cpu(), exact[s, [(p0 + i) % ring_len for i in range(window)]])


def test_smooth_sweep_and_list_events():
    lib = _lib.load_score()
    per_clip = [1, 9, 40, 3]
    n, n_windows = len(per_clip), sum(per_clip)
    offsets = _dev(np.concatenate([[0], np.cumsum(per_clip)]), I64)
    prob = torch.rand(n_windows, generator=torch.Generator().manual_seed(3))
    prob[12] = float("nan")
    for w in (1, 3, 9):
        smoothed = _both(lambda p: _lib.check_score(lib.cough_smooth_windows(p["prob"], offsets.data_ptr(), n, n_windows, w,
                                                                             p["smoothed"], _stream()), "cough_smooth_windows"),
                         {"prob": prob}, {"smoothed": ((n_windows,), F64, None)}, f"cough_smooth_windows W={w}", (0, 8))["smoothed"]
    smoothed = smoothed.cpu()
    thresholds = torch.linspace(0.05, 0.95, 65, dtype=F64)               # 65 thresholds: two groups of 64 lanes
    gap = 2
    outs = {"counts": ((n, 65), I32, None), "first": ((n, 65), I32, None), "peak_conf": ((n,), F64, None),
            "peak_window": ((n,), I32, None)}
    sweep = _both(lambda p: _lib.check_score(lib.cough_sweep_thresholds(
        p["smoothed"], offsets.data_ptr(), n, n_windows, p["thresholds"], 65, gap, p["counts"], p["first"], p["peak_conf"],
        p["peak_window"], _stream()), "cough_sweep_thresholds"),
        {"smoothed": smoothed, "thresholds": thresholds}, outs, "cough_sweep_thresholds", PHASES)
    k = 20
    counts = sweep["counts"][:, k].cpu().numpy().astype(np.int64)
    n_events = int(counts.sum())
    assert n_events >= 3
    event_offsets = _dev(np.concatenate([[0], np.cumsum(counts)]), I64)
    _both(lambda p: _lib.check_score(lib.cough_list_events(p["smoothed"], offsets.data_ptr(), n, n_windows, float(thresholds[k]), gap,
                                                           event_offsets.data_ptr(), n_events, p["window"], p["conf"], _stream()),
                                     "cough_list_events"),
          {"smoothed": smoothed}, {"window": ((n_events,), I32, None), "conf": ((n_events,), F64, None)}, "cough_list_events",
          PHASES)


@pytest.mark.parametrize("n", [1, 3, 300])
def test_epoch_meter_update(n):
    lib = _lib.load_loop()
    logits = _rand(n, 2, seed=n) * 5
    targets = torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(n)).cuda()
    meter = torch.zeros(_lib.EPOCH_METER_BYTES // 8, dtype=I64)
    for update, (cw, loss) in enumerate(((torch.tensor([1.0, 2.5]), None), (None, torch.tensor([0.625]))), 1):
        ins = {"logits": logits, **({"cw": cw} if cw is not None else {}), **({"loss": loss} if loss is not None else {})}
        want = _both(lambda p: _lib.check_loop(lib.cough_epoch_meter_update(p["logits"], targets.data_ptr(), n, p.get("cw"),
                                                                            p.get("loss"), p["meter"], p["preds"], _stream()),
                                               "cough_epoch_meter_update"),
                     ins, {"meter": ((8,), I64, meter), "preds": ((n,), I64, None)}, f"cough_epoch_meter_update n={n}", (0, 8))
        assert int(want["meter"][1]) == update and int(want["meter"][2]) == update * n
        meter = want["meter"].cpu()            # the second update starts from the first one's meter


def test_device_draws():
    """``cough_draw_batch``, ``cough_draw_speed``, ``cough_draw_pitch`` and ``cough_clear_shifts`` against their Python
    wrappers; the records and plans come out of guarded buffers, the lengths and the step table stay ordinary."""
    from cough_detector_amd import pitch, warp
    from cough_detector_amd.augmentation import SpecAugment
    aug, spec = _augmentor(), SpecAugment(p=0.7)
    aug.p_augment = 0.6
    dev = torch.device("cuda", torch.cuda.current_device())
    for b in (1, 3, 70):
        lens = _dev([16000 - 37 * i for i in range(b)], I32)
        clips, masks = draws.draw_batch(5, lens, aug, spec, (90, 101))
        n_f, n_t = draws.mask_counts(spec)
        nm, blens = n_f + n_t, aug._bank_tables_device(dev)[1]
        got = _both(lambda p: _lib.check_draws(_lib.load_draws().cough_draw_batch(
            5, b, lens.data_ptr(), 0.6, len(aug._bank_lengths), blens.data_ptr(), 0.7, n_f, int(spec.freq_mask_param), n_t,
            int(spec.time_mask_param), 90, 101, p["clips"], p["axis"], p["start"], p["end"], _stream()), "cough_draw_batch"),
            {}, {"clips": ((b, 5), I64, None), "axis": ((b, nm), I32, None), "start": ((b, nm), I32, None),
                 "end": ((b, nm), I32, None)}, f"cough_draw_batch b={b}", (0, 8))
        assert torch.equal(got["clips"].view(torch.uint8).view(b, 40), clips)
        assert torch.equal(torch.stack([got["axis"], got["start"], got["end"]]), masks)

        plans, new_lens = warp.draw_speed(9, lens, 0.6, (0.9, 1.1), 16000)
        got = _both(lambda p: _lib.check_warp(_lib.load_warp().cough_draw_speed(9, b, lens.data_ptr(), 0.6, 0.9, 1.1, 16000, p["plans"],
                                                                                 p["new"], _stream()), "cough_draw_speed"),
                    {}, {"plans": ((b, 3), I32, None), "new": ((b,), I32, None)}, f"cough_draw_speed b={b}", PHASES)
        assert torch.equal(got["plans"], plans) and torch.equal(got["new"], new_lens)

        table = torch.from_numpy(pitch.step_table((-2, 2), 16000, True)).to(dev)
        sp, wp, ns = pitch.draw_pitch(11, lens, 0.6, (-2, 2), 16000, table_dev=table)
        got = _both(lambda p: _lib.check_pitch(_lib.load_pitch().cough_draw_pitch(11, b, lens.data_ptr(), 0.6, -2, 2, table.data_ptr(),
                                                                                   16000, p["stretch"], p["warp"], p["ns"], _stream()),
                                               "cough_draw_pitch"),
                    {}, {"stretch": ((b, 2), I64, None), "warp": ((b, 3), I32, None), "ns": ((b,), I32, None)},
                    f"cough_draw_pitch b={b}", (0, 8))
        assert torch.equal(got["stretch"].view(torch.uint8).view(b, 16), sp) and torch.equal(got["warp"], wp)
        assert torch.equal(got["ns"], ns)

        cleared = clips.clone()
        warp.clear_shifts(cleared)
        got = _both(lambda p: _lib.check_warp(_lib.load_warp().cough_clear_shifts(p["clips"], b, _stream()), "cough_clear_shifts"),
                    {}, {"clips": ((b, 5), I64, clips.view(I64))}, f"cough_clear_shifts b={b}", (0, 8))
        assert torch.equal(got["clips"].view(torch.uint8).view(b, 40), cleared)
