"""Device-side draws without a GPU: the sixth library's symbols and argument checks, the build's staleness rule, the
loader's ``draws`` switch, and the restatement of the draw contract (tests/draws_ref.py): its generator against the
Random123 known answer and its distributions against bounds derived from the contract."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import draws as cdraws
import draws_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_draws.h")


# ------------------------------------------------------------------------------------------------ the library
def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_draws_library_exports_exactly_its_header():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(cough_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_lib.DRAWS_SYMBOLS), declared ^ set(_lib.DRAWS_SYMBOLS)
    assert len(_lib.DRAWS_SYMBOLS) == len(set(_lib.DRAWS_SYMBOLS)) == 5
    lib = _lib.load_draws()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cough_draws_abi_version() == 1
    assert "#define COUGH_DRAWS_ABI_VERSION 1" in text
    assert _exported(_lib.DRAWS_LIB_PATH) == declared
    assert C.sizeof(_lib.CoughAugClip) == R.CLIP_DTYPE.itemsize == cdraws.CLIP_BYTES == 40
    for name, (dtype, offset) in R.CLIP_DTYPE.fields.items():
        assert getattr(_lib.CoughAugClip, name).offset == offset, name


def test_the_other_five_libraries_are_untouched():
    others = (("cough_amd.h", _lib.SYMBOLS, _lib.LIB_PATH, 53, _lib.load().cough_amd_abi_version(), 5),
              ("cough_amd_loop.h", _lib.LOOP_SYMBOLS, _lib.LOOP_LIB_PATH, 3, _lib.load_loop().cough_loop_abi_version(), 1),
              ("cough_amd_data.h", _lib.DATA_SYMBOLS, _lib.DATA_LIB_PATH, 5, _lib.load_data().cough_data_abi_version(), 1),
              ("cough_amd_segments.h", _lib.SEGMENTS_SYMBOLS, _lib.SEGMENTS_LIB_PATH, 6,
               _lib.load_segments().cough_segments_abi_version(), 1),
              ("cough_amd_score.h", _lib.SCORE_SYMBOLS, _lib.SCORE_LIB_PATH, 5, _lib.load_score().cough_score_abi_version(), 1))
    for header, symbols, path, count, version, want in others:
        assert len(symbols) == count and version == want, header
        assert not set(_lib.DRAWS_SYMBOLS) & set(symbols), header
        assert _exported(path) == set(symbols), header
        text = open(os.path.join(ROOT, "include", header)).read()
        for s in _lib.DRAWS_SYMBOLS:
            assert s not in text, (header, s)


def test_both_libraries_compile_one_augment_kernel():
    src = lambda name: open(os.path.join(cbuild.CSRC, name)).read()      # noqa: E731
    for name in ("augment.hip", "draws.hip"):
        text = src(name)
        assert '#include "augment_kernel.h"' in text, name
        assert "void augment_kernel(" not in text and "struct AugRec" not in text, name
    assert src("augment_kernel.h").count("void augment_kernel(") == 1


FAKE = 1 << 20


def _err():
    return _lib.load_draws().cough_draws_last_error()


def test_draw_batch_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_draws()

    def call(seed=1, n=4, lens=FAKE, p=0.5, n_bank=3, blens=FAKE, sp=0.5, nf=2, fp=10, nt=2, tp=20, h=90, w=101, clips=FAKE,
             axis=FAKE, start=FAKE, end=FAKE):
        return lib.cough_draw_batch(seed, n, lens, p, n_bank, blens, sp, nf, fp, nt, tp, h, w, clips, axis, start, end, None)

    E = _lib.EINVAL
    for kw in ("lens", "blens", "clips", "axis", "start", "end"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_draw_batch" in _err(), kw
    assert call(n=-1) == E and b"n_rows" in _err()
    assert call(n_bank=-1) == E and b"n_bank" in _err()
    for nf, nt in ((17, 0), (0, 17), (9, 8), (16, 1), (-1, 2), (2, -1), (2**31 - 1, 2**31 - 1)):     # 17 masks; negative counts
        assert call(nf=nf, nt=nt) == E and b"n_masks" in _err() and b"cough_draw_batch" in _err(), (nf, nt)
    for v in (0, -3, 91):                                                  # mask_param outside 1..size on its axis
        assert call(fp=v) == E and b"freq_mask_param" in _err(), v
    for v in (0, -3, 102):
        assert call(tp=v) == E and b"time_mask_param" in _err(), v
    for kw in ("h", "w"):
        for v in (0, -5):
            assert call(**{kw: v}) == E and b"shape" in _err(), (kw, v)
    for kw in ("p", "sp"):
        assert call(**{kw: math.nan}) == E and b"NaN" in _err(), kw
    for kw in ("lens", "blens", "axis", "start", "end"):
        assert call(**{kw: FAKE + 2}) == E and b"4-byte" in _err(), kw
    assert call(clips=FAKE + 4) == E and b"8-byte" in _err()
    # what is switched off is not looked at, and nothing to do launches nothing
    assert call(n=0) == _lib.OK and call(n=0, nf=8, nt=8, fp=90, tp=101) == _lib.OK
    assert call(n=0, p=-1.0, lens=None, clips=None, blens=None) == _lib.OK
    assert call(n=0, sp=-1.0, axis=None, start=None, end=None, fp=0, tp=1000, h=0, w=0) == _lib.OK
    assert call(n=0, nf=0, nt=0, axis=None, start=None, end=None) == _lib.OK
    assert call(n=0, nf=0, fp=1000) == _lib.OK and call(n=0, nt=0, tp=1000) == _lib.OK     # no masks on that axis
    assert call(n=0, n_bank=0, blens=None) == _lib.OK
    assert call(p=-1.0, sp=-1.0, lens=None, clips=None, axis=None, start=None, end=None) == _lib.OK    # neither: no launch
    with pytest.raises(ValueError, match="cough_draw_batch: .*n_masks"):
        _lib.check_draws(call(nf=17), "cough_draw_batch")
    assert b"n_masks" not in _lib.load_score().cough_score_last_error()       # the messages stay apart


def test_augment_rows_drawn_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_draws()
    need = lib.cough_augment_rows_drawn_workspace_bytes(3)
    assert need == 256 and lib.cough_augment_rows_drawn_workspace_bytes(0) == 0
    assert lib.cough_augment_rows_drawn_workspace_bytes(-1) == 0 and lib.cough_augment_rows_drawn_workspace_bytes(6) == 512

    def call(src=FAKE, offs=FAKE, lens=FAKE, n=3, samples=16000, clips=FAKE, bank=FAKE, numel=1000, boffs=FAKE, blens=FAKE,
             n_bank=2, seed=1, out=2 * FAKE, ws=4 * FAKE, ws_bytes=need):
        return lib.cough_augment_rows_drawn(src, offs, lens, n, samples, clips, bank, numel, boffs, blens, n_bank, seed, out,
                                            ws, ws_bytes, None)

    E = _lib.EINVAL
    for kw in ("src", "offs", "lens", "clips", "out", "ws", "bank", "boffs", "blens"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_augment_rows_drawn" in _err(), kw
    for kw, v in (("n", -1), ("samples", 0), ("samples", -4), ("n_bank", -1), ("numel", -1)):
        assert call(**{kw: v}) == E and b"bad sizes" in _err(), (kw, v)
    assert call(samples=(1 << 30) + 1) == _lib.EUNSUPPORTED and b"2^30" in _err()
    assert call(out=FAKE) == E and b"alias" in _err()
    for kw in ("src", "lens", "bank", "blens", "out"):
        assert call(**{kw: 8 * FAKE + 2}) == E and b"4-byte" in _err(), kw
    for kw in ("offs", "clips", "boffs"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err(), kw
    assert call(ws_bytes=need - 1) == _lib.EWORKSPACE and call(ws=4 * FAKE + 128) == _lib.EWORKSPACE
    assert call(n=0) == _lib.OK and call(n=0, src=None, ws=None) == _lib.OK


# ------------------------------------------------------------------------------------------------ the Python front
def test_the_package_exports_the_draws():
    for name in ("draw_batch", "augment_rows_drawn"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cdraws, name), name


def _cpu_bank():
    return cda.DeviceClipBank([torch.zeros(800), torch.ones(20000), torch.ones(40000)], [0, 1, 0], device="cpu")


def test_the_loader_checks_its_draws_switch():
    bank, pre = _cpu_bank(), cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False,
                                                   use_spectral_contrast=False)
    aug = cda.AudioAugmentor(p_augment=0.5)
    with pytest.raises(ValueError, match="draws='device'.*noise='host'"):
        cda.DeviceDataLoader(bank, pre, audio_augmentor=aug, draws="device", noise="host")
    with pytest.raises(ValueError, match="draws must be"):
        cda.DeviceDataLoader(bank, pre, draws="gpu")
    assert cda.DeviceDataLoader(bank, pre).draws == "host"                 # the default: nothing changes
    loader = cda.DeviceDataLoader(bank, pre, batch_size=1, audio_augmentor=aug, draws="device",
                                  generator=torch.Generator().manual_seed(3))
    assert loader.draws == "device" and loader.last_epoch_seed is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # a CPU bank cannot launch; the seed was drawn first
        next(iter(loader))
    g = torch.Generator().manual_seed(3)
    cda.DeviceDataLoader(bank, pre, batch_size=1, generator=g).epoch_indices()
    assert loader.last_epoch_seed == int(torch.randint(0, 2**62, (1,), generator=g).item())
    train, val = cda.create_data_loaders(bank, bank, pre, batch_size=1, audio_augmentor=aug, draws="device")
    assert train.draws == "device" and val.draws == "host"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.draw_batch(1, torch.tensor([800], dtype=torch.int32), aug, None, (90, 101))
    with pytest.raises(ValueError, match="int32"):
        cda.draw_batch(1, torch.tensor([800]), aug, None, (90, 101))


# ------------------------------------------------------------------------------------------------ the restatement
def test_philox_known_answers():
    # Random123's kat_vectors, philox4x32 with 10 rounds: the zero counter and key, and all bits set
    got = [int(w) for w in R.philox4x32_10((0, 0, 0, 0), (0, 0))]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [hex(w) for w in got]
    got = [int(w) for w in R.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF))]
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD], [hex(w) for w in got]
    rows = np.arange(5, dtype=np.uint64)                                   # vectorised over rows = row by row
    vec = R.philox4x32_10((2, rows, 0, 1), (7, 9))
    for r in range(5):
        assert [int(w[r]) for w in vec] == [int(w) for w in R.philox4x32_10((2, r, 0, 1), (7, 9))]


def test_unit_is_exact_and_open():
    u = R.unit(np.array([0, 1, 2**31, 2**32 - 1], dtype=np.uint64))
    assert u.tolist() == [2.0 ** -33, 1.5 * 2.0 ** -32, 0.5 + 2.0 ** -33, 1.0 - 2.0 ** -33]
    assert 0.0 < u.min() and u.max() < 1.0


def test_coins_at_the_ends_and_blank_records():
    n = np.full(1000, 16000)
    for p, want in ((0.0, False), (1.0, True)):
        clips, masks, fired = R.draw_ref(5, n, p, [700, 9000, 20000], p, 2, 10, 2, 20, 90, 101)
        for name, f in fired.items():
            assert f.all() == want and f.any() == want, (p, name)
    blank = np.zeros(1, dtype=R.CLIP_DTYPE)
    blank["gain"], blank["bank_index"] = 1.0, -1
    assert (clips == blank[0]).sum() == 0                                  # p = 1: every record differs from the blank one
    clips, masks, _ = R.draw_ref(5, n, 0.0, [700, 9000, 20000], 0.0, 2, 10, 2, 20, 90, 101)
    assert (clips == blank[0]).all() and not masks.any()                   # p = 0: AudioAugmentor._blank(), (0, 0, 0) masks
    aug = cda.AudioAugmentor._blank()
    for name in R.CLIP_DTYPE.names:
        assert getattr(aug, name) == blank[0][name], name
    clips, masks, fired = R.draw_ref(5, n, 1.0, [], None, 0, 0, 0, 0, 90, 101)     # an empty bank: the step never fires
    assert masks is None and not fired["bank"].any() and (clips["bank_index"] == -1).all() and not clips["bank_start"].any()
    clips, masks, _ = R.draw_ref(5, n, None, [], 1.0, 1, 5, 0, 0, 5, 7)
    assert clips is None and masks.shape == (3, 1000, 1)


def test_distributions_of_the_restatement():
    N, p, size = 200_000, 0.3, (90, 101)
    bank = [700, 9000, 20000]
    clips, masks, fired = R.draw_ref(20261018, np.full(N, 16000), p, bank, p, 2, 10, 2, 20, *size)
    bound = 5.0 * math.sqrt(p * (1.0 - p) / N)                             # 5 binomial standard deviations: derived
    for name, f in fired.items():
        share = float(f.mean())
        print(f"{name}: fired {share:.5f} (p = {p}, bound {bound:.5f})")
        assert abs(share - p) <= bound, (name, share)
    # the coins are separate draws: two of them agree as often as independent ones do (within 5 standard deviations)
    both = float((fired["shift"] & fired["gain"]).mean())
    assert abs(both - p * p) <= 5.0 * math.sqrt(p * p * (1 - p * p) / N), both
    s, f = clips["shift"], fired["shift"]
    assert s.min() >= -3200 and s.max() <= 3200 and (s > 0).any() and (s < 0).any() and not s[~f].any()
    assert s.min() < -3100 and s.max() > 3100                              # and uses the range
    g = clips["gain"]
    assert g.dtype == np.float32 and g.min() >= np.float32(0.7) and g.max() <= np.float32(1.3) and (g[~fired["gain"]] == 1.0).all()
    assert g[fired["gain"]].min() < 0.71 and g[fired["gain"]].max() > 1.29
    snr, fg = clips["gaussian_snr_db"], fired["gaussian"]
    assert (clips["gaussian"] == fg).all() and snr[fg].min() > 10.0 and snr[fg].max() < 30.0 and not snr[~fg].any()
    snr, fb = clips["bank_snr_db"], fired["bank"]
    assert snr[fb].min() > 5.0 and snr[fb].max() < 20.0 and not snr[~fb].any()
    k = clips["bank_index"]
    assert set(k[fb].tolist()) == {0, 1, 2} and (k[~fb] == -1).all()
    counts = np.bincount(k[fb], minlength=3) / fb.sum()
    assert np.abs(counts - 1 / 3).max() <= 5.0 * math.sqrt((1 / 3) * (2 / 3) / fb.sum()), counts
    rep = R.repeated_length(np.asarray(bank)[np.maximum(k, 0)], 16000)
    assert rep[fb & (k == 0)].tolist()[:1] == [16100] and (rep[k == 1] == 16000 // 9000 * 9000 + 9000).all()
    start = clips["bank_start"]
    assert (start >= 0).all() and (start[fb] <= (rep - 16000)[fb]).all() and not start[~fb].any()
    assert start[fb & (k == 0)].max() == 100 and start[fb & (k == 2)].max() > 3900    # the top of each range is reached
    axis, lo, hi = masks
    fs = fired["spec"]
    assert not masks[:, ~fs].any()
    assert (axis[fs] == np.array([0, 0, 1, 1])).all()
    for m, (param, extent) in enumerate(((10, 90), (10, 90), (20, 101), (20, 101))):
        assert (0 <= lo[:, m]).all() and (lo[:, m] <= hi[:, m]).all() and (hi[:, m] <= extent).all(), m
        width = (hi - lo)[fs, m]
        assert width.max() == param - 1 and width.min() == 0, m            # value = u * param < param, truncated
        assert lo[fs, m].max() >= extent - param, m
