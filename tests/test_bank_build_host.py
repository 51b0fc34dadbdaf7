"""How banks are built and indexed, without a GPU: ``_offsets`` / ``_owner`` / ``_ragged`` against the expressions they
replaced, value and dtype, and ``DeviceClipBank.from_packed`` against the public constructor on CPU tensors."""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd.data import _offsets, _owner, _ragged

FIXED = [[], [0], [0, 0], [3], [2, 0, 5, 0, 1]]
FIELDS = ("data", "offsets", "lengths", "labels", "offsets_dev", "lengths_dev", "labels_dev")


def _count_vectors():
    rng = np.random.default_rng(11)
    return FIXED + [rng.integers(0, 8, size=int(rng.integers(0, 51))).tolist() for _ in range(200)]


def _same(got: np.ndarray, want: np.ndarray) -> None:
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want), (got, want)


def _same_bank(got: cda.DeviceClipBank, want: cda.DeviceClipBank) -> None:
    assert len(got) == len(want) and got.device == want.device
    for name in FIELDS:
        u, v = getattr(got, name), getattr(want, name)
        assert u.dtype == v.dtype and u.device == v.device and torch.equal(u, v), name


# ------------------------------------------------------------------------------------------------ _offsets, _ragged
def test_offsets_and_ragged_equal_the_expressions_they_replace():
    vectors = _count_vectors()
    assert len(vectors) == 205 and max(len(v) for v in vectors) == 50 and max(max(v, default=0) for v in vectors) == 7
    for counts in vectors:
        per = np.asarray(counts, dtype=np.int64)
        n, total = per.size, int(per.sum())
        offsets = np.concatenate([[0], np.cumsum(per, dtype=np.int64)]).astype(np.int64)
        owner = np.repeat(np.arange(n, dtype=np.int64), per)
        first = np.concatenate([[0], np.cumsum(per)[:-1]])
        # (without a row that spelling of the rank does not broadcast: its callers returned before it)
        rank = np.arange(total, dtype=np.int64) - np.repeat(first, per) if n else np.zeros(0, dtype=np.int64)
        assert offsets.dtype == owner.dtype == rank.dtype == np.int64 and offsets.shape == (n + 1,)
        forms = [list(counts), per, per.astype(np.int32), torch.tensor(counts, dtype=torch.int32)]
        for form in forms:
            _same(_offsets(form), offsets)
            _same(_owner(form), owner)
            got = _ragged(form)
            assert len(got) == 3
            for mine, want in zip(got, (offsets, owner, rank)):
                _same(mine, want)
        # the other spellings that were in use: without dtype=, without the last offset, indexed by the owner
        _same(_offsets(per), np.concatenate([[0], np.cumsum(per)]).astype(np.int64))
        _same(_offsets(per)[:-1], np.concatenate([[0], np.cumsum(per, dtype=np.int64)[:-1]]).astype(np.int64) if n
              else np.zeros(0, dtype=np.int64))                           # (the bank spelt its empty case out)
        _same(_ragged(per)[2], np.arange(total, dtype=np.int64) - offsets[:-1][owner])


# ------------------------------------------------------------------------------------------------ from_packed
def _clips(lengths, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in lengths]


@pytest.mark.parametrize("lengths,labels", [([5, 1, 16001, 7, 300], [0, 1, 0, 1, 1]), ([3], [1]), ([], [])])
def test_from_packed_equals_the_constructor(lengths, labels):
    clips = _clips(lengths)
    want = cda.DeviceClipBank(clips, labels, device="cpu")
    packed = torch.cat(clips) if clips else torch.zeros(0, dtype=torch.float32)
    got = cda.DeviceClipBank.from_packed(packed, lengths, labels)
    assert isinstance(got, cda.DeviceClipBank) and got.device == torch.device("cpu") and len(got) == len(lengths)
    _same_bank(got, want)
    assert got.data.data_ptr() == packed.data_ptr()                       # wrapped, not copied
    again = cda.DeviceClipBank.from_packed(packed, torch.tensor(lengths, dtype=torch.int32), np.asarray(labels, dtype=np.int64))
    _same_bank(again, want)


def test_subset_and_concat_are_unchanged():
    lengths, labels = [5, 1, 16001, 7, 300], [0, 1, 0, 1, 1]
    clips = _clips(lengths)
    bank = cda.DeviceClipBank(clips, labels, device="cpu")
    for idx in ([3, 0, 0, 4], [], [-1, 2], torch.tensor([1, 2, 3])):
        picked = [int(i) for i in idx]
        _same_bank(bank.subset(idx), cda.DeviceClipBank([clips[i] for i in picked], [labels[i] for i in picked], device="cpu"))
    with pytest.raises(IndexError, match="indices must lie in"):
        bank.subset([5])
    parts = [bank.subset([0, 1]), bank.subset([]), bank.subset([2, 3, 4])]
    _same_bank(cda.DeviceClipBank.concat(parts), bank)
    _same_bank(cda.DeviceClipBank.concat([bank, bank.subset([4])]),
               cda.DeviceClipBank(clips + [clips[4]], labels + [labels[4]], device="cpu"))


def test_from_packed_refuses_what_the_host_can_see():
    data = torch.zeros(10, dtype=torch.float32)
    with pytest.raises(ValueError, match=r"^DeviceClipBank\.from_packed: 2 lengths but 3 labels"):
        cda.DeviceClipBank.from_packed(data, [4, 6], [0, 1, 0])
    with pytest.raises(ValueError, match=r"^DeviceClipBank\.from_packed: lengths of 9 samples, data of 10$"):
        cda.DeviceClipBank.from_packed(data, [4, 5], [0, 1])
    for bad in (data.view(2, 5), data.to(torch.float64), torch.zeros(10, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"^DeviceClipBank\.from_packed: data is "):
            cda.DeviceClipBank.from_packed(bad, [4, 6], [0, 1])


def test_cut_needs_a_gpu():
    bank = cda.DeviceClipBank(_clips([5, 3]), [0, 1], device="cpu")
    with pytest.raises(RuntimeError, match="the kernels need it on the GPU"):
        bank.cut(np.array([0], dtype=np.int64), np.array([1]), np.array([2]))
