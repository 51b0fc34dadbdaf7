"""CPU checks of the host-side handle owner and per-stream scratch (cough_detector_amd/_native.py): fake streams, fake
create / destroy functions and CPU buffers; no GPU and no library call."""
import copy
import gc
import threading
import types

import pytest
import torch

from cough_detector_amd import _lib, _native

CPU = torch.device("cpu")


@pytest.fixture
def stream(monkeypatch):
    """The current "stream" of the calling thread: set ``stream.id``; threads start on stream 0."""
    cur = threading.local()
    monkeypatch.setattr(_native, "_current_stream", lambda dev: getattr(cur, "id", 0))
    return cur


@pytest.fixture
def destroyed(monkeypatch):
    """Handles passed to the fake library's ``fake_destroy``, in order (the real library has no such function: a fake handle
    that outlives the test is never handed to it)."""
    out = []
    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(fake_destroy=out.append))
    return out


def test_scratch_is_per_stream_and_grows(stream):
    s = _native.StreamScratch()
    a = s.get(100, CPU)
    assert a.dtype == torch.uint8 and a.numel() == 100
    assert s.get(50, CPU) is a                                     # big enough: the same buffer
    stream.id = 1
    assert s.lookup(CPU) is None                                   # another stream has none yet
    b = s.get(100, CPU, note=(2, 90, 101))
    assert b is not a and s.lookup(CPU) == (b, (2, 90, 101))
    stream.id = 0
    c = s.get(300, CPU)                                            # too small: replaced, at exactly the size asked for
    assert c is not a and c.numel() == 300 and len(s) == 2


def test_scratch_evicts_the_least_recently_used_stream(stream):
    s = _native.StreamScratch()
    bufs = {}
    for k in range(_native.MAX_STREAM_WORKSPACES):
        stream.id = k
        bufs[k] = s.get(16, CPU)
    stream.id = 0
    assert s.get(16, CPU) is bufs[0]                               # a hit makes stream 0 the most recently used
    stream.id = 99
    s.get(16, CPU)
    assert len(s) == _native.MAX_STREAM_WORKSPACES
    stream.id = 1
    assert s.lookup(CPU) is None                                   # stream 1 was the least recently used
    for k in [0] + list(range(2, _native.MAX_STREAM_WORKSPACES)):
        stream.id = k
        assert s.lookup(CPU)[0] is bufs[k]


def test_scratch_survives_threads_hammering_more_streams_than_it_keeps(stream):
    s = _native.StreamScratch()
    errors = []
    start = threading.Barrier(16)

    def worker(t):
        try:
            start.wait()
            for i in range(2000):
                stream.id = (t + i) % 12
                buf = s.get(64 + (i % 5) * 8, CPU, note=t)
                assert buf.numel() >= 64 + (i % 5) * 8
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    assert len(s) == _native.MAX_STREAM_WORKSPACES


def test_handle_is_built_once_per_key_and_replaced_on_a_new_one(destroyed):
    made = []

    def create():
        made.append(len(made) + 100)
        return made[-1]

    h = _native.NativeHandle("fake_destroy")
    assert h.get("k1", create) == 100 and h.get("k1", create) == 100
    assert made == [100] and destroyed == []
    assert h.get("k2", create) == 101
    assert destroyed == [100]
    h.invalidate()
    assert destroyed == [100]                                      # destroyed when replaced, not when invalidated
    assert h.get("k2", create) == 102
    assert made == [100, 101, 102] and destroyed == [100, 101]


def test_handle_creation_races_build_one_handle(destroyed):
    h = _native.NativeHandle("fake_destroy")
    made, got = [], []
    start = threading.Barrier(16)

    def create():
        made.append(object())
        return made[-1]

    def worker():
        start.wait()
        got.append(h.get(("weights", 1), create))

    threads = [threading.Thread(target=worker) for _ in range(16)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert len(made) == 1 and destroyed == [] and all(g is made[0] for g in got) and len(got) == 16


def test_dropping_the_owner_destroys_the_handle(destroyed):
    h = _native.NativeHandle("fake_destroy")
    h.get(1, lambda: "handle")
    del h
    gc.collect()
    assert destroyed == ["handle"]


def test_copies_start_empty_and_leave_the_original_alone(destroyed, stream):
    h = _native.NativeHandle("fake_destroy")
    h.get(1, lambda: "handle")
    twin = copy.deepcopy(h)
    assert twin.get(1, lambda: "twin") == "twin"                   # a copy owns nothing until it builds its own
    del twin
    gc.collect()
    assert destroyed == ["twin"]
    assert h.get(1, lambda: "rebuilt") == "handle"
    s = _native.StreamScratch()
    s.get(8, CPU)
    assert len(copy.deepcopy(s)) == 0 and len(s) == 1


def test_model_copies_start_empty_and_invalidate_reaches_every_block():
    import cough_detector_amd as cda
    m = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1)
    twin = copy.deepcopy(m)
    assert twin._handle is not m._handle and twin._ws is not m._ws
    assert twin.res_blocks[0]._handle is not m.res_blocks[0]._handle
    owners = [m] + list(m.res_blocks)
    for mod in owners:
        mod._tensors, mod._handle._key = [], ("weights",)
    m.invalidate()
    assert all(mod._tensors is None and mod._handle._key is _native._STALE for mod in owners)
