"""What a C-ABI launch needs besides its tensors, owned in one place and safe to use from several threads: the native
handle (``NativeHandle``) and a workspace per stream (``StreamScratch``; ``include/cough_amd.h``: any number of threads may
launch with one handle, each with its own workspace and stream).  ``NativeModule`` is the host side of the classifiers."""
from __future__ import annotations

import ctypes as C
import threading
from collections import OrderedDict
from typing import Callable, Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib

MAX_STREAM_WORKSPACES = 8
_STALE = object()           # a NativeHandle key that equals no caller's key


def cuda_device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("cough_detector_amd needs an AMD GPU (gfx950): torch.cuda.is_available() is False "
                           "and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _current_stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


_stream = _current_stream           # what a launch takes as its stream


def _on_gpu(who: str, **tensors) -> torch.device:
    """The GPU on which every ``name=(tensor, dtype)`` lives; refuses a tensor that is not contiguous, not of its dtype or
    not on the device of the others, and tensors that are not on a GPU."""
    dev = None
    for name, (t, dtype) in tensors.items():
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor")
        if dev is not None and t.device != dev:
            raise ValueError(f"{who}: {name} lives on {t.device}, not on {dev}")
        dev = t.device
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the tensors live on {dev}; the kernels need them on the GPU (there is no CPU fallback)")
    return dev


class StreamScratch:
    """A ``torch.uint8`` workspace per (device, current stream), at most ``MAX_STREAM_WORKSPACES`` of them, least recently
    used evicted first.  A buffer is allocated while its own stream is current, so when it is replaced or evicted torch's
    caching allocator hands its memory out again only in that stream's order."""

    def __init__(self):
        self._lock = threading.Lock()
        self._bufs: "OrderedDict[tuple, tuple]" = OrderedDict()     # (device, stream) -> (buffer, note)

    def get(self, nbytes: int, dev: torch.device, note=None) -> torch.Tensor:
        """The current stream's buffer, replaced by one of exactly ``nbytes`` if it is smaller; ``note`` (e.g. the shape of
        the launch that will fill it) is kept next to it for ``lookup``."""
        key = (dev, _current_stream(dev))
        with self._lock:
            buf = self._bufs.pop(key, (None, None))[0]         # re-inserted below, as the most recently used
            if buf is None or buf.numel() < nbytes:
                if len(self._bufs) >= MAX_STREAM_WORKSPACES:
                    self._bufs.popitem(last=False)
                buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self._bufs[key] = (buf, note)
            return buf

    def lookup(self, dev: torch.device) -> Optional[Tuple[torch.Tensor, object]]:
        """(buffer, note) of the current stream, or None; allocates nothing."""
        with self._lock:
            return self._bufs.get((dev, _current_stream(dev)))

    def __len__(self) -> int:
        return len(self._bufs)

    def __reduce__(self):
        # a copy starts empty: a lock cannot be copied, and two owners of one buffer would share scratch
        return StreamScratch, ()


class NativeHandle:
    """One C handle and the library function (``destroy``, its name) that frees it."""

    def __init__(self, destroy: str):
        self._destroy = destroy
        self._lock = threading.Lock()
        self._handle: Optional[C.c_void_p] = None
        self._key = _STALE

    def get(self, key, create: Callable[[], C.c_void_p]) -> C.c_void_p:
        """The handle built for ``key``; on another key the old handle is destroyed and ``create()`` builds the new one."""
        with self._lock:
            if self._handle is None or key != self._key:
                self._release()
                self._handle, self._key = create(), key
            return self._handle

    def invalidate(self) -> None:
        """Make the next ``get`` build a new handle whatever its key.  The old one is destroyed there, not here: destroying
        frees device memory, which waits for the device."""
        with self._lock:
            self._key = _STALE

    def _release(self) -> None:
        h, self._handle = self._handle, None
        if h is not None:
            getattr(_lib.load(), self._destroy)(h)

    def __del__(self):
        try:
            self._release()
        except Exception:       # noqa: BLE001  (interpreter teardown: the library may already be gone)
            pass

    def __reduce__(self):
        # a copy starts empty: two owners of one C handle would both destroy it
        return NativeHandle, (self._destroy,)


def conv_bn(sd: Dict[str, torch.Tensor], conv: str, bn: str) -> _lib.ConvBN:
    """The ``ConvBN`` of a convolution and the BatchNorm after it, from host f32 tensors the caller keeps alive."""
    return _lib.ConvBN(_lib.fptr(sd[conv + ".weight"]), _lib.fptr(sd[conv + ".bias"]), _lib.fptr(sd[bn + ".weight"]),
                       _lib.fptr(sd[bn + ".bias"]), _lib.fptr(sd[bn + ".running_mean"]), _lib.fptr(sd[bn + ".running_var"]))


class NativeModule(nn.Module):
    """A parameter container whose forward runs on a C handle that the subclass's ``_create()`` builds from its weights,
    with a workspace per stream."""

    def __init__(self, destroy: str):
        super().__init__()
        self._handle = NativeHandle(destroy)
        self._ws = StreamScratch()
        self._tensors = None

    def _native(self) -> C.c_void_p:
        # cheap per-call staleness check: the compute dtype, where the module has one, and identity + in-place version
        # counter of every weight tensor (load_state_dict copies in place and bumps _version; .to()/.cuda() replace .data)
        if self._tensors is None:
            self._tensors = list(self.parameters()) + list(self.buffers())
        key = (getattr(self, "compute_dtype", None),) + tuple((t.data_ptr(), t._version) for t in self._tensors)
        return self._handle.get(key, self._create)

    def _apply(self, fn, *args, **kwargs):
        self._tensors = None
        return super()._apply(fn, *args, **kwargs)

    def invalidate(self) -> None:
        """Rebuild the handles of this module and of every native module inside it on their next call: for writers that
        change the weights without bumping their versions, or rebind them to other tensors."""
        for m in self.modules():
            if isinstance(m, NativeModule):
                m._tensors = None
                m._handle.invalidate()

    def _host_weights(self) -> Dict[str, torch.Tensor]:
        return {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in self.state_dict().items()}

    def _gpu_input(self, x: torch.Tensor, channels: int = 1) -> torch.Tensor:
        """The refusals every forward shares, then ``x`` as a contiguous float32 tensor on the current GPU."""
        if self.training:
            raise RuntimeError(f"{type(self).__name__} on the MI355X path is inference-only: call .eval()")
        if x.dim() != 4 or x.shape[1] != channels:
            raise ValueError(f"expected input (B, {channels}, H, W), got {tuple(x.shape)}")
        return x.detach().to(device=cuda_device(), dtype=torch.float32).contiguous()
