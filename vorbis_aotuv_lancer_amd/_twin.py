"""What the two forms of a C object differ in, stated once.  Most objects of the Ogg and range-store ABI come as a device
form (vbm_<stem>) and a host twin (vbm_host_<stem>) whose arguments are the same, but for the stream the device form
takes last (tests/test_twin_signatures_cpu.py holds the ABI to that).  So a wrapper states each call once: Mem makes
the buffers where the object's live, ptr turns them into addresses, and _TwinHandle._call picks the entry point."""
import contextlib
import ctypes as C
import functools

import numpy as np
import torch

from ._lib import lib, check, SIGNATURES

_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}


def ptr(a, when=True):
    """The address of an optional tensor or numpy array for a C call: None for None, and when `when` is false"""
    if a is None or not when:
        return None
    return a.data_ptr() if torch.is_tensor(a) else a.ctypes.data


def size(a):
    """the elements of a tensor or numpy array"""
    return a.numel() if torch.is_tensor(a) else a.size


class Mem:
    """Where an object's buffers live: the host (numpy arrays) or one device (torch tensors)"""

    def __init__(self, device=None):
        self.device = device

    def new(self, n, dtype, zero=False):
        """n elements of a numpy dtype; on the device zeroed only when asked (one fill kernel), on the host always"""
        if self.device is None:
            return np.zeros(n, dtype)
        return (torch.zeros if zero else torch.empty)(n, dtype=_TORCH[np.dtype(dtype)], device=self.device)

    def host(self, a):
        """a buffer of this kind -> numpy: as it is on the host, one D2H copy (which waits for it) from the device"""
        return a if self.device is None else a.cpu().numpy()

    def upload(self, a):
        """a numpy array -> a buffer of this kind: as it is on the host, one H2D copy to the device"""
        if self.device is None:
            return a
        return torch.from_numpy(a.copy()).to(self.device) if len(a) else self.new(0, a.dtype)

    def join(self, blobs):
        """[bytes] -> (raw uint8 [all of them end to end] of this kind, offsets int64 [n + 1] numpy)"""
        off = np.zeros(len(blobs) + 1, np.int64)
        np.cumsum([len(b) for b in blobs], out=off[1:])
        return self.upload(np.frombuffer(b"".join(blobs), np.uint8)), off

    def csr(self, P, B):
        """-> (payload uint8 [B], offsets int64 [P + 1], granulepos int64 [P], eos uint8 [P]) for a fill"""
        return self.new(B, np.uint8), self.new(P + 1, np.int64), self.new(P, np.int64), self.new(P, np.uint8)

    def scope(self):
        """the context in which this kind's calls are made: its device the current one"""
        return contextlib.nullcontext() if self.device is None else torch.cuda.device(self.device)


HOST = Mem()


class Layout:
    """Arrays laid end to end in one block of bytes, so that one copy brings them all back: Layout(name=(dtype, count),
    ...) in the block's order -> .at[name], each one's byte offset, and .size"""

    def __init__(self, **parts):
        self.parts, self.at, self.size = parts, {}, 0
        for name, (dtype, count) in parts.items():
            self.at[name] = self.size
            self.size += np.dtype(dtype).itemsize * count

    def ptrs(self, block):
        """-> {name: the address of that array in the buffer `block`, None for an empty one}"""
        base = ptr(block)
        return {name: base + self.at[name] if count else None for name, (_, count) in self.parts.items()}

    def views(self, block):
        """the block on the host, uint8 numpy -> {name: that array, a view}"""
        return {name: block[self.at[name]:self.at[name] + np.dtype(dtype).itemsize * count].view(dtype)
                for name, (dtype, count) in self.parts.items()}


@functools.lru_cache(maxsize=None)
def _entry(stem, host):
    """-> (the entry point of that form, its name, whether it takes the stream behind the host twin's arguments)"""
    name = ("vbm_host_" if host else "vbm_") + stem
    takes_stream = not host and len(SIGNATURES[name][1]) == len(SIGNATURES["vbm_host_" + stem][1]) + 1
    return getattr(lib, name), name, takes_stream


class _Handle:
    """Owner of the C object ._h: close() destroys it, once, and so do collection and leaving a `with` block"""
    _destroy = None                  # the name of the entry point that destroys it

    def close(self):
        if self._h:
            getattr(lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TwinHandle(_Handle):
    """The handle of a C object that comes as a device form and a host twin (.host says which; .device and .mem: where
    its buffers live)"""
    host, device, mem = False, None, HOST

    def _create(self, stem, host, device, *args):
        """vbm_[host_]<stem>(&h, *args); the device form is made under its device (default: the current one)"""
        self.host, self.device, self._h = bool(host), None, C.c_void_p()
        if not host:
            self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.mem = Mem(self.device)
        fn, name, _ = _entry(stem, self.host)
        with self.mem.scope():
            check(fn(C.byref(self._h), *args), name)

    def _q(self):
        """the current stream of the device; None for the host twin"""
        return None if self.host else C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, stem, *args):
        """vbm_host_<stem>(h, *args) or vbm_<stem>(h, *args[, the current stream]), checked under its own name"""
        fn, name, takes_stream = _entry(stem, self.host)
        check(fn(self._h, *args, self._q()) if takes_stream else fn(self._h, *args), name)

    def _status(self, stem):
        """the status word behind the work enqueued so far: vbm_<stem>, one form that takes the stream or None"""
        st = C.c_int(-1)
        check(getattr(lib, "vbm_" + stem)(self._h, C.byref(st), self._q()), "vbm_" + stem)
        return st.value

    def close(self):
        if self._h and self.device is not None:
            torch.cuda.synchronize(self.device)
        super().close()
