"""One driver over the two forms of an Ogg object of the C ABI, the host twin (vbm_host_ogg_*) and the device form
(vbm_ogg_*): the handle, buffers as numpy arrays or torch tensors, the call by name, the status, and buffers with blank
guard elements behind them.  It talks to the library through ctypes with raw addresses, past the package's wrapper
classes: the tests that use it drive short capacities, guards and bad arguments."""
import ctypes as C

import numpy as np

BLANK = {np.uint8: 0xA5, np.int64: -0x5A5A}


def lib():
    from vorbis_aotuv_lancer_amd._lib import lib
    return lib


class Result:
    pass


class Twin:
    """impl 'host': numpy arrays and vbm_host_ogg_<name>; 'device': torch tensors and vbm_ogg_<name> on the current
    stream.  kind names create and destroy, status_name the status call (<kind>_status unless given)."""

    def __init__(self, impl, kind, *create_args, status_name=None):
        self.impl, self.kind, self.lib = impl, kind, lib()
        self.status_name = status_name or kind + "_status"
        self.h = C.c_void_p()
        rc = self.fn(kind + "_create")(C.byref(self.h), *create_args)
        assert rc == 0, (rc, self.lib.vbm_last_error())
        self.keep = None

    def close(self):
        if self.impl == "device":
            import torch
            torch.cuda.synchronize()
        getattr(self.lib, f"vbm_ogg_{self.kind}_destroy")(self.h)

    # buffers: numpy on the host, torch on the device; ptr / back convert
    def new(self, n, dtype, fill=None):
        if self.impl == "host":
            return np.zeros(n, dtype) if fill is None else np.full(n, fill, dtype)
        import torch
        t = {np.uint8: torch.uint8, np.int64: torch.int64}[dtype]
        return torch.zeros(n, dtype=t, device="cuda") if fill is None else torch.full((n,), fill, dtype=t, device="cuda")

    def ptr(self, a):
        return a.ctypes.data if self.impl == "host" else a.data_ptr()

    def back(self, a):
        return a if isinstance(a, np.ndarray) else a.cpu().numpy()

    def upload(self, data):
        """uint8 numpy -> the address a call takes (kept alive here), None for no bytes"""
        if self.impl == "device":
            import torch
            data = torch.from_numpy(data.copy()).cuda()
        self.keep = data
        return self.ptr(data) if len(data) else None

    def q(self):
        """the current stream; None on the host"""
        if self.impl == "host":
            return None
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn(self, name):
        return getattr(self.lib, f"vbm_host_ogg_{name}" if self.impl == "host" else f"vbm_ogg_{name}")

    def call(self, name, *args):
        """vbm_host_ogg_<name>(h, args) or vbm_ogg_<name>(h, args, stream) -> its return code"""
        return self.fn(name)(self.h, *args) if self.impl == "host" else self.fn(name)(self.h, *args, self.q())

    def status(self):
        st = C.c_int(-7)
        assert getattr(self.lib, f"vbm_ogg_{self.status_name}")(self.h, C.byref(st), self.q()) == 0
        return st.value

    # guards: a buffer is made blank, with blank elements behind it; after the call the part in front tells whether
    # anything was written, and the part behind must be as it was
    def guarded(self, n, dtype, guard):
        return self.new(n + guard, dtype, BLANK[dtype])

    def unguard(self, buf, n):
        """a guarded buffer of n elements (or a part of one, copied back already) -> (its n elements as numpy, touched,
        guards_ok)"""
        a = self.back(buf)
        blank = BLANK[a.dtype.type]
        return a[:n], bool((a[:n] != blank).any()), bool((a[n:] == blank).all())
