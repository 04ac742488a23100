"""What every library handle does the same way: creation from its config struct, close / __del__, the current stream
of its device as the stream argument, and the *_check call of the device-side handles.  A subclass names its symbol
prefix (uavtrack_<kind>_) and sets self.device before _create."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def current_device(device) -> torch.device:
    """torch.device(device), a bare "cuda" taken as the current device."""
    device = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


class Handle:
    _prefix = "uavtrack_"

    def _create(self, cfg: C.Structure) -> None:
        """The handle from its config struct (struct_size is filled in here)."""
        cfg.struct_size = C.sizeof(cfg)
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(getattr(self._lib, self._prefix + "create")(C.byref(cfg), C.byref(h)), self._prefix + "create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._lib, self._prefix + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self) -> None:
        """Synchronises; raises if a call since the last check was refused on the device."""
        _lib.check(getattr(self._lib, self._prefix + "check")(self._h, None, self._stream()), self._prefix + "check")
