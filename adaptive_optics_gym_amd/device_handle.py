"""What the wrappers of the library's stand-alone handles share (the six of ``_lib.STANDALONE``, ``aog_predictor`` to ``aog_servo``: per-env records on
one device, independent of any ``aog_env``): the handle's life, the stream, the argument checks and the checkpoint calls.  The host's side of
the same life is ``csrc/standalone_handle.h``."""
from __future__ import annotations

import ctypes as C

from . import _lib


def check_measurement(env, measurement):
    """ValueError unless ``measurement`` names a pseudo-open-loop measurement ``env`` can take (``predictor.pseudo_open_loop``)."""
    if measurement not in ("truth", "pyramid"):
        raise ValueError(f"measurement must be 'truth' or 'pyramid' (got {measurement!r})")
    if measurement == "pyramid" and getattr(env, "pyramid", None) is None:
        raise ValueError("measurement='pyramid' needs an env created with pyramid=dict(...)")


def ptr(t):   # the address of a tensor as a ctypes pointer argument (None: NULL)
    return C.c_void_p(t.data_ptr() if t is not None else None)


class DeviceHandle:
    """A subclass names its entry points (``prefix`` + ``_create`` / ``_destroy`` / ``_state_bytes`` / ``_get_state`` / ...) and what ``set_state``'s
    message calls it (``noun``), builds the ``aog_*_config`` in ``_config()`` and calls ``_bind`` first; ``_create()`` makes the handle (``lazy``: the first ``_call``)."""

    prefix = noun = ""
    lazy = False
    lib = None
    _handle = None

    def _bind(self, torch, device, batch):
        self._torch, self._batch = torch, int(batch)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda" and self.device.index is None:   # (the current one)
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)

    _load = staticmethod(_lib.load)

    def _create(self):
        self.lib = self.lib or self._load()
        cfg, h = self._config(), C.c_void_p()
        _lib.check(getattr(self.lib, self.prefix + "_create")(C.byref(cfg), self.device.index or 0, C.byref(h)))
        self._handle = h

    def _h(self):
        if self._handle is None and self.lazy:
            self._create()
        return self._handle

    def _call(self, name, *args):
        h = self._h()
        _lib.check(getattr(self.lib, f"{self.prefix}_{name}")(h, *args))

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _mask(self, mask, who):
        if mask is None:
            return None
        torch = self._torch
        m = torch.as_tensor(mask, device=self.device)
        if m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != (self._batch,):
            raise ValueError(f"{who}: mask must be a bool vector of {self._batch} entries")
        return m.to(torch.uint8).contiguous()

    def _tensor(self, t, shape, dtype, message):   # t if it is a contiguous dtype tensor of shape on the device; ValueError(message) otherwise
        if (not isinstance(t, self._torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape)
                or t.device != self.device):
            raise ValueError(message)
        return t

    def _state_bytes(self):
        h = self._h()
        return int(getattr(self.lib, self.prefix + "_state_bytes")(h))

    def get_state(self):
        """The state blob, a uint8 device tensor (``unpack`` names what it holds)."""
        blob = self._torch.empty((self._state_bytes(),), dtype=self._torch.uint8, device=self.device)
        self._call("get_state", ptr(blob), self._stream())
        return blob

    def set_state(self, blob):
        torch = self._torch
        n = self._state_bytes()
        b = torch.as_tensor(blob)
        if b.dtype != torch.uint8 or tuple(b.shape) != (n,):
            raise ValueError(f"set_state: the blob of this {self.noun} is a uint8 vector of {n} bytes")
        b = b.to(self.device).contiguous()
        self._call("set_state", ptr(b), self._stream())
        torch.cuda.current_stream(self.device).synchronize()   # (b may be a temporary)

    def close(self):
        h, self._handle = self._handle, None
        if h:
            getattr(self.lib, self.prefix + "_destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
