"""What the device-handle classes of the Python API share (CloudWindow ... MapGrower in mapping, online, graph and registration): the
two pointer helpers, the ONE check of a device tensor, the result helper for out= / info=, and the handle base class with its close /
__del__, its context refusals and its caller-or-own buffers.  Like api, importing this module does not import torch: torch is imported
inside the calls, and the callers hand in torch's dtypes and devices."""
from __future__ import annotations

import ctypes as C
import math

from ._context import default_context


def _ptr(a):
    """The pointer of a NumPy array for the C ABI (None: NULL)."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def ptr(t):
    """The device pointer of a torch tensor for the C ABI (None: NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def check(who, name, t, dtype, device, shape=None, numel=None, numel_min=None, on="the context's device", msg=None):
    """The tensor check in front of every library call: t must be a contiguous CUDA tensor of `dtype` on `device` and have the exact
    `shape`, exactly `numel` or at least `numel_min` elements (at most one of the three; none: any size).  Raises ValueError
    "who: name must be ..."; `on` is how the caller's family names the device; msg: the whole text instead, for the calls whose refusal
    spells the expected layout out.  Returns t."""
    ok = t.is_cuda and t.device == device and t.dtype == dtype and t.is_contiguous()
    sized = (numel is None or t.numel() == numel) and (numel_min is None or t.numel() >= numel_min)
    if msg is not None and not (ok and sized and (shape is None or tuple(t.shape) == tuple(shape))):
        raise ValueError(msg)
    if numel is not None or numel_min is not None:
        if not (ok and sized):
            raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor {dtype} of "
                             f"{numel if numel is not None else f'at least {numel_min}'} elements on {on}")
    elif not ok:
        raise ValueError(f"{who}: {name} must be a contiguous CUDA tensor {dtype} on {on}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be {list(shape)}")
    return t


def check_each(msg, device, tensors, dtypes):
    """check() of several tensors whose refusal is one text that names them all."""
    for t, dtype in zip(tensors, dtypes):
        check(None, None, t, dtype, device, msg=msg)


def result(who, name, t, dtype, shape, device, flat=False, zeros=False, **how):
    """An out= / info= tensor: None -> a new one of `shape` on `device` (zeros: filled), else the caller's earlier one, checked for
    that shape (flat: for that many elements), with check's on= / msg=."""
    import torch
    if t is None:
        return (torch.zeros if zeros else torch.empty)(shape, dtype=dtype, device=device)
    if flat:
        return check(who, name, t, dtype, device, numel=math.prod(shape), **how)
    return check(who, name, t, dtype, device, shape=shape, **how)


class Handle:
    """The base of every device-resident handle of one C family: .ctx (the context whose stream its calls are enqueued on), .lib, .h
    (None until created and after close).  A subclass names its family's destroy function (_DESTROY) and, where its refusals call the
    device something else, _ON and _device.  Nothing here runs at construction: an object made by __new__ with the attributes a method
    reads set by hand refuses like any other."""

    _DESTROY = None
    _ON = "the context's device"

    def _attach(self, ctx):
        self.ctx = ctx or default_context()
        self.lib, self.h = getattr(self.ctx, "lib", None), None      # (what is no Context is refused by the constructor's checks that follow)

    def _share(self, who, whom, *others):
        """a handle built over other handles, or given one in a call: all of them on this one's context"""
        if any(o.ctx is not self.ctx for o in others):
            raise ValueError(f"{who}: {whom} must share one context (one stream)")

    @property
    def _device(self):
        import torch
        return torch.device("cuda", self.ctx.device)

    def _t(self, who, name, t, dtype, shape=None, numel=None, numel_min=None, msg=None):
        # (a tensor that is on no GPU is refused whatever the device is: an object made without a context refuses it too)
        return check(who, name, t, dtype, self._device if t.is_cuda else None, shape, numel, numel_min, on=self._ON, msg=msg)

    def _result(self, who, name, t, dtype, shape, **how):
        return result(who, name, t, dtype, shape, self._device, on=self._ON, **how)

    def _buffers(self, who, shapes, buffers):
        """Caller-or-own buffers, shapes = {name: (shape, dtype)}: zeroed tensors on the handle's device unless the caller's dict
        `buffers` brings them; every one is checked before the first becomes an attribute of its name."""
        import torch
        if buffers is None:
            buffers = {n: torch.zeros(s, dtype=dt, device=self._device) for n, (s, dt) in shapes.items()}
        for n, (s, dt) in shapes.items():
            self._t(who, n, buffers[n], dt, shape=s, msg=f"{who}: buffer {n} must be a contiguous CUDA tensor {dt} {list(s)}")
        for n in shapes:
            setattr(self, n, buffers[n])

    def close(self):
        """No library call when the handle was never created, is closed already or its context is closed; .h is None afterwards."""
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            getattr(self.lib, self._DESTROY)(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
