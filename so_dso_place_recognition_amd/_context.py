"""Context: one HIP device + stream of the library (pr_ctx), the process-wide default context and the per-device contexts the torch
forms join to torch's current stream.  Everything else in the package is built over a Context; `api` re-exports these names."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib
from ._lib import PRError

class Context:
    """One HIP device + stream (pr_ctx)."""

    def __init__(self, device: int = 0, sc_arith: str | None = None, stream: int | None = None, nan_policy: str | None = None,
                 exact_statistics: bool | None = None, sc_binary: bool | None = None):
        """sc_arith: None (library default: "f16x2", or PR_SC_MATCH=f32 from the environment), "f16x2" or "f32".
        exact_statistics: True = every query of a top-k call gets fp64 row statistics (pr_set_exact_statistics: scores are the reference's
        doubles to rounding, at 2.3 ms per query and 100k entries).
        stream: a hipStream_t the caller owns (e.g. torch.cuda.current_stream().cuda_stream; 0 = the null stream): the
        context's kernels are enqueued there (pr_create_on_stream).  nan_policy: "exclude" (default, MATLAB's behaviour for
        zero-norm SC rows) or "fail" (PR_ENAN)."""
        self.lib = _lib.load()
        h = C.c_void_p()
        if stream is None:
            rc = self.lib.pr_create(device, C.byref(h))
        else:
            rc = self.lib.pr_create_on_stream(device, C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise PRError(rc, self.lib.pr_last_error(None).decode())
        self.h = h
        self.device = device
        if sc_arith is not None:
            self.check(self.lib.pr_set_sc_arith(h, {"f16x2": _lib.SC_ARITH_F16X2, "f32": _lib.SC_ARITH_F32, "f16": _lib.SC_ARITH_F16}[sc_arith]))
        if nan_policy is not None:
            self.check(self.lib.pr_set_nan_policy(h, {"exclude": _lib.NAN_EXCLUDE, "fail": _lib.NAN_FAIL}[nan_policy]))
        self.exact_statistics = bool(exact_statistics) if exact_statistics is not None else os.environ.get("PR_FORCE_ORDER_FLAGS") == "1"
        if exact_statistics is not None:
            self.check(self.lib.pr_set_exact_statistics(h, int(bool(exact_statistics))))
        if sc_binary is not None:      # False: a binary intensity channel goes through the split-f16 kernel like any other (pr_set_sc_binary)
            self.check(self.lib.pr_set_sc_binary(h, int(bool(sc_binary))))

    def kernel_timing(self, on: bool):
        """HIP events around the matcher launches of pr_distances_dev (pr_set_kernel_timing)."""
        self.check(self.lib.pr_set_kernel_timing(self.h, int(bool(on))))

    def last_distance_timing(self):
        """(ms channel-0 or only launch, ms channel-1 single-product launch, ms channel-1 split-f16 launch) of the last timed call."""
        ms = (C.c_float * 3)()
        self.check(self.lib.pr_last_distance_timing(self.h, ms))
        return float(ms[0]), float(ms[1]), float(ms[2])

    def take_warnings(self) -> int:
        """PR_WARN_* bits raised since the last call (1: zero-norm SC rows excluded, 2: an M2DP singular pair did not converge)."""
        return int(self.lib.pr_take_warnings(self.h))

    @property
    def sc_arith(self) -> str:
        return {_lib.SC_ARITH_F32: "f32", _lib.SC_ARITH_F16: "f16"}.get(self.lib.pr_get_sc_arith(self.h), "f16x2")

    def close(self):
        if getattr(self, "h", None):
            self.lib.pr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        _lib.check(self.h, rc)

    def sync(self):
        self.check(self.lib.pr_sync(self.h))

    @property
    def stream(self) -> int:
        return int(self.lib.pr_stream(self.h) or 0)


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


_torch_ctx = {}      # device -> (Context on its own stream, that stream as a torch.cuda.ExternalStream): one per device, for the process


def _torch_default_context(device: int):
    import torch
    if device not in _torch_ctx:
        c = Context(device)
        _torch_ctx[device] = (c, torch.cuda.ExternalStream(c.stream, device=device))
    return _torch_ctx[device]
