"""What every device-handle class of the Python API inherits (so_dso_place_recognition_amd/_handle.py), against a fake context and a fake
library that only record calls: close's rule, the one tensor check in its three modes, the out= / info= helper and the caller-or-own
buffers.  CPU tensors only: no GPU and no libpr_amd.so call is involved."""
import types

import pytest
import torch

from so_dso_place_recognition_amd import _handle


class FakeLib:
    def __init__(self):
        self.destroyed = []

    def pr_fake_destroy(self, h):
        self.destroyed.append(h)


class FakeHandle(_handle.Handle):
    _DESTROY = "pr_fake_destroy"


def make(h=7, ctx_h=1):
    x = FakeHandle.__new__(FakeHandle)                 # no constructor: the base needs none
    x.ctx = types.SimpleNamespace(h=ctx_h, device=0)
    x.lib, x.h = FakeLib(), h
    return x


def test_close_destroys_exactly_once():
    x = make()
    x.close()
    assert x.lib.destroyed == [7] and x.h is None
    x.close()                                          # closed already: no second call
    assert x.lib.destroyed == [7] and x.h is None


@pytest.mark.parametrize("h,ctx_h", [(None, 1), (7, None)])
def test_close_makes_no_call_without_a_handle_or_a_live_context(h, ctx_h):
    x = make(h, ctx_h)
    x.close()
    assert x.lib.destroyed == [] and x.h is None


def test_del_swallows_what_close_raises():
    x = make()
    x.lib.pr_fake_destroy = lambda h: 1 / 0
    with pytest.raises(ZeroDivisionError):
        x.close()
    x.h = 7
    x.__del__()                                        # the same failure, swallowed
    bare = FakeHandle.__new__(FakeHandle)              # not even a context: close raises AttributeError, __del__ does not
    bare.h = 7
    bare.__del__()


def test_contexts_must_be_shared():
    x = make()
    x._share("Fake", "the fake and the map", types.SimpleNamespace(ctx=x.ctx))
    with pytest.raises(ValueError, match=r"Fake: the fake and the map must share one context \(one stream\)"):
        x._share("Fake", "the fake and the map", types.SimpleNamespace(ctx=x.ctx), types.SimpleNamespace(ctx=object()))


CPU = torch.device("cpu")
MODES = [dict(shape=(4, 3)), dict(numel=12), dict(numel_min=12)]


class OnDevice:
    """A stand-in that is "on the device" the check asks for, so that the checks behind is_cuda can be reached without a GPU."""

    def __init__(self, t, device=CPU):
        self.t, self.is_cuda, self.device = t, True, device
        self.dtype, self.shape = t.dtype, t.shape

    def is_contiguous(self):
        return self.t.is_contiguous()

    def numel(self):
        return self.t.numel()


@pytest.mark.parametrize("mode", MODES, ids=lambda m: next(iter(m)))
def test_the_check_refuses_in_every_mode(mode):
    good = torch.zeros((4, 3), dtype=torch.float64)
    ok = OnDevice(good)
    assert _handle.check("who", "x", ok, torch.float64, CPU, **mode) is ok
    bad = {"not on a GPU": good,
           "another device": OnDevice(good, torch.device("meta")),
           "another dtype": OnDevice(good.to(torch.float32)),
           "not contiguous": OnDevice(torch.zeros((3, 4), dtype=torch.float64).t()),
           "another size": OnDevice(torch.zeros((5, 2), dtype=torch.float64))}
    for why, t in bad.items():
        with pytest.raises(ValueError, match="^who: x must be ") as e:
            _handle.check("who", "x", t, torch.float64, CPU, on="the fake's device", **mode)
        assert ("[4, 3]" in str(e.value)) if (why == "another size" and "shape" in mode) else ("the fake's device" in str(e.value)), why
        with pytest.raises(ValueError, match="^spelled out$"):
            _handle.check("who", "x", t, torch.float64, CPU, msg="spelled out", **mode)
    assert "of 12 elements" in str(pytest.raises(ValueError, _handle.check, "who", "x", good, torch.float64, CPU, numel=12).value)
    assert "of at least 12 elements" in str(pytest.raises(ValueError, _handle.check, "who", "x", good, torch.float64, CPU, numel_min=12).value)


def test_a_minimum_count_admits_more_and_an_exact_one_does_not():
    big = OnDevice(torch.zeros(13, dtype=torch.float64))
    assert _handle.check("who", "x", big, torch.float64, CPU, numel_min=12) is big
    with pytest.raises(ValueError, match="who: x must be"):
        _handle.check("who", "x", big, torch.float64, CPU, numel=12)


def test_a_handle_without_a_context_still_refuses_a_host_tensor():
    bare = FakeHandle.__new__(FakeHandle)
    with pytest.raises(ValueError, match="^who: x must be a contiguous CUDA tensor"):
        bare._t("who", "x", torch.zeros(3, dtype=torch.int32), torch.int32, numel=3)


def test_a_result_is_validated_or_made():
    made = _handle.result("who", "out", None, torch.int32, (2, 3), CPU, zeros=True)
    assert made.shape == (2, 3) and made.dtype == torch.int32 and not made.any()
    with pytest.raises(ValueError, match="who: out must be"):
        _handle.result("who", "out", made, torch.int32, (2, 3), CPU)          # an earlier result that is not on a GPU
    flat = OnDevice(torch.zeros(6, dtype=torch.int32))
    assert _handle.result("who", "out", flat, torch.int32, (2, 3), CPU, flat=True) is flat
    with pytest.raises(ValueError, match=r"who: out must be \[2, 3\]"):
        _handle.result("who", "out", flat, torch.int32, (2, 3), CPU)


def test_buffers_are_refused_before_anything_is_set(monkeypatch):
    x = make()
    monkeypatch.setattr(FakeHandle, "_device", CPU)
    shapes = dict(a=((2, 3), torch.float64), b=((4,), torch.int32))
    a, b = OnDevice(torch.zeros((2, 3), dtype=torch.float64)), OnDevice(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(KeyError):
        x._buffers("Fake", shapes, dict(a=a))                                 # a name is missing
    with pytest.raises(ValueError, match=r"Fake: buffer b must be a contiguous CUDA tensor torch.int32 \[4\]"):
        x._buffers("Fake", shapes, dict(a=a, b=OnDevice(torch.zeros(5, dtype=torch.int32))))
    assert not hasattr(x, "a") and not hasattr(x, "b") and x.lib.destroyed == []
    x._buffers("Fake", shapes, dict(a=a, b=b))
    assert x.a is a and x.b is b
