"""What the torch front ends do between a tensor and an argument of the C ABI, written once: pointers, streams,
padded rows, the agent's arrays and the launch itself."""
import contextlib
import ctypes as C

import torch

from . import _lib


def ptr(t, dtype=None, memory_format=torch.contiguous_format):
    """Address of a device tensor contiguous in `memory_format` (None stays None), of element type `dtype` if given."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(memory_format=memory_format), "expected a contiguous device tensor"
    assert dtype is None or t.dtype == dtype, "expected %s, got %s" % (dtype, t.dtype)
    return C.c_void_p(t.data_ptr())


def stream(where):
    """The current stream of a device, or of a tensor's device."""
    return C.c_void_p(torch.cuda.current_stream(getattr(where, "device", where)).cuda_stream)


def inner(t, nlead=1):
    """Elements of one row of a [*lead, ...] tensor; the dims after the nlead leading ones must be dense."""
    n = 1
    for d in range(t.dim() - 1, nlead - 1, -1):
        assert t.stride(d) == n or t.shape[d] == 1, "the rows must be dense"
        n *= t.shape[d]
    return n


def rows(t, dtype):
    """(pointer, pitch in elements, N, row elements) of a [N, ...] tensor whose rows are dense but may be padded."""
    assert t.is_cuda and t.dtype == dtype and t.dim() >= 2, "expected a [N, ...] %s device tensor" % dtype
    n = inner(t)
    pitch = t.stride(0) if t.shape[0] > 1 else n
    assert pitch >= n
    return C.c_void_p(t.data_ptr()), int(pitch), int(t.shape[0]), n


def agent_arrays(x, y, dir=None):
    """(pointer x, pointer y, pointer dir or None, stride): the agent arguments of the C ABI for 1-D int32 device
    tensors of one length that share one positive element stride -- contiguous arrays (stride 1), or column views of an
    [N, TW_REC_WORDS] record tensor (TwoarmyEngine.agent_views()), read where they live.  Length 1: stride 1."""
    given = [t for t in (x, y, dir) if t is not None]
    for t in given:
        assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 1, "expected 1-D int32 device tensors"
        assert t.shape == x.shape and t.device == x.device, "the agent arrays must have one length and device"
    strides = {t.stride(0) if x.shape[0] > 1 else 1 for t in given}
    assert len(strides) == 1 and min(strides) > 0, "the agent arrays must share one positive stride"
    return tuple(None if t is None else C.c_void_p(t.data_ptr()) for t in (x, y, dir)) + (strides.pop(),)


def call(name, dev, *args):
    """lib.<name>(*args, stream) on the torch.device `dev` (or a tensor's), whichever device is current, on its current
    stream.  No device guard where `dev` is current: one per launch cost the 256-env rollout 4 %."""
    dev = getattr(dev, "device", dev)
    here = dev.index in (None, torch.cuda.current_device())
    with contextlib.nullcontext() if here else torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), name)(*args, stream(dev)), name)


_constants = {}


def constant(key, values, dtype, device):
    """A small device constant made from Python numbers, once per (key, dtype, device) and kept: making it is a
    pageable host-to-device copy, which blocks the host and cannot be captured in a graph, so no call after the first
    makes one.  The copy is complete when the first call returns; the tensor is read-only to every user."""
    device = torch.device(device)
    k = (key, dtype, device)
    if k not in _constants:
        _constants[k] = torch.tensor(values, dtype=dtype, device=device)
    return _constants[k]


def query(name, *args):
    """lib.<name>(*args) of a size query: the value, or the error a negative one stands for."""
    n = getattr(_lib.lib(), name)(*args)
    _lib.check(min(n, 0), name)
    return n
