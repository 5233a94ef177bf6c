"""What the GPU tests of the PPO kernels (csrc/ppo_kernels.hip) share: the front end, the loaded library and its Python
module under two names, host -> device copies, raw pointers for calls made past the front end, and a rejected-call
check.  A plain module like nav_util.py; helpers whose behaviour differs between the test files stay in those files."""
import ctypes as C

import numpy as np
import torch

DEV = "cuda"
TW_E_ARG = -1


def ops():
    from twoarmy_amd import ppo_ops
    return ppo_ops


def lib_module():
    """twoarmy_amd._lib: TwoarmyLibraryError, check(), lib()."""
    from twoarmy_amd import _lib
    return _lib


def lib():
    """The loaded library: the C ABI itself."""
    return lib_module().lib()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ptr(t, off=0):
    """Address of a tensor's first element plus `off` bytes; None stays NULL."""
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def accepted(fn, args):
    rc = getattr(lib(), fn)(*args, stream())
    torch.cuda.synchronize()
    return rc == 0


def rejected(fn, args, canaries):
    """lib.<fn>(*args, stream) returns TW_E_ARG and launches nothing: every (tensor, fill value) of `canaries` is as it
    was once the device has caught up."""
    rc = getattr(lib(), fn)(*args, stream())
    torch.cuda.synchronize()
    return rc == TW_E_ARG and all(bool((t == v).all()) for t, v in canaries)
