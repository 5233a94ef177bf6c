"""What the GPU tests of the shortest-path kernels share: host <-> device copies, bit-for-bit comparison, 0xA5-filled
output buffers and hindsight records made of runs.  A plain module like golden_util.py; helpers whose behaviour differs
between the test files (positions, raw_call) stay in those files."""
import numpy as np
import torch

DEV = "cuda:0"


def dev(x):
    """A device copy of an array (the shared cases are read-only); None stays None."""
    return None if x is None else torch.from_numpy(np.array(x)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def all_same(got, want):
    return all(same(g, w) for g, w in zip(got, want))


def u16_full(shape, byte=0xA5):
    """A uint16 device tensor with every byte = `byte` (torch's uint16 has views and copies, little else)."""
    n = int(np.prod(shape))
    return torch.full((2 * n,), byte, dtype=torch.uint8, device=DEV).view(torch.uint16).view(shape)


class Boxed:
    """A device tensor of `n` elements at element offset `off` from a 16-byte boundary inside a 0xA5-filled buffer."""

    def __init__(self, n, dtype, off=0, shape=None):
        size = torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full(((16 // size + off + n) * size + 48,), 0xA5, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = 16 + off * size, 16 + (off + n) * size
        self.view = self.buf[self.lo:self.hi].view(dtype).view(shape if shape is not None else (n,))
        assert self.buf.data_ptr() % 16 == 0 and (n == 0 or self.view.data_ptr() % 16 == (off * size) % 16)

    def borders_intact(self):
        b = host(self.buf)
        return bool((b[:self.lo] == 0xA5).all() and (b[self.hi:] == 0xA5).all())

    def untouched(self):
        return bool((host(self.buf) == 0xA5).all())


def runs_to_records(rng, c, runs, T):
    """runs = [(env, goal cell, length)] -> (t, n, goal): consecutive steps inside a run, as ppo_her_relabel emits them,
    the goal anywhere inside its cell."""
    W = c["W"]
    t = np.concatenate([(rng.integers(0, T) + np.arange(L)) % T for _, _, L in runs]).astype(np.int32)
    n = np.concatenate([np.full(L, e) for e, _, L in runs]).astype(np.int32)
    g = np.concatenate([np.full(L, gc) for _, gc, L in runs])
    frac = rng.choice([0.0, 0.25, 0.999], (len(g), 2))
    goal = (np.stack([g // W, g % W], 1) + frac).astype(np.float32)
    return t, n, goal


def random_records(rng, c, R, T, mean_run=9):
    """R records as runs of one env under one goal of its pool, the runs in any env order."""
    runs, left = [], R
    while left:
        L = int(min(left, 1 + rng.integers(0, 2 * mean_run)))
        e = int(rng.integers(0, c["N"]))
        runs.append((e, int(c["pool"][e][rng.integers(0, 3)]), L))
        left -= L
    return runs_to_records(rng, c, runs, T)
