"""Torch front end of the observation wrappers (include/minigrid_obs.h, csrc/minigrid_obs.hip): the one-hot, fully
observable, symbolic and flat observations and the direction to the goal of the reference's gym_minigrid/wrappers.py
(:117-154, :220-246, :497-526, :367-425, :463-494), computed on the device for N envs per launch, byte for byte what the
reference returns.  World planes are uint8[N, H*W] with cell (x, y) at y*W + x; agent_* are int32[N] tensors, or
`agent_ptrs=(address_x, address_y, address_dir, stride)` to read them where they live (the engine's records).
No CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib

ONEHOT_BITS = 21
NUM_CHAR_CODES = 28
SLOPE, ANGLE = 0, 1
_MODES = {"slope": SLOPE, "angle": ANGLE}


def _p(t, dtype):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous() and t.dtype == dtype, "expected contiguous %s device tensor" % dtype
    return C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _rows(t, dtype):
    """(pointer, pitch in elements, N, row elements) of a [N, ...] tensor whose rows are dense but may be padded."""
    assert t.is_cuda and t.dtype == dtype and t.dim() >= 2, "expected a [N, ...] %s device tensor" % dtype
    inner = 1
    for d in range(t.dim() - 1, 0, -1):
        assert t.stride(d) == inner or t.shape[d] == 1, "the rows must be dense"
        inner *= t.shape[d]
    pitch = t.stride(0) if t.shape[0] > 1 else inner
    assert pitch >= inner
    return C.c_void_p(t.data_ptr()), int(pitch), int(t.shape[0]), int(inner)


def _agent(agent_x, agent_y, agent_dir, agent_ptrs):
    if agent_ptrs is not None:
        ax, ay, ad, stride = agent_ptrs
        return C.c_void_p(ax), C.c_void_p(ay), (C.c_void_p(ad) if ad is not None else None), int(stride)
    return _p(agent_x, torch.int32), _p(agent_y, torch.int32), _p(agent_dir, torch.int32), 1


def onehot(image, out=None, want_error=False):
    """image uint8[N, ..., 3] (rows may be padded) -> uint8[N, ..., 21], the reference's index semantics; with want_error
    also int32[N]: 1 where an index was 21 or more (the reference's IndexError)."""
    assert image.shape[-1] == 3
    ip, ipitch, N, row = _rows(image, torch.uint8)
    n_cells = row // 3
    dev = image.device
    if out is None:
        out = torch.empty(tuple(image.shape[:-1]) + (ONEHOT_BITS,), dtype=torch.uint8, device=dev)
    op, opitch, No, orow = _rows(out, torch.uint8)
    assert No == N and orow == n_cells * ONEHOT_BITS and out.device == dev
    err = torch.empty(N, dtype=torch.int32, device=dev) if want_error else None
    _lib.check(_lib.lib().mg_obs_onehot(ip, ipitch, N, n_cells, op, opitch, _p(err, torch.int32), _stream(dev)),
               "mg_obs_onehot")
    return (out, err) if want_error else out


def full_obs(type_plane, colour_plane, state_plane, width, height, agent_x=None, agent_y=None, agent_dir=None,
             agent_ptrs=None, out=None, want_error=False):
    """-> uint8[N, W, H, 3]: Grid.encode() with the agent's cell set to (10, 0, agent_dir).  With want_error also
    int32[N]: 2 where the agent lies outside the world."""
    N, W, H = type_plane.shape[0], int(width), int(height)
    assert type_plane.shape == (N, W * H) and colour_plane.shape == (N, W * H)
    dev = type_plane.device
    if out is None:
        out = torch.empty((N, W, H, 3), dtype=torch.uint8, device=dev)
    op, opitch, No, orow = _rows(out, torch.uint8)
    assert No == N and orow == W * H * 3
    err = torch.empty(N, dtype=torch.int32, device=dev) if want_error else None
    ax, ay, ad, stride = _agent(agent_x, agent_y, agent_dir, agent_ptrs)
    _lib.check(_lib.lib().mg_obs_full(_p(type_plane, torch.uint8), _p(colour_plane, torch.uint8),
                                      _p(state_plane, torch.uint8), N, W, H, ax, ay, ad, stride, op, opitch,
                                      _p(err, torch.int32), _stream(dev)), "mg_obs_full")
    return (out, err) if want_error else out


def symbolic_obs(type_plane, width, height, out=None):
    """-> int32[N, W, H, 3] = (x, y, idx), idx -1 for an empty cell; element [x][y] holds the object at flat index
    x*H + y, the reference's reshape (the transposed world on a square grid)."""
    N, W, H = type_plane.shape[0], int(width), int(height)
    assert type_plane.shape == (N, W * H)
    dev = type_plane.device
    if out is None:
        out = torch.empty((N, W, H, 3), dtype=torch.int32, device=dev)
    assert out.shape == (N, W, H, 3)
    _lib.check(_lib.lib().mg_obs_symbolic(_p(type_plane, torch.uint8), N, W, H, _p(out, torch.int32), _stream(dev)),
               "mg_obs_symbolic")
    return out


def mission_tail(mission, maxStrLen=96):
    """float32[maxStrLen * 28] numpy: FlatObsWrapper's one-hot of the mission string (wrappers.py:396-421): a-z, space
    = 26, comma = 27; any other character raises ValueError, a longer string AssertionError."""
    assert len(mission) <= maxStrLen, "mission string too long (%d chars)" % len(mission)
    arr = np.zeros((maxStrLen, NUM_CHAR_CODES), np.float32)
    for idx, ch in enumerate(mission.lower()):
        if "a" <= ch <= "z":
            no = ord(ch) - ord("a")
        elif ch == " ":
            no = 26
        elif ch == ",":
            no = 27
        else:
            raise ValueError("Character %s is not available in mission string." % ch)
        arr[idx, no] = 1
    return arr.reshape(-1)


def flat_obs(image, tail, out=None):
    """image uint8[N, ...] (rows may be padded), tail float32[n_tail] device tensor -> float32[N, n_img + n_tail]."""
    ip, ipitch, N, n_img = _rows(image, torch.uint8)
    dev = image.device
    n_tail = 0 if tail is None else int(tail.numel())
    if out is None:
        out = torch.empty((N, n_img + n_tail), dtype=torch.float32, device=dev)
    op, opitch, No, orow = _rows(out, torch.float32)
    assert No == N and orow == n_img + n_tail
    assert tail is None or tail.device == dev
    _lib.check(_lib.lib().mg_obs_flat(ip, ipitch, N, n_img, _p(tail, torch.float32), n_tail, op, opitch, _stream(dev)),
               "mg_obs_flat")
    return out


def goal_index(type_plane, width, height):
    """-> int32[N]: the first flat index (y*W + x) of a goal in each env's plane, or -1."""
    N = type_plane.shape[0]
    assert type_plane.shape == (N, int(width) * int(height))
    dev = type_plane.device
    out = torch.empty(N, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().mg_obs_goal_index(_p(type_plane, torch.uint8), N, int(width), int(height), _p(out, torch.int32),
                                            _stream(dev)), "mg_obs_goal_index")
    return out


def angle_table(width, height, device=None):
    """float64 table of np.arctan(p / q) for every (p, q) an agent inside the world can produce (layout: minigrid_obs.h);
    evaluated one scalar at a time, the way DirectionObsWrapper evaluates it."""
    W, H = int(width), int(height)
    n = _lib.lib().mg_obs_angle_table_size(W, H)
    assert n == (W + H - 1) * (2 * W - 1)
    tab = np.empty((W + H - 1, 2 * W - 1), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(-(H - 1), W):
            for q in range(-(W - 1), W):
                tab[p + H - 1, q + W - 1] = np.arctan(np.divide(p, q))
    t = torch.from_numpy(tab.reshape(-1))
    return t if device is None else t.to(device)


def goal_direction(goal_idx, width, height, agent_x=None, agent_y=None, agent_ptrs=None, mode="slope", table=None,
                   out=None, want_error=False):
    """-> float64[N]: the slope (goal_position[1] - agent_y) / (goal_position[0] - agent_x) with the reference's
    goal_position = (k // H, k % W), IEEE results kept, or (mode "angle") its np.arctan taken from `table`
    (angle_table(W, H, device)).  With want_error also int32[N]: 1 no goal, 2 agent outside the world (NaN for both)."""
    N = goal_idx.shape[0]
    dev = goal_idx.device
    m = _MODES[mode]
    assert m == SLOPE or (table is not None and table.numel() == (width + height - 1) * (2 * width - 1))
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=dev)
    assert out.shape == (N,)
    err = torch.empty(N, dtype=torch.int32, device=dev) if want_error else None
    ax, ay, _, stride = _agent(agent_x, agent_y, None, agent_ptrs)
    _lib.check(_lib.lib().mg_obs_goal_direction(_p(goal_idx, torch.int32), N, int(width), int(height), ax, ay, stride, m,
                                                _p(table if m == ANGLE else None, torch.float64), _p(out, torch.float64),
                                                _p(err, torch.int32), _stream(dev)), "mg_obs_goal_direction")
    return (out, err) if want_error else out
