"""Torch front end of the observation wrappers (include/minigrid_obs.h, csrc/minigrid_obs.hip): the one-hot, fully
observable, symbolic and flat observations and the direction to the goal of the reference's gym_minigrid/wrappers.py
(:117-154, :220-246, :497-526, :367-425, :463-494), computed on the device for N envs per launch, byte for byte what the
reference returns.  World planes are uint8[N, H*W] with cell (x, y) at y*W + x; agent_* are int32[N] tensors, dense or
the column views of the engine's records (TwoarmyEngine.agent_views()), which are then read where they live.  Every
launch goes to its tensors' device.  No CPU fallback."""
import numpy as np
import torch

from . import _lib
from ._marshal import agent_arrays, call, ptr, rows

ONEHOT_BITS = 21
NUM_CHAR_CODES = 28
SLOPE, ANGLE = 0, 1
_MODES = {"slope": SLOPE, "angle": ANGLE}


def onehot(image, out=None, want_error=False):
    """image uint8[N, ..., 3] (rows may be padded) -> uint8[N, ..., 21], the reference's index semantics; with want_error
    also int32[N]: 1 where an index was 21 or more (the reference's IndexError)."""
    assert image.shape[-1] == 3
    ip, ipitch, N, row = rows(image, torch.uint8)
    n_cells = row // 3
    dev = image.device
    if out is None:
        out = torch.empty(tuple(image.shape[:-1]) + (ONEHOT_BITS,), dtype=torch.uint8, device=dev)
    op, opitch, No, orow = rows(out, torch.uint8)
    assert No == N and orow == n_cells * ONEHOT_BITS and out.device == dev
    err = torch.empty(N, dtype=torch.int32, device=dev) if want_error else None
    call("mg_obs_onehot", dev, ip, ipitch, N, n_cells, op, opitch, ptr(err, torch.int32))
    return (out, err) if want_error else out


def full_obs(type_plane, colour_plane, state_plane, width, height, agent_x, agent_y, agent_dir, out=None,
             want_error=False):
    """-> uint8[N, W, H, 3]: Grid.encode() with the agent's cell set to (10, 0, agent_dir).  With want_error also
    int32[N]: 2 where the agent lies outside the world."""
    N, W, H = type_plane.shape[0], int(width), int(height)
    assert type_plane.shape == (N, W * H) and colour_plane.shape == (N, W * H)
    dev = type_plane.device
    if out is None:
        out = torch.empty((N, W, H, 3), dtype=torch.uint8, device=dev)
    op, opitch, No, orow = rows(out, torch.uint8)
    assert No == N and orow == W * H * 3
    err = torch.empty(N, dtype=torch.int32, device=dev) if want_error else None
    assert agent_x.shape[0] >= N
    call("mg_obs_full", dev, ptr(type_plane, torch.uint8), ptr(colour_plane, torch.uint8), ptr(state_plane, torch.uint8),
         N, W, H, *agent_arrays(agent_x, agent_y, agent_dir), op, opitch, ptr(err, torch.int32))
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
    call("mg_obs_symbolic", dev, ptr(type_plane, torch.uint8), N, W, H, ptr(out, torch.int32))
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
    ip, ipitch, N, n_img = rows(image, torch.uint8)
    dev = image.device
    n_tail = 0 if tail is None else int(tail.numel())
    if out is None:
        out = torch.empty((N, n_img + n_tail), dtype=torch.float32, device=dev)
    op, opitch, No, orow = rows(out, torch.float32)
    assert No == N and orow == n_img + n_tail
    assert tail is None or tail.device == dev
    call("mg_obs_flat", dev, ip, ipitch, N, n_img, ptr(tail, torch.float32), n_tail, op, opitch)
    return out


def goal_index(type_plane, width, height):
    """-> int32[N]: the first flat index (y*W + x) of a goal in each env's plane, or -1."""
    N = type_plane.shape[0]
    assert type_plane.shape == (N, int(width) * int(height))
    dev = type_plane.device
    out = torch.empty(N, dtype=torch.int32, device=dev)
    call("mg_obs_goal_index", dev, ptr(type_plane, torch.uint8), N, int(width), int(height), ptr(out, torch.int32))
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


def goal_direction(goal_idx, width, height, agent_x, agent_y, mode="slope", table=None, out=None, want_error=False):
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
    ax, ay, _, stride = agent_arrays(agent_x, agent_y)
    assert agent_x.shape[0] >= N
    call("mg_obs_goal_direction", dev, ptr(goal_idx, torch.int32), N, int(width), int(height), ax, ay, stride, m,
         ptr(table if m == ANGLE else None, torch.float64), ptr(out, torch.float64), ptr(err, torch.int32))
    return (out, err) if want_error else out
