"""numpy restatement of the six computations of include/minigrid_obs.h (the reference's observation wrappers,
gym_minigrid/wrappers.py:117-154, 220-246, 367-425, 463-494, 497-526), pinned to the recording of the reference's own
wrappers by tests/test_obs_wrappers_cpu.py and used as the expected value by tests/test_obs_wrappers_gpu.py.
World planes are uint8[N][H*W] with cell (x, y) at y*W + x."""
import numpy as np

BITS = 21


def planes_from_encoded(enc):
    """Grid.encode() [W][H][3] -> (type, colour, state) planes uint8[H*W]."""
    p = np.asarray(enc, np.uint8).transpose(1, 0, 2)
    return tuple(np.ascontiguousarray(p[:, :, k]).reshape(-1) for k in range(3))


def onehot(image):
    """uint8[..., 3] -> (uint8[..., 21], error int32[N]): a byte per INDEX type, 12 + colour, 18 + state; an index of 21
    or more sets nothing and flags its env (leading axis)."""
    img = np.asarray(image, np.uint8).astype(np.int64)
    idx = np.stack([img[..., 0], 12 + img[..., 1], 18 + img[..., 2]], -1)
    out = (idx[..., None] == np.arange(BITS)).any(-2).astype(np.uint8)
    err = (idx >= BITS).reshape(img.shape[0], -1).any(1).astype(np.int32)
    return out, err


def full(type_p, colour_p, state_p, W, H, ax, ay, ad):
    """-> (uint8[N][W][H][3], error int32[N]): empty cells (type 0 / 1) are (1, 0, 0); the agent's cell (10, 0, dir);
    an agent outside the world stamps nothing and flags 2."""
    t = np.asarray(type_p, np.uint8).reshape(-1, H, W)
    N = t.shape[0]
    c = np.asarray(colour_p, np.uint8).reshape(N, H, W)
    s = np.zeros_like(t) if state_p is None else np.asarray(state_p, np.uint8).reshape(N, H, W)
    empty = t <= 1
    out = np.stack([np.where(empty, 1, t), np.where(empty, 0, c), np.where(empty, 0, s)], -1).astype(np.uint8)
    out = np.ascontiguousarray(out.transpose(0, 2, 1, 3))
    err = np.zeros(N, np.int32)
    for e in range(N):
        x, y = int(ax[e]), int(ay[e])
        if 0 <= x < W and 0 <= y < H:
            out[e, x, y] = (10, 0, int(ad[e]) & 255)
        else:
            err[e] = 2
    return out, err


def symbolic(type_p, W, H):
    """-> int32[N][W][H][3] = (x, y, idx): idx is the type at FLAT index x*H + y (the reference reshapes the cell list,
    whose index is j*W + i, as (W, H)), -1 where that cell is empty."""
    t = np.asarray(type_p, np.uint8).reshape(-1, W * H).astype(np.int32)
    N = t.shape[0]
    obj = np.where(t <= 1, -1, t).reshape(N, W, H)
    xs, ys = np.mgrid[:W, :H]
    return np.stack([np.broadcast_to(xs, (N, W, H)), np.broadcast_to(ys, (N, W, H)), obj], -1).astype(np.int32)


def mission_tail(mission, max_len=96):
    assert len(mission) <= max_len
    arr = np.zeros((max_len, 28), np.float32)
    for i, ch in enumerate(mission.lower()):
        if "a" <= ch <= "z":
            arr[i, ord(ch) - 97] = 1
        elif ch in " ,":
            arr[i, 26 + " ,".index(ch)] = 1
        else:
            raise ValueError(ch)
    return arr.reshape(-1)


def flat(image, tail):
    """uint8[N, ...] -> float32[N][n_img + n_tail]."""
    img = np.asarray(image, np.uint8)
    N = img.shape[0]
    return np.concatenate([img.reshape(N, -1).astype(np.float32), np.broadcast_to(np.asarray(tail, np.float32), (N, len(tail)))], 1)


def goal_index(type_p, W, H):
    t = np.asarray(type_p, np.uint8).reshape(-1, W * H)
    return np.where((t == 8).any(1), (t == 8).argmax(1), -1).astype(np.int32)


def goal_direction(k, W, H, ax, ay, mode="slope"):
    """-> (float64[N], error int32[N]): goal_position = (k // H, k % W); slope = (gp[1] - y) / (gp[0] - x) in IEEE double
    (-0.0, +-inf, NaN kept); "angle" = np.arctan(slope), one scalar at a time."""
    N = len(k)
    out, err = np.full(N, np.nan), np.zeros(N, np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for e in range(N):
            if not 0 <= k[e] < W * H:
                err[e] = 1
            elif not (0 <= ax[e] < W and 0 <= ay[e] < H):
                err[e] = 2
            else:
                v = np.divide(int(k[e]) % W - int(ay[e]), int(k[e]) // H - int(ax[e]))
                out[e] = np.arctan(v) if mode == "angle" else v
    return out, err


def same_f64(a, b):
    """Bit equality of float64 arrays, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))
