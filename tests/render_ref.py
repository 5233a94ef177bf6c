"""numpy restatement of the reference renderer (gym_minigrid/rendering.py, Grid.render_tile / Grid.render,
MiniGridEnv.get_full_render's highlight loop): float64, one operation at a time in the reference's order.  It is the
checker of the device renderer where no recording exists (other tile sizes, other worlds) and is itself pinned byte
for byte against tests/golden/render.npz (recorded from the reference by tools/record_render_golden.py).

World planes as everywhere in this package: uint8[H*W], cell (x, y) at y*W + x."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLORS = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [112, 39, 195], [255, 255, 0], [100, 100, 100]])
EMPTY, WALL, FLOOR, DOOR, KEY, BALL, BOX, GOAL = 1, 2, 3, 4, 5, 6, 7, 8
DIR_TO_VEC = [(1, 0), (0, 1), (-1, 0), (0, -1)]
N_KINDS, N_TILES = 10, 600


def drawable(t, c):
    """Does the device renderer draw a cell of this type / colour?  (lava, agent, subgoal and unknown codes: no.)"""
    return t in (0, 1) or t == GOAL or (2 <= t <= 7 and 0 <= c <= 5)


def tile_index(t, c, s, agent, hl):
    """Atlas slot of include/minigrid_render.h; -1 for a cell that is not drawn."""
    if not drawable(t, c):
        return -1
    if t in (0, 1):
        kind, c = 0, 0
    elif t == DOOR:
        kind = 3 if s == 0 else (5 if s == 2 else 4)
    elif t == GOAL:
        kind, c = 9, 1
    else:
        kind = {WALL: 1, FLOOR: 2, KEY: 6, BALL: 7, BOX: 8}[t]
    return ((kind * 6 + c) * 5 + (0 if agent < 0 else 1 + agent % 4)) * 2 + (1 if hl else 0)


def triangle_constants():
    """The float32 side of point_in_triangle((0.12, 0.19), (0.87, 0.50), (0.12, 0.81)) and the rotation terms, in the
    order of mg_render_constants (18 doubles)."""
    f = np.float32
    a, b, c = (f(0.12), f(0.19)), (f(0.87), f(0.50)), (f(0.12), f(0.81))
    v0, v1 = (c[0] - a[0], c[1] - a[1]), (b[0] - a[0], b[1] - a[1])
    dot00 = v0[0] * v0[0] + v0[1] * v0[1]
    dot01 = v0[0] * v1[0] + v0[1] * v1[1]
    dot11 = v1[0] * v1[0] + v1[1] * v1[1]
    inv = f(1) / (dot00 * dot11 - dot01 * dot01)
    assert all(isinstance(v, np.float32) for v in (dot00, dot01, dot11, inv))
    cs = [math.cos(-(0.5 * math.pi * d)) for d in range(4)]
    sn = [math.sin(-(0.5 * math.pi * d)) for d in range(4)]
    return cs + sn + [float(v) for v in (a[0], a[1], v0[0], v0[1], v1[0], v1[1], dot00, dot01, dot11, inv)]


def _rect(x, y, xmin, xmax, ymin, ymax):
    return (x >= xmin) & (x <= xmax) & (y >= ymin) & (y <= ymax)


def _circle(x, y, cx, cy, r):
    return (x - cx) * (x - cx) + (y - cy) * (y - cy) <= r * r


def _agent(x, y, d):
    k = triangle_constants()
    cs, sn = k[d], k[4 + d]
    ax, ay, v0x, v0y, v1x, v1y, dot00, dot01, dot11, inv = k[8:]
    cx = cy = 0.5
    x = x - cx
    y = y - cy
    x2 = cx + x * cs - y * sn
    y2 = cy + y * cs + x * sn
    v2x, v2y = x2 - ax, y2 - ay
    dot02 = v0x * v2x + v0y * v2y
    dot12 = v1x * v2x + v1y * v2y
    u = (dot11 * dot02 - dot01 * dot12) * inv
    v = (dot00 * dot12 - dot01 * dot02) * inv
    return (u >= 0) & (v >= 0) & ((u + v) < 1)


_tiles = {}


def render_tile(t, c, s, agent, hl, ts):
    """uint8[ts][ts][3]: Grid.render_tile(WorldObj.decode(t, c, s), agent_dir, highlight, ts) as Grid.render stores it.
    agent -1 = none."""
    key = (tile_index(t, c, s, agent, hl), ts)
    assert key[0] >= 0
    if key in _tiles:
        return _tiles[key]
    S = 3 * ts
    f = (np.arange(S) + 0.5) / S
    x, y = np.meshgrid(f, f)                                   # x along axis 1, y along axis 0
    img = np.zeros((S, S, 3), np.uint8)
    col = COLORS[1 if t == GOAL else (c if 2 <= t <= 7 else 0)]
    black, grey = (0, 0, 0), (100, 100, 100)

    def fill(mask, colour):
        img[mask] = colour                                     # float colours truncate on assignment, as in fill_coords

    fill(_rect(x, y, 0, 0.031, 0, 1), grey)
    fill(_rect(x, y, 0, 1, 0, 0.031), grey)
    if t in (WALL, GOAL):
        fill(_rect(x, y, 0, 1, 0, 1), col)
    elif t == FLOOR:
        fill(_rect(x, y, 0.031, 1, 0.031, 1), col / 2)
    elif t == DOOR and s == 0:
        fill(_rect(x, y, 0.88, 1.00, 0.00, 1.00), col)
        fill(_rect(x, y, 0.92, 0.96, 0.04, 0.96), black)
    elif t == DOOR and s == 2:
        fill(_rect(x, y, 0.00, 1.00, 0.00, 1.00), col)
        fill(_rect(x, y, 0.06, 0.94, 0.06, 0.94), 0.45 * col)
        fill(_rect(x, y, 0.52, 0.75, 0.50, 0.56), col)
    elif t == DOOR:
        fill(_rect(x, y, 0.00, 1.00, 0.00, 1.00), col)
        fill(_rect(x, y, 0.04, 0.96, 0.04, 0.96), black)
        fill(_rect(x, y, 0.08, 0.92, 0.08, 0.92), col)
        fill(_rect(x, y, 0.12, 0.88, 0.12, 0.88), black)
        fill(_circle(x, y, 0.75, 0.50, 0.08), col)
    elif t == KEY:
        fill(_rect(x, y, 0.50, 0.63, 0.31, 0.88), col)
        fill(_rect(x, y, 0.38, 0.50, 0.59, 0.66), col)
        fill(_rect(x, y, 0.38, 0.50, 0.81, 0.88), col)
        fill(_circle(x, y, 0.56, 0.28, 0.190), col)
        fill(_circle(x, y, 0.56, 0.28, 0.064), black)
    elif t == BALL:
        fill(_circle(x, y, 0.5, 0.5, 0.31), col)
    elif t == BOX:
        fill(_rect(x, y, 0.12, 0.88, 0.12, 0.88), col)
        fill(_rect(x, y, 0.18, 0.82, 0.18, 0.82), black)
        fill(_rect(x, y, 0.16, 0.84, 0.47, 0.53), col)
    if agent >= 0:
        fill(_agent(x, y, agent % 4), (255, 0, 0))
    if hl:
        v = img.astype(np.float64)
        img = (v + 0.30 * (255.0 - v)).clip(0, 255).astype(np.uint8)
    q = img.astype(np.float64).reshape(ts, 3, ts, 3, 3)
    m = ((q[:, :, :, 0] + q[:, :, :, 1]) + q[:, :, :, 2]) / 3.0          # mean over the samples of a row (axis 3)
    m = ((m[:, 0] + m[:, 1]) + m[:, 2]) / 3.0                            # then over the three rows (axis 1)
    out = m.astype(np.uint8)                                            # truncating cast of Grid.render's assignment
    _tiles[key] = out
    return out


def render_frame(ty, co, st, W, H, ax, ay, ad, ts, highlight=None):
    """Grid.render: uint8[H*ts][W*ts][3].  ty / co / st / highlight: uint8[H*W] (st, highlight may be None).  Cells the
    device renderer does not draw come out as empty tiles; -> (frame, error flag)."""
    img = np.zeros((H * ts, W * ts, 3), np.uint8)
    err = 0
    for j in range(H):
        for i in range(W):
            k = j * W + i
            t, c, s = int(ty[k]), int(co[k]), int(st[k]) if st is not None else 0
            if not drawable(t, c):
                t, c, s, err = 1, 0, 0, 1
            agent = int(ad) if (i, j) == (int(ax), int(ay)) else -1
            hl = bool(highlight[k]) if highlight is not None else False
            img[j * ts:(j + 1) * ts, i * ts:(i + 1) * ts] = render_tile(t, c, s, agent, hl, ts)
    return img, err


def highlight_mask(vis, W, H, ax, ay, ad, V):
    """get_full_render's loop: vis uint8[V][V] indexed [i][j] (None = all visible) -> uint8[H*W] world mask."""
    fx, fy = DIR_TO_VEC[ad % 4]
    rx, ry = -fy, fx
    tx, ty = ax + fx * (V - 1) - rx * (V // 2), ay + fy * (V - 1) - ry * (V // 2)
    out = np.zeros(H * W, np.uint8)
    for vj in range(V):
        for vi in range(V):
            if vis is not None and not vis[vi][vj]:
                continue
            i, j = tx - fx * vj + rx * vi, ty - fy * vj + ry * vi
            if 0 <= i < W and 0 <= j < H:
                out[j * W + i] = 1
    return out


_golden = {}


def load_golden():
    if "z" not in _golden:
        _golden["z"] = np.load(os.path.join(GOLDEN, "render.npz"))
    return _golden["z"]


def load_frames(name):
    """Recorded frames of one script, uint8[1 + n_ops][289][289][3] (stored as XOR deltas of consecutive frames)."""
    return np.bitwise_xor.accumulate(load_golden()["frames_" + name], axis=0)


def render_frames(ty, co, st, W, H, ax, ay, ad, ts, highlight=None):
    """render_frame for N worlds at once (planes uint8[N][H*W], agent int[N]): the same tiles, gathered per cell.
    -> (uint8[N][H*ts][W*ts][3], error int[N])."""
    ty, co = np.asarray(ty), np.asarray(co)
    N = ty.shape[0]
    st = np.zeros_like(ty) if st is None else np.asarray(st)
    hl = np.zeros_like(ty) if highlight is None else (np.asarray(highlight) != 0).astype(np.uint8)
    agent = np.full((N, H * W), -1, np.int64)
    ax, ay, ad = np.asarray(ax), np.asarray(ay), np.asarray(ad)
    inside = (ax >= 0) & (ax < W) & (ay >= 0) & (ay < H)
    agent[np.nonzero(inside)[0], (ay * W + ax)[inside]] = ad[inside] % 4
    keys = np.stack([ty.astype(np.int64), co.astype(np.int64), st.astype(np.int64), agent, hl.astype(np.int64)], -1)
    uniq, inv = np.unique(keys.reshape(-1, 5), axis=0, return_inverse=True)
    tiles = np.zeros((len(uniq), ts, ts, 3), np.uint8)
    bad = np.zeros(len(uniq), bool)
    for u, (t, c, s, a, h) in enumerate(uniq.tolist()):
        if not drawable(t, c):
            t, c, s, bad[u] = 1, 0, 0, True
        tiles[u] = render_tile(t, c, s, a, h, ts)
    inv = inv.reshape(N, H, W)
    img = tiles[inv].transpose(0, 1, 3, 2, 4, 5).reshape(N, H * ts, W * ts, 3)
    return img, bad[inv].reshape(N, -1).any(axis=1).astype(np.int32)
