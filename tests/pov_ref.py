"""numpy restatement of the agent-view frame (MiniGridEnv.get_pov_render): the V x V grid of gen_obs_grid -- the
window of get_view_exts, padded with grey walls outside the world, turned agent_dir + 1 times to the left, the carried
object on the agent's cell, the cells the visibility mask hides cleared (process_vis does that to the grid before the
carried object is placed) -- drawn by Grid.render with the agent at (V // 2, V - 1) pointing up and the visibility
mask as highlight.  Tiles come from tests/render_ref.py.  It is the checker of mg_render_pov where no recording exists
and is itself pinned byte for byte against tests/golden/pov.npz (tools/record_pov_golden.py) by tests/test_pov_cpu.py.

World planes as everywhere in this package: uint8[H*W], cell (x, y) at y*W + x."""
import os

import numpy as np

import render_ref as rr

WALL_CELL = (2, 5, 0)


def view_cells(ty, co, st, W, H, ax, ay, ad, V, carrying=None, vis=None):
    """-> int[V][V][3], cell (i, j) at [j][i]: what gen_obs_grid's grid holds, straight from the reference's steps."""
    ad = int(ad) % 4
    half = V // 2
    topx = ax if ad == 0 else (ax - V + 1 if ad == 2 else ax - half)
    topy = ay if ad == 1 else (ay - V + 1 if ad == 3 else ay - half)
    g = np.zeros((V, V, 3), np.int64)
    for j in range(V):                                         # Grid.slice
        for i in range(V):
            x, y = topx + i, topy + j
            if 0 <= x < W and 0 <= y < H:
                k = y * W + x
                g[j, i] = (ty[k], co[k], st[k] if st is not None else 0)
            else:
                g[j, i] = WALL_CELL
    for _ in range(ad + 1):                                    # Grid.rotate_left: new (j, V-1-i) <- old (i, j)
        n = np.zeros_like(g)
        for i in range(V):
            for j in range(V):
                n[V - 1 - i, j] = g[j, i]
        g = n
    if vis is not None:                                        # process_vis: self.set(i, j, None) where not mask[i, j]
        g[np.asarray(vis).T == 0] = (1, 0, 0)
    c = (1, 0, 0)
    if carrying is not None and int(carrying[0]) != 0:
        c = tuple(int(v) for v in carrying)
    g[V - 1, half] = c
    return g


def _cells(ty, co, st, W, H, ax, ay, ad, V, carrying, vis):
    return np.stack([view_cells(ty[e], co[e], None if st is None else st[e], W, H, int(ax[e]), int(ay[e]), int(ad[e]), V,
                                None if carrying is None else carrying[e], None if vis is None else vis[e])
                     for e in range(len(ty))]).reshape(len(ty), V * V, 3)


def undrawn_pixels(ty, co, st, W, H, ax, ay, ad, V, ts, carrying=None, vis=None):
    """bool[N][V*ts][V*ts]: the pixels of the view cells the device renderer does not draw (lava, unknown codes) and
    replaces by empty tiles; the reference's picture differs from the device's there and nowhere else."""
    cells = _cells(ty, co, st, W, H, ax, ay, ad, V, carrying, vis)
    bad = np.array([[not rr.drawable(int(t), int(c)) for t, c, _ in row] for row in cells]).reshape(len(ty), V, V)
    return np.repeat(np.repeat(bad, ts, axis=1), ts, axis=2)


def pov_frames(ty, co, st, W, H, ax, ay, ad, V, ts, carrying=None, vis=None):
    """N frames at once: planes uint8[N][H*W] (st may be None), agent int[N], carrying uint8[N][3] or None, vis
    uint8[N][V][V] indexed [i][j] or None (= all visible) -> (uint8[N][V*ts][V*ts][3], error int[N])."""
    N = len(ty)
    cells = _cells(ty, co, st, W, H, ax, ay, ad, V, carrying, vis)
    hl = np.ones((N, V * V), np.uint8) if vis is None else (np.asarray(vis) != 0).transpose(0, 2, 1).reshape(N, V * V)
    full = np.full(N, V // 2), np.full(N, V - 1), np.full(N, 3)
    return rr.render_frames(cells[..., 0], cells[..., 1], cells[..., 2], V, V, *full, ts, hl)


_golden = {}


def load_golden():
    if "z" not in _golden:
        _golden["z"] = np.load(os.path.join(rr.GOLDEN, "pov.npz"))
    return _golden["z"]


def load_script(name):
    """Recorded frames of one script, uint8[1 + n_ops][V*ts][V*ts][3] (stored as XOR deltas of consecutive frames)."""
    return np.bitwise_xor.accumulate(load_golden()["s_pov_" + name], axis=0)


def world_planes(c):
    """World c of the recording -> (ty, co, st uint8[H*W], W, H, ax, ay, carrying uint8[3])."""
    z = load_golden()
    p = np.ascontiguousarray(np.transpose(z["w_grid_%02d" % c], (1, 0, 2)))
    W, H, ax, ay = (int(v) for v in z["w_meta_%02d" % c])
    return tuple(p[..., k].reshape(-1) for k in range(3)) + (W, H, ax, ay, z["w_carry_%02d" % c])
