"""Literal host reference of include/minigrid_nav.h: a collections.deque breadth-first search per world, the expert
action's tie-break and the error codes.  Deliberately the textbook formulation (a queue of cells), nothing like the
kernel's row masks."""
from collections import deque

import numpy as np

UNREACHABLE = 0xFFFF
PASS_DEFAULT = 0x0B1B
DOORS_OPEN = 1
MOVES = ((0, -1, 0), (1, 1, 0), (2, 0, -1), (3, 0, 1))          # (action, dx, dy): left, right, up, down


def enterable(t, s, pass_types, flags):
    t, s = int(t), int(s)
    if t >= 16 or not (pass_types >> t) & 1:
        return False
    if t == 4 and s != 0 and not flags & DOORS_OPEN:
        return False
    return True


def open_cells(type_plane, state_plane, W, H, pass_types=PASS_DEFAULT, flags=0):
    ty = np.asarray(type_plane).reshape(H, W)
    st = np.zeros((H, W), np.uint8) if state_plane is None else np.asarray(state_plane).reshape(H, W)
    return np.array([[enterable(ty[y, x], st[y, x], pass_types, flags) for x in range(W)] for y in range(H)], bool)


def field(type_plane, state_plane, W, H, pass_types=PASS_DEFAULT, flags=0, goal=None, agent=None):
    """One world -> dict(dist uint16[H*W], error, agent_dist, agent_action, depth).  depth = the largest finite
    distance (the number of flood steps an iterative implementation needs)."""
    ok = open_cells(type_plane, state_plane, W, H, pass_types, flags)
    ty = np.asarray(type_plane).reshape(H, W)
    dist = np.full((H, W), UNREACHABLE, np.int64)
    err = 0
    sources = []
    if goal is not None:
        gx, gy = int(goal[0]), int(goal[1])
        if not (0 <= gx < W and 0 <= gy < H):
            err = 2
        elif ok[gy, gx]:
            sources = [(gx, gy)]
    else:
        sources = [(x, y) for y in range(H) for x in range(W) if ty[y, x] == 8 and ok[y, x]]
    if err == 0 and not sources:
        err = 1
    q = deque()
    for x, y in sources:
        dist[y, x] = 0
        q.append((x, y))
    while q:
        x, y = q.popleft()
        for _, dx, dy in MOVES:
            nx, ny = x + dx, y + dy
            if 0 <= nx < W and 0 <= ny < H and ok[ny, nx] and dist[ny, nx] == UNREACHABLE:
                dist[ny, nx] = dist[y, x] + 1
                q.append((nx, ny))
    finite = dist[dist != UNREACHABLE]
    res = dict(dist=dist.reshape(-1).astype(np.uint16), error=err, agent_dist=None, agent_action=None,
               depth=int(finite.max()) if finite.size else 0)
    if agent is not None:
        ax, ay = int(agent[0]), int(agent[1])
        d, a = UNREACHABLE, -1
        if not (0 <= ax < W and 0 <= ay < H):
            if err == 0:
                res["error"] = 3
        else:
            d = int(dist[ay, ax])
            if d == 0:
                a = 6
            elif d != UNREACHABLE:
                for act, dx, dy in MOVES:
                    nx, ny = ax + dx, ay + dy
                    if 0 <= nx < W and 0 <= ny < H and dist[ny, nx] == d - 1:
                        a = act
                        break
        res["agent_dist"], res["agent_action"] = d, a
    return res


def fields(type_planes, state_planes, W, H, pass_types=PASS_DEFAULT, flags=0, goal=None, agent=None):
    """N worlds -> (dist uint16[N, H*W], agent_dist int32[N] or None, agent_action int32[N] or None, error int32[N],
    depth int[N]).  goal / agent: (x[N], y[N]) or None."""
    N = len(type_planes)
    out = [field(type_planes[n], None if state_planes is None else state_planes[n], W, H, pass_types, flags,
                 None if goal is None else (goal[0][n], goal[1][n]), None if agent is None else (agent[0][n], agent[1][n]))
           for n in range(N)]
    dist = np.stack([o["dist"] for o in out])
    err = np.array([o["error"] for o in out], np.int32)
    depth = np.array([o["depth"] for o in out])
    if agent is None:
        return dist, None, None, err, depth
    return (dist, np.array([o["agent_dist"] for o in out], np.int32), np.array([o["agent_action"] for o in out], np.int32),
            err, depth)


def relax(type_plane, state_plane, W, H, pass_types=PASS_DEFAULT, flags=0, goal=None):
    """The independent formulation: d = min(d, 1 + min over the four neighbours) on enterable cells, repeated to a fixed
    point.  -> int64[H*W] with UNREACHABLE."""
    ok = open_cells(type_plane, state_plane, W, H, pass_types, flags)
    ty = np.asarray(type_plane).reshape(H, W)
    INF = 1 << 30
    d = np.full((H, W), INF, np.int64)
    if goal is not None:
        gx, gy = int(goal[0]), int(goal[1])
        if 0 <= gx < W and 0 <= gy < H and ok[gy, gx]:
            d[gy, gx] = 0
    else:
        d[(ty == 8) & ok] = 0
    while True:
        p = np.pad(d, 1, constant_values=INF)
        nb = np.minimum(np.minimum(p[1:-1, :-2], p[1:-1, 2:]), np.minimum(p[:-2, 1:-1], p[2:, 1:-1]))
        nd = np.where(ok, np.minimum(d, nb + 1), INF)
        if (nd == d).all():
            break
        d = nd
    return np.where(d >= INF, UNREACHABLE, d).reshape(-1)


def random_world(rng, W, H, wall_density, all_types=True):
    """(type, state) uint8[H*W]: empty cells, walls at the given density, and (all_types) a sprinkle of every type code
    0..17 with doors in all three states."""
    ty = np.where(rng.random(W * H) < wall_density, 2, 1).astype(np.uint8)
    st = np.zeros(W * H, np.uint8)
    if all_types:
        k = max(1, (W * H) // 6)
        idx = rng.integers(0, W * H, k)
        ty[idx] = rng.integers(0, 18, k)
        st[ty == 4] = rng.integers(0, 3, int((ty == 4).sum()))
    return ty, st


def serpentine(W, H):
    """Walls on every odd row but one gap, alternating between the right and the left end: one corridor through all
    even rows.  -> (type uint8[H*W], source (x, y) = the corridor's first cell)."""
    ty = np.ones((H, W), np.uint8)
    for y in range(1, H, 2):
        ty[y, :] = 2
        ty[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return ty.reshape(-1), (0, 0)


def lookup(dist, pos, W, H, cell_rule):
    """dist uint16[N, H*W], pos float32[T, N, 2] -> uint16[T, N] by `cell_rule(pos, W, H)` (visit_ref.cells: bin H*W
    for every position outside the world)."""
    c = cell_rule(pos, W, H)
    T, N = c.shape
    ext = np.concatenate([np.asarray(dist), np.full((N, 1), UNREACHABLE, np.uint16)], axis=1)
    return ext[np.arange(N)[None, :], c]
