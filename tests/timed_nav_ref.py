"""Literal host reference of the time-expanded fields of include/minigrid_nav.h: a collections.deque breadth-first search
over (cell, phase) states, backwards from the sources, then the expert action and the move set read off the distances.
Deliberately the textbook formulation (a queue of states), nothing like the kernel's row masks."""
from collections import deque

import numpy as np

import nav_ref

UNREACHABLE = nav_ref.UNREACHABLE
MAX_PERIOD = 16
MOVE_STAY = 1 << 4
STEPS = ((0, -1, 0), (1, 1, 0), (2, 0, -1), (3, 0, 1))           # (bit / action, dx, dy): left, right, up, down


def phase_of(clock, P):
    clock = int(clock)
    return 0 if clock <= 0 else clock % P


def free_cells(type_plane, state_plane, W, H, blocked, P, pass_types=nav_ref.PASS_DEFAULT, flags=0):
    """bool[P, H, W]: enterable and not blocked at the phase.  blocked: integer[P, H], bit x of word y."""
    ok = nav_ref.open_cells(type_plane, state_plane, W, H, pass_types, flags)
    blocked = np.asarray(blocked).astype(np.int64) & 0xFFFFFFFF
    assert blocked.shape == (P, H)
    occ = np.array([[[(int(blocked[p, y]) >> x) & 1 for x in range(W)] for y in range(H)] for p in range(P)], bool)
    return ok[None] & ~occ


def field(type_plane, state_plane, W, H, blocked, P, pass_types=nav_ref.PASS_DEFAULT, flags=0, goal=None, agent=None):
    """One world -> dict(dist uint16[P, H*W], error, agent_dist, agent_action, depth).  agent = (x, y) or (x, y, clock)."""
    assert 1 <= P <= MAX_PERIOD
    free = free_cells(type_plane, state_plane, W, H, blocked, P, pass_types, flags)
    ty = np.asarray(type_plane).reshape(H, W)
    dist = np.full((P, H, W), UNREACHABLE, np.int64)
    err = 0
    cells = []
    if goal is not None:
        gx, gy = int(goal[0]), int(goal[1])
        if not (0 <= gx < W and 0 <= gy < H):
            err = 2
        else:
            cells = [(gx, gy)]
    else:
        cells = [(x, y) for y in range(H) for x in range(W) if ty[y, x] == 8]
    q = deque()
    for p in range(P):
        for x, y in cells:
            if free[p, y, x]:
                dist[p, y, x] = 0
                q.append((p, x, y))
    if err == 0 and not q:
        err = 1
    while q:
        p, x, y = q.popleft()                                    # the state a transition arrives in
        pp = (p - 1) % P                                         # ... and the phase it leaves from
        for dx, dy in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
            sx, sy = x - dx, y - dy
            if 0 <= sx < W and 0 <= sy < H and free[pp, sy, sx] and dist[pp, sy, sx] == UNREACHABLE:
                dist[pp, sy, sx] = dist[p, y, x] + 1
                q.append((pp, sx, sy))
    finite = dist[dist != UNREACHABLE]
    res = dict(dist=dist.reshape(P, -1).astype(np.uint16), error=err, agent_dist=None, agent_action=None,
               depth=int(finite.max()) if finite.size else 0)
    if agent is not None:
        ax, ay = int(agent[0]), int(agent[1])
        clock = agent[2] if len(agent) > 2 else 0
        d, a = UNREACHABLE, -1
        if not (0 <= ax < W and 0 <= ay < H):
            if err == 0:
                res["error"] = 3
        else:
            m, d = move_set(res["dist"], W, H, ay * W + ax, phase_of(clock, P))
            a = action_of(m)
        res["agent_dist"], res["agent_action"] = d, a
    return res


def move_set(dist, W, H, c, p):
    """dist uint16[P, H*W] -> (move set, distance) of the state (cell c, phase p)."""
    P = dist.shape[0]
    d = int(dist[p, c])
    if d == 0:
        return MOVE_STAY, d
    if d == UNREACHABLE:
        return 0, d
    nxt = dist[(p + 1) % P]
    x, y = c % W, c // W
    m = 0
    for bit, dx, dy in STEPS:
        nx, ny = x + dx, y + dy
        if 0 <= nx < W and 0 <= ny < H and int(nxt[ny * W + nx]) == d - 1:
            m |= 1 << bit
    if int(nxt[c]) == d - 1:
        m |= MOVE_STAY
    return m, d


def action_of(m):
    """The expert action of a move set: its lowest set bit, bit 4 read as 6; -1 for the empty set."""
    if m == 0:
        return -1
    low = (m & -m).bit_length() - 1
    return 6 if low == 4 else low


def fields(type_planes, state_planes, W, H, blocked, P, pass_types=nav_ref.PASS_DEFAULT, flags=0, goal=None, agent=None):
    """N worlds -> (dist uint16[N, P, H*W], agent_dist int32[N] or None, agent_action int32[N] or None, error int32[N],
    depth int[N]).  blocked: [P, H] shared or [N, P, H]; goal = (x[N], y[N]); agent = (x[N], y[N]) or (x, y, clock)."""
    N = len(type_planes)
    blocked = np.asarray(blocked)
    out = [field(type_planes[n], None if state_planes is None else state_planes[n], W, H,
                 blocked if blocked.ndim == 2 else blocked[n], P, pass_types, flags,
                 None if goal is None else (goal[0][n], goal[1][n]),
                 None if agent is None else tuple(a[n] for a in agent)) for n in range(N)]
    dist = np.stack([o["dist"] for o in out])
    err = np.array([o["error"] for o in out], np.int32)
    depth = np.array([o["depth"] for o in out])
    if agent is None:
        return dist, None, None, err, depth
    return (dist, np.array([o["agent_dist"] for o in out], np.int32), np.array([o["agent_action"] for o in out], np.int32),
            err, depth)


def moves(dist, pos, age, init_pos, W, H, cell_of):
    """dist uint16[N, P, H*W], pos float32[T, N, 2], age int32[T, N], init_pos float32[2] -> (moves uint8[T, N],
    acting_dist uint16[T, N]); cell_of(y, x, W, H) is the rule of the visit counters (visit_ref.cell_of: W*H = no cell)."""
    T, N = age.shape
    P = dist.shape[1]
    m = np.zeros((T, N), np.uint8)
    d = np.full((T, N), UNREACHABLE, np.uint16)
    for t in range(T):
        for n in range(N):
            q = init_pos if age[t, n] <= 0 else pos[t, n]
            c = cell_of(q[0], q[1], W, H)
            if c < W * H:
                m[t, n], d[t, n] = move_set(dist[n], W, H, c, phase_of(age[t, n], P))
    return m, d


def random_schedule(rng, P, H, density=0.15):
    """uint32[P, H] with every bit of all 32 columns drawn (bits at or above the width are to be ignored)."""
    bits = rng.random((P, H, 32)) < density
    return (bits * (1 << np.arange(32, dtype=np.uint64))).sum(axis=2).astype(np.uint32)


# ---- Twoarmy: the row-8 balls as a function of step_move % 6, restated from the rule of the reference's step()
TWOARMY_P = 6
TWOARMY_BLOCKS = [(4, 11), (5, 11), (4, 12), (5, 12), (8, 11), (8, 12), (9, 11), (9, 12)]      # v6's constant 2x2 walls


def twoarmy_balls(step_move):
    """x of the three balls after the move of the step that raised step_move to this value (7, 8, 9 at a reset)."""
    x = 7
    for k in range(1, (step_move % TWOARMY_P) + 1):
        x += 1 if k % 6 in (0, 1) else -1 if k % 6 in (2, 3) else 0
    return [x, x + 1, x + 2]
