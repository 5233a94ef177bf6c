"""Host restatement of the look-ahead of include/minigrid_nav.h ("Look-ahead"), written from the header text: one frontier
loop per element over sets of (cell, ended) states, on the fields nav_ref.py / timed_nav_ref.py compute.  Nothing like the
kernel's 64-bit frontier word.  Test-side only."""
import numpy as np

import nav_ref
import prior_ref
import visit_ref

UNREACHABLE = nav_ref.UNREACHABLE
SIDE, MAX_STEPS = 7, 3
SAME = 24                                                        # bit of the displacement (0, 0)
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))                  # (dx, dy): left, right, up, down


def bit_of(dy, dx):
    assert -3 <= dy <= 3 and -3 <= dx <= 3
    return (dy + 3) * SIDE + (dx + 3)


def successors(dist, W, H, c, p):
    """dist uint16[P, H*W]: the successors of the state (cell c, phase p) as cells; None for a state at distance 0 (the
    episode has ended: the state stays whatever the next phase holds)."""
    P = dist.shape[0]
    d = int(dist[p, c])
    assert d != UNREACHABLE
    if d == 0:
        return None
    nxt = dist[p if P == 1 else (p + 1) % P]
    x, y = c % W, c // W
    out = [ny * W + nx for nx, ny in ((x + dx, y + dy) for dx, dy in NEIGHBOURS)
           if 0 <= nx < W and 0 <= ny < H and int(nxt[ny * W + nx]) == d - 1]
    if P > 1 and int(nxt[c]) == d - 1:                           # waiting is optimal
        out.append(c)
    return out


def label(dist, W, H, c, p, steps):
    """dist uint16[P, H*W] (P = 1: a static field) -> (label, distance) of the acting state (cell c, phase p)."""
    assert 1 <= steps <= MAX_STEPS
    P = dist.shape[0]
    d = int(dist[p, c])
    if d == UNREACHABLE:
        return 0, d
    front = {(c, False)}                                         # (cell, the episode has ended there)
    for _ in range(steps):
        new = set()
        for cell, ended in front:
            succ = None if ended else successors(dist, W, H, cell, p)
            if succ is None:
                new.add((cell, True))
            else:
                new.update((s, False) for s in succ)
        front = new
        p = p if P == 1 else (p + 1) % P
    lab = 0
    for cell, _ in front:
        lab |= 1 << bit_of(cell // W - c // W, cell % W - c % W)
    return lab, d


def phase_of(clock, P):
    clock = int(clock)
    return 0 if clock <= 0 else clock % P


def ahead(dist, pos, W, H, steps, age=None, init_pos=None):
    """dist uint16[N, H*W] or uint16[N, P, H*W]; pos float32[T, N, 2] BEFORE each step; age int[T, N] with init_pos (the
    clock of a timed field) -> (labels uint64[T, N], acting_dist uint16[T, N])."""
    dist = np.asarray(dist)
    if dist.ndim == 2:
        dist = dist[:, None]
    p = prior_ref.acting_positions(pos, age, init_pos)
    T, N = p.shape[:2]
    P = dist.shape[1]
    lab, ad = np.zeros((T, N), np.uint64), np.full((T, N), UNREACHABLE, np.uint16)
    for t in range(T):
        for n in range(N):
            c = visit_ref.cell_of(p[t, n, 0], p[t, n, 1], W, H)
            if c < W * H:
                ph = phase_of(age[t, n], P) if (age is not None and P > 1) else 0
                lab[t, n], ad[t, n] = label(dist[n], W, H, c, ph, steps)
    return lab, ad


def goal_ahead(type_planes, state_planes, W, H, rec_t, rec_n, rec_goal, pos, steps, age=None, init_pos=None,
               pass_types=nav_ref.PASS_DEFAULT, flags=0, memo=None):
    """Per record: nav_ref.field from the record's goal cell, then label() of the acting cell in it -> (labels uint64[R],
    acting_dist uint16[R]).  memo: (env, goal cell) -> field, kept by the caller across calls on the same worlds."""
    N = len(type_planes)
    p = prior_ref.acting_positions(pos, age, init_pos)
    T = p.shape[0]
    rec_goal = np.asarray(rec_goal, np.float32).reshape(-1, 2)
    R = len(rec_t)
    memo = {} if memo is None else memo
    lab, ad = np.zeros(R, np.uint64), np.full(R, UNREACHABLE, np.uint16)
    for b in range(R):
        t, n = int(rec_t[b]), int(rec_n[b])
        if not (0 <= t < T and 0 <= n < N):
            continue
        gc = visit_ref.cell_of(rec_goal[b, 0], rec_goal[b, 1], W, H)
        if gc >= W * H:
            continue
        if (n, gc) not in memo:
            memo[(n, gc)] = nav_ref.field(type_planes[n], None if state_planes is None else state_planes[n], W, H,
                                          pass_types, flags, goal=(gc % W, gc // W))["dist"][None]
        c = visit_ref.cell_of(p[t, n, 0], p[t, n, 1], W, H)
        if c < W * H:
            lab[b], ad[b] = label(memo[(n, gc)], W, H, c, 0, steps)
    return lab, ad


def cells_of(lab, c, W):
    """The cells a label names from the acting cell c."""
    lab = int(lab)
    return [c + (b // SIDE - 3) * W + (b % SIDE - 3) for b in range(SIDE * SIDE) if (lab >> b) & 1]


def bits(labels):
    """uint64[...] -> bool[..., 7, 7]."""
    lab = np.asarray(labels).astype(np.uint64)
    return (((lab[..., None] >> np.arange(SIDE * SIDE, dtype=np.uint64)) & np.uint64(1)) != 0).reshape(*lab.shape, SIDE, SIDE)
