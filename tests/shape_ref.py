"""Numpy restatement of the reward shaping of include/minigrid_nav.h ("Reward shaping"; mg_nav_shape, mg_nav_goal_shape):
the distances come from the breadth-first searches of nav_ref.py / timed_nav_ref.py, one cell at a time, and the three
float operations are np.float32 ones, one per line, so each is rounded once as the header demands.  Test-side only."""
import numpy as np

import goal_moves_ref
import nav_ref
import timed_nav_ref
import visit_ref

UNREACHABLE = nav_ref.UNREACHABLE
ZERO_TERMINAL = 2


def phi(scale, d):
    """-(scale * (float)d) with one rounding, +0.0 exactly at d == 0; d: integer array."""
    m = np.float32(scale) * np.asarray(d).astype(np.float32)
    return np.where(np.asarray(d) == 0, np.float32(0.0), -m).astype(np.float32)


def terms(d_before, d_after, done, scale, gamma, zero_terminal):
    """Distances (integer arrays, UNREACHABLE = no cell or no path) -> (F float32, mask uint8)."""
    d_before, d_after = np.asarray(d_before).astype(np.int64), np.asarray(d_after).astype(np.int64)
    terminal = np.zeros(d_before.shape, bool) if not zero_terminal else np.asarray(done) != 0
    shaped = (d_before != UNREACHABLE) & (terminal | (d_after != UNREACHABLE))
    phi_after = np.where(terminal, np.float32(0.0), phi(scale, np.where(shaped, d_after, 0))).astype(np.float32)
    phi_before = phi(scale, np.where(shaped, d_before, 0))
    g = np.float32(gamma) * phi_after
    f = g - phi_before
    assert g.dtype == np.float32 and f.dtype == np.float32
    return np.where(shaped, f, np.float32(0.0)).astype(np.float32), shaped.astype(np.uint8)


def apply(reward, f, mask):
    """reward + F where shaped, the reward's own bits elsewhere."""
    reward = np.asarray(reward, np.float32)
    with np.errstate(invalid="ignore"):
        s = reward + f
    assert s.dtype == np.float32
    return np.where(mask != 0, s.view(np.uint32), reward.view(np.uint32)).view(np.float32)


def distances(dist, pos_before, pos_after, W, H, age=None, init_pos=None):
    """dist uint16[N, H*W] or [N, P, H*W]; pos_* float32[T, N, 2]; age int[T, N] with init_pos -> (d_before, d_after)
    int64[T, N]: the acting state (age <= 0 ? init_pos : pos_before, phase of age) and the after state (pos_after, the
    phase after the acting one)."""
    dist = np.asarray(dist)
    if dist.ndim == 2:
        dist = dist[:, None]
    P = dist.shape[1]
    T, N = pos_before.shape[:2]
    db, da = np.full((T, N), UNREACHABLE, np.int64), np.full((T, N), UNREACHABLE, np.int64)
    for t in range(T):
        for n in range(N):
            clock = 1 if age is None else int(age[t, n])
            q = init_pos if clock <= 0 else pos_before[t, n]
            cb = visit_ref.cell_of(q[0], q[1], W, H)
            ca = visit_ref.cell_of(pos_after[t, n, 0], pos_after[t, n, 1], W, H)
            pb = timed_nav_ref.phase_of(clock, P)
            pa = timed_nav_ref.phase_of(max(clock, 0) + 1, P)
            if cb < W * H:
                db[t, n] = dist[n, pb, cb]
            if ca < W * H:
                da[t, n] = dist[n, pa, ca]
    return db, da


def shape(dist, pos_before, pos_after, W, H, reward=None, age=None, init_pos=None, done=None, scale=1.0, gamma=0.99,
          flags=0):
    """mg_nav_shape -> (reward_out or None, F, mask)."""
    db, da = distances(dist, pos_before, pos_after, W, H, age, init_pos)
    f, mask = terms(db, da, done, scale, gamma, bool(flags & ZERO_TERMINAL))
    return None if reward is None else apply(reward, f, mask), f, mask


def goal_distances(type_planes, state_planes, W, H, rec_t, rec_n, rec_goal, pos_before, pos_after, age=None, init_pos=None,
                   pass_types=nav_ref.PASS_DEFAULT, flags=0, memo=None):
    """Per record: the distances of the acting and the after cell in the field of the record's env flooded from the
    record's goal cell (goal_moves_ref.goal_table); UNREACHABLE for both where rec_t, rec_n or the goal name nothing."""
    N = len(type_planes)
    T = pos_before.shape[0]
    rec_goal = np.asarray(rec_goal, np.float32).reshape(-1, 2)
    R = len(rec_t)
    memo = {} if memo is None else memo
    db, da = np.full(R, UNREACHABLE, np.int64), np.full(R, UNREACHABLE, np.int64)
    for b in range(R):
        t, n = int(rec_t[b]), int(rec_n[b])
        if not (0 <= t < T and 0 <= n < N):
            continue
        gc = visit_ref.cell_of(rec_goal[b, 0], rec_goal[b, 1], W, H)
        if gc >= W * H:
            continue
        if (n, gc) not in memo:
            memo[(n, gc)] = goal_moves_ref.goal_table(type_planes[n], None if state_planes is None else state_planes[n],
                                                      W, H, gc, pass_types, flags & nav_ref.DOORS_OPEN)
        field = memo[(n, gc)][1]                                  # uint16[H*W + 1], the last slot "no cell"
        clock = 1 if age is None else int(age[t, n])
        q = init_pos if clock <= 0 else pos_before[t, n]
        db[b] = field[visit_ref.cell_of(q[0], q[1], W, H)]
        da[b] = field[visit_ref.cell_of(pos_after[t, n, 0], pos_after[t, n, 1], W, H)]
    return db, da


def goal_shape(type_planes, state_planes, W, H, rec_t, rec_n, rec_goal, pos_before, pos_after, reward=None, done=None,
               age=None, init_pos=None, pass_types=nav_ref.PASS_DEFAULT, flags=0, scale=1.0, gamma=0.99, memo=None):
    """mg_nav_goal_shape -> (reward_out or None, F, mask), per record."""
    db, da = goal_distances(type_planes, state_planes, W, H, rec_t, rec_n, rec_goal, pos_before, pos_after, age, init_pos,
                            pass_types, flags, memo)
    f, mask = terms(db, da, done, scale, gamma, bool(flags & ZERO_TERMINAL))
    return None if reward is None else apply(reward, f, mask), f, mask
