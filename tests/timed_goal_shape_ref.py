"""Host restatement of mg_nav_timed_goal_shape (include/minigrid_nav.h): per record, the queue BFS over (cell, phase) of the
record's env from the record's goal cell (timed_goal_moves_ref.goal_field), the distance of the acting cell at the phase of
the record's clock and of the after cell at the phase that follows (timed_nav_ref.phase_of, visit_ref.cell_of), and the
float rule of shape_ref (terms / apply: not restated here).  The only thing shared between records is a memo of (env, goal
cell) -> field; the order of the records is immaterial.  Test-side only."""
import numpy as np

import nav_ref
import shape_ref
import timed_goal_moves_ref as tgref
import timed_nav_ref as tref
import visit_ref

UNREACHABLE = tref.UNREACHABLE
ZERO_TERMINAL = shape_ref.ZERO_TERMINAL


def goal_distances(type_planes, state_planes, W, H, blocked, P, rec_t, rec_n, rec_goal, pos_before, pos_after, age, init_pos,
                   pass_types=nav_ref.PASS_DEFAULT, flags=0, memo=None):
    """-> (d_before, d_after) int64[R]: UNREACHABLE for both where rec_t, rec_n or the goal name nothing; for either where
    its position is no cell (a cell that is not free at its phase is UNREACHABLE in the field already)."""
    N = len(type_planes)
    blocked = np.asarray(blocked)
    age = np.asarray(age)
    T = age.shape[0]
    assert age.shape == (T, N) and np.asarray(pos_before).shape == (T, N, 2) and np.asarray(pos_after).shape == (T, N, 2)
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
            memo[(n, gc)] = tgref.goal_field(type_planes[n], None if state_planes is None else state_planes[n], W, H,
                                             blocked if blocked.ndim == 2 else blocked[n], P, gc, pass_types,
                                             flags & nav_ref.DOORS_OPEN)
        field = memo[(n, gc)]                                     # uint16[P, H*W]
        clock = int(age[t, n])
        q = init_pos if clock <= 0 else pos_before[t, n]
        cb = visit_ref.cell_of(q[0], q[1], W, H)
        ca = visit_ref.cell_of(pos_after[t, n, 0], pos_after[t, n, 1], W, H)
        if cb < W * H:
            db[b] = field[tref.phase_of(clock, P), cb]
        if ca < W * H:
            da[b] = field[tref.phase_of(max(clock, 0) + 1, P), ca]
    return db, da


def timed_goal_shape(type_planes, state_planes, W, H, blocked, P, rec_t, rec_n, rec_goal, pos_before, pos_after, age,
                     init_pos, reward=None, done=None, pass_types=nav_ref.PASS_DEFAULT, flags=0, scale=1.0, gamma=0.99,
                     memo=None):
    """mg_nav_timed_goal_shape -> (reward_out or None, F, mask), per record.  type_planes (state_planes or None)
    uint8[N, H*W]; blocked integer[P, H] (shared) or [N, P, H]; rec_t, rec_n int[R]; rec_goal float32[R, 2] = (y, x);
    pos_before / pos_after float32[T, N, 2]; age int[T, N] (the clock as well) and init_pos float32[2], both required;
    reward float32[R], done uint8[R]; flags: nav_ref.DOORS_OPEN | ZERO_TERMINAL.  memo: a dict the caller keeps across
    calls on the same worlds, schedule, pass mask and door flag."""
    db, da = goal_distances(type_planes, state_planes, W, H, blocked, P, rec_t, rec_n, rec_goal, pos_before, pos_after, age,
                            init_pos, pass_types, flags, memo)
    f, mask = shape_ref.terms(db, da, done, scale, gamma, bool(flags & ZERO_TERMINAL))
    return None if reward is None else shape_ref.apply(reward, f, mask), f, mask
