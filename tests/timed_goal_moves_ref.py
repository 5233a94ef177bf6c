"""Host restatement of mg_nav_timed_goal_moves (include/minigrid_nav.h): per record, the queue BFS over (cell, phase) of the
record's env from the record's goal cell (timed_nav_ref.field) and the move set of the acting cell at the phase of the
record's clock (timed_nav_ref.move_set).  The only thing shared between records is a memo of (env, goal cell) -> field; the
order of the records is immaterial.  Test-side only."""
import numpy as np

import nav_ref
import timed_nav_ref as tref
import visit_ref

UNREACHABLE = tref.UNREACHABLE
MOVE_STAY = tref.MOVE_STAY


def goal_field(type_plane, state_plane, W, H, blocked, P, goal_cell, pass_types=nav_ref.PASS_DEFAULT, flags=0):
    """One world and one goal cell -> dist uint16[P, H*W]; all UNREACHABLE where the goal cell is free at no phase."""
    return tref.field(type_plane, state_plane, W, H, blocked, P, pass_types, flags, goal=(goal_cell % W, goal_cell // W))["dist"]


def timed_goal_moves(type_planes, state_planes, W, H, blocked, P, rec_t, rec_n, rec_goal, pos, age, init_pos,
                     pass_types=nav_ref.PASS_DEFAULT, flags=0, memo=None):
    """type_planes (state_planes or None) uint8[N, H*W]; blocked integer[P, H] (shared) or [N, P, H]; rec_t, rec_n int[R];
    rec_goal float32[R, 2] = (y, x); pos float32[T, N, 2] BEFORE each step, age int[T, N] (the clock as well) and init_pos
    float32[2], both required -> (moves uint8[R], acting_dist uint16[R]).  memo: a dict the caller keeps across calls on
    the same worlds, schedule, pass mask and flags."""
    N = len(type_planes)
    blocked = np.asarray(blocked)
    age = np.asarray(age)
    T = age.shape[0]
    assert age.shape == (T, N) and np.asarray(pos).shape == (T, N, 2)
    rec_goal = np.asarray(rec_goal, np.float32).reshape(-1, 2)
    R = len(rec_t)
    memo = {} if memo is None else memo
    moves, ad = np.zeros(R, np.uint8), np.full(R, UNREACHABLE, np.uint16)
    for b in range(R):
        t, n = int(rec_t[b]), int(rec_n[b])
        if not (0 <= t < T and 0 <= n < N):
            continue
        gc = visit_ref.cell_of(rec_goal[b, 0], rec_goal[b, 1], W, H)
        if gc >= W * H:
            continue
        q = init_pos if age[t, n] <= 0 else pos[t, n]
        c = visit_ref.cell_of(q[0], q[1], W, H)
        if c >= W * H:
            continue
        if (n, gc) not in memo:
            memo[(n, gc)] = goal_field(type_planes[n], None if state_planes is None else state_planes[n], W, H,
                                       blocked if blocked.ndim == 2 else blocked[n], P, gc, pass_types, flags)
        moves[b], ad[b] = tref.move_set(memo[(n, gc)], W, H, c, tref.phase_of(age[t, n], P))
    return moves, ad
