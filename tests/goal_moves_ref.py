"""Host restatement of mg_nav_goal_moves (include/minigrid_nav.h): per record, the BFS field of the record's env from the
record's goal cell (nav_ref.field) and the optimal-move set of the acting cell in it (prior_ref.cell_moves).  The only
thing shared between records is a memo of (env, goal cell) -> field; the order of the records is immaterial.  Test-side
only."""
import numpy as np

import nav_ref
import prior_ref
import visit_ref

UNREACHABLE = nav_ref.UNREACHABLE


def goal_table(type_plane, state_plane, W, H, goal_cell, pass_types=nav_ref.PASS_DEFAULT, flags=0):
    """One world and one goal cell -> (moves uint8[H*W + 1], dist uint16[H*W + 1]) of every acting cell, the extra slot
    H*W ("no cell") holding 0 / UNREACHABLE.  A goal that is not enterable leaves the whole field UNREACHABLE."""
    f = nav_ref.field(type_plane, state_plane, W, H, pass_types, flags, goal=(goal_cell % W, goal_cell // W))
    return prior_ref.cell_moves(f["dist"], W, H), np.concatenate([f["dist"], np.array([UNREACHABLE], np.uint16)])


def goal_moves(type_planes, state_planes, W, H, rec_t, rec_n, rec_goal, pos, age=None, init_pos=None,
               pass_types=nav_ref.PASS_DEFAULT, flags=0, memo=None):
    """type_planes (state_planes or None) uint8[N, H*W]; rec_t, rec_n int[R]; rec_goal float32[R, 2] = (y, x); pos
    float32[T, N, 2] BEFORE each step, age int[T, N] with init_pos float32[2] -> (moves uint8[R], acting_dist
    uint16[R]).  memo: a dict the caller keeps across calls on the same worlds, pass mask and flags."""
    N = len(type_planes)
    p = prior_ref.acting_positions(pos, age, init_pos)
    T = p.shape[0]
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
        if (n, gc) not in memo:
            memo[(n, gc)] = goal_table(type_planes[n], None if state_planes is None else state_planes[n], W, H, gc,
                                       pass_types, flags)
        c = visit_ref.cell_of(p[t, n, 0], p[t, n, 1], W, H)
        moves[b], ad[b] = memo[(n, gc)][0][c], memo[(n, gc)][1][c]
    return moves, ad

