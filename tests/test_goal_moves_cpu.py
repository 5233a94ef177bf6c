"""The host reference of mg_nav_goal_moves (goal_moves_ref.py) against the independent relaxation of nav_ref.py, and the
header's invariant restated on the references: one goal per env equals field + optimal_moves."""
import numpy as np

import goal_moves_ref
import nav_ref
import prior_ref

U = nav_ref.UNREACHABLE


def moves_from_relax(d, W, H, c):
    """The definition, from a relaxed field: which neighbours of cell c lie inside the world and one move nearer."""
    if c >= W * H or d[c] == U:
        return 0, U
    if d[c] == 0:
        return prior_ref.STAY, 0
    x, y, m = c % W, c // W, 0
    for k, dx, dy in nav_ref.MOVES:
        nx, ny = x + dx, y + dy
        if 0 <= nx < W and 0 <= ny < H and d[ny * W + nx] == d[c] - 1:
            m |= 1 << k
    return m, int(d[c])


def test_reference_equals_the_relaxation_on_random_worlds():
    rng = np.random.default_rng(2024)
    seen = set()
    for i in range(100):
        W, H = [(1, 1), (1, 7), (9, 4), (5, 5), (17, 17), (7, 12)][i % 6]
        ty, st = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[i % 3])
        pass_types = (nav_ref.PASS_DEFAULT, nav_ref.PASS_DEFAULT | 1 << 6, 0x0002, 0xFFFF)[i % 4]
        flags = (0, nav_ref.DOORS_OPEN)[(i // 4) % 2]
        state = None if i % 5 == 0 else st
        T, N, R = 3, 1, 12
        pos = (rng.random((T, N, 2)) * (H, W)).astype(np.float32)
        pos[0, 0] = (H, 0.5) if i % 7 == 0 else pos[0, 0]                   # a position that is no cell
        age = rng.integers(-1, 2, (T, N)).astype(np.int32)
        init = np.array([H - 0.5, 0.25], np.float32)
        rec_t = rng.integers(-1, T + 1, R)
        rec_n = rng.integers(-1, N + 1, R)
        rec_n[:8], rec_t[:8] = 0, rng.integers(0, T, 8)
        goal = (rng.random((R, 2)) * (H, W)).astype(np.float32)
        goal[1] = pos[rec_t[1], 0] if age[rec_t[1], 0] > 0 else init       # the acting position itself
        goal[2] = (np.nan, 0.5)
        goal[3] = (0.5, -0.25)
        m, d = goal_moves_ref.goal_moves(ty[None], None if state is None else state[None], W, H, rec_t, rec_n, goal, pos,
                                         age, init, pass_types, flags)
        for b in range(R):
            ok = 0 <= rec_t[b] < T and 0 <= rec_n[b] < N
            gy, gx = goal[b]
            want = (0, U)
            if ok and 0 <= gy < H and 0 <= gx < W:
                rd = nav_ref.relax(ty, state, W, H, pass_types, flags, goal=(int(gx), int(gy)))
                a = init if age[rec_t[b], 0] <= 0 else pos[rec_t[b], 0]
                c = int(a[0]) * W + int(a[1]) if 0 <= a[0] < H and 0 <= a[1] < W else W * H
                want = moves_from_relax(rd, W, H, c)
            assert (int(m[b]), int(d[b])) == want, (i, b)
            seen.add("stay" if m[b] == prior_ref.STAY else "cut" if d[b] == U else bin(int(m[b])).count("1"))
    assert seen >= {"stay", "cut", 1, 2}


def test_one_goal_per_env_is_field_plus_optimal_moves():
    rng = np.random.default_rng(7)
    for W, H in [(5, 5), (9, 4), (17, 17)]:
        N, T = 4, 6
        worlds = [nav_ref.random_world(rng, W, H, 0.2) for _ in range(N)]
        ty, st = np.stack([w[0] for w in worlds]), np.stack([w[1] for w in worlds])
        gx, gy = rng.integers(0, W, N), rng.integers(0, H, N)
        gx[0], gy[0] = np.flatnonzero(ty[0] == 2)[0] % W, np.flatnonzero(ty[0] == 2)[0] // W     # a goal on a wall
        pos = (rng.random((T, N, 2)) * (H, W)).astype(np.float32)
        age = rng.integers(-1, 3, (T, N)).astype(np.int32)
        init = np.array([0.5, W - 0.5], np.float32)
        dist = nav_ref.fields(ty, st, W, H, goal=(gx, gy))[0]
        want_m, want_d = prior_ref.optimal_moves(dist, pos, W, H, age, init)
        t, n = np.divmod(rng.permutation(T * N), N)
        goal = np.stack([gy[n] + 0.5, gx[n] + 0.25], 1).astype(np.float32)
        m, d = goal_moves_ref.goal_moves(ty, st, W, H, t, n, goal, pos, age, init)
        assert np.array_equal(m, want_m[t, n]) and np.array_equal(d, want_d[t, n])
        assert (d[n == 0] == U).all() and (d != U).any()

