"""Properties of the path-efficiency restatement (tests/path_ref.py; include/minigrid_nav.h, "Path efficiency") on worlds
small enough to follow by hand.  No GPU."""
import numpy as np

import nav_ref
import path_ref
import timed_nav_ref as tref

U = nav_ref.UNREACHABLE
MOVE = {0: (-1, 0), 1: (1, 0), 2: (0, -1), 3: (0, 1), 6: (0, 0)}          # action -> (dx, dy)


def centre(x, y):
    return (y + 0.5, x + 0.5)                                             # pos = (y, x)


def static_world():
    """5 x 4, walled, interior x 1..3, y 1..2 with a wall on (2, 1): from (1, 1) the goal (3, 1) is 4 moves away, round
    the wall through the lower row."""
    W, H = 5, 4
    ty = np.full((H, W), 2, np.uint8)
    ty[1:3, 1:4] = 1
    ty[1, 2] = 2
    ty[1, 3] = 8
    dist = nav_ref.field(ty.reshape(-1), None, W, H)["dist"]
    assert dist[1 * W + 1] == 4 and dist[1 * W + 3] == 0 and dist[1 * W + 2] == U
    return W, H, dist[None]                                               # [N = 1, H*W]


def timed_world():
    """5 x 5, walled: the lower room is the single cell (2, 3), the upper room y = 1, the gap (2, 2) between them is free at
    phase 0 only (period 3).  From (2, 3) at phase 0: wait, wait, up, up -- 4 transitions."""
    W, H, P = 5, 5, 3
    ty = np.full((H, W), 2, np.uint8)
    ty[1, 1:4] = 1
    ty[2, 2] = ty[3, 2] = 1
    ty[1, 2] = 8
    blocked = np.zeros((P, H), np.int64)
    blocked[1, 2] = blocked[2, 2] = 1 << 2
    dist = tref.field(ty.reshape(-1), None, W, H, blocked, P)["dist"]
    assert dist[0, 3 * W + 2] == 4 and dist[1, 2 * W + 2] == U and dist[0, 2 * W + 2] == 1
    return W, H, P, dist[None]                                            # [N = 1, P, H*W]


def follow(dist, W, H, x, y, actions=None, limit=20):
    """One episode of one env from (x, y) at age 0: the expert (the lowest set bit of the move set at every step) or the
    given actions -> (pos_before, pos_after [T, 1, 2], age [T, 1], the actions taken)."""
    P = dist.shape[1] if dist.ndim == 3 else 1
    d = dist[0] if dist.ndim == 3 else dist
    before, after, taken = [], [], []
    for t in range(limit if actions is None else len(actions)):
        if actions is None:
            m, here = tref.move_set(d, W, H, y * W + x, tref.phase_of(t, P))
            if here == 0:
                break
            a = tref.action_of(m)
        else:
            a = actions[t]
        before.append(centre(x, y))
        x, y = x + MOVE[a][0], y + MOVE[a][1]
        after.append(centre(x, y))
        taken.append(a)
    T = len(taken)
    return (np.array(before, np.float32).reshape(T, 1, 2), np.array(after, np.float32).reshape(T, 1, 2),
            np.arange(T, dtype=np.int32).reshape(T, 1), taken)


def flags(T, term_last=False, trunc_last=False):
    te, tr = np.zeros((T, 1), np.uint8), np.zeros((T, 1), np.uint8)
    te[-1], tr[-1] = term_last, trunc_last
    return te, tr


def scan(dist, W, H, before, after, age, te, tr, init):
    field = dist[:, 0] if dist.ndim == 3 and dist.shape[1] == 1 else dist
    return path_ref.path_scan(field, before, after, W, H, te, tr, path_ref.zero_carry(1), age, np.array(init, np.float32))


def test_the_expert_is_on_path_all_the_way():
    W, H, dist = static_world()
    before, after, age, taken = follow(dist[:, None], W, H, 1, 1)
    assert taken == [3, 1, 1, 2]                                          # down, right, right, up: round the wall
    te, tr = flags(4, term_last=True)
    (s, b, o, k), carry = scan(dist, W, H, before, after, age, te, tr, centre(1, 1))
    assert s[:, 0].tolist() == [4] * 4 and b[:, 0].tolist() == [3, 2, 1, 0]
    assert o[:, 0].tolist() == [0] * 4 and k[:, 0].tolist() == [1, 2, 3, 4]
    assert carry[3][0] == 0                                               # the episode ended: none is running
    v = path_ref.path_summary(s, b, o, k, te, tr)
    assert v.tolist() == [1, 1, 1, 1.0, 4, 0, 1.0, 0, 4, 0]               # SPL 1, steps == start, all progress made
    d = path_ref.derived(v)
    assert d == {"spl": 1.0, "success_rate": 1.0, "progress": 1.0, "off_path_rate": 0.0}


def test_an_agent_that_never_moves():
    W, H, dist = static_world()
    before, after, age, _ = follow(dist[:, None], W, H, 1, 1, actions=[6] * 6)
    te, tr = flags(6, trunc_last=True)
    (s, b, o, k), _ = scan(dist, W, H, before, after, age, te, tr, centre(1, 1))
    assert o[:, 0].tolist() == k[:, 0].tolist() == [1, 2, 3, 4, 5, 6] and b[:, 0].tolist() == s[:, 0].tolist() == [4] * 6
    v = path_ref.path_summary(s, b, o, k, te, tr)
    assert v.tolist() == [1, 0, 1, 0.0, 4, 4, 0.0, 6, 6, 4]
    assert path_ref.derived(v) == {"spl": 0.0, "success_rate": 0.0, "progress": 0.0, "off_path_rate": 1.0}


def test_a_detour_costs_path_length():
    """Down, up again, then the expert's four moves: 6 steps for a start distance of 4, one of them off path."""
    W, H, dist = static_world()
    before, after, age, _ = follow(dist[:, None], W, H, 1, 1, actions=[3, 2, 3, 1, 1, 2])
    te, tr = flags(6, term_last=True)
    (s, b, o, k), _ = scan(dist, W, H, before, after, age, te, tr, centre(1, 1))
    assert o[:, 0].tolist() == [0, 1, 1, 1, 1, 1] and b[-1, 0] == 0       # up again is off path; down a second time: d 4 -> 3
    v = path_ref.path_summary(s, b, o, k, te, tr)
    assert v[3] == 4 / 6 and v[7] == 1 and v[8] == 6


def test_the_timed_expert_waits_and_its_waits_are_on_path():
    W, H, P, dist = timed_world()
    before, after, age, taken = follow(dist, W, H, 2, 3)
    assert taken == [6, 6, 2, 2]                                          # wait, wait, up, up
    te, tr = flags(4, term_last=True)
    (s, b, o, k), _ = scan(dist, W, H, before, after, age, te, tr, centre(2, 3))
    assert o[:, 0].tolist() == [0] * 4 and b[:, 0].tolist() == [3, 2, 1, 0] and s[-1, 0] == k[-1, 0] == 4
    v = path_ref.path_summary(s, b, o, k, te, tr)
    assert v[3] == 1.0 and v[6] == 1.0 and v[7] == 0
    # the same waits are off path on the static map, where nothing blocks the gap: distance 2 all along
    static = nav_ref.field(np.where(dist[0, 0] == U, 2, 1).astype(np.uint8), None, W, H, goal=(2, 1))["dist"][None]
    (s1, b1, o1, k1), _ = scan(static, W, H, before, after, age, te, tr, centre(2, 3))
    assert s1[0, 0] == 2 and o1[:, 0].tolist() == [1, 2, 2, 2]


def test_stepping_into_the_blocker_is_off_path_and_leaves_best_alone():
    W, H, P, dist = timed_world()
    before, after, age, _ = follow(dist, W, H, 2, 3, actions=[2])         # up at phase 0: the gap is blocked at phase 1
    te, tr = flags(1, trunc_last=True)
    db, da = path_ref.shape_ref.distances(dist, before, after, W, H, age, np.array(centre(2, 3), np.float32))
    assert db[0, 0] == 4 and da[0, 0] == U
    (s, b, o, k), _ = scan(dist, W, H, before, after, age, te, tr, centre(2, 3))
    assert (s[0, 0], b[0, 0], o[0, 0], k[0, 0]) == (4, 4, 1, 1)
    v = path_ref.path_summary(s, b, o, k, te, tr)
    assert v.tolist() == [1, 0, 1, 0.0, 4, 4, 0.0, 1, 1, 4]


def test_an_unreachable_start_is_counted_and_not_rated():
    W, H, dist = static_world()
    before, after, age, _ = follow(dist[:, None], W, H, 2, 1, actions=[6, 6])          # it stands on the interior wall
    te, tr = flags(2, trunc_last=True)
    (s, b, o, k), _ = scan(dist, W, H, before, after, age, te, tr, centre(2, 1))
    assert s[:, 0].tolist() == b[:, 0].tolist() == [U, U] and o[:, 0].tolist() == [1, 2]
    v = path_ref.path_summary(s, b, o, k, te, tr)
    assert v.tolist() == [1, 0, 0, 0.0, 0, 0, 0.0, 2, 2, np.inf]
    assert path_ref.derived(v) == {"spl": None, "success_rate": 0.0, "progress": None, "off_path_rate": 1.0}
    assert path_ref.derived(np.zeros(10)) == {"spl": None, "success_rate": None, "progress": None, "off_path_rate": None}


def test_cutting_the_rollout_anywhere_changes_nothing():
    W, H, dist = static_world()
    N, T = 3, 12
    rng = np.random.default_rng(3)
    field = np.repeat(dist, N, 0)
    xy = rng.integers(0, 5, (T + 1, N, 2)).astype(np.float32) + 0.5       # any cell of the world, walls included
    xy[..., 0] = np.minimum(xy[..., 0], H - 0.5)
    before, after = xy[:-1], xy[1:]
    te = (rng.random((T, N)) < 0.2).astype(np.uint8)
    tr = (rng.random((T, N)) < 0.2).astype(np.uint8)
    age = rng.integers(-1, 3, (T, N)).astype(np.int32)
    init = np.array(centre(1, 1), np.float32)
    carry0 = (np.array([4, 0, 2], np.uint16), np.array([1, 0, 2], np.uint16), np.array([5, 0, 0], np.int32),
              np.array([7, 0, 1], np.int32))                              # env 0 and 2 in a running episode
    whole, carry = path_ref.path_scan(field, before, after, W, H, te, tr, carry0, age, init)
    assert (te | tr).any() and whole[3].max() > 7
    for t in range(T + 1):
        a, mid = path_ref.path_scan(field, before[:t], after[:t], W, H, te[:t], tr[:t], carry0, age[:t], init)
        b, end = path_ref.path_scan(field, before[t:], after[t:], W, H, te[t:], tr[t:], mid, age[t:], init)
        assert all(np.array_equal(np.concatenate([x, y]), w) for x, y, w in zip(a, b, whole)), t
        assert all(np.array_equal(x, y) for x, y in zip(end, carry)), t
