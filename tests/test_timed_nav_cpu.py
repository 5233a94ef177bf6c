"""Host-side checks of the time-expanded fields (include/minigrid_nav.h): the (cell, phase) reference against the static
one, Twoarmy's ball schedule against the C oracle, the reference expert driving the oracle through the door gap, the
invariant between move set and action, and the header against the ctypes table."""
import os
import re

import numpy as np
import pytest

import nav_ref
import timed_nav_ref as tref
import twoarmy_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = tref.UNREACHABLE
STATIC = nav_ref.PASS_DEFAULT | (1 << 6)                     # balls enterable: only the schedule blocks


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def _header():
    return open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()


# ------------------------------------------------------------------------------------------------ 1. P = 1 is the static field
@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (7, 1), (5, 9), (9, 4), (17, 17), (31, 32), (32, 32)])
def test_period_one_with_an_empty_schedule_is_the_static_reference(W, H):
    rng = np.random.default_rng(77 * W + H)
    for k in range(9):
        ty, st = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[k % 3])
        for g in rng.integers(0, W * H, k % 4):
            ty[g] = 8
        pass_types = [nav_ref.PASS_DEFAULT, nav_ref.PASS_DEFAULT & ~(1 << 9), STATIC][k % 3]
        flags = nav_ref.DOORS_OPEN if k % 4 == 3 else 0
        state = None if k % 5 == 4 else st
        goal = None if k % 2 == 0 else (int(rng.integers(-1, W + 1)), int(rng.integers(0, H)))
        agent = (int(rng.integers(-1, W + 1)), int(rng.integers(0, H)))
        a = nav_ref.field(ty, state, W, H, pass_types, flags, goal, agent)
        b = tref.field(ty, state, W, H, np.zeros((1, H), np.uint32), 1, pass_types, flags, goal, agent + (k - 3,))
        assert np.array_equal(a["dist"], b["dist"][0]), (W, H, k)
        assert (a["error"], a["agent_dist"], a["agent_action"], a["depth"]) == \
               (b["error"], b["agent_dist"], b["agent_action"], b["depth"]), (W, H, k)


# ------------------------------------------------------------------------------------------------ 2. the schedule
def _schedule(**kw):
    return nav().twoarmy_schedule(**kw).numpy().astype(np.int64)


def test_twoarmy_schedule_is_where_the_oracle_puts_the_balls():
    """20 consecutive v6 steps from a reset (the agent stays in its corner): after the step that raised step_move to k
    the balls of the oracle's plane are exactly the cells of phase k % 6, and step_move restarts with the episode."""
    sched = _schedule()
    assert sched.shape == (6, 17) and nav().TWOARMY_PERIOD == tref.TWOARMY_P == 6
    env = orc.OracleEnv(6)

    def balls():
        ty = np.frombuffer(env.e.type, np.uint8).reshape(17, 17)
        return np.array([sum(1 << x for x in range(17) if ty[y, x] == 6) for y in range(17)], np.int64)

    assert env.e.step_move == 0 and np.array_equal(balls(), sched[0])
    for k in range(1, 21):
        _, reward, term, trunc, err = env.step(6)
        assert err is None and not term and not trunc and reward == -0.01
        assert env.e.step_move == k
        assert np.array_equal(balls(), sched[k % 6]), k
        assert sorted(env.e.ob_x) == tref.twoarmy_balls(k) and set(env.e.ob_y) == {8}
    assert [tref.twoarmy_balls(k) for k in range(6)] == [[7, 8, 9], [8, 9, 10], [7, 8, 9], [6, 7, 8], [6, 7, 8], [6, 7, 8]]
    risk = _schedule(avoid_risk=True)
    assert np.array_equal(risk[:, 9], sched[:, 8]) and np.array_equal(np.delete(risk, 9, axis=1), np.delete(sched, 9, axis=1))
    blocks = _schedule(blocks=True) ^ sched
    want = np.zeros(17, np.int64)
    for x, y in tref.TWOARMY_BLOCKS:
        want[y] |= 1 << x
    assert (blocks == want[None]).all()


# ------------------------------------------------------------------------------------------------ 3. end to end on the oracle
def _planes(env):
    return np.frombuffer(env.e.type, np.uint8).copy(), np.frombuffer(env.e.state, np.uint8).copy()


@pytest.mark.parametrize("avoid_risk", [False, True])
def test_reference_expert_crosses_the_gap_on_the_oracle(avoid_risk):
    """From a v6 reset the expert of ONE field computed at the reset (the schedule with the two wall blocks present)
    reaches the goal after exactly the predicted number of steps, never hit by a ball (-0.9) and, with avoid_risk,
    never beside one (-0.1)."""
    env = orc.OracleEnv(6)
    sched = _schedule(avoid_risk=avoid_risk, blocks=True)
    ty, st = _planes(env)
    r = tref.field(ty, st, 17, 17, sched, 6, STATIC, agent=(env.e.ax, env.e.ay, env.e.step_move))
    d0 = r["agent_dist"]
    static = nav_ref.field(ty, st, 17, 17, STATIC, agent=(env.e.ax, env.e.ay))["agent_dist"]
    assert r["error"] == 0 and static == 24 and static <= d0 < 50, (static, d0)
    rewards, waits = [], 0
    for k in range(d0):
        c = env.e.ay * 17 + env.e.ax
        m, d = tref.move_set(r["dist"], 17, 17, c, tref.phase_of(env.e.step_move, 6))
        assert d == d0 - k and env.e.step_move == k
        a = tref.action_of(m)
        assert a in (0, 1, 2, 3, 6)
        waits += a == 6
        _, reward, term, trunc, err = env.step(a)
        assert err is None and not trunc
        rewards.append(reward)
        assert term == (k == d0 - 1), (k, d0)
        if k == 0:                                           # the blocks the field was planned with are there now
            g = np.frombuffer(env.e.type, np.uint8).reshape(17, 17)
            assert all(g[y, x] == 2 for x, y in tref.TWOARMY_BLOCKS)
    assert rewards[-1] == 0.9 and -0.9 not in rewards
    assert 0.2 in rewards                                    # it went through the gap into the second room
    if avoid_risk:
        assert -0.1 not in rewards
    print("avoid_risk=%s: static %d, timed %d, waits %d, rewards %s" % (avoid_risk, static, d0, waits, sorted(set(rewards))))


def test_the_gap_is_crossable_under_avoid_risk_by_the_named_path():
    """(6, 9) at phase 0 -> (6, 8) at phase 1 -> (6, 7): free cells of the schedule at those phases."""
    risk = _schedule(avoid_risk=True)
    assert not (risk[0, 9] >> 6) & 1 and not (risk[1, 8] >> 6) & 1 and not (risk[2, 7] >> 6) & 1


# ------------------------------------------------------------------------------------------------ 4. move set and action
def _literal_action(dist, W, H, c, p):
    """The expert action as include/minigrid_nav.h words it."""
    P = dist.shape[0]
    d = int(dist[p, c])
    if d == 0:
        return 6
    if d == U:
        return -1
    x, y = c % W, c // W
    nxt = dist[(p + 1) % P]
    for a, (nx, ny) in enumerate(((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1))):
        if 0 <= nx < W and 0 <= ny < H and nxt[ny * W + nx] == d - 1:
            return a
    assert nxt[c] == d - 1, "a reachable state has an optimal transition"
    return 6


@pytest.mark.parametrize("W,H,P", [(1, 7, 3), (5, 9, 6), (9, 4, 7), (17, 17, 6), (12, 11, 16), (6, 5, 1), (7, 7, 2)])
def test_lowest_bit_of_the_move_set_is_the_expert_action(W, H, P):
    rng = np.random.default_rng(W * 100 + H * 10 + P)
    seen = set()
    for k in range(4):
        ty, st = nav_ref.random_world(rng, W, H, (0.0, 0.2)[k % 2])
        ty[rng.integers(0, W * H)] = 8
        sched = tref.random_schedule(rng, P, H, 0.25)
        r = tref.field(ty, st, W, H, sched, P)
        free = tref.free_cells(ty, st, W, H, sched, P)
        assert ((r["dist"].reshape(P, H, W) != U) <= free).all()      # a distance is defined on free states only
        for p in range(P):
            for c in range(W * H):
                m, d = tref.move_set(r["dist"], W, H, c, p)
                a = tref.action_of(m)
                assert a == _literal_action(r["dist"], W, H, c, p), (k, p, c)
                assert (m == 0) == (d == U) and (d != 0 or m == tref.MOVE_STAY)
                seen.add(a if d else "source")
        for c, p in zip(rng.integers(0, W * H, 6), rng.integers(0, P, 6)):      # the agent outputs are that state's
            agent = tref.field(ty, st, W, H, sched, P, agent=(c % W, c // W, p + 5 * P))
            assert (agent["agent_dist"], agent["agent_action"]) == (int(r["dist"][p, c]), _literal_action(r["dist"], W, H, c, p))
    if W * H >= 30 and P > 1:
        assert seen >= {0, 1, 2, 3, 6, -1, "source"}, seen           # waiting is optimal somewhere


def test_clock_rule():
    assert [tref.phase_of(k, 6) for k in (-7, -1, 0, 1, 5, 6, 7, 6000005)] == [0, 0, 0, 1, 5, 0, 1, 5]


# ------------------------------------------------------------------------------------------------ 5. header and ctypes table
def test_header_arguments_are_the_ctypes_table():
    import twoarmy_amd
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    want = {"mg_nav_timed_field": "type state n_envs width height pass_types flags blocked blocked_env_stride period goal_x "
                                  "goal_y goal_stride agent_x agent_y agent_clock agent_stride dist dist_pitch agent_dist "
                                  "agent_action error stream",
            "mg_nav_timed_moves": "dist dist_pitch period n_envs width height pos age init_pos T moves acting_dist stream"}
    for name, names in want.items():
        args = [a.strip() for a in re.search(r"\b%s\s*\((.*?)\);" % name, txt, re.S).group(1).split(",")]
        assert [re.search(r"(\w+)$", a).group(1) for a in args] == names.split(), name
        res, sig = twoarmy_amd._lib._SIGS[name]
        assert len(sig) == len(args) and name in twoarmy_amd._lib.exported_symbols()
        for a, c in zip(args, sig):
            is_ptr = "*" in a
            assert is_ptr == (c is twoarmy_amd._lib._vp), (name, a)
            if not is_ptr:
                assert {"int": "c_int", "int64_t": "c_long", "uint32_t": "c_uint"}[a.split()[0]] == c.__name__, (name, a)
    assert int(re.search(r"#define MG_NAV_MAX_PERIOD\s+(\d+)", _header()).group(1)) == 16 == nav().MAX_PERIOD == tref.MAX_PERIOD
    assert nav().MOVE_STAY == tref.MOVE_STAY == 1 << int(re.search(r"#define MG_NAV_MOVE_STAY_BIT\s+(\d+)", _header()).group(1))
