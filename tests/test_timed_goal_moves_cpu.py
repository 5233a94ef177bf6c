"""Host-side checks of mg_nav_timed_goal_moves (include/minigrid_nav.h): the per-record reference against the references of
the kernels it must agree with, its labels driving the C oracle through Twoarmy's door gap towards hindsight goals, the
header against the ctypes table, and the argument checks of the trainer and the command line."""
import os
import re
import types

import numpy as np
import pytest

import goal_moves_ref
import nav_ref
import timed_goal_moves_ref as tgref
import timed_nav_ref as tref
import twoarmy_oracle as orc
import visit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = tref.UNREACHABLE
STATIC = nav_ref.PASS_DEFAULT | (1 << 6)                     # balls enterable: only the schedule blocks


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def _world(rng, W, H, N, P, density=0.25):
    ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
    for n in range(N):
        ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.0, 0.2)[n % 2])
    sched = np.stack([tref.random_schedule(rng, P, H, density) for _ in range(N)])
    return ty, st, sched


def _positions(rng, T, N, W, H):
    c = rng.integers(0, W * H, (T, N))
    pos = np.stack([c // W + 0.5, c % W + 0.25], -1).astype(np.float32)
    if T * N > 8:
        pos.reshape(-1, 2)[3] = (np.nan, 0.5)
        pos.reshape(-1, 2)[5] = (H, 0.0)
    return pos


# ------------------------------------------------------------------------------------------------ 1. the reference against itself
@pytest.mark.parametrize("W,H,P", [(1, 5, 2), (5, 1, 3), (7, 9, 6), (17, 17, 6), (9, 4, 16), (6, 5, 1)])
def test_one_goal_per_env_is_the_timed_field_then_the_timed_moves(W, H, P):
    """Invariant (a) on the host."""
    rng = np.random.default_rng(1000 * W + 10 * H + P)
    N, T = 3, 7
    ty, st, sched = _world(rng, W, H, N, P)
    for shared in (False, True):
        blocked = sched[0] if shared else sched
        gc = rng.integers(0, W * H, N)
        pos = _positions(rng, T, N, W, H)
        age = rng.integers(-1, 3 * P + 2, (T, N)).astype(np.int32)
        init = np.array([H - 0.5, 0.25], np.float32)
        dist = tref.fields(ty, st, W, H, blocked, P, goal=(gc % W, gc // W))[0]
        fm, fd = tref.moves(dist, pos, age, init, W, H, visit_ref.cell_of)
        order = rng.permutation(T * N)
        t, n = order // N, order % N
        goal = np.stack([gc[n] // W + 0.5, gc[n] % W + 0.75], 1).astype(np.float32)
        m, d = tgref.timed_goal_moves(ty, st, W, H, blocked, P, t, n, goal, pos, age, init)
        assert np.array_equal(m, fm[t, n]) and np.array_equal(d, fd[t, n])
        if W * H >= 30:
            assert (d != U).any() and (m != 0).any()


@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (9, 4), (17, 17)])
def test_period_one_with_an_empty_schedule_is_the_static_reference(W, H):
    """Invariant (b) on the host."""
    rng = np.random.default_rng(31 * W + H)
    N, T, R = 3, 6, 120
    ty, st, _ = _world(rng, W, H, N, 1)
    pos = _positions(rng, T, N, W, H)
    age = rng.integers(-1, 4, (T, N)).astype(np.int32)
    init = np.array([0.5, W - 0.5], np.float32)
    t, n = rng.integers(-1, T + 1, R), rng.integers(-1, N + 1, R)
    gc = rng.integers(0, W * H, R)
    goal = np.stack([gc // W + 0.5, gc % W + 0.5], 1).astype(np.float32)
    goal[::17] = (np.nan, 0.5)
    for pass_types in (nav_ref.PASS_DEFAULT, STATIC):
        want = goal_moves_ref.goal_moves(ty, st, W, H, t, n, goal, pos, age, init, pass_types)
        got = tgref.timed_goal_moves(ty, st, W, H, np.zeros((1, H), np.uint32), 1, t, n, goal, pos, age, init, pass_types)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not (got[0] & tref.MOVE_STAY)[got[1] != 0].any()          # nobody waits in a world that stands still


@pytest.mark.parametrize("W,H,P", [(5, 9, 6), (17, 17, 6), (12, 11, 16), (7, 7, 2)])
def test_lowest_bit_is_the_timed_expert_action_towards_the_goal(W, H, P):
    rng = np.random.default_rng(W * 100 + H * 10 + P)
    N, T, R = 2, 3 * P, 300
    ty, st, sched = _world(rng, W, H, N, P)
    pos = _positions(rng, T, N, W, H)
    age = rng.integers(0, 3 * P, (T, N)).astype(np.int32)
    init = np.array([0.5, 0.5], np.float32)
    t, n = rng.integers(0, T, R), rng.integers(0, N, R)
    pool = rng.integers(0, W * H, (N, 4))
    gc = pool[n, rng.integers(0, 4, R)]
    goal = np.stack([gc // W + 0.5, gc % W + 0.5], 1).astype(np.float32)
    m, d = tgref.timed_goal_moves(ty, st, W, H, sched, P, t, n, goal, pos, age, init)
    seen = set()
    for b in range(R):
        q = init if age[t[b], n[b]] <= 0 else pos[t[b], n[b]]
        c = visit_ref.cell_of(q[0], q[1], W, H)
        if c >= W * H:
            assert (m[b], d[b]) == (0, U)
            continue
        r = tref.field(ty[n[b]], st[n[b]], W, H, sched[n[b]], P, goal=(gc[b] % W, gc[b] // W),
                       agent=(c % W, c // W, age[t[b], n[b]]))
        assert tref.action_of(int(m[b])) == r["agent_action"] and int(d[b]) == r["agent_dist"], b
        seen.add(r["agent_action"])
    assert seen >= {0, 1, 2, 3, -1} and (6 in seen or W * H < 100), seen


# ------------------------------------------------------------------------------------------------ 2. closed loop on the oracle
# (x, y): beyond the door gap; three in row 8 of the gap itself, under the balls in three, three and one of the six phases
GOALS = [(9, 8), (8, 6), (8, 4), (3, 4), (12, 5), (10, 8), (6, 8)]


def _planes(env):
    return np.frombuffer(env.e.type, np.uint8).copy()[None], np.frombuffer(env.e.state, np.uint8).copy()[None]


def _follow(gx, gy, label):
    """A v6 episode from the reset under label(planes, x, y, step_move) -> (moves, dist), the lowest bit taken, until the
    agent stands on (gx, gy) or the episode is cut off -> (steps or None, the first label's distance, rewards, moves onto
    a ball).  A move onto a ball: its target cell holds a ball once the balls have moved (the oracle then leaves the agent
    where it is), or a ball lands on the agent (-0.9)."""
    env = orc.OracleEnv(6)
    rewards, d0, onto = [], None, 0
    for k in range(80):
        m, d = label(_planes(env), env.e.ax, env.e.ay, env.e.step_move)
        d0 = d if d0 is None else d0
        if (env.e.ax, env.e.ay) == (gx, gy):
            assert (m, d) == (tref.MOVE_STAY, 0)
            return k, d0, rewards, onto
        a = tref.action_of(m)
        assert a in (0, 1, 2, 3, 6), (k, m, d)
        x, y = env.e.ax, env.e.ay
        _, reward, term, trunc, err = env.step(a)
        assert err is None and not term
        rewards.append(reward)
        if a < 4:
            tx, ty = x + (-1, 1, 0, 0)[a], y + (0, 0, -1, 1)[a]
            if _planes(env)[0][0, ty * 17 + tx] == 6:
                assert (env.e.ax, env.e.ay) == (x, y)
                onto += 1
            else:
                assert (env.e.ax, env.e.ay) == (tx, ty)          # every other labelled move is one the oracle makes
        onto += reward == -0.9
        if trunc:
            return None, d0, rewards, onto
    raise AssertionError("the goal was not reached")


def test_reference_labels_reach_hindsight_goals_beyond_the_gap_on_the_oracle():
    """The timed label of a record whose goal lies beyond the door gap, recomputed at every step from the agent's cell
    and clock in the field of the reset (schedule with the two wall blocks present), leads there in exactly
    acting_dist steps, never onto a ball and never under a -0.9; the static label of mg_nav_goal_moves, followed the
    same way, does step onto a ball for the goals behind the middle of the gap (and is cut off pushing against it)."""
    sched = nav().twoarmy_schedule(blocks=True).numpy().astype(np.int64)
    hit_static = []
    for gx, gy in GOALS:
        goal = np.array([[gy + 0.5, gx + 0.5]], np.float32)
        memo = {}
        ty0, st0 = _planes(orc.OracleEnv(6))

        def timed(planes, x, y, clock):                          # the clock of the reset is <= 0: init_pos acts, at phase 0
            pos = np.array([[[y + 0.5, x + 0.5]]], np.float32)
            m, d = tgref.timed_goal_moves(ty0, st0, 17, 17, sched, 6, [0], [0], goal, pos, np.array([[clock]]), pos[0, 0],
                                          STATIC, memo=memo)
            return int(m[0]), int(d[0])

        def static(planes, x, y, clock):
            pos = np.array([[[y + 0.5, x + 0.5]]], np.float32)
            m, d = goal_moves_ref.goal_moves(planes[0], planes[1], 17, 17, [0], [0], goal, pos, pass_types=STATIC)
            return int(m[0]), int(d[0])

        steps, d0, rewards, onto = _follow(gx, gy, timed)
        assert steps == d0 and d0 != U and onto == 0 and -0.9 not in rewards, (gx, gy, steps, d0, onto, rewards)
        s_steps, s_d0, s_rewards, s_onto = _follow(gx, gy, static)
        assert s_d0 <= d0                                        # waiting costs steps, never saves any
        hit_static.append(s_onto > 0)
        print("goal (%d, %d): timed %d steps, static distance %d, static moves onto a ball: %d, static arrives: %s"
              % (gx, gy, steps, s_d0, s_onto, s_steps is not None))
    assert any(hit_static)


# ------------------------------------------------------------------------------------------------ 3. header and ctypes table
def test_header_arguments_are_the_ctypes_table():
    import twoarmy_amd
    header = open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"mg_nav_timed_goal_moves": "type state n_envs width height pass_types flags blocked blocked_env_stride period "
                                       "rec_t rec_n rec_goal n_records pos age init_pos T moves acting_dist stream",
            "mg_nav_timed_goal_floods": "width height period"}
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
    for word in ("depends on record b alone", "(a)", "(b)", "free at no phase", "launches nothing"):
        assert word in header[header.index("mg_nav_goal_moves over (cell, phase)"):], word


# ------------------------------------------------------------------------------------------------ 4. trainer and command line
def test_hindsight_timed_needs_hindsight():
    from twoarmy_amd.soa import train_ppo
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    with pytest.raises(ValueError, match="hindsight=True"):
        VecPPOTrainer.enable_prior(types.SimpleNamespace(), 0.5, hindsight_timed=True)       # before anything is touched
    with pytest.raises(ValueError, match="hindsight=True"):
        VecPPOTrainer.enable_prior(types.SimpleNamespace(), 0.5, timed=True, hindsight_timed=True)
    with pytest.raises(SystemExit, match="--prior_hindsight_timed needs --prior_hindsight"):
        train_ppo.main(["--expert_agreement", "--prior_hindsight_timed"])
    with pytest.raises(SystemExit, match="--prior_hindsight_timed needs --prior_hindsight"):
        train_ppo.main(["--prior_coef", "0.1", "--prior_timed", "--prior_hindsight_timed"])
    args = train_ppo.build_parser().parse_args(["--expert_agreement", "--prior_hindsight", "--prior_hindsight_timed"])
    assert args.prior_hindsight_timed and not train_ppo.build_parser().parse_args([]).prior_hindsight_timed
