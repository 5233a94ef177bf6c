"""The shortest-path kernels (include/minigrid_nav.h) on the device against the deque BFS of nav_ref.py, through the C
ABI, the torch front end, TwoarmyEngine, TwoarmyVecEnv and VecPPOTrainer.  Every comparison is exact integer equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import nav_ref
import visit_ref
from golden_util import load_traces
from nav_util import dev, host, u16_full

pytestmark = pytest.mark.gpu
_, SEED = load_traces()
DEV = "cuda:0"
SIZES = [(1, 1), (1, 7), (7, 1), (5, 9), (9, 4), (17, 17), (31, 32), (32, 32)]          # (W, H)
U = nav_ref.UNREACHABLE


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def worlds(seed, N, W, H, goals="random"):
    """N random worlds (walls at 0 / 0.2 / 0.45 in turn, every type code, doors in three states); goals: "random"
    leaves what random_world put there, "multi" sets exactly 0, 1 or 3 goal cells in turn."""
    rng = np.random.default_rng(seed)
    ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
    for n in range(N):
        ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[n % 3])
        if goals == "multi":
            ty[n][ty[n] == 8] = 1
            k = min((0, 1, 3)[(n // 3) % 3], W * H)
            ty[n][rng.permutation(W * H)[:k]] = 8
    return rng, ty, st


_CASES = {}


def case(W, H, N):
    """The worlds of one (size, N) with both references, computed once and never modified."""
    key = (W, H, N)
    if key not in _CASES:
        rng, ty, st = worlds(7 * W + 31 * H + 1000 * N, N, W, H, "multi")
        ax, ay = rng.integers(0, W, N).astype(np.int32), rng.integers(0, H, N).astype(np.int32)
        gx, gy = rng.integers(0, W, N).astype(np.int32), rng.integers(0, H, N).astype(np.int32)
        multi = nav_ref.fields(ty, st, W, H, agent=(ax, ay))
        single = nav_ref.fields(ty, st, W, H, goal=(gx, gy), agent=(ax, ay))
        for a in (ty, st, ax, ay, gx, gy) + multi + single:
            a.setflags(write=False)
        _CASES[key] = dict(ty=ty, st=st, agent=(ax, ay), goal=(gx, gy), multi=multi, single=single)
    return _CASES[key]


def check(got, want):
    dist, adist, aact, err = (host(g) for g in got)
    assert np.array_equal(dist, want[0])
    assert np.array_equal(err, want[3])
    if want[1] is not None:
        assert np.array_equal(adist, want[1]) and np.array_equal(aact, want[2])


# ------------------------------------------------------------------------------------------------ fields
@pytest.mark.parametrize("N", [1, 3, 65, 130])
@pytest.mark.parametrize("W,H", SIZES)
def test_fields_equal_the_bfs(W, H, N):
    c = case(W, H, N)
    ty, st = dev(c["ty"]), dev(c["st"])
    agent = tuple(dev(a) for a in c["agent"])
    check(nav().distance_field(ty, st, W, H, agent=agent), c["multi"])
    check(nav().distance_field(ty, st, W, H, goal=tuple(dev(g) for g in c["goal"]), agent=agent), c["single"])
    if N >= 65 and W * H > 1:                               # the cases are worth their name: every error code but 2, 3
        assert set(c["multi"][3].tolist()) == {0, 1} and set(c["single"][3].tolist()) == {0, 1}
        assert (c["multi"][1] == U).any() and (c["multi"][1] > 1).any()
        assert W * H > 289 or (c["multi"][1] == 0).any()     # an agent on a source, where the world is small enough


@pytest.mark.parametrize("W,H", [(32, 32), (31, 32)])
def test_long_paths(W, H):
    """A serpentine corridor: the far end is more than 255 moves away and the flood needs about W*H/2 steps, so an 8-bit
    or iteration-capped implementation fails."""
    ty, src = nav_ref.serpentine(W, H)
    last = H - 1 if H % 2 else H - 2                        # the corridor's last row
    ends = [src, (0 if (last // 2) % 2 else W - 1, last), (W // 2, 16)]
    tys = np.stack([ty] * 3)
    goal = (np.array([e[0] for e in ends], np.int32), np.array([e[1] for e in ends], np.int32))
    agent = (np.array([ends[1][0], ends[0][0], 0], np.int32), np.array([ends[1][1], ends[0][1], 0], np.int32))
    want = nav_ref.fields(tys, None, W, H, goal=goal, agent=agent)
    assert want[4][0] > 255 and want[4][0] >= W * H // 2 - W and want[1][0] > 255 and want[1][0] == want[1][1]
    check(nav().distance_field(dev(tys), None, W, H, goal=tuple(dev(g) for g in goal), agent=tuple(dev(a) for a in agent)),
          want)


def test_blocked_worlds():
    W, H = 9, 7
    ty = np.ones((4, W * H), np.uint8)
    g = ty.reshape(4, H, W)
    g[0, 3, 4] = 2                                          # env 0: the source is a wall -> error 1
    g[1, 2:5, 3:6] = 2; g[1, 3, 4] = 1                      # env 1: the source is walled in -> only itself, no error
    gx = np.array([4, 4, 9, 4], np.int32)                   # env 2: x = W -> error 2
    gy = np.array([3, 3, 3, -1], np.int32)                  # env 3: y = -1 -> error 2
    want = nav_ref.fields(ty, None, W, H, goal=(gx, gy))
    assert want[3].tolist() == [1, 0, 2, 2]
    assert (want[0][[0, 2, 3]] == U).all() and (want[0][1] != U).sum() == 1
    check(nav().distance_field(dev(ty), None, W, H, goal=(dev(gx), dev(gy))), want)
    ty[:] = 1                                               # no goal cell anywhere, and only walled-off goals
    ty[1, 0] = 8; ty[1, 1] = 2; ty[1, W] = 2
    ty[2, 5] = 8
    want = nav_ref.fields(ty, None, W, H, pass_types=nav_ref.PASS_DEFAULT & ~(1 << 8))
    assert want[3].tolist() == [1, 1, 1, 1]                 # a goal that may not be entered is no source
    check(nav().distance_field(dev(ty), None, W, H, pass_types=nav_ref.PASS_DEFAULT & ~(1 << 8)), want)
    want = nav_ref.fields(ty, None, W, H)
    assert want[3].tolist() == [1, 0, 0, 1] and (want[0][1] != U).sum() == 1
    check(nav().distance_field(dev(ty), None, W, H), want)


def test_pass_mask_and_doors():
    W, H = 9, 5
    ty = np.ones((1, H, W), np.uint8)
    st = np.zeros((1, H, W), np.uint8)
    ty[0, :, 3] = 9                                         # a lava moat
    ty[0, :, 6] = 2                                         # a wall with three doors: open, closed, locked
    ty[0, 0, 6] = ty[0, 2, 6] = ty[0, 4, 6] = 4
    st[0, 2, 6], st[0, 4, 6] = 1, 2
    ty[0, 1, 5] = 6                                         # a ball
    ty[0, 2, 0] = 8
    ty, st = ty.reshape(1, -1), st.reshape(1, -1)
    D = nav_ref.PASS_DEFAULT
    far = np.zeros((H, W), bool); far[:, 7:] = True
    for pass_types, flags, state in [(D, 0, st), (D & ~(1 << 9), 0, st), (D | (1 << 6), 0, st), (D, nav_ref.DOORS_OPEN, st),
                                     (D, 0, None), (D & ~(1 << 4), 0, None), (D & ~(1 << 4), nav_ref.DOORS_OPEN, st),
                                     (0xFFFF, 0, st), (0, 0, st)]:
        want = nav_ref.fields(ty, state, W, H, pass_types, flags)
        got = nav().distance_field(dev(ty), None if state is None else dev(state), W, H, pass_types,
                                   doors_open=bool(flags))
        check(got, want)
    d = nav_ref.fields(ty, st, W, H, D)[0].reshape(H, W)
    assert d[0, 8] == 10 and d[2, 7] == 11                   # through the open door at the top only
    assert nav_ref.fields(ty, None, W, H, D)[0].reshape(H, W)[2, 7] == 7            # state NULL: every door is open
    assert nav_ref.fields(ty, st, W, H, D, nav_ref.DOORS_OPEN)[0].reshape(H, W)[2, 7] == 7
    moat = nav_ref.fields(ty, st, W, H, D & ~(1 << 9))[0].reshape(H, W)
    assert (moat[:, 3:] == U).all() and (moat[:, :3] != U).all()
    assert d[1, 5] == U and nav_ref.fields(ty, st, W, H, D | (1 << 6))[0].reshape(H, W)[1, 5] == 6


# ------------------------------------------------------------------------------------------------ store discipline
@pytest.mark.parametrize("W,H", [(17, 17), (5, 9), (1, 1), (32, 32)])
def test_field_bases_and_pitches(W, H):
    N = 3
    c = case(W, H, N)
    ty, st = dev(c["ty"]), dev(c["st"])
    for off in (0, 2, 6, 14):
        for pitch in (W * H, W * H + 1, W * H + 7):
            buf = torch.full((16 + off + 2 * N * pitch + 32,), 0xA5, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 16 == 0
            rows = buf[16 + off:16 + off + 2 * N * pitch].view(torch.uint16).view(N, pitch)
            out = rows[:, :W * H]
            assert out.data_ptr() % 16 == off
            got = nav().distance_field(ty, st, W, H, out=out)
            assert got[0] is out
            want = np.full(buf.numel(), 0xA5, np.uint8)
            w16 = want[16 + off:16 + off + 2 * N * pitch].view(np.uint16).reshape(N, pitch)
            w16[:, :W * H] = c["multi"][0]
            assert np.array_equal(host(buf), want), (off, pitch)


@pytest.mark.parametrize("W,H", [(17, 17), (5, 9), (7, 1)])
def test_planes_off_a_word_boundary(W, H):
    N = 3
    c = case(W, H, N)
    want = c["multi"]
    n = N * W * H

    def inside(a, off):
        buf = torch.full((((4 + off + n + 3) & ~3) + 4,), 0xFF, dtype=torch.uint8, device=DEV)
        v = buf[4 + off:4 + off + n]
        v.copy_(dev(a).view(-1))
        assert v.data_ptr() % 4 == off
        return buf, v.view(N, W * H)
    for off_t in (1, 2, 3):
        for off_s in (0, 1, 3):
            bt, ty = inside(c["ty"], off_t)
            bs, st = inside(c["st"], off_s)
            check(nav().distance_field(ty, st, W, H, agent=tuple(dev(a) for a in c["agent"])), want)
            assert int((bt == 0xFF).sum()) >= bt.numel() - n and int((bs == 0xFF).sum()) >= bs.numel() - n


# ------------------------------------------------------------------------------------------------ agent outputs
def test_agent_outputs_contiguous_strided_and_without_field():
    W, H, N = 17, 17, 65
    c = case(W, H, N)
    ty, st = dev(c["ty"]), dev(c["st"])
    want = c["multi"]
    rec = torch.full((N, 48), -7, dtype=torch.int32, device=DEV)
    rec[:, 0], rec[:, 1] = dev(c["agent"][0]), dev(c["agent"][1])
    grec = torch.full((N, 48), -7, dtype=torch.int32, device=DEV)
    grec[:, 35], grec[:, 36] = dev(c["goal"][0]), dev(c["goal"][1])
    check(nav().distance_field(ty, st, W, H, agent=(rec[:, 0], rec[:, 1])), want)
    check(nav().distance_field(ty, st, W, H, goal=(grec[:, 35], grec[:, 36]), agent=(rec[:, 0], rec[:, 1])), c["single"])
    dist, adist, aact, err = nav().distance_field(ty, st, W, H, agent=(rec[:, 0], rec[:, 1]), want_field=False)
    assert dist is None
    assert np.array_equal(host(adist), want[1]) and np.array_equal(host(aact), want[2]) and np.array_equal(host(err), want[3])
    dist, adist, aact, err = nav().distance_field(ty, st, W, H, agent=tuple(dev(a) for a in c["agent"]), want_field=False,
                                                  want_error=False)
    assert err is None and np.array_equal(host(adist), want[1]) and np.array_equal(host(aact), want[2])
    given = [torch.full((N,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]         # results into the caller's tensors
    got = nav().distance_field(ty, st, W, H, agent=(rec[:, 0], rec[:, 1]), want_field=False, agent_out=tuple(given[:2]),
                               error_out=given[2])
    assert got[0] is None and all(g is t for g, t in zip(got[1:], given))
    assert all(np.array_equal(host(t), w) for t, w in zip(given, want[1:4]))


def test_expert_tie_break_source_unreachable_and_outside():
    W, H = 7, 7
    agents = [(5, 5), (1, 5), (5, 1), (1, 1), (3, 3), (0, 0), (-1, 3), (3, 7), (3, 2), (4, 3)]
    N = len(agents)
    ty = np.ones((N, H, W), np.uint8)
    ty[5, 0, 1] = ty[5, 1, 0] = 2                           # env 5: the agent's corner is cut off
    ty = ty.reshape(N, -1)
    gx, gy = np.full(N, 3, np.int32), np.full(N, 3, np.int32)
    ax, ay = np.array([a[0] for a in agents], np.int32), np.array([a[1] for a in agents], np.int32)
    want = nav_ref.fields(ty, None, W, H, goal=(gx, gy), agent=(ax, ay))
    # from the four diagonals: left before up / down, right before up / down; then the source, cut off, outside twice
    assert want[2].tolist() == [0, 1, 0, 1, 6, -1, -1, -1, 3, 0]
    assert want[1].tolist() == [4, 4, 4, 4, 0, U, U, U, 1, 1]
    assert want[3].tolist() == [0, 0, 0, 0, 0, 0, 3, 3, 0, 0]
    assert (want[0][6] != U).all()                           # error 3 leaves the field intact
    check(nav().distance_field(dev(ty), None, W, H, goal=(dev(gx), dev(gy)), agent=(dev(ax), dev(ay))), want)


# ------------------------------------------------------------------------------------------------ closed loop with mg_step
def test_expert_actions_drive_mg_step_to_the_goal():
    """The movement rule is mg_step's own: following the expert action, every env terminates at exactly step dist0
    with the reward mg_step computes for that step count, and the distance falls by one per step."""
    from twoarmy_amd import minigrid_view as mv
    W = H = 9
    N, max_steps = 64, 100
    rng = np.random.default_rng(42)
    tys, sts, axs, ays, d0 = [], [], [], [], []
    while len(tys) < N:
        ty, st = nav_ref.random_world(rng, W, H, 0.25)
        g = ty.reshape(H, W)
        g[ty.reshape(H, W) == 8] = 1
        g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 2
        g[rng.integers(1, H - 1), rng.integers(1, W - 1)] = 8
        ax, ay = int(rng.integers(1, W - 1)), int(rng.integers(1, H - 1))
        r = nav_ref.field(ty, st, W, H, agent=(ax, ay))
        if r["agent_dist"] in (0, U):
            continue
        tys.append(ty); sts.append(st); axs.append(ax); ays.append(ay); d0.append(r["agent_dist"])
    d0 = np.array(d0)
    assert d0.max() >= 6
    ty, st = dev(np.stack(tys)), dev(np.stack(sts))
    ax, ay = dev(np.array(axs, np.int32)), dev(np.array(ays, np.int32))
    adir = torch.zeros(N, dtype=torch.int32, device=DEV)
    count = torch.zeros(N, dtype=torch.int32, device=DEV)
    done_at = np.zeros(N, np.int64)
    for k in range(int(d0.max())):
        _, adist, aact, err = nav().distance_field(ty, st, W, H, agent=(ax, ay), want_field=False)
        live = done_at == 0
        assert not host(err).any()
        assert np.array_equal(host(adist)[live], d0[live] - k)
        assert np.array_equal(host(adist)[~live], np.zeros((~live).sum()))
        act = host(aact)
        assert set(act[live].tolist()) <= {0, 1, 2, 3} and (act[~live] == 6).all()
        reward, term, trunc, serr = mv.step(ty, st, W, H, aact, ax, ay, adir, count, max_steps)
        assert not host(serr).any() and not host(trunc).any()
        term, reward = host(term), host(reward)
        assert np.array_equal(term[live] != 0, d0[live] == k + 1)
        for n in np.nonzero(live & (term != 0))[0]:
            done_at[n] = k + 1
            assert reward[n] == 1 - 0.9 * (int(d0[n]) / max_steps)
    assert np.array_equal(done_at, d0)


# ------------------------------------------------------------------------------------------------ lookup
@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("T", [1, 7, 130])
def test_lookup(T, N):
    W, H = 17, 13
    c = case(W, H, N)
    rng = np.random.default_rng(T * 100 + N)
    pos = rng.uniform(-2, 19, (T, N, 2)).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, -0.0, 0.0, W - 1, W, H - 1, H, -1, -0.5, 0.999, np.float32(H) - np.float32(1e-6)]
    k = 0
    for a in special:
        for b in special:
            pos.reshape(-1, 2)[k % (T * N)] = (a, b)
            k += 5
    cells = np.array([[visit_ref.cell_of(pos[t, n, 0], pos[t, n, 1], W, H) for n in range(N)] for t in range(T)])
    want = nav_ref.lookup(c["multi"][0], pos, W, H, lambda p, w, h: cells)
    dist = dev(c["multi"][0])
    got = nav().lookup(dist, dev(pos), W, H)
    assert got.dtype == torch.uint16 and np.array_equal(host(got), want)
    if T * N > 100:
        assert (cells == W * H).any() and (N == 1 or (want != U).any())            # env 0 of a case has no goal
    wide = dev(np.concatenate([c["multi"][0], np.full((N, 5), 0xA5A5, np.uint16)], axis=1))
    out = u16_full((T, N))
    assert nav().lookup(wide[:, :W * H], dev(pos), W, H, out=out) is out and np.array_equal(host(out), want)
    if T == 1:
        assert np.array_equal(host(nav().lookup(dist, dev(pos[0]), W, H)), want[0])


# ------------------------------------------------------------------------------------------------ engine, env, trainer
def _engine_want(eng, pass_types=nav_ref.PASS_DEFAULT):
    ty, _, rec = eng.get_state()
    return nav_ref.fields(ty, None, 17, 17, pass_types, agent=(rec[:, 0], rec[:, 1]))


@pytest.mark.parametrize("variant", [4, 6])
def test_engine_distance_field(variant):
    from twoarmy_amd.engine import TwoarmyEngine
    N = 64
    eng = TwoarmyEngine(variant, N, 17, seed=SEED)
    eng.reset()
    want = _engine_want(eng)
    check(eng.distance_field(), want)
    assert (want[1] > 0).all() and (want[1] != U).all() and not want[3].any()
    out = eng.alloc_outputs(T=64)
    eng.rollout(64, out, actions=eng.fill_actions(64))
    check(eng.distance_field(), _engine_want(eng))
    static = nav_ref.PASS_DEFAULT | (1 << 6)
    check(eng.distance_field(pass_types=static), _engine_want(eng, static))
    gx = dev(np.full(N, 1, np.int32)), dev(np.full(N, 15, np.int32))
    ty = eng.get_state()[0]
    check(eng.distance_field(goal=gx, agent=False), nav_ref.fields(ty, None, 17, 17, goal=(np.full(N, 1), np.full(N, 15))))
    eng.close()


def test_engine_views_follow_a_pipelined_rollout():
    """A rollout of 8 steps or more with auto-reset writes the state's ping-pong partner and swaps the two: the views
    render() and distance_field() share must show the state as it stands, as views of a host copy of it do."""
    from twoarmy_amd import minigrid_render as mr
    from twoarmy_amd.engine import TwoarmyEngine
    N = 16
    eng = TwoarmyEngine(4, N, 17, seed=SEED)
    eng.reset()
    first = eng.render(tile_size=4).clone()                 # builds the views before the swap
    out = eng.alloc_outputs(T=16)
    eng.rollout(16, out, actions=eng.fill_actions(16))
    ty, co, rec = eng.get_state()
    rec = dev(rec)
    want = mr.render(dev(ty), dev(co), None, 17, 17, rec[:, 0], rec[:, 1], rec[:, 2], 4)
    got = eng.render(tile_size=4)
    assert torch.equal(got, want) and not torch.equal(got, first)
    eng.close()


def test_vecenv_goal_distance_adds_two_info_fields_and_changes_nothing_else():
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    N = 16
    envs = [TwoarmyVecEnv("v4", N, seed=SEED, goal_distance=g) for g in (True, False, False)]
    obs = [e.reset() for e in envs]
    assert all(torch.equal(obs[0], o) for o in obs[1:])
    g = torch.Generator().manual_seed(5)
    dones = 0
    for step in range(60):
        a = torch.randint(0, 5, (N,), generator=g).to(DEV)
        res = [e.step(a) for e in envs]
        for r in res[1:]:
            for x, y in zip(res[0][:4], r[:4]):
                assert torch.equal(x, y)
            assert set(res[0][4]) == set(r[4]) | {"goal_distance", "expert_action"}
            for key in r[4]:
                assert torch.equal(res[0][4][key], r[4][key])
        assert set(res[1][4]) == set(res[2][4]) == {"final_observation", "_final_observation"}
        want = _engine_want(envs[0].engine)
        info = res[0][4]
        assert info["goal_distance"].dtype == torch.int32 and info["expert_action"].dtype == torch.int32
        assert np.array_equal(host(info["goal_distance"]), want[1]) and np.array_equal(host(info["expert_action"]), want[2])
        dones += int((res[0][2] | res[0][3]).sum())
    assert dones > 0                                        # max_steps = 50 < 60: auto-reset happened
    for e in envs:
        e.close()


def test_trainer_account_distance():
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    from twoarmy_amd.soa.train_ppo import distance_fields
    N, T = 64, 32
    torch.manual_seed(9981)
    eng = TwoarmyEngine(4, N, 17, seed=SEED)
    agent = PPO()
    agent.to(eng.device).use_nhwc()
    tr = VecPPOTrainer(agent, eng, rollout_steps=T, minibatch=256)
    twin = TwoarmyEngine(4, N, 17, seed=SEED)                # replays the trainer's actions: positions and planes that do
    step_out = twin.alloc_outputs()                         # not pass through the trainer's own buffers
    with pytest.raises(RuntimeError):
        tr.distance_stats()
    ended = 0
    for _ in range(2):
        tr.collect()
        got = tr.account_distance()
        term, trunc = host(tr.term), host(tr.trunc)
        pos = np.empty((T, N, 2), np.float32)
        for t in range(T):
            twin.step(tr.action[t].to(torch.int32).contiguous(), step_out, autoreset=True, policy_idx=True)
            pos[t] = host(step_out["pos"])
        ty = twin.get_state()[0]
        assert np.array_equal(ty, eng.get_state()[0])
        field = nav_ref.fields(ty, None, 17, 17, nav_ref.PASS_DEFAULT | (1 << 6))[0]
        cells = np.array([[visit_ref.cell_of(pos[t, n, 0], pos[t, n, 1], 17, 17) for n in range(N)] for t in range(T)])
        want = nav_ref.lookup(field, pos, 17, 17, lambda p, w, h: cells).astype(np.int64)
        assert np.array_equal(host(got).astype(np.int64), want)
        ds = tr.distance_stats()
        ok, done = want != U, (term | trunc) != 0
        assert ds["cut_off"] == int((~ok).sum()) and ds["mean"] == want[ok].sum() / ok.sum()
        if (ok & done).any():
            assert ds["end_mean"] == want[ok & done].sum() / (ok & done).sum() and ds["end_min"] == want[ok & done].min()
        else:
            assert ds["end_mean"] is None and ds["end_min"] is None
        assert distance_fields(ds).startswith(" goal_dist end mean/min ")
        ended += int(done.sum())
        tr.update()
        tr.carry_over()
    assert ended > 0
    eng.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ argument rejection
def test_bad_arguments_launch_nothing():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    W, H, N = 5, 4, 3
    ty = torch.ones((N, W * H), dtype=torch.uint8, device=DEV)
    xy = torch.zeros(N, dtype=torch.int32, device=DEV)
    dist = u16_full((N, W * H + 2))
    outs = [torch.full((N,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=DEV) for _ in range(3)]
    pos = torch.zeros((2, N, 2), dtype=torch.float32, device=DEV)
    look = u16_full((2, N))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                       # noqa: E731
    good = dict(type=ty, state=None, n=N, W=W, H=H, pass_types=nav_ref.PASS_DEFAULT, flags=0, gx=xy, gy=xy, gs=1, ax=xy,
                ay=xy, as_=1, dist=dist, pitch=W * H + 2, adist=outs[0], aact=outs[1], err=outs[2])

    def field(**kw):
        a = dict(good, **kw)
        dptr = a["dist"] if isinstance(a["dist"], (int, type(None))) else a["dist"].data_ptr()
        return lib.mg_nav_field(p(a["type"]), p(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"], p(a["gx"]),
                                p(a["gy"]), a["gs"], p(a["ax"]), p(a["ay"]), a["as_"], C.c_void_p(dptr), a["pitch"],
                                p(a["adist"]), p(a["aact"]), p(a["err"]), None)

    bad = [dict(n=0), dict(W=0), dict(H=0), dict(W=33), dict(H=33), dict(W=-1), dict(type=None), dict(pitch=W * H - 1),
           dict(pitch=1), dict(pitch=-1), dict(gx=None), dict(gy=None), dict(ax=None), dict(ay=None),
           dict(ax=None, ay=None), dict(ax=None, ay=None, aact=None), dict(ax=None, ay=None, adist=None),
           dict(gs=0), dict(as_=0), dict(as_=-1), dict(pass_types=0x10000), dict(flags=2), dict(dist=dist.data_ptr() + 1)]
    for kw in bad:
        assert field(**kw) == -1, kw
    with torch.cuda.device(DEV):
        torch.cuda.synchronize()
    assert (host(dist) == 0xA5A5).all() and all((host(o) == 0xA5A5A5A5 - (1 << 32)).all() for o in outs)

    def lookup(**kw):
        a = dict(dict(dist=dist.data_ptr(), pitch=W * H + 2, n=N, W=W, H=H, pos=pos.data_ptr(), T=2, out=look.data_ptr()), **kw)
        return lib.mg_nav_lookup(C.c_void_p(a["dist"]), a["pitch"], a["n"], a["W"], a["H"], C.c_void_p(a["pos"]), a["T"],
                                 C.c_void_p(a["out"]), None)
    for kw in [dict(dist=None), dict(pos=None), dict(out=None), dict(n=0), dict(T=-1), dict(W=0), dict(H=33),
               dict(pitch=W * H - 1), dict(pitch=-3), dict(dist=dist.data_ptr() + 1), dict(out=look.data_ptr() + 1),
               dict(pos=pos.data_ptr() + 4), dict(n=1 << 20, T=1 << 20)]:
        assert lookup(**kw) == -1, kw
    assert lookup(T=0) == 0
    torch.cuda.synchronize()
    assert (host(look) == 0xA5A5).all()
    # and the good calls do launch
    assert field() == 0 and lookup() == 0
    torch.cuda.synchronize()
    manhattan = np.add.outer(np.arange(H), np.arange(W)).reshape(-1)                    # an empty room, source (0, 0)
    assert (host(dist)[:, :W * H] == manhattan).all() and (host(dist)[:, W * H:] == 0xA5A5).all()
    assert host(outs[0]).tolist() == [0] * N and host(outs[1]).tolist() == [6] * N and host(outs[2]).tolist() == [0] * N
    assert (host(look) == 0).all()
