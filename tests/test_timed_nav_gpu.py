"""The time-expanded shortest-path kernels (mg_nav_timed_field, mg_nav_timed_moves: include/minigrid_nav.h) on the device
against the (cell, phase) queue BFS of timed_nav_ref.py, through the C ABI, the torch front end, TwoarmyEngine,
TwoarmyVecEnv and VecPPOTrainer.  Every comparison is exact integer equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import nav_ref
import timed_nav_ref as tref
import visit_ref
from nav_util import dev, host, u16_full

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = tref.UNREACHABLE
SIZES = [(1, 1), (1, 7), (2, 2), (5, 9), (9, 4), (17, 17), (31, 32), (32, 32)]            # (W, H)
PERIODS = [1, 2, 6, 7, 16]
COUNTS = [1, 2, 3, 9, 65]          # one env, both envs of a wavefront, ragged workgroups of 8, 4 and 2 envs
STATIC = nav_ref.PASS_DEFAULT | (1 << 6)


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def sched(b):
    return dev(np.asarray(b, np.uint32).view(np.int32))


def check(got, want):
    dist, adist, aact, err = (host(g) for g in got)
    assert np.array_equal(dist, want[0])
    assert np.array_equal(err, want[3])
    if want[1] is not None:
        assert np.array_equal(adist, want[1]) and np.array_equal(aact, want[2])


_CASES = {}


def case(W, H, P, N, per_env):
    """Random worlds (every type code 0..17, doors in three states) with a random schedule and the reference's results,
    computed once and never modified.  Clocks: <= 0, = P, small and large."""
    key = (W, H, P, N, per_env)
    if key not in _CASES:
        rng = np.random.default_rng(7 * W + 31 * H + 1000 * N + 13 * P + per_env)
        ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
        for n in range(N):
            ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[n % 3])
            ty[n][ty[n] == 8] = 1
            ty[n][rng.permutation(W * H)[:min((1, 0, 3)[(n // 3) % 3], W * H)]] = 8
        if W * H >= 18:
            ty[0][rng.permutation(W * H)[:18]] = np.arange(18)
            st[0][ty[0] == 4] = rng.integers(0, 3, int((ty[0] == 4).sum()))
        blocked = np.stack([tref.random_schedule(rng, P, H) for _ in range(N)]) if per_env else tref.random_schedule(rng, P, H)
        ax, ay = rng.integers(0, W, N).astype(np.int32), rng.integers(0, H, N).astype(np.int32)
        gx, gy = rng.integers(0, W, N).astype(np.int32), rng.integers(0, H, N).astype(np.int32)
        clock = np.array([(-3, 0, P, 1, P - 1, 2 * P + 1, 2 ** 31 - 1, 1000003)[n % 8] for n in range(N)], np.int32)
        clock = rng.permutation(clock)
        multi = tref.fields(ty, st, W, H, blocked, P, agent=(ax, ay, clock))
        single = tref.fields(ty, st, W, H, blocked, P, goal=(gx, gy), agent=(ax, ay, clock))
        for a in (ty, st, blocked, ax, ay, gx, gy, clock) + multi + single:
            a.setflags(write=False)
        _CASES[key] = dict(ty=ty, st=st, blocked=blocked, agent=(ax, ay), clock=clock, goal=(gx, gy), multi=multi, single=single)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ fields
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("W,H", SIZES)
def test_fields_equal_the_bfs(W, H, P):
    """Every size with every period; the env counts and shared / per-env schedules rotate through the grid so that each
    count meets small and large worlds and short and long periods."""
    k = SIZES.index((W, H)) + PERIODS.index(P)
    N, per_env = COUNTS[k % 5], (k // 5) % 2
    c = case(W, H, P, N, per_env)
    ty, st, b = dev(c["ty"]), dev(c["st"]), sched(c["blocked"])
    agent, clock = tuple(dev(a) for a in c["agent"]), dev(c["clock"])
    check(nav().timed_field(ty, st, W, H, b, agent=agent, clock=clock), c["multi"])
    check(nav().timed_field(ty, st, W, H, b, goal=tuple(dev(g) for g in c["goal"]), agent=agent, clock=clock), c["single"])


@pytest.mark.parametrize("N", COUNTS)
@pytest.mark.parametrize("per_env", [0, 1])
def test_env_counts_and_schedules_at_the_twoarmy_shape(N, per_env):
    W, H, P = 17, 17, 6
    c = case(W, H, P, N, per_env)
    got = nav().timed_field(dev(c["ty"]), dev(c["st"]), W, H, sched(c["blocked"]), agent=tuple(dev(a) for a in c["agent"]),
                            clock=dev(c["clock"]))
    check(got, c["multi"])
    if N == 65:
        assert set(c["multi"][3].tolist()) == {0, 1} and (c["multi"][1] == U).any() and (c["multi"][1] > 1).any()
        assert (c["multi"][2] == 6).any()
    # the clock and the agent as strided columns of one record tensor, the schedule as uint32
    rec = torch.full((N, 48), -7, dtype=torch.int32, device=DEV)
    rec[:, 0], rec[:, 1], rec[:, 4] = dev(c["agent"][0]), dev(c["agent"][1]), dev(c["clock"])
    got = nav().timed_field(dev(c["ty"]), dev(c["st"]), W, H, sched(c["blocked"]).view(torch.uint32),
                            agent=(rec[:, 0], rec[:, 1]), clock=rec[:, 4])
    check(got, c["multi"])
    # no clock: phase 0
    want0 = tref.fields(c["ty"], c["st"], W, H, c["blocked"], P, agent=c["agent"])
    check(nav().timed_field(dev(c["ty"]), dev(c["st"]), W, H, sched(c["blocked"]), agent=tuple(dev(a) for a in c["agent"])), want0)


def test_hand_made_worlds():
    # a 1 x 7 corridor, source at the right end, a blocker that stands on cell 3 except at phase 2 (of 4): the agent on
    # cell 2 can only wait until the blocker lifts
    W, H, P = 7, 1, 4
    ty = np.ones((4, W), np.uint8)
    b = np.zeros((4, P, H), np.uint32)
    b[0, :, 0] = 1 << 3
    b[0, 2, 0] = 0
    b[1, :, 0] = 1 << 3                                      # env 1: cell 3 is blocked at every phase: cut off
    b[2, 1:, 0] = 1 << 6                                     # env 2: the goal is free at phase 0 only
    b[3, :, 0] = 0
    b[3, 1, 0] = 1 << 1                                      # env 3: the agent stands on a cell blocked at its phase
    gx, gy = np.full(4, 6, np.int32), np.zeros(4, np.int32)
    ax, ay = np.array([2, 2, 5, 1], np.int32), np.zeros(4, np.int32)
    clock = np.array([0, 0, 2, 1], np.int32)
    want = tref.fields(ty, None, W, H, b, P, goal=(gx, gy), agent=(ax, ay, clock))
    d = want[0]
    # env 0: from (2, phase 0) wait once, step onto 3 at phase 2, then three more moves
    assert want[1][0] == 5 and want[2][0] == 6 and d[0, 1, 2] == 4 and d[0, 2, 3] == 3 and d[0, 0, 3] == U
    assert tref.move_set(d[0], W, H, 2, 0)[0] == tref.MOVE_STAY and tref.move_set(d[0], W, H, 2, 1)[0] == 2
    assert want[1][1] == U and want[2][1] == -1 and (d[1, :, :4] == U).all() and (d[1, :, 4:] != U).all() and want[3][1] == 0
    assert d[2, 0, 6] == 0 and (d[2, 1:, 6] == U).all() and want[1][2] == 2 and want[2][2] == 6     # arrive at phase 0
    assert want[1][3] == U and want[2][3] == -1 and d[3, 0, 1] == 5
    check(nav().timed_field(dev(ty), None, W, H, sched(b), goal=(dev(gx), dev(gy)), agent=(dev(ax), dev(ay)),
                            clock=dev(clock)), want)
    # errors: a source blocked at every phase (1), outside (2), the agent outside (3)
    b2 = np.zeros((3, P, H), np.uint32)
    b2[0, :, 0] = 1 << 6
    gx2, ax2 = np.array([6, 7, 6], np.int32), np.array([0, 0, -1], np.int32)
    want = tref.fields(ty[:3], None, W, H, b2, P, goal=(gx2, gy[:3]), agent=(ax2, ay[:3], clock[:3]))
    assert want[3].tolist() == [1, 2, 3] and (want[0][:2] == U).all() and (want[0][2] != U).all()
    check(nav().timed_field(dev(ty[:3]), None, W, H, sched(b2), goal=(dev(gx2), dev(gy[:3])), agent=(dev(ax2), dev(ay[:3])),
                            clock=dev(clock[:3])), want)


def test_serpentine_at_sixteen_phases():
    """A 32 x 32 serpentine whose corridor has turnstiles that open at one phase of 16: the far end is thousands of
    transitions away, so a flood capped below W*H*P rounds, or an 8-bit distance, fails; P = 16 at the largest world
    is also the largest image a launch asks for."""
    W = H = 32
    P = 16
    ty, src = nav_ref.serpentine(W, H)
    b = np.zeros((P, H), np.uint32)
    for y in range(0, H, 2):
        for p in range(P):
            if p != (3 * y) % P:
                b[p, y] |= 1 << 15                           # a turnstile in the middle of every corridor row
    last = (W - 1, H - 2)
    tys = np.stack([ty, ty])
    goal = (np.array([src[0], last[0]], np.int32), np.array([src[1], last[1]], np.int32))
    agent = (np.array([last[0], src[0]], np.int32), np.array([last[1], src[1]], np.int32))
    clock = np.array([5, 0], np.int32)
    want = tref.fields(tys, None, W, H, b, P, goal=goal, agent=agent + (clock,))
    assert want[4][0] > 527 and want[1][0] > 527 and want[1][1] > 527 and want[4].max() < W * H * P
    check(nav().timed_field(dev(tys), None, W, H, sched(b), goal=tuple(dev(g) for g in goal),
                            agent=tuple(dev(a) for a in agent), clock=dev(clock)), want)


@pytest.mark.parametrize("W,H", SIZES)
def test_period_one_empty_schedule_is_mg_nav_field_bit_for_bit(W, H):
    N = 9
    rng = np.random.default_rng(W * 40 + H)
    ty = np.stack([nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[n % 3])[0] for n in range(N)])
    st = (rng.integers(0, 3, ty.shape) * (ty == 4)).astype(np.uint8)
    ax, ay = dev(rng.integers(-1, W + 1, N).astype(np.int32)), dev(rng.integers(0, H, N).astype(np.int32))
    a = nav().distance_field(dev(ty), dev(st), W, H, agent=(ax, ay))
    b = nav().timed_field(dev(ty), dev(st), W, H, torch.zeros((1, H), dtype=torch.int32, device=DEV), agent=(ax, ay),
                          clock=dev(rng.integers(-5, 100, N).astype(np.int32)))
    assert torch.equal(a[0].view(torch.int16), b[0].view(N, W * H).view(torch.int16))
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


# ------------------------------------------------------------------------------------------------ store discipline, NULLs
@pytest.mark.parametrize("W,H,P", [(17, 17, 6), (5, 9, 7), (1, 1, 2), (32, 32, 2)])
def test_field_bases_and_pitches(W, H, P):
    N = 3
    c = case(W, H, P, N, 0)
    ty, st, b = dev(c["ty"]), dev(c["st"]), sched(c["blocked"])
    for off in (0, 2):
        for pitch in (W * H, W * H + 1, W * H + 7):
            buf = torch.full((16 + off + 2 * N * P * pitch + 32,), 0xA5, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 16 == 0
            rows = buf[16 + off:16 + off + 2 * N * P * pitch].view(torch.uint16).view(N, P, pitch)
            out = rows[:, :, :W * H]
            assert out.data_ptr() % 16 == off
            got = nav().timed_field(ty, st, W, H, b, out=out)
            assert got[0] is out
            want = np.full(buf.numel(), 0xA5, np.uint8)
            w16 = want[16 + off:16 + off + 2 * N * P * pitch].view(np.uint16).reshape(N, P, pitch)
            w16[:, :, :W * H] = c["multi"][0]
            assert np.array_equal(host(buf), want), (off, pitch)


def test_null_dist_state_and_error():
    W, H, P, N = 17, 17, 6, 9
    c = case(W, H, P, N, 1)
    ty, b = dev(c["ty"]), sched(c["blocked"])
    agent, clock = tuple(dev(a) for a in c["agent"]), dev(c["clock"])
    want = tref.fields(c["ty"], None, W, H, c["blocked"], P, agent=c["agent"] + (c["clock"],))
    dist, adist, aact, err = nav().timed_field(ty, None, W, H, b, agent=agent, clock=clock, want_field=False, want_error=False)
    assert dist is None and err is None
    assert np.array_equal(host(adist), want[1]) and np.array_equal(host(aact), want[2])
    dist, adist, aact, err = nav().timed_field(ty, None, W, H, b, want_error=False)
    assert adist is None and aact is None and err is None and np.array_equal(host(dist), want[0])
    given = [torch.full((N,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    got = nav().timed_field(ty, None, W, H, b, agent=agent, clock=clock, want_field=False, agent_out=tuple(given[:2]),
                            error_out=given[2])
    assert got[0] is None and all(np.array_equal(host(t), w) for t, w in zip(given, want[1:4]))


def test_rejected_calls_launch_nothing():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    W, H, N, P = 5, 4, 3, 3
    ty = torch.ones((N, W * H), dtype=torch.uint8, device=DEV)
    xy = torch.zeros(N, dtype=torch.int32, device=DEV)
    blk = torch.zeros((N, P, H), dtype=torch.int32, device=DEV)
    dist = u16_full((N, P, W * H + 2))
    outs = [torch.full((N,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=DEV) for _ in range(3)]
    p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())     # noqa: E731
    good = dict(type=ty, state=None, n=N, W=W, H=H, pass_types=nav_ref.PASS_DEFAULT, flags=0, blk=blk, bs=P * H, P=P, gx=xy,
                gy=xy, gs=1, ax=xy, ay=xy, clk=xy, as_=1, dist=dist, pitch=W * H + 2, adist=outs[0], aact=outs[1], err=outs[2])

    def field(**kw):
        a = dict(good, **kw)
        return lib.mg_nav_timed_field(p(a["type"]), p(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"],
                                      p(a["blk"]), a["bs"], a["P"], p(a["gx"]), p(a["gy"]), a["gs"], p(a["ax"]), p(a["ay"]),
                                      p(a["clk"]), a["as_"], p(a["dist"]), a["pitch"], p(a["adist"]), p(a["aact"]),
                                      p(a["err"]), None)

    bad = [dict(n=0), dict(W=0), dict(H=0), dict(W=33), dict(H=33), dict(W=-1), dict(type=None), dict(pitch=W * H - 1),
           dict(pitch=1), dict(pitch=-1), dict(gx=None), dict(gy=None), dict(ax=None), dict(ay=None),
           dict(ax=None, ay=None), dict(ax=None, ay=None, aact=None, clk=None), dict(ax=None, ay=None, adist=None, clk=None),
           dict(gs=0), dict(as_=0), dict(as_=-1), dict(pass_types=0x10000), dict(flags=2), dict(dist=dist.data_ptr() + 1),
           # the timed ones: the period, the schedule, its stride, a clock without the agent arrays
           dict(P=0), dict(P=17), dict(P=-1), dict(blk=None), dict(blk=blk.data_ptr() + 2), dict(bs=P * H - 1), dict(bs=1),
           dict(bs=-1), dict(bs=-P * H), dict(ax=None, ay=None, adist=None, aact=None)]
    for kw in bad:
        assert field(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (host(dist) == 0xA5A5).all() and all((host(o) == 0xA5A5A5A5 - (1 << 32)).all() for o in outs)
    # and the good calls do launch: per-env and shared schedule, with and without the clock
    assert field() == 0 and field(bs=0) == 0 and field(clk=None) == 0 and field(ax=None, ay=None, adist=None, aact=None, clk=None) == 0
    torch.cuda.synchronize()
    manhattan = np.add.outer(np.arange(H), np.arange(W)).reshape(-1)                    # an empty room, source (0, 0)
    assert (host(dist)[:, :, :W * H] == manhattan).all() and (host(dist)[:, :, W * H:] == 0xA5A5).all()
    assert host(outs[0]).tolist() == [0] * N and host(outs[1]).tolist() == [6] * N and host(outs[2]).tolist() == [0] * N

    pos = torch.zeros((2, N, 2), dtype=torch.float32, device=DEV)
    age = torch.zeros((2, N), dtype=torch.int32, device=DEV)
    init = torch.zeros(2, dtype=torch.float32, device=DEV)
    mv = torch.full((2 * N,), 0xA5, dtype=torch.uint8, device=DEV)
    ad = u16_full((2, N))
    g2 = dict(dist=dist, pitch=W * H + 2, P=P, n=N, W=W, H=H, pos=pos, age=age, init=init, T=2, mv=mv, ad=ad)

    def moves(**kw):
        a = dict(g2, **kw)
        return lib.mg_nav_timed_moves(p(a["dist"]), a["pitch"], a["P"], a["n"], a["W"], a["H"], p(a["pos"]), p(a["age"]),
                                      p(a["init"]), a["T"], p(a["mv"]), p(a["ad"]), None)
    for kw in [dict(dist=None), dict(pos=None), dict(mv=None), dict(age=None), dict(init=None), dict(age=None, init=None),
               dict(n=0), dict(T=-1), dict(W=0), dict(H=33), dict(pitch=W * H - 1), dict(pitch=-3), dict(P=0), dict(P=17),
               dict(dist=dist.data_ptr() + 1), dict(ad=ad.data_ptr() + 1), dict(pos=pos.data_ptr() + 4),
               dict(age=age.data_ptr() + 2), dict(init=init.data_ptr() + 2), dict(n=1 << 20, T=1 << 20)]:
        assert moves(**kw) == -1, kw
    assert moves(T=0) == 0
    torch.cuda.synchronize()
    assert (host(mv) == 0xA5).all() and (host(ad) == 0xA5A5).all()
    assert moves() == 0 and moves(ad=None) == 0
    torch.cuda.synchronize()
    assert (host(mv) == tref.MOVE_STAY).all() and (host(ad) == 0).all()      # everyone stands on the source (0, 0)


# ------------------------------------------------------------------------------------------------ move sets of a rollout
@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("T", [0, 1, 5])
def test_timed_moves(T, N):
    W, H, P = 17, 17, 6
    c = case(W, H, P, N, 1)
    field = c["multi"][0]                                    # uint16[N, P, H*W]
    rng = np.random.default_rng(100 * T + N)
    pos = rng.uniform(-1, 18, (T, N, 2)).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, -0.0, W - 1, W, -1, -0.5, 0.999]
    for k, (a, b) in enumerate((a, b) for a in special for b in special):
        if T * N:
            pos.reshape(-1, 2)[(5 * k) % (T * N)] = (a, b)
    age = (rng.integers(0, 14, (1, N)) + np.arange(T)[:, None]).astype(np.int32)
    for n in range(0, N, 2):                                 # episode starts inside the rollout, and a large clock
        age[n % max(T, 1):, n] = np.arange(T - n % max(T, 1))
    if T * N > 4:
        age.reshape(-1)[3] = 2 ** 31 - 1
        age.reshape(-1)[4] = -2
    init = np.array([15.0, 3.0], np.float32)
    want_m, want_d = tref.moves(field, pos, age, init, W, H, visit_ref.cell_of)
    wide = dev(np.concatenate([field, np.full((N, P, 5), 0xA5A5, np.uint16)], axis=2))[:, :, :W * H]
    for off in (0, 1):                                       # moves off a 16-byte boundary
        buf = torch.full((16 + off + T * N + 32,), 0xA5, dtype=torch.uint8, device=DEV)
        mv = buf[16 + off:16 + off + T * N].view(T, N)
        ad = u16_full((T, N))
        got = nav().timed_moves(wide if off else dev(field), dev(pos), W, H, dev(age), dev(init), out=mv, dist_out=ad)
        assert got[0] is mv and got[1] is ad
        assert np.array_equal(host(mv), want_m) and np.array_equal(host(ad), want_d)
        assert (host(buf[:16 + off]) == 0xA5).all() and (host(buf[16 + off + T * N:]) == 0xA5).all()
    m2, none = nav().timed_moves(dev(field), dev(pos), W, H, dev(age), dev(init), dist_out=False)
    assert none is None and np.array_equal(host(m2), want_m)
    if T * N >= 15:
        assert (want_m == 0).any() and (want_m & 15).any() and (age <= 0).any()
        # the invariant: the lowest set bit is the field kernel's expert action for that cell and clock
        cells = np.array([[visit_ref.cell_of(*(init if age[t, n] <= 0 else pos[t, n]), W, H) for n in range(N)] for t in range(T)])
        for t in range(T):
            ok = cells[t] < W * H
            ax, ay = np.where(ok, cells[t] % W, -1).astype(np.int32), np.where(ok, cells[t] // W, 0).astype(np.int32)
            _, adist, aact, _ = nav().timed_field(dev(c["ty"]), dev(c["st"]), W, H, sched(c["blocked"]), agent=(dev(ax), dev(ay)),
                                                  clock=dev(age[t]), want_field=False)
            assert host(aact).tolist() == [tref.action_of(int(m)) for m in want_m[t]]
            assert np.array_equal(host(adist), want_d[t].astype(np.int32))


# ------------------------------------------------------------------------------------------------ engine, env, trainer
def _engine_want(eng, avoid_risk=False):
    ty, _, rec = eng.get_state()
    b = host(nav().twoarmy_schedule(avoid_risk, blocks=eng.variant == 6)).view(np.uint32)
    return tref.fields(ty, None, 17, 17, b, 6, STATIC, agent=(rec[:, 0], rec[:, 1], rec[:, 4]))


@pytest.mark.parametrize("avoid_risk", [False, True])
def test_engine_expert_crosses_the_gap(avoid_risk):
    """v6, three envs: ONE field at the reset, then tw_step with the action looked up in it for the agent's cell and
    step_move: the episode terminates after exactly the agent_dist of the reset, no step is rewarded -0.9 and, with
    avoid_risk, none -0.1."""
    from twoarmy_amd.engine import TwoarmyEngine
    N = 3
    eng = TwoarmyEngine(6, N, 17, seed=9981)
    eng.reset()
    want = _engine_want(eng, avoid_risk)
    dist, adist, aact, err = eng.timed_field(avoid_risk)
    check((dist, adist, aact, err), want)
    field, d0 = host(dist), int(host(adist)[0])
    assert not host(err).any() and (host(adist) == d0).all() and 24 <= d0 < 50
    out = eng.alloc_outputs()
    rewards = []
    for k in range(d0):
        rec = eng.get_state()[2]
        assert (rec[:, 4] == k).all()
        sets = [tref.move_set(field[n], 17, 17, int(rec[n, 1]) * 17 + int(rec[n, 0]), tref.phase_of(rec[n, 4], 6)) for n in range(N)]
        assert all(d == d0 - k for _, d in sets)
        act = np.array([tref.action_of(m) for m, _ in sets], np.int32)
        _, now_d, now_a, _ = eng.timed_field(avoid_risk, want_field=False)      # planning again mid-episode agrees
        assert host(now_d).tolist() == [d0 - k] * N and np.array_equal(host(now_a), act)
        eng.step(dev(act), out)
        r, term, trunc = host(out["reward"]), host(out["terminated"]), host(out["truncated"])
        rewards += r.tolist()
        assert not trunc.any() and (term != 0).all() == (k == d0 - 1) and (term != 0).any() == (k == d0 - 1), k
    rewards = np.array(rewards, np.float32)
    assert not np.isclose(rewards, -0.9).any() and np.isclose(rewards[-N:], 0.9).all() and np.isclose(rewards, 0.2).sum() == N
    if avoid_risk:
        assert not np.isclose(rewards, -0.1).any()
    eng.close()


def test_engine_v4_plans_on_the_planes_as_they_stand():
    from twoarmy_amd.engine import TwoarmyEngine
    eng = TwoarmyEngine(4, 16, 17, seed=9981)
    eng.reset()
    out = eng.alloc_outputs(T=24)
    eng.rollout(24, out, actions=eng.fill_actions(24))
    check(eng.timed_field(), _engine_want(eng))
    eng.close()


def test_vecenv_timed_goal_distance():
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    N = 8
    envs = [TwoarmyVecEnv("v6", N, seed=9981, goal_distance=g) for g in ("timed", True)]
    for e in envs:
        e.reset()
    g = torch.Generator().manual_seed(5)
    for step in range(12):
        a = torch.randint(0, 5, (N,), generator=g).to(DEV)
        res = [e.step(a) for e in envs]
        assert all(torch.equal(x, y) for x, y in zip(res[0][:4], res[1][:4])) and set(res[0][4]) == set(res[1][4])
        want = _engine_want(envs[0].engine)
        info = res[0][4]
        assert info["goal_distance"].dtype == torch.int32 and info["expert_action"].dtype == torch.int32
        assert np.array_equal(host(info["goal_distance"]), want[1]) and np.array_equal(host(info["expert_action"]), want[2])
    for e in envs:
        e.close()


def test_trainer_labels_with_the_timed_expert():
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    T, N = 16, 8
    torch.manual_seed(5)
    eng = TwoarmyEngine(6, N, 17, seed=9981)
    agent = PPO()
    agent.K_epochs = 1
    agent.to(eng.device).use_nhwc()
    tr = VecPPOTrainer(agent, eng, rollout_steps=T, minibatch=32)
    tr.enable_prior(0.25, timed=True)
    for u in range(2):
        tr.collect()
        moves = tr.label_expert()
        want = _engine_want(eng)
        assert np.array_equal(host(tr.timed_field), want[0]) and tr.nav_field is None
        pos, age = host(tr.pos[3:3 + T]), host(tr.age[:-1])
        want_m, want_d = tref.moves(want[0], pos, age, host(tr.init_pos), 17, 17, visit_ref.cell_of)
        assert np.array_equal(host(moves), want_m) and np.array_equal(host(tr.expert_dist).view(np.uint16), want_d)
        assert (want_m != 0).any()
        ps = tr.prior_stats()
        assert ps["labelled"] == int((want_m != 0).sum()) and 0 <= ps["agree"] <= 1
        tr.update()
        tr.carry_over()
    assert "loss/prior_loss_update" in tr.agent.writer.scalars
    eng.close()


def test_train_ppo_prior_timed_flag(capsys):
    from twoarmy_amd.soa import train_ppo
    args = ["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", "8", "--rollout_steps", "8", "--minibatch", "32",
            "--k_epochs", "1", "--updates", "1"]
    a = train_ppo.main(args + ["--expert_agreement"])
    b = train_ppo.main(args + ["--expert_agreement", "--prior_timed"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]
    assert len(lines) == 2 and all(" expert agree " in ln for ln in lines)
    assert not a.prior["timed"] and a.timed_field is None and b.prior["timed"] and b.timed_field is not None
    with pytest.raises(SystemExit):
        train_ppo.main(args + ["--prior_timed"])
