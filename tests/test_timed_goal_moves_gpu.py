"""mg_nav_timed_goal_moves on the device: the timed move sets of records that each name their own goal, exact integers
against timed_goal_moves_ref.py (a queue BFS over (cell, phase) per record's env and goal), and against the kernels it must
agree with (timed field + timed moves; the static goal moves at period 1); the engine, the trainer and the command line
around it."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import goal_moves_ref
import nav_ref
import prior_ref
import timed_goal_moves_ref as tgref
import timed_nav_ref as tref
from nav_util import dev, host, random_records, runs_to_records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = tref.UNREACHABLE
STAY = tref.MOVE_STAY
CHUNK = 1024                                                          # records per workgroup (NAV_GOAL_ELEMS)
BALL = 1 << 6
# Floods at a time, from the LDS arithmetic of the kernel: an image is P * ((W*H + 7) & ~7) * 2 bytes, the staging of a
# workgroup takes under 15 KiB, and the most images (8, 4, 2, 1) that fit 64 KiB with it flood together.
#   7 x 31, P = 16: 7168 B -> 8 images are 56 KiB: 4.     17 x 17, P = 16: 9472 B: 4.     32 x 32, P = 6: 12 KiB: 4.
#   32 x 16, P = 16 and 32 x 32, P = 8: 16 KiB: 2.        32 x 32, P = 16: 32 KiB: 1.     Everything else below 6 KiB: 8.
FLOODS = {(7, 31, 16): 4, (17, 17, 16): 4, (32, 32, 6): 4, (32, 16, 16): 2, (32, 32, 8): 2, (32, 32, 16): 1}
SIDES = [(1, 1), (1, 5), (5, 1), (7, 31), (17, 17), (32, 32)]
PERIODS = [1, 2, 6, 16]


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


_CASES = {}


def case(W, H, N, P):
    """N random worlds of one size, a schedule per env (every bit of all 32 columns drawn: those at or above W are to be
    ignored), a pool of three goal cells per env and one memo of reference fields per schedule layout.  Made once,
    read-only."""
    key = (W, H, N, P)
    if key not in _CASES:
        rng = np.random.default_rng(13 * W + 41 * H + 1000 * N + 7 * P)
        ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
        for n in range(N):
            ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.4)[n % 3])
        sched = np.stack([tref.random_schedule(rng, P, H, 0.2) for _ in range(N)])
        pool = np.stack([rng.permutation(W * H)[np.arange(3) % (W * H)] for _ in range(N)])
        for a in (ty, st, sched, pool):
            a.setflags(write=False)
        _CASES[key] = dict(ty=ty, st=st, sched=sched, pool=pool, memo={True: {}, False: {}}, W=W, H=H, N=N, P=P)
    return _CASES[key]


def positions(rng, T, N, W, H):
    """Random cells at their corners, centres and far edges, and a sprinkle of positions that are no cell."""
    c = rng.integers(0, W * H, T * N)
    pos = np.stack([c // W + rng.choice([0.0, 0.5, 0.999], T * N), c % W + rng.choice([0.0, 0.5, 0.999], T * N)], 1)
    pos = pos.astype(np.float32)
    special = [(np.nan, 0.5), (0.5, np.inf), (-np.inf, 0.0), (H, 0.0), (0.0, W), (-0.5, 0.5)]
    if T * N > 16:
        for i, s in enumerate(special):
            pos[(i * 5 + 2) % (T * N)] = s
    return pos.reshape(T, N, 2)


def raw_call(lib, a):
    v = lambda x: None if x is None else C.c_void_p(x)                                     # noqa: E731
    return lib.mg_nav_timed_goal_moves(v(a["type"]), v(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"],
                                       v(a["blocked"]), a["bstride"], a["P"], v(a["t"]), v(a["rn"]), v(a["goal"]), a["R"],
                                       v(a["pos"]), v(a["age"]), v(a["init"]), a["T"], v(a["moves"]), v(a["ad"]), None)


def run(c, rec, pos, age, init, shared=False, pad=0, off_m=0, off_d=0, want_dist=True, pass_types=nav_ref.PASS_DEFAULT,
        with_state=True):
    """The kernel with `moves` at byte offset off_m and `acting_dist` at byte offset off_d inside 0xA5-filled buffers;
    checks that nothing but the outputs changed.  shared: env 0's schedule for all envs; pad > 0: the per-env schedules
    `pad` words apart more than P*H (through the C ABI; the front end takes dense tensors).  -> (moves, acting_dist)."""
    W, H, N, P = c["W"], c["H"], c["N"], c["P"]
    t, n, goal = rec
    R = len(t)
    mbuf = torch.full((16 + off_m + R + 37,), 0xA5, dtype=torch.uint8, device=DEV)
    dbuf = torch.full((16 + off_d + 2 * R + 38,), 0xA5, dtype=torch.uint8, device=DEV)
    mv = mbuf[16 + off_m:16 + off_m + R]
    dv = dbuf[16 + off_d:16 + off_d + 2 * R].view(torch.uint16)
    assert mbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0 and off_d % 2 == 0
    ty, st = dev(c["ty"]), dev(c["st"]) if with_state else None
    dpos, dage, dinit = dev(pos), dev(age), dev(init)
    if pad:
        assert not shared
        sb = torch.full((N, P * H + pad), -1, dtype=torch.int32, device=DEV)              # the padding: every cell blocked
        sb[:, :P * H] = dev(c["sched"].view(np.int32).reshape(N, P * H))
        dt, dn, dg = dev(t), dev(n), dev(goal)
        from twoarmy_amd import _lib
        rc = raw_call(_lib.lib(), dict(type=ty.data_ptr(), state=None if st is None else st.data_ptr(), n=N, W=W, H=H,
                                       pass_types=pass_types, flags=0, blocked=sb.data_ptr(), bstride=P * H + pad, P=P,
                                       t=dt.data_ptr(), rn=dn.data_ptr(), goal=dg.data_ptr(), R=R, pos=dpos.data_ptr(),
                                       age=dage.data_ptr(), init=dinit.data_ptr(), T=pos.shape[0], moves=mv.data_ptr(),
                                       ad=dv.data_ptr() if want_dist else None))
        assert rc == 0
        torch.cuda.synchronize()
    else:
        blocked = dev(c["sched"][0] if shared else c["sched"]).view(torch.int32)
        got = nav().timed_goal_moves(ty, dev(t), dev(n), dev(goal), dpos, W, H, blocked, dage, dinit,
                                     pass_types=pass_types, state=st, out=mv, dist_out=dv if want_dist else False)
        assert got[0] is mv and (got[1] is dv if want_dist else got[1] is None)
    hm, hd = host(mbuf), host(dbuf)
    assert (hm[:16 + off_m] == 0xA5).all() and (hm[16 + off_m + R:] == 0xA5).all()
    assert (hd[:16 + off_d] == 0xA5).all() and (hd[16 + off_d + 2 * R:] == 0xA5).all()
    if not want_dist:
        assert (hd == 0xA5).all()
    return host(mv), host(dv) if want_dist else None


def ref(c, rec, pos, age, init, shared=False, pass_types=nav_ref.PASS_DEFAULT, with_state=True):
    memo = c["memo"][shared].setdefault((pass_types, with_state), {})
    return tgref.timed_goal_moves(c["ty"], c["st"] if with_state else None, c["W"], c["H"],
                                  c["sched"][0] if shared else c["sched"], c["P"], rec[0], rec[1], rec[2], pos, age, init,
                                  pass_types, memo=memo)


def check(c, rec, pos, age, init, shared=False, pass_types=nav_ref.PASS_DEFAULT, with_state=True, **kw):
    want = ref(c, rec, pos, age, init, shared, pass_types, with_state)
    m, d = run(c, rec, pos, age, init, shared=shared, pass_types=pass_types, with_state=with_state, **kw)
    assert np.array_equal(m, want[0]), np.flatnonzero(m != want[0])[:8]
    assert d is None or np.array_equal(d, want[1]), np.flatnonzero(d != want[1])[:8]
    return want


def floods(W, H, P):
    return FLOODS.get((W, H, P), 8)


# ------------------------------------------------------------------------------------------------ sizes, periods, levels
@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("W,H", SIDES + [(32, 16)])
def test_records_equal_the_reference(W, H, P):
    assert nav().timed_goal_floods(W, H, P) == floods(W, H, P)
    N = 3
    c = case(W, H, N, P)
    rng = np.random.default_rng(W * 100 + H + P)
    init = np.array([H - 0.5, 0.25], np.float32)
    seen_m, seen_d = set(), set()
    for i, (T, R) in enumerate([(1, 1), (40, CHUNK - 1), (40, CHUNK + 1)]):
        pos = positions(rng, T, N, W, H)
        age = rng.integers(-1, 3 * P + 2, (T, N)).astype(np.int32)              # <= 0: init_pos at phase 0; beyond P: wraps
        rec = random_records(rng, c, R, T)
        want = check(c, rec, pos, age, init, shared=i == 1, pad=5 if i == 2 else 0, off_m=(0, 1, 3)[i], off_d=(0, 2, 6)[i],
                     pass_types=(nav_ref.PASS_DEFAULT, nav_ref.PASS_DEFAULT | BALL)[i % 2], with_state=i != 1)
        seen_m |= set(want[0].tolist())
        seen_d |= set(want[1].tolist())
    if W * H >= 200:                                                  # the cases are worth their name
        assert {bin(v & 15).count("1") for v in seen_m} >= {0, 1, 2}
        assert U in seen_d and len(seen_d) > 3


def test_two_floods_at_a_time_at_the_largest_world():
    """32 x 32 with P = 8: the level between the ones the period list reaches there."""
    assert nav().timed_goal_floods(32, 32, 8) == 2 and floods(32, 32, 8) == 2
    c = case(32, 32, 3, 8)
    rng = np.random.default_rng(328)
    T = 40
    pos = positions(rng, T, 3, 32, 32)
    age = rng.integers(-1, 30, (T, 3)).astype(np.int32)
    check(c, random_records(rng, c, CHUNK + 1, T), pos, age, np.array([0.5, 0.5], np.float32))


@pytest.mark.parametrize("W,H,P", [(17, 17, 6), (32, 32, 16)])
def test_record_counts_layouts_and_order(W, H, P):
    c = case(W, H, 3, P)
    rng = np.random.default_rng(99 + P)
    T = 64
    pos = positions(rng, T, 3, W, H)
    age = rng.integers(-1, 4 * P, (T, 3)).astype(np.int32)
    init = np.array([H - 1.5, 1.5], np.float32)
    for R in (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        check(c, random_records(rng, c, R, T), pos, age, init)
    g = lambda e, k: int(c["pool"][e][k])                                                  # noqa: E731
    # a run that straddles a workgroup boundary, between two short ones
    rec = runs_to_records(rng, c, [(0, g(0, 0), CHUNK - 20), (1, g(1, 0), 40), (2, g(2, 0), 30)], T)
    check(c, rec, pos, age, init, off_m=15, off_d=14)
    # ppo_her_relabel's order, then the same records shuffled: almost every record its own run, equal record for record
    rec = random_records(rng, c, 2 * CHUNK + 1, T)
    m, d = run(c, rec, pos, age, init)
    perm = rng.permutation(len(rec[0]))
    shuffled = tuple(a[perm] for a in rec)
    assert ((shuffled[1][1:] != shuffled[1][:-1]) | (shuffled[2][1:] != shuffled[2][:-1]).any(-1)).mean() > 0.6
    pm, pd = run(c, shuffled, pos, age, init)
    assert np.array_equal(pm, m[perm]) and np.array_equal(pd, d[perm])
    want = ref(c, rec, pos, age, init)
    assert np.array_equal(m, want[0]) and np.array_equal(d, want[1])


def test_no_records_launch_nothing():
    c = case(5, 1, 3, 2)
    e32, ef = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty((0, 2), dtype=torch.float32, device=DEV)
    pos = torch.zeros((2, 3, 2), dtype=torch.float32, device=DEV)
    age = torch.ones((2, 3), dtype=torch.int32, device=DEV)
    m0, d0 = nav().timed_goal_moves(dev(c["ty"]), e32, e32, ef, pos, 5, 1, dev(c["sched"]).view(torch.int32), age,
                                    torch.zeros(2, device=DEV))
    assert m0.shape == (0,) and m0.dtype == torch.uint8 and d0.shape == (0,)


# ------------------------------------------------------------------------------------------------ edges of the semantics
def _corridor():
    """A 5 x 1 corridor, P = 2: cell 2 is blocked at phase 1, cell 3 at both phases of env 1 only."""
    W, H, N, P = 5, 1, 2, 2
    sched = np.zeros((N, P, H), np.uint32)
    sched[:, 1, 0] = 1 << 2 | 0xFFFFFFE0                     # bits at and above the width: ignored
    sched[1, :, 0] |= 1 << 3
    return dict(ty=np.ones((N, W * H), np.uint8), st=np.zeros((N, W * H), np.uint8), sched=sched, W=W, H=H, N=N, P=P,
                memo={True: {}, False: {}})


def test_edges_of_the_semantics():
    c = _corridor()
    W, N, T = 5, 2, 4
    pos = np.zeros((T, N, 2), np.float32)
    pos[:, :, 1] = 1.5                                        # everybody acts on cell 1 ...
    pos[3, 0] = (np.nan, 1.5)                                 # ... but one position that is no cell
    age = np.array([[2, 2], [1, 1], [0, -3], [4, 13]], np.int32)      # phases 0, 1, 0 (init_pos), 0 / 1
    init = np.array([0.5, 0.5], np.float32)                   # cell 0
    inf = np.inf
    # (t, n, goal y, goal x) -> (moves, dist)
    cases = [
        ((0, 0, 0.5, 4.5), (STAY, 4)),        # (1, phase 0): cell 2 is blocked at phase 1 -- waiting is the ONLY optimal move
        ((1, 0, 0.5, 4.5), (0x2, 3)),         # (1, phase 1): right, into phase 0
        ((2, 0, 0.5, 4.5), (0x2, 4)),         # age 0: init_pos = cell 0 at phase 0: right to (1, phase 1)
        ((2, 1, 0.5, 0.5), (STAY, 0)),        # age < 0 alike: on its goal
        ((0, 0, 0.5, 2.5), (STAY, 2)),        # a goal blocked in some phases: wait, then enter at phase 0
        ((1, 0, 0.5, 2.5), (0x2, 1)),
        ((0, 0, 0.5, 1.5), (STAY, 0)),        # on the goal
        ((0, 1, 0.5, 3.5), (0, U)),           # a goal blocked in all phases
        ((0, 1, 0.5, 4.5), (0, U)),           # ... and what lies behind it
        ((0, 1, 0.5, 0.5), (0x1, 1)),
        ((3, 1, 0.5, 0.0), (0x1, 1)),         # age 13: phase 1, and the other way at age 4: phase 0
        ((3, 0, 0.5, 0.5), (0, U)),           # the acting position is no cell
        ((-1, 0, 0.5, 0.5), (0, U)),          # rec_t outside [0, T)
        ((T, 0, 0.5, 0.5), (0, U)),
        ((0, -1, 0.5, 0.5), (0, U)),          # rec_n outside [0, N)
        ((0, N, 0.5, 0.5), (0, U)),
        ((0x7FFFFFFF, 0x7FFFFFFF, 0.5, 0.5), (0, U)),
        ((-0x80000000, -0x80000000, 0.5, 0.5), (0, U)),
        ((0, 0, np.nan, 0.5), (0, U)),        # goals that are no cell
        ((0, 0, 0.5, inf), (0, U)),
        ((0, 0, -inf, 0.5), (0, U)),
        ((0, 0, 1.0, 0.5), (0, U)),
        ((0, 0, 0.5, 5.0), (0, U)),
        ((0, 0, 0.5, 0.5), (0x1, 1)),         # a valid record after them: unaffected
    ]
    t = np.array([k[0][0] for k in cases], np.int64).astype(np.int32)
    n = np.array([k[0][1] for k in cases], np.int64).astype(np.int32)
    goal = np.array([k[0][2:] for k in cases], np.float32)
    want_m = np.array([k[1][0] for k in cases], np.uint8)
    want_d = np.array([k[1][1] for k in cases], np.uint16)
    r = ref(c, (t, n, goal), pos, age, init)
    assert np.array_equal(r[0], want_m) and np.array_equal(r[1], want_d)     # the reference agrees with the table
    m, d = run(c, (t, n, goal), pos, age, init)
    assert np.array_equal(m, want_m) and np.array_equal(d, want_d)
    m, d = run(c, (t, n, goal), pos, age, init, pad=3, off_m=3, off_d=6)
    assert np.array_equal(m, want_m) and np.array_equal(d, want_d)


def test_invalid_records_among_valid_ones_and_a_goal_on_a_wall():
    c = case(17, 17, 3, 6)
    rng = np.random.default_rng(17)
    T, R = 40, CHUNK + 200
    pos = positions(rng, T, 3, 17, 17)
    pos[7, 1] = (np.nan, 3.0)                                 # an acting position that is no cell
    age = rng.integers(-1, 20, (T, 3)).astype(np.int32)
    age[7, 1] = 3
    init = np.array([15.5, 1.5], np.float32)
    t, n, goal = (a.copy() for a in random_records(rng, c, R, T))
    wall = int(np.flatnonzero(c["ty"][0] == 2)[0])
    bad = {5: ("t", -1), 6: ("t", T), 300: ("n", -1), 301: ("n", 3), 600: ("g", (np.nan, 1.0)), 601: ("g", (1.0, np.inf)),
           602: ("g", (-np.inf, 1.0)), 603: ("g", (17.0, 1.0)), 1023: ("g", (1.0, -0.5)), 1024: ("t", 1 << 30),
           1025: ("wall", wall), 1100: ("nan_pos", None)}
    for b, (what, v) in bad.items():
        if what == "t":
            t[b] = v
        elif what == "n":
            n[b] = v
        elif what == "g":
            goal[b] = v
        elif what == "wall":
            n[b], goal[b] = 0, (wall // 17 + 0.5, wall % 17 + 0.5)
        else:
            t[b], n[b] = 7, 1
    want = check(c, (t, n, goal), pos, age, init, off_m=1, off_d=2)
    idx = np.array(sorted(bad))
    assert (want[0][idx] == 0).all() and (want[1][idx] == U).all()
    others = np.setdiff1d(np.arange(R), idx)
    assert (want[0][others] != 0).any()


# ------------------------------------------------------------------------------------------------ writes, NULL output
@pytest.mark.parametrize("R", [5, CHUNK + 1])
def test_write_bounds_at_the_named_alignments(R):
    c = case(17, 17, 3, 6)
    rng = np.random.default_rng(R)
    T = 40
    pos = positions(rng, T, 3, 17, 17)
    age = rng.integers(-1, 20, (T, 3)).astype(np.int32)
    init = np.array([15.5, 1.5], np.float32)
    rec = random_records(rng, c, R, T)
    want = ref(c, rec, pos, age, init)
    for off_m, off_d in zip((0, 1, 3, 15), (0, 2, 6, 14)):
        m, d = run(c, rec, pos, age, init, off_m=off_m, off_d=off_d)
        assert np.array_equal(m, want[0]) and np.array_equal(d, want[1]), (off_m, off_d)
    for off_m in (0, 3):
        m, d = run(c, rec, pos, age, init, off_m=off_m, want_dist=False)                   # acting_dist NULL
        assert np.array_equal(m, want[0]) and d is None


# ------------------------------------------------------------------------------------------------ kernel to kernel
@pytest.mark.parametrize("W,H,P", [(7, 31, 2), (17, 17, 6), (32, 32, 16)])
def test_one_goal_per_env_equals_timed_field_then_timed_moves(W, H, P):
    """Invariant (a) on the device."""
    N, T = 9, 12
    rng = np.random.default_rng(W + H + P)
    ty = np.stack([nav_ref.random_world(rng, W, H, 0.15)[0] for _ in range(N)])
    sched = np.stack([tref.random_schedule(rng, P, H, 0.2) for _ in range(N)])
    dty, dsched = dev(ty), dev(sched).view(torch.int32)
    gc = rng.integers(0, W * H, N)
    gx, gy = (gc % W).astype(np.int32), (gc // W).astype(np.int32)
    pos = positions(rng, T, N, W, H)
    age = rng.integers(-1, 3 * P, (T, N)).astype(np.int32)
    init = np.array([0.5, W - 0.5], np.float32)
    field = nav().timed_field(dty, None, W, H, dsched, goal=(dev(gx), dev(gy)))[0]
    fm, fd = nav().timed_moves(field, dev(pos), W, H, dev(age), dev(init))
    order = rng.permutation(T * N)
    order = order[np.argsort(order % N, kind="stable")]              # runs of one env, steps in any order
    t, n = (order // N).astype(np.int32), (order % N).astype(np.int32)
    goal = np.stack([gy[n] + 0.5, gx[n] + 0.25], 1).astype(np.float32)
    m, d = nav().timed_goal_moves(dty, dev(t), dev(n), dev(goal), dev(pos), W, H, dsched, dev(age), dev(init))
    assert np.array_equal(host(m), host(fm)[t, n]) and np.array_equal(host(d).view(np.uint16), host(fd).view(np.uint16)[t, n])
    assert (host(d).view(np.uint16) != U).any() and (host(m) != 0).any()


@pytest.mark.parametrize("W,H", [(9, 4), (17, 17), (32, 32)])
def test_period_one_with_an_empty_schedule_equals_goal_moves(W, H):
    """Invariant (b) on the device."""
    N, T, R = 5, 12, CHUNK + 77
    rng = np.random.default_rng(W * H)
    worlds = [nav_ref.random_world(rng, W, H, 0.2) for _ in range(N)]
    ty, st = dev(np.stack([w[0] for w in worlds])), dev(np.stack([w[1] for w in worlds]))
    pos = dev(positions(rng, T, N, W, H))
    age, init = dev(rng.integers(-1, 4, (T, N)).astype(np.int32)), dev(np.array([0.5, 0.5], np.float32))
    n = np.sort(rng.integers(-1, N + 1, R)).astype(np.int32)
    t = rng.integers(-1, T + 1, R).astype(np.int32)
    gc = rng.integers(0, W * H, R) // 7 * 7 % (W * H)
    goal = np.stack([gc // W + 0.5, gc % W + 0.5], 1).astype(np.float32)
    zero = torch.zeros((1, H), dtype=torch.int32, device=DEV)
    for pass_types in (nav_ref.PASS_DEFAULT, nav_ref.PASS_DEFAULT | BALL):
        sm, sd = nav().goal_moves(ty, dev(t), dev(n), dev(goal), pos, W, H, pass_types, age=age, init_pos=init, state=st)
        m, d = nav().timed_goal_moves(ty, dev(t), dev(n), dev(goal), pos, W, H, zero, age, init, pass_types, state=st)
        assert torch.equal(m, sm) and torch.equal(d.view(torch.int16), sd.view(torch.int16))
    assert (host(sm) != 0).any() and (host(sm) == 0).any()


def test_the_longest_flood():
    """The serpentine at 32 x 32 with P = 16 and a single record at the far end of the corridor: one flood at a time, the
    64 KiB launch, about W*H/2 rounds until nothing is new."""
    W = H = 32
    ty, _ = nav_ref.serpentine(W, H)
    c = dict(ty=ty[None], st=np.zeros((1, W * H), np.uint8), sched=np.zeros((1, 16, H), np.uint32), W=W, H=H, N=1, P=16,
             memo={True: {}, False: {}})
    far = W * (H - 2) + (0 if ty[W * (H - 2)] != 2 else W - 1)
    pos = np.array([[[far // W + 0.5, far % W + 0.5]]], np.float32)
    rec = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.array([[0.5, 0.5]], np.float32))
    want = check(c, rec, pos, np.array([[5]], np.int32), np.zeros(2, np.float32))
    assert 255 < want[1][0] < U and want[0][0] in (1, 2, 4, 8)


# ------------------------------------------------------------------------------------------------ TW_E_ARG
def test_bad_arguments_launch_nothing():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    W, H, N, T, R, P = 5, 4, 3, 2, 6, 3
    ty = torch.ones((N, W * H), dtype=torch.uint8, device=DEV)
    st = torch.zeros((N, W * H), dtype=torch.uint8, device=DEV)
    blocked = torch.zeros((N, P * H + 2), dtype=torch.int32, device=DEV)
    t = torch.zeros(R + 1, dtype=torch.int32, device=DEV)
    rn = torch.zeros(R + 1, dtype=torch.int32, device=DEV)
    goal = torch.zeros((R + 1, 2), dtype=torch.float32, device=DEV)
    pos = torch.zeros((T + 1, N, 2), dtype=torch.float32, device=DEV)
    age = torch.ones((T + 1, N), dtype=torch.int32, device=DEV)
    init = torch.zeros(4, dtype=torch.float32, device=DEV)
    moves = torch.full((R + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    ad = torch.full((2 * R + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    good = dict(type=ty.data_ptr(), state=st.data_ptr(), n=N, W=W, H=H, pass_types=nav_ref.PASS_DEFAULT, flags=0,
                blocked=blocked.data_ptr(), bstride=P * H + 2, P=P, t=t.data_ptr(), rn=rn.data_ptr(), goal=goal.data_ptr(),
                R=R, pos=pos.data_ptr(), age=age.data_ptr(), init=init.data_ptr(), T=T, moves=moves.data_ptr(),
                ad=ad.data_ptr())
    bad = [dict(type=None), dict(t=None), dict(rn=None), dict(goal=None), dict(pos=None), dict(moves=None),
           dict(n=0), dict(n=-1), dict(W=0), dict(H=0), dict(W=33), dict(H=33), dict(W=-1),
           dict(pass_types=0x10000), dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(pos=good["pos"] + 4), dict(t=good["t"] + 2), dict(rn=good["rn"] + 1), dict(goal=good["goal"] + 2),
           dict(age=good["age"] + 2), dict(init=good["init"] + 1), dict(ad=good["ad"] + 1),
           dict(T=-1), dict(R=-1), dict(R=1 << 40), dict(R=1 << 62),
           dict(age=None), dict(init=None), dict(age=None, init=None),                    # both required here
           dict(P=0), dict(P=17), dict(P=-1), dict(blocked=None), dict(blocked=good["blocked"] + 2),
           dict(bstride=-1), dict(bstride=P * H - 1), dict(bstride=1)]
    for kw in bad:
        assert raw_call(lib, dict(good, **kw)) == -1, kw
    assert raw_call(lib, dict(good, R=0)) == 0                                           # no records: ok, no launch
    assert lib.mg_nav_timed_goal_floods(0, 5, 1) == -1 and lib.mg_nav_timed_goal_floods(5, 33, 1) == -1
    assert lib.mg_nav_timed_goal_floods(5, 5, 0) == -1 and lib.mg_nav_timed_goal_floods(5, 5, 17) == -1
    torch.cuda.synchronize()
    assert (host(moves) == 0xA5).all() and (host(ad) == 0xA5).all()
    # and the good calls launch: every record acts on cell 0 with goal cell 0
    assert raw_call(lib, good) == 0
    assert raw_call(lib, dict(good, bstride=0, ad=None, state=None, flags=1, moves=good["moves"] + 1,
                              goal=good["goal"] + 4, T=0)) == 0                           # T = 0: no record has a step
    torch.cuda.synchronize()
    assert host(moves).tolist() == [STAY] + [0] * R + [0xA5] * 3
    assert (host(ad)[:2 * R] == 0).all() and (host(ad)[2 * R:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ engine, trainer, command line
N_ENVS, T_ROLL, MAX_STEPS, MB = 8, 16, 12, 64
STATIC = nav_ref.PASS_DEFAULT | BALL


def _sched6():
    return nav().twoarmy_schedule(blocks=True).numpy().astype(np.int64)


def test_engine_timed_goal_moves_reads_the_engines_planes():
    from twoarmy_amd.engine import TwoarmyEngine
    eng = TwoarmyEngine(6, N_ENVS, 17, seed=9981)
    eng.reset()
    rng = np.random.default_rng(4)
    T = 12
    pos = positions(rng, T, N_ENVS, 17, 17)
    age = rng.integers(-1, 15, (T, N_ENVS)).astype(np.int32)
    init = np.array([15.5, 3.5], np.float32)
    ty = eng.get_state()[0]
    gap = [8 * 17 + 6, 8 * 17 + 8, 6 * 17 + 8]                 # under the balls in three phases, in all six, beyond the gap
    c = dict(W=17, N=N_ENVS, pool=np.stack([gap] * N_ENVS))
    t, n, goal = random_records(rng, c, 600, T)
    her = dict(t=dev(t), n=dev(n), goal=dev(goal))
    m, d = eng.timed_goal_moves(her, dev(pos), dev(age), dev(init))
    want = tgref.timed_goal_moves(ty, None, 17, 17, _sched6(), 6, t, n, goal, pos, age, init, STATIC)
    assert np.array_equal(host(m), want[0]) and np.array_equal(host(d).view(np.uint16), want[1])
    g8 = (goal.astype(np.int64) == (8, 8)).all(1)
    assert g8.any() and (want[0][g8] == 0).all() and (want[0][~g8] != 0).any()
    assert ((want[0] & STAY != 0) & (want[1] != 0)).any()        # somebody waits for the balls
    static = eng.goal_moves(her, dev(pos), dev(age), dev(init), pass_types=STATIC)
    assert not np.array_equal(host(static[0]), want[0])          # and the static labels are others
    eng.close()


def _trainer():
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(5)
    eng = TwoarmyEngine(6, N_ENVS, 17, seed=9981, max_steps=MAX_STEPS)
    agent = PPO()
    agent.K_epochs = 1
    agent.to(eng.device).use_nhwc()
    return VecPPOTrainer(agent, eng, rollout_steps=T_ROLL, minibatch=MB, value_chunk=MB), eng


def test_trainer_labels_hindsight_records_with_the_timed_search():
    timed, e1 = _trainer()
    plain, e0 = _trainer()
    with pytest.raises(ValueError, match="hindsight=True"):
        timed.enable_prior(0.5, hindsight_timed=True)
    timed.enable_prior(0.5, hindsight=True, hindsight_timed=True)
    plain.enable_prior(0.5, hindsight=True, timed=True)          # the argument absent: static hindsight labels, as before
    assert timed.prior["hindsight_timed"] is True and plain.prior["hindsight_timed"] is False
    for tr, eng in ((timed, e1), (plain, e0)):
        tr.collect()
        tr.relabel()
        tr.label_expert()
        h = tr.her
        R = int(h["t"].numel())
        assert R > 0 and tr.her_moves.shape == (R,) and tr.her_dist.shape == (R,)
        ty = host(eng.plane_views()[0])
        t, n, goal = host(h["t"]), host(h["n"]), host(h["goal"])
        pos, age, init = host(tr.pos[3:3 + T_ROLL]), host(tr.age[:-1]), host(tr.init_pos)
        if tr is timed:
            want_m, want_d = tgref.timed_goal_moves(ty, None, 17, 17, _sched6(), 6, t, n, goal, pos, age, init, STATIC)
        else:
            want_m, want_d = goal_moves_ref.goal_moves(ty, None, 17, 17, t, n, goal, pos, age, init, pass_types=STATIC)
            sm, sd = eng.goal_moves(h, tr.pos[3:3 + T_ROLL], tr.age[:-1], tr.init_pos, pass_types=STATIC)
            assert torch.equal(tr.her_moves, sm) and torch.equal(tr.her_dist.view(torch.int16), sd.view(torch.int16))
        m, d = host(tr.her_moves), host(tr.her_dist).view(np.uint16)
        assert np.array_equal(m, want_m) and np.array_equal(d, want_d)
        assert (m != 0).any()
        # the statistics against numpy
        ps = tr.prior_stats()
        act = host(tr.action)[t, n]
        pm = prior_ref.to_policy_mask(want_m, 5).astype(np.int64)
        lab = pm != 0
        hit = ((pm >> act) & 1) != 0
        assert ps["her_labelled"] == int(lab.sum()) and ps["her_agree"] == (hit & lab).sum() / lab.sum()
        total = T_ROLL * N_ENVS + R
        perm = torch.randperm(total, generator=torch.Generator().manual_seed(1))[:total // MB * MB]
        tr.update(permutations=[perm])
        assert tr.her is None
    e0.close(); e1.close()


def test_train_ppo_prints_her_agree_with_the_timed_hindsight_labels(capsys):
    from twoarmy_amd.soa import train_ppo
    args = ["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", str(N_ENVS), "--rollout_steps", str(T_ROLL), "--minibatch",
            str(MB), "--k_epochs", "1", "--updates", "1", "--max_steps", str(MAX_STEPS), "--expert_agreement"]
    with pytest.raises(SystemExit):
        train_ppo.main(args + ["--prior_hindsight_timed"])                               # needs --prior_hindsight
    capsys.readouterr()
    tr = train_ppo.main(args + ["--prior_hindsight", "--prior_hindsight_timed"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]
    assert len(lines) == 1 and re.search(r" her agree (\d\.\d{3}|-)$", lines[0]), lines
    assert tr.prior["hindsight"] is True and tr.prior["hindsight_timed"] is True and tr.prior["timed"] is False
