"""mg_nav_ahead and mg_nav_goal_ahead on the device, bit for bit against ahead_ref.py (a frontier loop per element, written
from the header).  The rollout kernel is defined ON a field, so its fields come from the field kernels (pinned by their own
tests) and the reference reads the same distances; the goal kernel floods itself and is checked against nav_ref's BFS."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import ahead_ref
import nav_ref
import timed_nav_ref
from nav_util import Boxed, dev, host, random_records, runs_to_records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = nav_ref.UNREACHABLE
SHARE = 2048                                                          # elements per workgroup (NAV_MOVES_ELEMS)
CHUNK = 1024                                                          # records per workgroup (NAV_GOAL_ELEMS)
BALL = 1 << 6


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def u64(t):
    return host(t).view(np.uint64)


_WORLDS = {}


def world(name, N):
    """(type uint8[N, H*W], W, H, goal (x[N], y[N]) or None, pass_types), made once and read-only."""
    key = (name, N)
    if key in _WORLDS:
        return _WORLDS[key]
    rng = np.random.default_rng(len(name) * 7 + N)
    goal, pass_types = None, nav_ref.PASS_DEFAULT
    if name == "1x1":
        W = H = 1
        ty = np.ones((N, 1), np.uint8)
        goal = (np.zeros(N, np.int32), np.zeros(N, np.int32))
    elif name == "5x4":
        W, H = 5, 4
        one = np.ones((H, W), np.uint8)
        one[1, 2] = 2
        ty = np.stack([one.reshape(-1)] * N)
        g = rng.choice(np.flatnonzero(one.reshape(-1) != 2), N)
        g[0] = 1 * W + 4
        goal = ((g % W).astype(np.int32), (g // W).astype(np.int32))
    elif name == "v6":
        from twoarmy_amd.engine import TwoarmyEngine
        W = H = 17
        eng = TwoarmyEngine(6, N, 17, seed=9981)
        eng.reset()
        ty = np.array(eng.get_state()[0])
        eng.close()
        pass_types |= BALL                                             # goal None: the cells of type 8
    else:
        W = H = 32
        s, _ = nav_ref.serpentine(W, H)
        ty = np.stack([s if n % 2 == 0 else np.ones(W * H, np.uint8) for n in range(N)])
        g = rng.integers(0, W, N)                                      # somewhere in the first corridor row
        goal = (g.astype(np.int32), np.zeros(N, np.int32))
    ty.setflags(write=False)
    _WORLDS[key] = (ty, W, H, goal, pass_types)
    return _WORLDS[key]


_FIELDS = {}


def field(name, N, P, per_env=False):
    """-> (device field uint16[N, H*W] or [N, P, H*W], its host copy): the field kernels' output for the world."""
    key = (name, N, P, per_env)
    if key not in _FIELDS:
        ty, W, H, goal, pass_types = world(name, N)
        g = None if goal is None else (dev(goal[0]), dev(goal[1]))
        if P == 1:
            f = nav().distance_field(dev(ty), None, W, H, pass_types=pass_types, goal=g)[0]
        else:
            rng = np.random.default_rng(P * 31 + N)
            if name == "v6" and P == 6 and not per_env:
                sched = nav().twoarmy_schedule(device=DEV)
            elif per_env:
                sched = dev(np.stack([timed_nav_ref.random_schedule(rng, P, H, 0.1) for _ in range(N)]).view(np.int32))
            else:
                sched = dev(timed_nav_ref.random_schedule(rng, P, H, 0.1).view(np.int32))
            f = nav().timed_field(dev(ty), None, W, H, sched, pass_types=pass_types, goal=g)[0]
        _FIELDS[key] = (f, host(f).view(np.uint16))
    return _FIELDS[key]


def positions(rng, T, N, W, H):
    """Random cells at their corners, centres and far edges; border cells; and positions that are no cell."""
    c = rng.integers(0, W * H, T * N)
    pos = np.stack([c // W + rng.choice([0.0, 0.5, 0.999], T * N), c % W + rng.choice([0.0, 0.5, 0.999], T * N)], 1)
    pos = pos.astype(np.float32)
    special = [(np.nan, 0.5), (0.5, np.inf), (-np.inf, 0.0), (-0.0, -0.0), (H, 0.0), (0.0, W), (-0.5, 0.5), (H - 1, W - 1),
               (H - 0.001, 0.0), (0.0, W - 0.001), (np.nan, np.nan), (1e30, 1.0)]
    if T * N > 24:
        for i, s in enumerate(special):
            pos[(i * 5 + 2) % (T * N)] = s
    return pos.reshape(T, N, 2)


def check(f, fh, pos, W, H, steps, age=None, init=None, off_a=0, off_d=0, want_dist=True, want=None):
    """The launch into 0xA5-boxed outputs (ahead at element offset off_a, acting_dist at byte offset off_d) against the
    reference on the same field; the bytes around the outputs stay."""
    T, N = pos.shape[:2]
    a = Boxed(T * N, torch.int64, off_a, (T, N))
    d = Boxed(T * N, torch.uint16, off_d // 2, (T, N))
    got = nav().ahead(f, dev(pos), W, H, steps=steps, age=None if age is None else dev(age),
                      init_pos=None if init is None else dev(init), out=a.view, dist_out=d.view if want_dist else False)
    assert got[0] is a.view and (got[1] is d.view if want_dist else got[1] is None)
    want = ahead_ref.ahead(fh, pos, W, H, steps, age, init) if want is None else want
    assert a.borders_intact() and (d.borders_intact() if want_dist else d.untouched())
    assert np.array_equal(u64(a.view), want[0]), np.argwhere(u64(a.view) != want[0])[:8]
    if want_dist:
        assert np.array_equal(host(d.view).view(np.uint16), want[1])
    return want


# ------------------------------------------------------------------------------------------------ the main grid
@pytest.mark.parametrize("P", [1, 2, 6, 16])
@pytest.mark.parametrize("name", ["1x1", "5x4", "v6", "32x32"])
def test_rollout_labels_equal_the_reference(name, P):
    rng = np.random.default_rng(P * 100 + len(name))
    seen = set()
    for i, (N, T, steps) in enumerate(itertools.product((1, 3, 65), (1, 7, 40), (1, 2, 3))):
        _, W, H, _, _ = world(name, N)
        f, fh = field(name, N, P, per_env=((i // 3) % 2 == 1))       # a shared schedule and a per-env one
        pos = positions(rng, T, N, W, H)
        age = rng.integers(-1, 2 * P + 3, (T, N)).astype(np.int32)                # ages <= 0 and beyond P
        init = np.array([H - 0.5, 0.25], np.float32)
        want = check(f, fh, pos, W, H, steps, age, init, off_a=i % 2, off_d=(0, 2, 6, 14)[i % 4])
        if P == 1:
            check(f, fh, pos, W, H, steps)                                          # age / init_pos NULL
        seen |= set(want[0].reshape(-1).tolist())
    if name != "1x1":                                                 # the cases are worth their name
        assert 0 in seen and len(seen) > 4 and any(bin(v).count("1") > 1 for v in seen)


def test_a_padded_per_env_schedule_and_a_padded_pitch():
    """The timed field of a schedule whose env stride is padded (a raw call: the front end takes dense ones), written into
    rows of a padded pitch; the labels read that pitch."""
    from twoarmy_amd import _lib
    N, P, T = 3, 6, 7
    ty, W, H, goal, pass_types = world("5x4", N)
    rng = np.random.default_rng(77)
    stride = P * H + 5
    sched = np.zeros((N, stride), np.uint32)
    for n in range(N):
        sched[n, :P * H] = timed_nav_ref.random_schedule(rng, P, H, 0.15).reshape(-1)
    pitch = W * H + 12
    buf = torch.full((N, P, pitch), 0x5A5A, dtype=torch.int16, device=DEV).view(torch.uint16)
    dty, dsched, gx, gy = dev(ty), dev(sched.view(np.int32)), dev(goal[0]), dev(goal[1])
    v = lambda t: C.c_void_p(t.data_ptr())                                                  # noqa: E731
    rc = _lib.lib().mg_nav_timed_field(v(dty), None, N, W, H, pass_types, 0, v(dsched), stride, P, v(gx), v(gy), 1, None, None,
                                       None, 1, v(buf), pitch, None, None, None, None)
    assert rc == 0
    f = buf[:, :, :W * H]
    fh = host(f).view(np.uint16)
    want_f = np.stack([timed_nav_ref.field(ty[n], None, W, H, sched[n, :P * H].reshape(P, H), P, pass_types,
                                           goal=(goal[0][n], goal[1][n]))["dist"] for n in range(N)])
    assert np.array_equal(fh, want_f)
    pos = positions(rng, T, N, W, H)
    age = rng.integers(-1, 15, (T, N)).astype(np.int32)
    init = np.array([3.5, 0.5], np.float32)
    for steps in (1, 2, 3):
        want = check(f, fh, pos, W, H, steps, age, init)
    assert (want[0] != 0).any()
    g = nav().distance_field(dty, None, W, H, goal=(gx, gy), out=torch.zeros((N, pitch), dtype=torch.int16, device=DEV)
                             .view(torch.uint16)[:, :W * H])[0]
    assert g.stride(0) == pitch
    check(g, host(g).view(np.uint16), pos, W, H, 3, age, init)


# ------------------------------------------------------------------------------------------------ sizes and buffers
@pytest.mark.parametrize("M", [SHARE - 1, SHARE, SHARE + 1])
def test_element_counts_around_a_workgroups_share(M):
    f, fh = field("5x4", 1, 1)
    rng = np.random.default_rng(M)
    pos = positions(rng, M, 1, 5, 4)
    want = None
    for off_a in (0, 1):
        for off_d in (0, 2, 6, 14):
            want = check(f, fh, pos, 5, 4, 3, off_a=off_a, off_d=off_d, want=want)
    check(f, fh, pos, 5, 4, 2, off_a=1, want_dist=False)                                   # acting_dist NULL
    f6, fh6 = field("5x4", 1, 6)
    age = rng.integers(-1, 20, (M, 1)).astype(np.int32)
    check(f6, fh6, pos, 5, 4, 3, age, np.array([0.5, 0.5], np.float32), off_a=1, off_d=6)


# ------------------------------------------------------------------------------------------------ positions and states
def test_edges_of_the_semantics():
    """The 5 x 4 world of test_ahead_cpu.py under goal (4, 1), every expectation written out; then states that are not
    free at their phase and a cell a wall has dropped onto."""
    ty, W, H, goal, _ = world("5x4", 1)
    f, fh = field("5x4", 1, 1)
    B = lambda dy, dx: 1 << ((dy + 3) * 7 + (dx + 3))                                       # noqa: E731
    inf = np.inf
    cases = [((3.5, 3.5), B(-2, 1), 3), ((0.5, 3.5), B(1, 1), 2), ((1.5, 4.5), B(0, 0), 0), ((1.5, 2.5), 0, U),
             ((3.999, 0.0), B(-1, 2) | B(0, 3), 6), ((0.0, 0.0), B(0, 3), 5), ((-0.0, -0.0), B(0, 3), 5),
             ((np.nan, 1.0), 0, U), ((1.0, np.nan), 0, U), ((inf, 1.0), 0, U), ((1.0, -inf), 0, U), ((4.0, 0.0), 0, U),
             ((0.0, 5.0), 0, U), ((-0.001, 0.0), 0, U), ((3.0e9, 1.0), 0, U), ((-3.0e9, -3.0e9), 0, U)]
    pos = np.array([[c[0]] for c in cases], np.float32)
    lab, d = nav().ahead(f, dev(pos), W, H, steps=3)
    assert u64(lab)[:, 0].tolist() == [c[1] for c in cases] and host(d).view(np.uint16)[:, 0].tolist() == [c[2] for c in cases]
    age = np.ones((len(cases), 1), np.int32)
    age[3], age[7], age[8] = 0, -5, 0                                # these act from init_pos = the cell (3, 3)
    lab, d = nav().ahead(f, dev(pos), W, H, steps=3, age=dev(age), init_pos=dev(np.array([3.25, 3.75], np.float32)))
    assert [u64(lab)[i, 0] for i in (3, 7, 8)] == [B(-2, 1)] * 3 and u64(lab)[0, 0] == B(-2, 1) and u64(lab)[9, 0] == 0
    # the wall cell above is what a dropped wall leaves in a field: unreachable, no label.  A state that is not free at
    # its phase has no label either.
    blocked = np.zeros((2, H), np.uint32)
    blocked[1, 0] = 1 << 3                                            # (3, 0) is occupied at phase 1
    tf = nav().timed_field(dev(ty), None, W, H, dev(blocked.view(np.int32)), goal=(dev(goal[0]), dev(goal[1])))[0]
    tfh = host(tf).view(np.uint16)
    p2 = np.array([[(0.5, 3.5)], [(0.5, 3.5)], [(0.5, 2.5)], [(0.5, 2.5)]], np.float32)
    a2 = np.array([[1], [2], [2], [1]], np.int32)
    want = ahead_ref.ahead(tfh, p2, W, H, 1, a2, np.zeros(2, np.float32))
    assert want[0][0, 0] == 0 and want[1][0, 0] == U and want[0][1, 0] != 0            # not free at phase 1, free at phase 0
    for steps in (1, 2, 3):
        check(tf, tfh, p2, W, H, steps, a2, np.zeros(2, np.float32))


# ------------------------------------------------------------------------------------------------ kernel to kernel
@pytest.mark.parametrize("P", [1, 6])
def test_invariants_a_and_c_on_the_device(P):
    N, T = 65, 40
    _, W, H, _, _ = world("v6", N)
    f, _ = field("v6", N, P)
    rng = np.random.default_rng(P)
    pos = dev(positions(rng, T, N, W, H))
    age = dev(rng.integers(-1, 14, (T, N)).astype(np.int32))
    init = dev(np.array([15.0, 3.0], np.float32))
    labs = [u64(nav().ahead(f, pos, W, H, steps=k, age=age, init_pos=init)[0]) for k in (1, 2, 3)]
    if P == 1:
        m, d = nav().optimal_moves(f, pos, W, H, age=age, init_pos=init)
    else:
        m, d = nav().timed_moves(f, pos, W, H, age, init)
    m = host(m).astype(np.uint64)
    img = sum(((m >> np.uint64(b)) & np.uint64(1)) << np.uint64(t) for b, t in ((0, 23), (1, 25), (2, 17), (3, 31), (4, 24)))
    assert np.array_equal(labs[0], img) and (img != 0).any()                               # (a)
    d = host(d).view(np.uint16)
    assert np.array_equal(labs[2] != 0, d != U)                                            # (d)
    # (c): the label at k from the labels at k - 1 and one-step labels taken at the displaced positions, a step later
    p = host(pos)
    ag = host(age)
    acting = np.where((ag <= 0)[..., None], host(init), p)
    cell_y, cell_x = np.floor(acting[..., 0]), np.floor(acting[..., 1])
    clock = np.maximum(ag, 0)
    for k in (2, 3):
        union = np.zeros((T, N), np.uint64)
        for b in range(49):
            has = ((labs[k - 2] >> np.uint64(b)) & np.uint64(1)) != 0
            if not has.any():
                continue
            dy, dx = b // 7 - 3, b % 7 - 3
            q = np.stack([cell_y + dy + 0.5, cell_x + dx + 0.5], -1).astype(np.float32)
            q[~has] = np.nan
            one = u64(nav().ahead(f, dev(q), W, H, steps=1, age=dev((clock + k - 1).astype(np.int32) if P > 1 else np.ones((T, N), np.int32)), init_pos=init)[0])
            for b1 in (17, 23, 24, 25, 31):
                on = has & (((one >> np.uint64(b1)) & np.uint64(1)) != 0)
                union |= on.astype(np.uint64) << np.uint64(b + b1 - 24)
        assert np.array_equal(union, labs[k - 1]), k


# ------------------------------------------------------------------------------------------------ records
_CASES = {}


def case(W, H, N):
    key = (W, H, N)
    if key not in _CASES:
        rng = np.random.default_rng(13 * W + 41 * H + 1000 * N)
        ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
        for n in range(N):
            ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[n % 3])
        pool = np.stack([rng.permutation(W * H)[np.arange(3) % (W * H)] for _ in range(N)])
        _CASES[key] = dict(ty=ty, st=st, pool=pool, memo={}, W=W, H=H, N=N)
    return _CASES[key]


def run_goal(c, rec, pos, steps, age=None, init=None, off_a=0, off_d=0, want_dist=True):
    t, n, goal = rec
    R = len(t)
    a = Boxed(R, torch.int64, off_a)
    d = Boxed(R, torch.uint16, off_d // 2)
    got = nav().goal_ahead(dev(c["ty"]), dev(t), dev(n), dev(goal), dev(pos), c["W"], c["H"], steps=steps,
                           age=None if age is None else dev(age), init_pos=None if init is None else dev(init),
                           state=dev(c["st"]), out=a.view, dist_out=d.view if want_dist else False)
    assert got[0] is a.view
    assert a.borders_intact() and (d.borders_intact() if want_dist else d.untouched())
    return u64(a.view), host(d.view).view(np.uint16) if want_dist else None


def check_goal(c, rec, pos, steps, age=None, init=None, **kw):
    want = ahead_ref.goal_ahead(c["ty"], c["st"], c["W"], c["H"], rec[0], rec[1], rec[2], pos, steps, age, init, memo=c["memo"])
    a, d = run_goal(c, rec, pos, steps, age, init, **kw)
    assert np.array_equal(a, want[0]), np.flatnonzero(a != want[0])[:8]
    assert d is None or np.array_equal(d, want[1])
    return want


@pytest.mark.parametrize("R", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_record_counts(R):
    c = case(9, 4, 3)
    rng = np.random.default_rng(R)
    T = 40
    pos = positions(rng, T, 3, 9, 4)
    age = rng.integers(-1, 3, (T, 3)).astype(np.int32)
    init = np.array([3.5, 0.25], np.float32)
    if R == 0:
        e32, ef = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty((0, 2), dtype=torch.float32, device=DEV)
        a0, d0 = nav().goal_ahead(dev(c["ty"]), e32, e32, ef, dev(pos), 9, 4)
        assert a0.shape == (0,) and a0.dtype == torch.int64 and d0.shape == (0,)
        return
    rec = random_records(rng, c, R, T)
    for steps in (1, 2, 3):
        want = check_goal(c, rec, pos, steps, age, init, off_a=steps % 2, off_d=(0, 2, 6, 14)[steps])
    check_goal(c, rec, pos, 3, want_dist=False)
    if R > 1:
        assert (want[0] != 0).any() and (want[0] == 0).any()


def test_run_layouts_order_and_invalid_records():
    c = case(17, 17, 3)
    rng = np.random.default_rng(99)
    T = 40
    pos = positions(rng, T, 3, 17, 17)
    age = rng.integers(-1, 5, (T, 3)).astype(np.int32)
    init = np.array([15.5, 1.5], np.float32)
    g = lambda e, k: int(c["pool"][e][k])                                                  # noqa: E731
    layouts = {
        "a run across a workgroup boundary": [(0, g(0, 0), CHUNK - 20), (1, g(1, 0), 40), (2, g(2, 0), 30)],
        "one record per goal": [(e % 3, g(e % 3, e % 3), 1) for e in range(70)],
    }
    for name, runs in layouts.items():
        want = check_goal(c, runs_to_records(rng, c, runs, T), pos, 3, age, init, off_a=1, off_d=6)
        assert (want[0] != 0).any(), name
    # relabel order against a shuffle: a record's result depends on the record alone
    rec = random_records(rng, c, CHUNK + 200, T)
    a, d = run_goal(c, rec, pos, 3, age, init)
    perm = rng.permutation(len(rec[0]))
    pa, pd = run_goal(c, tuple(x[perm] for x in rec), pos, 3, age, init)
    assert np.array_equal(pa, a[perm]) and np.array_equal(pd, d[perm])
    # invalid records among valid ones: nothing outside the arrays is addressed, their label is 0 / UNREACHABLE
    t, n, goal = (x.copy() for x in rec)
    wall = int(np.flatnonzero(~nav_ref.open_cells(c["ty"][0], c["st"][0], 17, 17).reshape(-1))[0])   # not enterable
    t[5], t[6], t[7] = -1, T, 0x7FFFFFFF
    n[8], n[9], n[10] = -1, 3, -0x80000000
    n[11], goal[11] = 0, (wall // 17 + 0.5, wall % 17 + 0.5)
    goal[12], goal[13], goal[14] = (np.nan, 1.0), (1.0, np.inf), (17.0, 0.0)
    want = check_goal(c, (t, n, goal), pos, 3, age, init)
    assert (want[0][5:15] == 0).all() and (want[1][5:15] == U).all() and (want[0] != 0).any()


@pytest.mark.parametrize("W,H", [(9, 4), (17, 17)])
def test_one_goal_per_env_equals_field_then_ahead(W, H):
    N, T = 65, 5
    c = case(W, H, N)
    rng = np.random.default_rng(W + H)
    gc = c["pool"][:, 0]
    gx, gy = (gc % W).astype(np.int32), (gc // W).astype(np.int32)
    pos = positions(rng, T, N, W, H)
    age = rng.integers(-1, 3, (T, N)).astype(np.int32)
    init = np.array([0.5, W - 0.5], np.float32)
    f = nav().distance_field(dev(c["ty"]), dev(c["st"]), W, H, goal=(dev(gx), dev(gy)))[0]
    order = rng.permutation(T * N)
    order = order[np.argsort(order % N, kind="stable")]
    t, n = (order // N).astype(np.int32), (order % N).astype(np.int32)
    goal = np.stack([gy[n] + 0.5, gx[n] + 0.25], 1).astype(np.float32)
    for steps in (1, 3):
        fa, fd = nav().ahead(f, dev(pos), W, H, steps=steps, age=dev(age), init_pos=dev(init))
        a, d = run_goal(c, (t, n, goal), pos, steps, age, init)
        assert np.array_equal(a, u64(fa)[t, n]) and np.array_equal(d, host(fd).view(np.uint16)[t, n])
        assert (a != 0).any()


def test_engine_goal_ahead_reads_the_engines_planes():
    from twoarmy_amd.engine import TwoarmyEngine
    N, T = 16, 8
    eng = TwoarmyEngine(6, N, 17, seed=9981)
    eng.reset()
    rng = np.random.default_rng(4)
    pos = positions(rng, T, N, 17, 17)
    ty = eng.get_state()[0]
    c = dict(ty=ty, st=None, W=17, H=17, N=N, pool=np.stack([np.flatnonzero(ty[n] == 1)[[3, 20, 40]] for n in range(N)]))
    t, n, goal = random_records(rng, c, 300, T)
    her = dict(t=dev(t), n=dev(n), goal=dev(goal))
    a, d = eng.goal_ahead(her, dev(pos), steps=3, pass_types=nav_ref.PASS_DEFAULT | BALL)
    want = ahead_ref.goal_ahead(ty, None, 17, 17, t, n, goal, pos, 3, pass_types=nav_ref.PASS_DEFAULT | BALL)
    assert np.array_equal(u64(a), want[0]) and np.array_equal(host(d).view(np.uint16), want[1]) and (want[0] != 0).any()
    eng.close()


# ------------------------------------------------------------------------------------------------ rejections on the device build
def test_bad_arguments_launch_nothing():
    """Every TW_E_ARG case of both entry points (the lists of test_ahead_cpu.py) with device arrays behind the pointers, with
    and without something to launch: nothing is written; then the good calls launch."""
    from twoarmy_amd import _lib
    lib = _lib.lib()
    W, H, N, T, R = 5, 4, 3, 2, 6
    v = lambda x: None if x is None else C.c_void_p(x)                                     # noqa: E731
    ty = torch.ones((N, W * H), dtype=torch.uint8, device=DEV)
    st = torch.zeros((N, W * H), dtype=torch.uint8, device=DEV)
    f = torch.zeros((N, 16, W * H + 4), dtype=torch.int16, device=DEV)                     # distance 0 everywhere
    t = torch.zeros(R + 1, dtype=torch.int32, device=DEV)
    rn = torch.zeros(R + 1, dtype=torch.int32, device=DEV)
    goal = torch.zeros((R + 1, 2), dtype=torch.float32, device=DEV)
    pos = torch.zeros((T + 1, N, 2), dtype=torch.float32, device=DEV)
    age = torch.ones((T + 1, N), dtype=torch.int32, device=DEV)
    init = torch.zeros(4, dtype=torch.float32, device=DEV)
    out = torch.full((8 * (R + 2),), 0xA5, dtype=torch.uint8, device=DEV)
    ad = torch.full((2 * R + 4,), 0xA5, dtype=torch.uint8, device=DEV)

    def ahead(a):
        return lib.mg_nav_ahead(v(a["dist"]), a["pitch"], a["P"], a["n"], a["W"], a["H"], v(a["pos"]), v(a["age"]),
                                v(a["init"]), a["T"], a["steps"], v(a["ahead"]), v(a["ad"]), None)

    good = dict(dist=f.data_ptr(), pitch=0, P=1, n=N, W=W, H=H, pos=pos.data_ptr(), age=age.data_ptr(), init=init.data_ptr(),
                T=T, steps=3, ahead=out.data_ptr(), ad=ad.data_ptr())
    bad = [dict(dist=None), dict(pos=None), dict(ahead=None), dict(n=0), dict(n=-1), dict(T=-1), dict(W=0), dict(H=0),
           dict(W=33), dict(H=33), dict(pitch=19), dict(pitch=-1), dict(dist=good["dist"] + 1), dict(ad=good["ad"] + 1),
           dict(pos=good["pos"] + 4), dict(age=good["age"] + 2), dict(init=good["init"] + 1), dict(init=None),
           dict(P=0), dict(P=17), dict(P=-1),
           dict(P=2, age=None, init=None), dict(P=2, age=None), dict(P=6, init=None),       # the age is the clock
           dict(steps=0), dict(steps=4), dict(steps=-1),
           dict(ahead=good["ahead"] + 4), dict(ahead=good["ahead"] + 2), dict(ahead=good["ahead"] + 1)]
    for kw in bad:
        for T_ in (0, T):                                         # rejected whether or not there is anything to launch
            assert ahead(dict(good, T=T_, **kw) if "T" not in kw else dict(good, **kw)) == -1, (kw, T_)
    assert ahead(dict(good, n=1 << 20, T=1 << 20)) == -1                                   # T * n_envs >= 2^40
    assert ahead(dict(good, T=0)) == 0                                                     # nothing to launch

    def goal_ahead(a):
        return lib.mg_nav_goal_ahead(v(a["type"]), v(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"],
                                     v(a["t"]), v(a["rn"]), v(a["goal"]), a["R"], v(a["pos"]), v(a["age"]), v(a["init"]),
                                     a["T"], a["steps"], v(a["ahead"]), v(a["ad"]), None)

    ggood = dict(type=ty.data_ptr(), state=st.data_ptr(), n=N, W=W, H=H, pass_types=nav_ref.PASS_DEFAULT, flags=0,
                 t=t.data_ptr(), rn=rn.data_ptr(), goal=goal.data_ptr(), R=R, pos=pos.data_ptr(), age=age.data_ptr(),
                 init=init.data_ptr(), T=T, steps=3, ahead=out.data_ptr(), ad=ad.data_ptr())
    gbad = [dict(type=None), dict(t=None), dict(rn=None), dict(goal=None), dict(pos=None), dict(ahead=None),
            dict(n=0), dict(n=-1), dict(W=0), dict(H=0), dict(W=33), dict(H=33), dict(W=-1),
            dict(pass_types=0x10000), dict(flags=2), dict(flags=3), dict(flags=-1),
            dict(pos=ggood["pos"] + 4), dict(t=ggood["t"] + 2), dict(rn=ggood["rn"] + 1), dict(goal=ggood["goal"] + 2),
            dict(age=ggood["age"] + 2), dict(init=ggood["init"] + 1), dict(ad=ggood["ad"] + 1),
            dict(init=None), dict(T=-1), dict(R=-1), dict(R=1 << 40), dict(R=1 << 62),
            dict(steps=0), dict(steps=4), dict(steps=-1),
            dict(ahead=ggood["ahead"] + 4), dict(ahead=ggood["ahead"] + 2), dict(ahead=ggood["ahead"] + 1)]
    for kw in gbad:
        for R_ in (0, R):
            assert goal_ahead(dict(ggood, R=R_, **kw) if "R" not in kw else dict(ggood, **kw)) == -1, (kw, R_)
    assert goal_ahead(dict(ggood, R=0)) == 0                                               # no records: ok, no launch
    torch.cuda.synchronize()
    assert (host(out) == 0xA5).all() and (host(ad) == 0xA5).all()
    # and the good calls launch
    assert ahead(dict(good, P=2, pitch=W * H + 4, ahead=good["ahead"] + 8)) == 0           # T * N = 6 labels behind one slot
    torch.cuda.synchronize()
    o = host(out)
    assert (o[:8] == 0xA5).all() and (o[56:] == 0xA5).all()
    assert (o[8:56].view(np.uint64) == 1 << 24).all()                                      # distance 0 everywhere: the same cell
    assert (host(ad)[:2 * T * N] == 0).all() and (host(ad)[2 * T * N:] == 0xA5).all()
    assert goal_ahead(dict(ggood, age=None, init=None, ad=None, state=None, flags=1)) == 0  # every record acts on its goal cell 0
    torch.cuda.synchronize()
    assert (host(out)[:48].view(np.uint64) == 1 << 24).all() and (host(out)[56:] == 0xA5).all()
