"""mg_nav_goal_moves on the device: the optimal-move sets of records that each name their own goal, exact integers against
goal_moves_ref.py (a BFS per record's env and goal), and against the field + optimal-moves kernels it must agree with."""
import ctypes as C

import numpy as np
import pytest
import torch

import goal_moves_ref
import nav_ref
import prior_ref
from nav_util import dev, host, random_records, runs_to_records

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = nav_ref.UNREACHABLE
CHUNK = 1024                                                          # records per workgroup (NAV_GOAL_ELEMS)
SIDES = [(1, 1), (1, 7), (9, 4), (5, 5), (17, 17)]                    # (W, H)
BALL, LAVA = 1 << 6, 1 << 9
# (pass_types, state plane given, MG_NAV_DOORS_OPEN)
VARIANTS = [(nav_ref.PASS_DEFAULT, True, False), (nav_ref.PASS_DEFAULT | BALL, False, False),
            (nav_ref.PASS_DEFAULT & ~LAVA, True, True)]


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


_CASES = {}


def case(W, H, N):
    """N random worlds of one size (every type code, doors in all states), a small pool of goal cells per env -- enterable
    ones, a wall and whatever else comes -- and one memo of reference fields per variant.  Made once, worlds read-only."""
    key = (W, H, N)
    if key not in _CASES:
        rng = np.random.default_rng(13 * W + 41 * H + 1000 * N)
        ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
        for n in range(N):
            ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[n % 3])
        pool = np.stack([rng.permutation(W * H)[np.arange(3) % (W * H)] for _ in range(N)])
        for a in (ty, st, pool):
            a.setflags(write=False)
        _CASES[key] = dict(ty=ty, st=st, pool=pool, memo=[{} for _ in VARIANTS], W=W, H=H, N=N)
    return _CASES[key]


def positions(rng, T, N, W, H):
    """Random cells at their corners, centres and far edges, and a sprinkle of positions that are no cell."""
    c = rng.integers(0, W * H, T * N)
    pos = np.stack([c // W + rng.choice([0.0, 0.5, 0.999], T * N), c % W + rng.choice([0.0, 0.5, 0.999], T * N)], 1)
    pos = pos.astype(np.float32)
    special = [(np.nan, 0.5), (0.5, np.inf), (-np.inf, 0.0), (-0.0, -0.0), (H, 0.0), (0.0, W), (-0.5, 0.5), (H - 1, W - 1)]
    if T * N > 16:
        for i, s in enumerate(special):
            pos[(i * 5 + 2) % (T * N)] = s
    return pos.reshape(T, N, 2)


def run(c, variant, rec, pos, age=None, init=None, off_m=0, off_d=0, want_dist=True, planes=None):
    """The kernel through the front end, `moves` at byte offset off_m and `acting_dist` at byte offset off_d inside
    0xA5-filled buffers; checks that nothing but the outputs changed.  -> (moves, acting_dist) on the host."""
    pass_types, with_state, doors_open = VARIANTS[variant]
    W, H = c["W"], c["H"]
    t, n, goal = rec
    R = len(t)
    mbuf = torch.full((16 + off_m + R + 37,), 0xA5, dtype=torch.uint8, device=DEV)
    dbuf = torch.full((16 + off_d + 2 * R + 38,), 0xA5, dtype=torch.uint8, device=DEV)
    mv = mbuf[16 + off_m:16 + off_m + R]
    dv = dbuf[16 + off_d:16 + off_d + 2 * R].view(torch.uint16)
    assert mbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0 and off_d % 2 == 0
    ty, st = planes if planes is not None else (dev(c["ty"]), dev(c["st"]))
    got = nav().goal_moves(ty, dev(t), dev(n), dev(goal), dev(pos), W, H, pass_types=pass_types,
                           age=None if age is None else dev(age), init_pos=None if init is None else dev(init),
                           state=st if with_state else None, doors_open=doors_open, out=mv,
                           dist_out=dv if want_dist else False)
    assert got[0] is mv and (got[1] is dv if want_dist else got[1] is None)
    hm, hd = host(mbuf), host(dbuf)
    assert (hm[:16 + off_m] == 0xA5).all() and (hm[16 + off_m + R:] == 0xA5).all()
    assert (hd[:16 + off_d] == 0xA5).all() and (hd[16 + off_d + 2 * R:] == 0xA5).all()
    if not want_dist:
        assert (hd == 0xA5).all()
    return host(mv), host(dv) if want_dist else None


def ref(c, variant, rec, pos, age=None, init=None):
    pass_types, with_state, doors_open = VARIANTS[variant]
    return goal_moves_ref.goal_moves(c["ty"], c["st"] if with_state else None, c["W"], c["H"], rec[0], rec[1], rec[2], pos,
                                     age, init, pass_types, nav_ref.DOORS_OPEN if doors_open else 0, memo=c["memo"][variant])


def check(c, variant, rec, pos, age=None, init=None, **kw):
    want = ref(c, variant, rec, pos, age, init)
    m, d = run(c, variant, rec, pos, age, init, **kw)
    assert np.array_equal(m, want[0]), np.flatnonzero(m != want[0])[:8]
    assert d is None or np.array_equal(d, want[1]), np.flatnonzero(d != want[1])[:8]
    return want


# ------------------------------------------------------------------------------------------------ worlds, sizes, counts
@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("W,H", SIDES)
def test_records_equal_the_reference(W, H, N):
    c = case(W, H, N)
    rng = np.random.default_rng(W * 100 + H + N)
    init = np.array([H - 0.5, 0.25], np.float32)
    seen_m, seen_d = set(), set()
    for i, (T, R) in enumerate([(1, 1), (5, 63), (64, CHUNK - 1), (5, CHUNK + 1), (64, 2 * CHUNK + 17)]):
        pos = positions(rng, T, N, W, H)
        age = rng.integers(-1, 3, (T, N)).astype(np.int32)
        rec = random_records(rng, c, R, T)
        want = check(c, i % 3, rec, pos, age, init, off_m=i, off_d=2 * i)
        check(c, (i + 1) % 3, rec, pos)                                                    # age / init_pos NULL
        seen_m |= set(want[0].tolist())
        seen_d |= set(want[1].tolist())
    if W * H >= 25 and N > 1:                                     # the cases are worth their name
        assert {bin(v).count("1") for v in seen_m} >= {0, 1, 2} and prior_ref.STAY in seen_m
        assert U in seen_d and len(seen_d) > 3


def test_long_paths_in_a_serpentine():
    """32 x 32, one corridor through all even rows: distances beyond 255 and a flood of about W*H/2 steps."""
    W = H = 32
    ty, src = nav_ref.serpentine(W, H)
    open_world = np.ones(W * H, np.uint8)
    c = dict(ty=np.stack([ty, open_world]), st=np.zeros((2, W * H), np.uint8), W=W, H=H, N=2, memo=[{} for _ in VARIANTS])
    rng = np.random.default_rng(32)
    T = 40
    cells = np.flatnonzero(ty != 2)
    pick = cells[rng.integers(0, cells.size, T)]
    pos = np.zeros((T, 2, 2), np.float32)
    pos[:, 0] = np.stack([pick // W + 0.5, pick % W + 0.5], 1)
    pos[:, 1] = rng.random((T, 2)) * 32
    pos[0, 0] = (30.5, 31.5 if ty[30 * W + 31] != 2 else 0.5)
    far = W * (H - 2)                                              # the first cell of the last corridor row
    runs = [(0, 0, T), (1, 0, T), (0, far, T), (0, int(cells[cells.size // 2]), T), (1, W * H - 1, T)]
    t = np.tile(np.arange(T), len(runs)).astype(np.int32)
    n = np.concatenate([np.full(T, e) for e, _, _ in runs]).astype(np.int32)
    goal = np.concatenate([np.tile([gc // W + 0.5, gc % W + 0.5], (T, 1)) for _, gc, _ in runs]).astype(np.float32)
    want = check(c, 0, (t, n, goal), pos)
    finite = want[1][want[1] != U]
    assert finite.max() > 255 and (want[1][:T] != U).all()


# ------------------------------------------------------------------------------------------------ run layouts
def test_run_layouts():
    c = case(17, 17, 3)
    rng = np.random.default_rng(99)
    T = 64
    pos = positions(rng, T, 3, 17, 17)
    age = rng.integers(-1, 5, (T, 3)).astype(np.int32)
    init = np.array([15.5, 1.5], np.float32)
    p = c["pool"]
    g = lambda e, k: int(p[e][k])                                                          # noqa: E731
    layouts = {
        "a run that straddles a chunk boundary": [(0, g(0, 0), CHUNK - 20), (1, g(1, 0), 40), (2, g(2, 0), 30)],
        "a run longer than a chunk": [(2, g(2, 1), 7), (1, g(1, 1), CHUNK + 300), (0, g(0, 1), 5)],
        "a run of exactly two chunks": [(1, g(1, 2), 2 * CHUNK)],
        "same env, different goals; different envs, the same goal cell":
            [(0, g(0, 0), 16), (0, g(0, 1), 16), (1, g(0, 1), 16), (2, g(0, 1), 16), (2, g(0, 1), 1), (0, g(0, 1), 1)],
        "runs of one record": [(e % 3, g(e % 3, e % 2), 1) for e in range(70)],
    }
    for name, runs in layouts.items():
        rec = runs_to_records(rng, c, runs, T)
        for off_m, off_d in ((0, 0), (5, 6)):
            want = check(c, 0, rec, pos, age, init, off_m=off_m, off_d=off_d)
        assert (want[0] != 0).any(), name


def test_every_record_a_different_goal():
    """The worst case for floods: no two neighbours share (env, goal cell); 5 x 5 keeps the reference small."""
    W = H = 5
    c = case(W, H, 3)
    rng = np.random.default_rng(55)
    T, R = 5, 2 * CHUNK + 17
    b = np.arange(R)
    n = ((b // 25) % 3).astype(np.int32)
    gc = (b * 7) % 25
    t = (b % T).astype(np.int32)
    goal = np.stack([gc // W + 0.5, gc % W + 0.5], 1).astype(np.float32)
    assert ((gc[1:] != gc[:-1]) | (n[1:] != n[:-1])).all()
    pos = positions(rng, T, 3, W, H)
    want = check(c, 1, (t, n, goal), pos)
    assert len(set(want[1].tolist())) > 4


def test_the_order_of_the_records_does_not_matter():
    c = case(17, 17, 3)
    rng = np.random.default_rng(3)
    T, R = 64, 2 * CHUNK + 17
    pos = positions(rng, T, 3, 17, 17)
    age = rng.integers(-1, 5, (T, 3)).astype(np.int32)
    init = np.array([15.5, 1.5], np.float32)
    rec = random_records(rng, c, R, T)
    m, d = run(c, 0, rec, pos, age, init)
    perm = rng.permutation(R)
    pm, pd = run(c, 0, tuple(a[perm] for a in rec), pos, age, init)
    assert np.array_equal(pm, m[perm]) and np.array_equal(pd, d[perm])
    want = ref(c, 0, rec, pos, age, init)
    assert np.array_equal(m, want[0]) and np.array_equal(d, want[1])


# ------------------------------------------------------------------------------------------------ edges of the semantics
def test_edges_of_the_semantics():
    """A 7 x 7 room with a wall down column 4 that cuts columns 5, 6 off; every record's expectation written out."""
    W = H = 7
    ty = np.ones((H, W), np.uint8)
    ty[:, 4] = 2
    N, T = 2, 3
    c = dict(ty=np.stack([ty.reshape(-1)] * N), st=np.zeros((N, W * H), np.uint8), W=W, H=H, N=N,
             memo=[{} for _ in VARIANTS])
    pos = np.zeros((T, N, 2), np.float32)
    pos[0, 0] = (3.5, 3.5)            # (y, x)
    pos[1, 0] = (1.5, 1.5)
    pos[2, 0] = (2.5, 5.5)            # behind the wall
    pos[0, 1] = (np.nan, 1.0)         # no cell
    pos[1, 1] = (0.0, 0.0)
    pos[2, 1] = (6.999, 0.0)
    age = np.ones((T, N), np.int32)
    age[2, 1] = 0                     # record at (2, 1) acts from init_pos
    age[1, 1] = -1
    init = np.array([3.25, 3.75], np.float32)
    inf = np.inf
    # (t, n, goal y, goal x) -> (moves, dist)
    cases = [
        ((0, 0, 3.0, 3.0), (0x10, 0)),                 # acting position on the goal
        ((0, 0, 3.9, 3.9), (0x10, 0)),
        ((1, 0, 3.5, 3.5), (0x2 | 0x8, 4)),            # a tie: right and down
        ((1, 0, 1.5, 3.5), (0x2, 2)),
        ((1, 0, 0.5, 0.5), (0x1 | 0x4, 2)),            # a tie: left and up
        ((0, 0, 6.5, 3.5), (0x8, 3)),
        ((2, 0, 3.5, 3.5), (0, U)),                    # the acting cell is cut off from the goal
        ((0, 0, 2.5, 5.5), (0, U)),                    # and the other way round
        ((2, 0, 2.5, 6.5), (0x2, 1)),                  # both behind the wall
        ((0, 0, 3.5, 4.5), (0, U)),                    # a goal on a wall
        ((0, 0, np.nan, 3.5), (0, U)),                 # goals that are no cell
        ((0, 0, 3.5, inf), (0, U)),
        ((0, 0, -inf, 3.5), (0, U)),
        ((0, 0, 7.0, 3.5), (0, U)),
        ((0, 0, 3.5, -0.001), (0, U)),
        ((0, 0, 3.5, np.float32(7.0)), (0, U)),
        ((-1, 0, 3.5, 3.5), (0, U)),                   # rec_t outside [0, T)
        ((T, 0, 3.5, 3.5), (0, U)),
        ((0, -1, 3.5, 3.5), (0, U)),                   # rec_n outside [0, N)
        ((0, N, 3.5, 3.5), (0, U)),
        ((0x7FFFFFFF, 0x7FFFFFFF, 3.5, 3.5), (0, U)),
        ((-0x80000000, -0x80000000, 3.5, 3.5), (0, U)),
        ((0, 1, 3.5, 3.5), (0, U)),                    # the acting position is no cell
        ((2, 1, 3.5, 3.5), (0x10, 0)),                 # age <= 0: init_pos = cell (3, 3), not (0, 6)
        ((1, 1, 3.5, 0.5), (0x1, 3)),                  # age < 0 alike
        ((2, 1, 6.5, 3.5), (0x8, 3)),
    ]
    t = np.array([k[0][0] for k in cases], np.int64).astype(np.int32)
    n = np.array([k[0][1] for k in cases], np.int64).astype(np.int32)
    goal = np.array([k[0][2:] for k in cases], np.float32)
    want_m = np.array([k[1][0] for k in cases], np.uint8)
    want_d = np.array([k[1][1] for k in cases], np.uint16)
    r = ref(c, 0, (t, n, goal), pos, age, init)
    assert np.array_equal(r[0], want_m) and np.array_equal(r[1], want_d)     # the reference agrees with the table
    m, d = run(c, 0, (t, n, goal), pos, age, init)
    assert np.array_equal(m, want_m) and np.array_equal(d, want_d)
    # age / init_pos NULL: the positions as they stand
    want = ref(c, 0, (t, n, goal), pos)
    m, d = run(c, 0, (t, n, goal), pos)
    assert np.array_equal(m, want[0]) and np.array_equal(d, want[1])
    assert (m[-3], d[-3]) == (0x2 | 0x4, 6) and (m[-2], d[-2]) == (0x8, 3)     # from (6, 0) and from (0, 0)


# ------------------------------------------------------------------------------------------------ kernel to kernel
@pytest.mark.parametrize("W,H", [(9, 4), (17, 17)])
def test_one_goal_per_env_equals_field_then_optimal_moves(W, H):
    N, T = 65, 5
    c = case(W, H, N)
    rng = np.random.default_rng(W + H)
    ty, st = dev(c["ty"]), dev(c["st"])
    gc = c["pool"][:, 0]
    gx, gy = (gc % W).astype(np.int32), (gc // W).astype(np.int32)
    pos = positions(rng, T, N, W, H)
    age = rng.integers(-1, 3, (T, N)).astype(np.int32)
    init = np.array([0.5, W - 0.5], np.float32)
    field = nav().distance_field(ty, st, W, H, goal=(dev(gx), dev(gy)))[0]
    fm, fd = nav().optimal_moves(field, dev(pos), W, H, age=dev(age), init_pos=dev(init))
    order = rng.permutation(T * N)
    order = order[np.argsort(order % N, kind="stable")]              # runs of one env, steps in any order
    t, n = (order // N).astype(np.int32), (order % N).astype(np.int32)
    goal = np.stack([gy[n] + 0.5, gx[n] + 0.25], 1).astype(np.float32)
    m, d = run(c, 0, (t, n, goal), pos, age, init)
    assert np.array_equal(m, host(fm)[t, n]) and np.array_equal(d, host(fd).view(np.uint16)[t, n])
    assert (d != U).any() and (m != 0).any()


# ------------------------------------------------------------------------------------------------ writes, NULL outputs
@pytest.mark.parametrize("R", [5, CHUNK + 1])
def test_write_bounds_at_every_alignment(R):
    c = case(17, 17, 3)
    rng = np.random.default_rng(R)
    T = 64
    pos = positions(rng, T, 3, 17, 17)
    rec = random_records(rng, c, R, T)
    want = ref(c, 0, rec, pos)
    for off_m in range(16):
        off_d = (0, 2, 6, 14)[off_m % 4]
        m, d = run(c, 0, rec, pos, off_m=off_m, off_d=off_d)
        assert np.array_equal(m, want[0]) and np.array_equal(d, want[1]), (off_m, off_d)
    for off_m in (0, 9):
        m, d = run(c, 0, rec, pos, off_m=off_m, want_dist=False)                         # acting_dist NULL
        assert np.array_equal(m, want[0]) and d is None


def raw_call(lib, a):
    v = lambda x: None if x is None else C.c_void_p(x)                                     # noqa: E731
    return lib.mg_nav_goal_moves(v(a["type"]), v(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"], v(a["t"]),
                                 v(a["rn"]), v(a["goal"]), a["R"], v(a["pos"]), v(a["age"]), v(a["init"]), a["T"],
                                 v(a["moves"]), v(a["ad"]), None)


def test_bad_arguments_and_no_records_launch_nothing():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    W, H, N, T, R = 5, 4, 3, 2, 6
    ty = torch.ones((N, W * H), dtype=torch.uint8, device=DEV)
    st = torch.zeros((N, W * H), dtype=torch.uint8, device=DEV)
    t = torch.zeros(R + 1, dtype=torch.int32, device=DEV)
    rn = torch.zeros(R + 1, dtype=torch.int32, device=DEV)
    goal = torch.zeros((R + 1, 2), dtype=torch.float32, device=DEV)
    pos = torch.zeros((T + 1, N, 2), dtype=torch.float32, device=DEV)
    age = torch.ones((T + 1, N), dtype=torch.int32, device=DEV)
    init = torch.zeros(4, dtype=torch.float32, device=DEV)
    moves = torch.full((R + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    ad = torch.full((2 * R + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    good = dict(type=ty.data_ptr(), state=st.data_ptr(), n=N, W=W, H=H, pass_types=nav_ref.PASS_DEFAULT, flags=0,
                t=t.data_ptr(), rn=rn.data_ptr(), goal=goal.data_ptr(), R=R, pos=pos.data_ptr(), age=age.data_ptr(),
                init=init.data_ptr(), T=T, moves=moves.data_ptr(), ad=ad.data_ptr())
    bad = [dict(type=None), dict(t=None), dict(rn=None), dict(goal=None), dict(pos=None), dict(moves=None),
           dict(n=0), dict(n=-1), dict(W=0), dict(H=0), dict(W=33), dict(H=33), dict(W=-1),
           dict(pass_types=0x10000), dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(pos=good["pos"] + 4), dict(t=good["t"] + 2), dict(rn=good["rn"] + 1), dict(goal=good["goal"] + 2),
           dict(age=good["age"] + 2), dict(init=good["init"] + 1), dict(ad=good["ad"] + 1),
           dict(init=None), dict(T=-1), dict(R=-1), dict(R=1 << 40), dict(R=1 << 62)]
    for kw in bad:
        assert raw_call(lib, dict(good, **kw)) == -1, kw
    assert raw_call(lib, dict(good, R=0)) == 0                                           # no records: ok, no launch
    torch.cuda.synchronize()
    assert (host(moves) == 0xA5).all() and (host(ad) == 0xA5).all()
    # and the good calls launch: every record acts on cell 0 with goal cell 0
    assert raw_call(lib, good) == 0
    assert raw_call(lib, dict(good, age=None, init=None, ad=None, state=None, flags=1, moves=good["moves"] + 1,
                              goal=good["goal"] + 4, T=0)) == 0                           # T = 0: no record has a step
    torch.cuda.synchronize()
    assert host(moves).tolist() == [prior_ref.STAY] + [0] * R + [0xA5] * 3
    assert (host(ad)[:2 * R] == 0).all() and (host(ad)[2 * R:] == 0xA5).all()
    # the front end with no records: nothing allocated beyond the empty outputs, nothing launched
    e32, ef = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty((0, 2), dtype=torch.float32, device=DEV)
    m0, d0 = nav().goal_moves(ty, e32, e32, ef, pos[:T], W, H)
    assert m0.shape == (0,) and m0.dtype == torch.uint8 and d0.shape == (0,)


# ------------------------------------------------------------------------------------------------ reading in place
@pytest.mark.parametrize("W,H", [(17, 17), (9, 4), (1, 7)])
def test_planes_off_a_word_boundary(W, H):
    N, T, R = 3, 5, 200
    c = case(W, H, N)
    rng = np.random.default_rng(W)
    pos = positions(rng, T, N, W, H)
    rec = random_records(rng, c, R, T)
    want = ref(c, 0, rec, pos)
    cells = N * W * H

    def inside(a, off):
        buf = torch.full((((4 + off + cells + 3) & ~3) + 4,), 0xFF, dtype=torch.uint8, device=DEV)
        v = buf[4 + off:4 + off + cells]
        v.copy_(dev(a).view(-1))
        assert v.data_ptr() % 4 == off
        return buf, v.view(N, W * H)
    for off_t, off_s in ((1, 0), (2, 1), (3, 3)):
        bt, ty = inside(c["ty"], off_t)
        bs, st = inside(c["st"], off_s)
        m, d = run(c, 0, rec, pos, planes=(ty, st))
        assert np.array_equal(m, want[0]) and np.array_equal(d, want[1]), (off_t, off_s)
        assert int((bt == 0xFF).sum()) >= bt.numel() - cells and int((bs == 0xFF).sum()) >= bs.numel() - cells


def test_engine_goal_moves_reads_the_engines_planes():
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
    for pass_types in (None, nav_ref.PASS_DEFAULT | BALL):
        m, d = eng.goal_moves(her, dev(pos), pass_types=pass_types)
        want = goal_moves_ref.goal_moves(ty, None, 17, 17, t, n, goal, pos,
                                         pass_types=nav_ref.PASS_DEFAULT if pass_types is None else pass_types)
        assert np.array_equal(host(m), want[0]) and np.array_equal(host(d).view(np.uint16), want[1])
        assert (want[0] != 0).any()
    eng.close()
