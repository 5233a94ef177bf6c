"""mg_nav_shape and mg_nav_goal_shape on the device (include/minigrid_nav.h, "Reward shaping") against shape_ref.py,
through the torch front end, the C ABI, TwoarmyEngine and VecPPOTrainer.  Every comparison is bit for bit: float outputs
are compared as uint32 views.  NaN rewards sit on elements that are unshaped by construction (the sum of a NaN and a
number has no pinned payload); -0.0 rewards sit anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import nav_ref
import shape_ref
import timed_nav_ref as tref
from nav_util import Boxed, bits, dev, host, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = nav_ref.UNREACHABLE
ZT = shape_ref.ZERO_TERMINAL
BALL = 1 << 6
CHUNK = 1024                                                          # records per workgroup of mg_nav_goal_shape
ARITH = [(1.0, 0.125), (0.99, 0.01)]                                  # (gamma, scale)


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


# ------------------------------------------------------------------------------------------------ worlds and fields
def synthetic(W, H):
    """Walls across the middle with one gap and one closed door, and a pocket walled off in the last corner."""
    ty, st = np.ones((H, W), np.uint8), np.zeros((H, W), np.uint8)
    if H > W:
        ty[H // 2, :] = 2
        ty[H // 2, 1], st[H // 2, 1] = 4, 1                           # a closed door
        ty[H // 2, 3] = 1                                             # the gap
    else:
        ty[:, W // 2] = 2
        ty[2, W // 2], st[2, W // 2] = 4, 1
        ty[0, W // 2] = 1
    ty[H - 1, W - 2] = ty[H - 2, W - 1] = 2                           # the pocket: cell (W - 1, H - 1)
    return ty.reshape(-1), st.reshape(-1)


_CASES = {}


def case(kind, N):
    """The worlds of one kind and N with their host fields (period 1 and a timed one), made once and read-only."""
    key = (kind, N)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(sum(map(ord, str(kind))) + 17 * N)
    if kind == "twoarmy":
        from twoarmy_amd.engine import TwoarmyEngine
        W = H = 17
        eng = TwoarmyEngine(6, N, 17, seed=9981)
        eng.reset()
        ty = eng.get_state()[0].reshape(N, W * H).copy()
        eng.close()
        st, goal, pass_types, P = None, None, nav_ref.PASS_DEFAULT | BALL, 6
        sched = nav().twoarmy_schedule(blocks=True).numpy().astype(np.int64)
        uniq, inv = np.unique(ty, axis=0, return_inverse=True)        # a reset leaves few distinct planes
        d1 = nav_ref.fields(uniq, None, W, H, pass_types)[0][inv.reshape(-1)]
        dP = tref.fields(uniq, None, W, H, sched, P, pass_types)[0][inv.reshape(-1)]
    else:
        W, H = kind
        base_ty, base_st = synthetic(W, H)
        ty, st = np.tile(base_ty, (N, 1)), np.tile(base_st, (N, 1))
        extra = rng.random((N, W * H)) < 0.08                         # every env but the first its own few walls more
        extra[0] = False
        ty[extra & (ty == 1)] = 2
        gc = np.array([rng.choice(np.flatnonzero(ty[n] == 1)) for n in range(N)])
        goal, pass_types, P = ((gc % W).astype(np.int32), (gc // W).astype(np.int32)), nav_ref.PASS_DEFAULT, 3
        sched = tref.random_schedule(rng, P, H, 0.12).astype(np.int64)
        d1 = nav_ref.fields(ty, st, W, H, pass_types, goal=goal)[0]
        dP = tref.fields(ty, st, W, H, sched, P, pass_types, goal=goal)[0]
    assert (d1 == U).any() and (d1 != U).any() and (dP != U).any()
    c = dict(W=W, H=H, N=N, P=P, ty=ty, st=st, goal=goal, pass_types=pass_types, dist={1: d1, P: dP})
    for a in (ty, d1, dP):
        a.setflags(write=False)
    _CASES[key] = c
    return c


def rollout(c, T, seed):
    """Seeded random walks, one per env: a move or a wait per step, walls and the world's edge no obstacle, so positions
    on walls and outside the world come by themselves; a NaN, an infinity and a wall cell are planted.  -> dict of
    pos_before, pos_after [T, N, 2], age [T, N] (zeros and negatives), init, done, reward (-0.0 anywhere; NaNs on elements
    whose after position is no cell and that are not done: unshaped under either flag)."""
    W, H, N = c["W"], c["H"], c["N"]
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.integers(0, W, N), rng.integers(0, H, N)], 1)
    walk = np.zeros((T + 1, N, 2), np.float32)
    for t in range(T + 1):
        walk[t, :, 0], walk[t, :, 1] = xy[:, 1] + rng.choice([0.0, 0.5, 0.999], N), xy[:, 0] + rng.choice([0.0, 0.5, 0.999], N)
        xy = xy + np.array([(-1, 0), (1, 0), (0, -1), (0, 1), (0, 0)])[rng.integers(0, 5, N)]
        xy = np.clip(xy, -1, (W, H))
    before, after = walk[:-1].copy(), walk[1:].copy()
    M = T * N
    done = (rng.random((T, N)) < 0.2).astype(np.uint8)
    reward = rng.standard_normal((T, N)).astype(np.float32)
    reward.reshape(-1)[rng.integers(0, M, max(1, M // 9))] = -0.0
    walls = np.flatnonzero(c["ty"][0] == 2)
    wall = int(walls[0]) if walls.size else 0
    fb, fa, fd, fr = before.reshape(-1, 2), after.reshape(-1, 2), done.reshape(-1), reward.reshape(-1).view(np.uint32)
    fa[0], fd[0], fr[0] = (np.nan, 0.5), 0, 0x7FC00001              # element 0 always: a NaN position, a NaN reward
    if M > 8:
        fa[M // 2], fd[M // 2], fr[M // 2] = (0.5, np.inf), 0, 0xFFC12345
        fb[M // 3] = (np.nan, np.nan)
        fb[M - 1] = fa[M - 2] = (wall // W + 0.5, wall % W + 0.5)     # env (M - 1) % N may have other walls: still a cell
        fa[M // 4], fd[M // 4] = (-0.5, 0.5), 1                       # done and outside: shaped only under the flag
    age = rng.integers(-2, 4 * c["P"], (T, N)).astype(np.int32)
    age.reshape(-1)[:: max(1, M // 7)] = 0
    init = np.array([H - 0.5, 0.25], np.float32)
    return dict(before=before, after=after, age=age, init=init, done=done, reward=reward, T=T)


def run_shape(c, r, period, gamma, scale, flags, want=(True, True, True), off=(0, 0, 0), in_place=False, pad=0,
              with_age=True, with_reward=True):
    """mg_nav_shape through the front end; outputs inside 0xA5 buffers whose borders are checked.  -> host outputs,
    None for an output that was not asked for."""
    W, H, N, T = c["W"], c["H"], c["N"], r["T"]
    d = c["dist"][period]
    if pad:
        full = torch.full(d.shape[:-1] + (W * H + pad,), 0x5A5A, dtype=torch.int16, device=DEV).view(torch.uint16)
        dist = full[..., :W * H]
        dist.copy_(dev(d))
    else:
        dist = dev(d)
    shape = (T, N)
    boxes = [Boxed(T * N, dt, o, shape) for dt, o in zip((torch.float32, torch.float32, torch.uint8), off)]
    reward = dev(r["reward"]) if with_reward else None
    if in_place:
        boxes[0].view.copy_(reward)
        reward = boxes[0].view
    outs = [b.view if w else False for b, w in zip(boxes, want)]
    got = nav().shape(dist, dev(r["before"]), dev(r["after"]), W, H, reward=reward, age=dev(r["age"]) if with_age else None,
                      init_pos=dev(r["init"]) if with_age else None, done=dev(r["done"]) if flags & ZT else None,
                      scale=scale, gamma=gamma, zero_terminal=bool(flags & ZT), out=outs[0], shaping_out=outs[1],
                      mask_out=outs[2])
    for g, b, w in zip(got, boxes, want):
        assert (g is b.view) if w else (g is None and b.untouched())
        assert b.borders_intact()
    if pad:
        assert (host(full.view(torch.int16))[..., W * H:] == 0x5A5A).all()
    return tuple(host(g) for g in got)


def ref_shape(c, r, period, gamma, scale, flags, dists=None, with_age=True):
    db, da = dists if dists is not None else shape_ref.distances(
        c["dist"][period], r["before"], r["after"], c["W"], c["H"], r["age"] if with_age else None,
        r["init"] if with_age else None)
    f, mask = shape_ref.terms(db, da, r["done"], scale, gamma, bool(flags & ZT))
    return shape_ref.apply(r["reward"], f, mask), f, mask


# ------------------------------------------------------------------------------------------------ mg_nav_shape
@pytest.mark.parametrize("T", [1, 7, 40])
@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("kind", [(5, 9), (9, 4), "twoarmy"], ids=["5x9", "9x4", "twoarmy"])
def test_shape_equals_the_reference(kind, N, T):
    c = case(kind, N)
    r = rollout(c, T, 100 * N + T)
    seen = set()
    for period in (1, c["P"]):
        dists = shape_ref.distances(c["dist"][period], r["before"], r["after"], c["W"], c["H"], r["age"], r["init"])
        for flags in (0, ZT):
            for gamma, scale in ARITH:
                want = ref_shape(c, r, period, gamma, scale, flags, dists)
                got = run_shape(c, r, period, gamma, scale, flags)
                for g, w, name in zip(got, want, ("reward_out", "shaping", "mask")):
                    assert same(g, w), (name, period, flags, gamma, np.flatnonzero(bits(g) != bits(w))[:8])
                seen |= set(want[2].reshape(-1).tolist())
    assert bits(got[0]).reshape(-1)[0] == 0x7FC00001                  # the NaN reward of an unshaped element, untouched
    assert seen == {0, 1} or T * N < 8


def test_shape_without_age_and_positions_as_they_stand():
    c = case((5, 9), 3)
    r = rollout(c, 40, 7)
    want = ref_shape(c, r, 1, 0.99, 0.01, ZT, with_age=False)
    got = run_shape(c, r, 1, 0.99, 0.01, ZT, with_age=False)
    assert all(same(g, w) for g, w in zip(got, want))
    aged = ref_shape(c, r, 1, 0.99, 0.01, ZT)
    assert not same(aged[1], want[1])                                 # the age rule does move acting positions here


@pytest.mark.parametrize("kind,N,T", [((9, 4), 3, 7), ("twoarmy", 65, 40)], ids=["21", "2600"])
def test_shape_outputs_absent_in_place_misaligned_and_padded(kind, N, T):
    c = case(kind, N)
    r = rollout(c, T, 3)
    period, gamma, scale = c["P"], 0.99, 0.01
    want = ref_shape(c, r, period, gamma, scale, ZT)
    for absent in range(3):                                           # each nullable output absent in turn
        w = tuple(k != absent for k in range(3))
        got = run_shape(c, r, period, gamma, scale, ZT, want=w)
        assert all(g is None if not k else same(g, x) for g, x, k in zip(got, want, w)), absent
    got = run_shape(c, r, period, gamma, scale, ZT, want=(False, True, True), with_reward=False)     # reward NULL
    assert got[0] is None and same(got[1], want[1]) and same(got[2], want[2])
    for off_f in range(4):                                            # in place against out of place, at every alignment
        for in_place in (False, True):
            got = run_shape(c, r, period, gamma, scale, ZT, off=(off_f, (off_f + 1) % 4, 0), in_place=in_place)
            assert all(same(g, x) for g, x in zip(got, want)), (off_f, in_place)
    for off_m in range(1, 16):                                        # the mask at every byte offset, the floats moving along
        got = run_shape(c, r, period, gamma, scale, ZT, off=(off_m % 4, (3 * off_m) % 4, off_m))
        assert all(same(g, x) for g, x in zip(got, want)), off_m
    for p in (1, period):                                             # dist_pitch above W * H
        got = run_shape(c, r, p, gamma, scale, 0, pad=5, off=(1, 2, 3))
        assert all(same(g, x) for g, x in zip(got, ref_shape(c, r, p, gamma, scale, 0))), p


def test_shape_of_an_empty_rollout_launches_nothing():
    c = case((5, 9), 3)
    e = torch.empty((0, 3, 2), dtype=torch.float32, device=DEV)
    out, f, m = nav().shape(dev(c["dist"][1]), e, e, 5, 9, reward=torch.empty((0, 3), dtype=torch.float32, device=DEV))
    assert out.shape == f.shape == m.shape == (0, 3) and m.dtype == torch.uint8


# ------------------------------------------------------------------------------------------------ mg_nav_goal_shape
_GOAL_CASES = {}


def goal_case(W, H, N):
    """Random worlds (every type code, doors in all states), a pool of three goal cells per env -- whatever comes, walls
    included -- and one rollout of positions; the memo of reference fields is shared by every test on the case."""
    key = (W, H, N)
    if key not in _GOAL_CASES:
        rng = np.random.default_rng(13 * W + 41 * H + N)
        ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
        for n in range(N):
            ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.3)[n % 3])
            ty[n][[5, W + 7]] = 2                                     # every env has a wall, also the one drawn without
        pool = np.stack([rng.permutation(W * H)[:3] for _ in range(N)])
        pool[0, 2] = 5                                                # a goal on a wall
        c = dict(W=W, H=H, N=N, P=1, ty=ty, st=st, pool=pool, memo={}, pass_types=nav_ref.PASS_DEFAULT)
        c["roll"] = rollout(c, 24, 5)
        for a in (ty, st, pool):
            a.setflags(write=False)
        _GOAL_CASES[key] = c
    return _GOAL_CASES[key]


def records(c, R, seed):
    """R records as ppo_her_relabel emits them: runs of consecutive steps of one env under one goal of its pool, the last
    record of a run done; then, from 16 records on, the records that name nothing."""
    rng = np.random.default_rng(seed)
    W, H, N, T = c["W"], c["H"], c["N"], c["roll"]["T"]
    t, n, g, done = [], [], [], []
    while len(t) < R:
        L = int(min(R - len(t), 1 + rng.integers(0, 18)))
        e = int(rng.integers(0, N))
        t0 = int(rng.integers(0, T))
        t += [(t0 + k) % T for k in range(L)]
        n += [e] * L
        g += [int(c["pool"][e][rng.integers(0, 3)])] * L
        done += [0] * (L - 1) + [1]
    t, n, g = np.array(t, np.int32), np.array(n, np.int32), np.array(g)
    goal = (np.stack([g // W, g % W], 1) + rng.choice([0.0, 0.25, 0.999], (R, 2))).astype(np.float32)
    done = np.array(done, np.uint8)
    if R >= 16:
        t[3], t[5] = -1, T                                            # rec_t outside [0, T)
        n[7], n[9] = -1, N                                            # rec_n outside [0, n_envs)
        t[R - 1] = n[R - 1] = 0x7FFFFFFF
        t[R - 2] = n[R - 2] = -0x80000000
        goal[11], goal[12], goal[13] = (np.nan, 1.0), (H, 0.5), (0.5, -0.25)      # goals that are no cell
        wall = np.flatnonzero(c["ty"][n[14]] == 2)
        if wall.size:
            goal[14] = (wall[0] // W + 0.5, wall[0] % W + 0.5)        # a goal on a wall
    reward = rng.standard_normal(R).astype(np.float32)
    if R >= 16:
        reward.view(np.uint32)[[3, 11]] = (0x7FC00001, 0xFFC12345)    # NaNs on records that name nothing
        reward[[0, 7]] = -0.0
    return dict(t=t, n=n, goal=goal, done=done, reward=reward)


def run_goal(c, rec, gamma, scale, flags, want=(True, True, True), off=(0, 0, 0), in_place=False, doors_open=False):
    r = c["roll"]
    R = len(rec["t"])
    boxes = [Boxed(R, dt, o) for dt, o in zip((torch.float32, torch.float32, torch.uint8), off)]
    reward = dev(rec["reward"])
    if in_place:
        boxes[0].view.copy_(reward)
        reward = boxes[0].view
    outs = [b.view if w else False for b, w in zip(boxes, want)]
    got = nav().goal_shape(dev(c["ty"]), dev(rec["t"]), dev(rec["n"]), dev(rec["goal"]), dev(r["before"]), dev(r["after"]),
                           c["W"], c["H"], reward=reward, done=dev(rec["done"]) if flags & ZT else None,
                           pass_types=c["pass_types"], age=dev(r["age"]), init_pos=dev(r["init"]), state=dev(c["st"]),
                           doors_open=doors_open, scale=scale, gamma=gamma, zero_terminal=bool(flags & ZT), out=outs[0],
                           shaping_out=outs[1], mask_out=outs[2])
    for g, b, w in zip(got, boxes, want):
        assert (g is b.view) if w else (g is None and b.untouched())
        assert b.borders_intact()
    return tuple(host(g) for g in got)


def ref_goal(c, rec, gamma, scale, flags, doors_open=False):
    r = c["roll"]
    memo = c["memo"].setdefault(doors_open, {})
    return shape_ref.goal_shape(c["ty"], c["st"], c["W"], c["H"], rec["t"], rec["n"], rec["goal"], r["before"], r["after"],
                                rec["reward"], rec["done"], r["age"], r["init"], c["pass_types"],
                                flags | (nav_ref.DOORS_OPEN if doors_open else 0), scale, gamma, memo)


@pytest.mark.parametrize("R", [0, 1, 1023, 1025, 1041, 2100])
def test_goal_shape_equals_the_reference_in_any_order(R):
    c = goal_case(17, 17, 3)
    rec = records(c, R, R)
    rng = np.random.default_rng(R + 1)
    perm = rng.permutation(R)
    shuffled = {k: v[perm] for k, v in rec.items()}
    for i, (flags, (gamma, scale)) in enumerate([(0, ARITH[0]), (ZT, ARITH[1])]):
        want = ref_goal(c, rec, gamma, scale, flags)
        got = run_goal(c, rec, gamma, scale, flags, off=(i, 2 * i + 1, 5 * i))
        assert all(same(g, w) for g, w in zip(got, want)), [np.flatnonzero(bits(g) != bits(w))[:8] for g, w in zip(got, want)]
        again = run_goal(c, shuffled, gamma, scale, flags, in_place=True)          # a seeded shuffle, in place
        assert all(same(a, g[perm]) for a, g in zip(again, got))
    if R >= 16:
        bad = [3, 5, 7, 9, 11, 12, 13, 14, R - 1, R - 2]
        assert not got[2][bad].any() and not got[1][bad].any()        # unshaped: mask 0, F = +0.0 ...
        assert same(got[0][bad], rec["reward"][bad])                  # ... and the reward as it came, NaN payloads included
        assert got[2].any()


def test_goal_shape_small_world_doors_and_absent_outputs():
    c = goal_case(9, 4, 3)
    rec = records(c, 1041, 2)
    for doors_open in (False, True):
        want = ref_goal(c, rec, 0.99, 0.01, ZT, doors_open)
        for absent in range(3):
            w = tuple(k != absent for k in range(3))
            got = run_goal(c, rec, 0.99, 0.01, ZT, want=w, off=(3, 1, 9), doors_open=doors_open)
            assert all(g is None if not k else same(g, x) for g, x, k in zip(got, want, w)), (doors_open, absent)
    assert want[2].any() and not want[2].all()


@pytest.mark.parametrize("W,H", [(9, 4), (17, 17)])
def test_one_goal_per_env_equals_field_then_shape(W, H):
    """The invariant, kernel to kernel: mg_nav_field from the goal, then mg_nav_shape on the same elements."""
    N = 3
    c = goal_case(W, H, N)
    r = c["roll"]
    T = r["T"]
    rng = np.random.default_rng(W)
    gc = c["pool"][:, 0]
    gx, gy = (gc % W).astype(np.int32), (gc // W).astype(np.int32)
    field = nav().distance_field(dev(c["ty"]), dev(c["st"]), W, H, goal=(dev(gx), dev(gy)))[0]
    order = rng.permutation(T * N)
    order = order[np.argsort(order % N, kind="stable")]               # runs of one env, steps in any order
    t, n = (order // N).astype(np.int32), (order % N).astype(np.int32)
    rec = dict(t=t, n=n, goal=np.stack([gy[n] + 0.5, gx[n] + 0.25], 1).astype(np.float32), done=r["done"][t, n],
               reward=r["reward"][t, n])
    for flags in (0, ZT):
        fo, ff, fm = nav().shape(field, dev(r["before"]), dev(r["after"]), W, H, reward=dev(r["reward"]), age=dev(r["age"]),
                                 init_pos=dev(r["init"]), done=dev(r["done"]), scale=0.01, gamma=0.99,
                                 zero_terminal=bool(flags))
        got = run_goal(c, rec, 0.99, 0.01, flags)
        for g, w in zip(got, (fo, ff, fm)):
            assert same(g, host(w)[t, n])
        assert got[2].any()


# ------------------------------------------------------------------------------------------------ argument rejection
def test_bad_arguments_launch_nothing():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    v = lambda x: None if x is None else C.c_void_p(x)                                     # noqa: E731
    W, H, N, T, R = 5, 4, 3, 2, 6
    f32, u8 = torch.float32, torch.uint8
    dist = torch.zeros((N, 2, W * H + 1), dtype=torch.int16, device=DEV)
    ty = torch.ones((N, W * H), dtype=u8, device=DEV)
    pos = torch.zeros((T + 1, N, 2), dtype=f32, device=DEV)
    age = torch.ones((T + 1, N), dtype=torch.int32, device=DEV)
    init = torch.zeros(4, dtype=f32, device=DEV)
    done = torch.zeros(T * N + R, dtype=u8, device=DEV)
    reward = torch.zeros(T * N + R + 1, dtype=f32, device=DEV)
    rt = torch.zeros(R + 1, dtype=torch.int32, device=DEV)
    goal = torch.zeros((R + 1, 2), dtype=f32, device=DEV)
    outs = [Boxed(T * N + R + 2, dt) for dt in (f32, f32, u8)]
    o, f, m = (b.view.data_ptr() for b in outs)
    nan, inf = float("nan"), float("inf")

    def shape(a):
        return lib.mg_nav_shape(v(a["dist"]), a["pitch"], a["P"], a["n"], a["W"], a["H"], v(a["pb"]), v(a["pa"]), v(a["age"]),
                                v(a["init"]), v(a["done"]), v(a["reward"]), a["T"], a["scale"], a["gamma"], a["flags"],
                                v(a["out"]), v(a["f"]), v(a["mask"]), None)

    def goal_shape(a):
        return lib.mg_nav_goal_shape(v(a["type"]), v(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"],
                                     v(a["t"]), v(a["rn"]), v(a["goal"]), v(a["done"]), v(a["reward"]), a["R"], v(a["pb"]),
                                     v(a["pa"]), v(a["age"]), v(a["init"]), a["T"], a["scale"], a["gamma"], v(a["out"]),
                                     v(a["f"]), v(a["mask"]), None)

    common = dict(n=N, W=W, H=H, pb=pos.data_ptr(), pa=pos.data_ptr() + 8, age=age.data_ptr(), init=init.data_ptr(),
                  done=done.data_ptr(), reward=reward.data_ptr(), T=T, scale=0.5, gamma=0.99, flags=ZT, out=o, f=f, mask=m)
    good = dict(common, dist=dist.data_ptr(), pitch=0, P=1)
    bad_common = [dict(pb=None), dict(pa=None), dict(n=0), dict(n=-1), dict(W=0), dict(H=0), dict(W=33), dict(H=33),
                  dict(T=-1), dict(pb=common["pb"] + 4), dict(pa=common["pa"] + 4), dict(age=common["age"] + 2),
                  dict(init=common["init"] + 1), dict(init=None),                       # age without init_pos
                  dict(reward=common["reward"] + 2), dict(out=o + 2), dict(f=f + 1),    # float arrays off 4 bytes
                  dict(out=None, f=None, mask=None),                                     # no output
                  dict(reward=None),                                                     # reward_out without reward
                  dict(done=None),                                                       # the terminal flag without done
                  dict(flags=4), dict(flags=8 | ZT), dict(flags=-1),                     # unknown flag bits
                  dict(scale=nan), dict(scale=inf), dict(scale=-inf), dict(gamma=nan), dict(gamma=inf)]
    bad_shape = bad_common + [dict(dist=None), dict(dist=good["dist"] + 1), dict(pitch=-1), dict(pitch=W * H - 1),
                              dict(P=0), dict(P=17), dict(P=-1), dict(P=2, age=None, init=None), dict(P=2, age=None),
                              dict(T=1 << 30, n=1 << 10),
                              dict(flags=1), dict(flags=3)]                              # the doors are the field's business
    for kw in bad_shape:
        assert shape(dict(good, **kw)) == -1, kw
    ggood = dict(common, type=ty.data_ptr(), state=None, pass_types=nav_ref.PASS_DEFAULT, t=rt.data_ptr(), rn=rt.data_ptr(),
                 goal=goal.data_ptr(), R=R)
    bad_goal = bad_common + [dict(type=None), dict(t=None), dict(rn=None), dict(goal=None), dict(pass_types=0x10000),
                             dict(t=ggood["t"] + 2), dict(rn=ggood["rn"] + 1), dict(goal=ggood["goal"] + 2), dict(R=-1),
                             dict(R=1 << 40)]
    for kw in bad_goal:
        assert goal_shape(dict(ggood, **kw)) == -1, kw
    assert shape(dict(good, T=0)) == 0 and goal_shape(dict(ggood, R=0)) == 0               # nothing to do: ok, no launch
    torch.cuda.synchronize()
    assert all(b.untouched() for b in outs)
    # and the good calls launch: every element acts on cell 0 of an all-zero field / with goal cell 0, and stays there
    assert shape(good) == 0 and shape(dict(good, P=2, pitch=W * H + 1, flags=0, done=None, reward=None, out=None)) == 0
    torch.cuda.synchronize()
    assert all(b.borders_intact() for b in outs)
    assert host(outs[2].view)[:T * N].tolist() == [1] * (T * N) and not host(outs[1].view)[:T * N].any()
    assert goal_shape(dict(ggood, flags=ZT | 1, age=None, init=None, mask=m + 1)) == 0
    torch.cuda.synchronize()
    assert host(outs[2].view)[1:R + 1].tolist() == [1] * R and all(b.borders_intact() for b in outs)


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(N, T, max_steps):
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(5)
    eng = TwoarmyEngine(6, N, 17, seed=9981, max_steps=max_steps)
    agent = PPO()
    agent.to(eng.device).use_nhwc()
    return VecPPOTrainer(agent, eng, rollout_steps=T, minibatch=64, value_chunk=64), eng


@pytest.mark.parametrize("timed", [False, True], ids=["static", "timed"])
def test_trainer_shapes_reward_train_and_records_and_nothing_else(timed):
    N, T, scale = 8, 16, 0.05
    plain, e0 = _trainer(N, T, 6)
    shaped, e1 = _trainer(N, T, 6)
    assert shaped.reward_train is shaped.reward
    shaped.enable_shaping(scale, hindsight=True, timed=timed)
    assert shaped.reward_train is not shaped.reward
    with pytest.raises(RuntimeError, match="shape_potential"):
        shaped.shaping_stats()
    gamma = np.float32(shaped.agent.gamma)
    sched = nav().twoarmy_schedule(blocks=True).numpy().astype(np.int64)
    static = nav_ref.PASS_DEFAULT | BALL
    for u in range(2):
        for tr in (plain, shaped):
            tr.collect()
            tr.shape_rewards()
        for k in ("reward", "action", "pos", "term", "trunc", "age"):
            assert torch.equal(getattr(plain, k), getattr(shaped, k)), (u, k)
        reward = host(shaped.reward)
        assert same(host(shaped.reward_train), reward)                # the copy the potential is added to
        if u == 1:
            with pytest.raises(RuntimeError, match="relabel\\(\\) before shape_potential"):
                shaped.shape_potential(expect_her=True)               # the caller relabels this rollout, and has not yet
        plain.relabel()
        shaped.relabel()
        h = {k: host(v) for k, v in shaped.her.items()}
        assert all(torch.equal(plain.her[k], shaped.her[k]) for k in ("t", "n", "goal", "reward", "done"))
        R = len(h["t"])
        assert R > 0
        ty = shaped.engine.get_state()[0].reshape(N, 289)
        shaped.shape_potential(expect_her=True)
        with pytest.raises(RuntimeError, match="ran already"):
            shaped.shape_potential()
        with pytest.raises(RuntimeError, match="relabel\\(\\) before shape_potential"):
            shaped.relabel()
        before, after = host(shaped.pos[3:3 + T]), host(shaped.pos[4:4 + T])
        age, init = host(shaped.age[:-1]), host(shaped.init_pos)
        if timed:
            dist = tref.fields(ty, None, 17, 17, sched, 6, static)[0]
        else:
            dist = nav_ref.fields(ty, None, 17, 17, static)[0]
        want = shape_ref.shape(dist, before, after, 17, 17, reward, age, init, None, scale, gamma, 0)
        assert same(host(shaped.reward_train), want[0]) and same(host(shaped.shape_f), want[1])
        assert same(host(shaped.shape_mask), want[2]) and want[2].any()
        hwant = shape_ref.goal_shape(ty, None, 17, 17, h["t"], h["n"], h["goal"], before, after, h["reward"], h["done"], age,
                                     init, static, 0, scale, gamma)
        assert same(host(shaped.her["reward"]), hwant[0]) and same(host(shaped.her_shape_f), hwant[1])
        assert same(host(shaped.her_shape_mask), hwant[2]) and hwant[2].any()
        assert same(host(shaped.reward), reward) and torch.equal(plain.reward, shaped.reward)         # extrinsic as it was
        assert same(host(plain.her["reward"]), h["reward"])
        ss = shaped.shaping_stats()
        m, hm = want[2] != 0, hwant[2] != 0
        assert ss["mean"] == pytest.approx(float(want[1][m].astype(np.float64).mean()), rel=1e-9, abs=1e-12)
        assert ss["unshaped"] == pytest.approx(1.0 - m.mean()) and ss["her_unshaped"] == pytest.approx(1.0 - hm.mean())
        assert ss["her_mean"] == pytest.approx(float(hwant[1][hm].astype(np.float64).mean()), rel=1e-9, abs=1e-12)
        done = (h["done"] != 0) & hm                                  # a relabelled end stands on its goal: -phi(s) alone
        assert done.any() and same(hwant[1][done], np.float32(0.0) - shape_ref.phi(scale, shape_ref.goal_distances(
            ty, None, 17, 17, h["t"], h["n"], h["goal"], before, after, age, init, static)[0][done]))
        for tr in (plain, shaped):
            tr.carry_over()
            tr.her = None
    e0.close(); e1.close()
