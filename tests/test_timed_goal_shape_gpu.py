"""mg_nav_timed_goal_shape on the device (include/minigrid_nav.h): potential-based shaping of records that each name their
own goal in a world whose blockers move, against timed_goal_shape_ref.py (a queue BFS over (cell, phase) per record's env
and goal, the float rule of shape_ref.py) and against the kernels it must agree with, through the torch front end, the C
ABI, TwoarmyEngine and VecPPOTrainer.  Every comparison is bit for bit: float outputs are compared as uint32 views.  NaN
rewards sit on records that are unshaped by construction; -0.0 rewards sit anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nav_ref
import shape_ref
import timed_goal_moves_ref as tgref
import timed_goal_shape_ref as tsref
import timed_nav_ref as tref
import visit_ref
from nav_util import Boxed, all_same, bits, dev, host, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = tref.UNREACHABLE
ZT = tsref.ZERO_TERMINAL
BALL = 1 << 6
STATIC = nav_ref.PASS_DEFAULT | BALL                                  # balls enterable: only the schedule blocks
CHUNK = 1024                                                          # records per workgroup
ARITH = [(1.0, 0.125), (0.99, 0.01)]                                  # (gamma, scale): exact / every operation rounds


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def floods(W, H, P):
    """The header's formula from the header's byte count."""
    fixed = int(re.search(r"#define MG_NAV_TIMED_GOAL_SHAPE_LDS (\d+)", open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()).group(1))
    cells = (W * H + 7) & ~7
    return next((f for f in (8, 4, 2) if fixed + f * P * cells * 2 <= 65536), 1)


# ------------------------------------------------------------------------------------------------ worlds, rollouts, records
_CASES = {}


def v6_planes(N):
    from twoarmy_amd.engine import TwoarmyEngine
    eng = TwoarmyEngine(6, N, 17, seed=9981)
    eng.reset()
    ty = eng.get_state()[0].reshape(N, 289).copy()
    eng.close()
    return ty


def case(W, H, P, N=2):
    """Worlds of one size and period with a per-env schedule (every bit of all 32 columns drawn: those at or above the width
    are to be ignored), a pool of goal cells per env -- whatever comes, walls included -- and one rollout of positions and
    clocks (ages <= 0 and far beyond P); the memo of reference fields is shared by every test on the case.  17 x 17 is the
    v6 map, at P = 6 under the schedule of its balls."""
    key = (W, H, P, N)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * W + 10 * H + P)
    if (W, H) == (17, 17):
        ty, st, pass_types = v6_planes(N), None, STATIC
    else:
        ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
        for n in range(N):
            ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.1, 0.25)[n % 2])
        pass_types = nav_ref.PASS_DEFAULT
    sched = np.stack([tref.random_schedule(rng, P, H, 0.08 if P > 1 else 0.03) for _ in range(N)])
    if (W, H, P) == (17, 17, 6):
        sched[:] = nav().twoarmy_schedule(blocks=True).numpy().astype(np.uint32) | (sched & ~np.uint32((1 << 17) - 1))
    pool = np.stack([rng.permutation(W * H)[:2] for _ in range(N)])
    walls = np.flatnonzero(ty[0] == 2)
    pool[0, 1] = walls[0] if walls.size else 0                        # a goal on a wall
    c = dict(W=W, H=H, N=N, P=P, ty=ty, st=st, sched=sched, pool=pool, memo={}, pass_types=pass_types)
    c["roll"] = rollout(c, 24, 5)
    for a in (ty, sched, pool):
        a.setflags(write=False)
    _CASES[key] = c
    return c


def rollout(c, T, seed):
    """Seeded random walks, one per env: a move or a wait per step, walls and the world's edge no obstacle, so positions on
    walls, on blocked cells and outside the world come by themselves; a NaN and an infinity are planted."""
    W, H, N, P = c["W"], c["H"], c["N"], c["P"]
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.integers(0, W, N), rng.integers(0, H, N)], 1)
    walk = np.zeros((T + 1, N, 2), np.float32)
    for t in range(T + 1):
        walk[t, :, 0], walk[t, :, 1] = xy[:, 1] + rng.choice([0.0, 0.5, 0.999], N), xy[:, 0] + rng.choice([0.0, 0.5, 0.999], N)
        xy = xy + np.array([(-1, 0), (1, 0), (0, -1), (0, 1), (0, 0)])[rng.integers(0, 5, N)]
        xy = np.clip(xy, -1, (W, H))
    before, after = walk[:-1].copy(), walk[1:].copy()
    M = T * N
    after.reshape(-1, 2)[0] = (np.nan, 0.5)
    after.reshape(-1, 2)[M // 2] = (0.5, np.inf)
    before.reshape(-1, 2)[M // 3] = (np.nan, np.nan)
    age = rng.integers(-2, 4 * P + 3, (T, N)).astype(np.int32)
    age.reshape(-1)[::7] = 0
    age.reshape(-1)[5] = 0x7FFFFFFF
    init = np.array([H - 0.5, 0.25], np.float32)
    return dict(before=before, after=after, age=age, init=init, T=T)


def records(c, R, seed):
    """R records as ppo_her_relabel emits them: runs of consecutive steps of one env under one goal of its pool, the last
    record of a run done -- one run laid across the first workgroup boundary --; then, from 16 records on, the records that
    name nothing, among them the -0.0 and NaN-payload rewards."""
    rng = np.random.default_rng(seed)
    W, H, N, T = c["W"], c["H"], c["N"], c["roll"]["T"]
    t, n, g, done = [], [], [], []
    while len(t) < R:
        L = int(min(R - len(t), 1 + rng.integers(0, 18)))
        if len(t) < CHUNK - 8 <= len(t) + L or CHUNK - 8 <= len(t) < CHUNK:
            L = int(min(R - len(t), 40))                              # records 1016 .. 1031 at the least: one run
        e = int(rng.integers(0, N))
        t0 = int(rng.integers(0, T))
        t += [(t0 + k) % T for k in range(L)]
        n += [e] * L
        g += [int(c["pool"][e][rng.integers(0, c["pool"].shape[1])])] * L
        done += [0] * (L - 1) + [1]
    t, n, g = np.array(t, np.int32), np.array(n, np.int32), np.array(g)
    goal = (np.stack([g // W, g % W], 1) + rng.choice([0.0, 0.25, 0.999], (R, 2))).astype(np.float32)
    done = np.array(done, np.uint8)
    reward = rng.standard_normal(R).astype(np.float32)
    if R >= 16:
        t[3], t[5] = -1, T
        n[7], n[9] = -1, N
        t[R - 1] = n[R - 1] = 0x7FFFFFFF
        t[R - 2] = n[R - 2] = -0x80000000
        goal[11], goal[12], goal[13] = (np.nan, 1.0), (H, 0.5), (0.5, -0.25)
        reward.view(np.uint32)[[3, 11]] = (0x7FC00001, 0xFFC12345)    # NaN payloads on records that name nothing
        reward[[0, 7]] = -0.0
    return dict(t=t, n=n, goal=goal, done=done, reward=reward)


BAD = [3, 5, 7, 9, 11, 12, 13]


def run(c, rec, gamma, scale, flags, want=(True, True, True), off=(0, 0, 0), in_place=False, shared=False, doors_open=False,
        with_reward=True):
    """mg_nav_timed_goal_shape through the front end; outputs inside 0xA5 buffers whose borders are checked.  -> host
    outputs, None for an output that was not asked for."""
    r = c["roll"]
    R = len(rec["t"])
    boxes = [Boxed(R, dt, o) for dt, o in zip((torch.float32, torch.float32, torch.uint8), off)]
    reward = dev(rec["reward"]) if with_reward else None
    if in_place:
        boxes[0].view.copy_(reward)
        reward = boxes[0].view
    outs = [b.view if w else False for b, w in zip(boxes, want)]
    sched = dev((c["sched"][0] if shared else c["sched"]).view(np.int32))
    got = nav().timed_goal_shape(dev(c["ty"]), dev(rec["t"]), dev(rec["n"]), dev(rec["goal"]), dev(r["before"]),
                                 dev(r["after"]), c["W"], c["H"], sched, dev(r["age"]), dev(r["init"]), reward=reward,
                                 done=dev(rec["done"]) if flags & ZT else None, pass_types=c["pass_types"], state=dev(c["st"]),
                                 doors_open=doors_open, scale=scale, gamma=gamma, zero_terminal=bool(flags & ZT),
                                 out=outs[0], shaping_out=outs[1], mask_out=outs[2])
    for g, b, w in zip(got, boxes, want):
        assert (g is b.view) if w else (g is None and b.untouched())
        assert b.borders_intact()
    return tuple(host(g) for g in got)


def ref(c, rec, gamma, scale, flags, shared=False, doors_open=False):
    r = c["roll"]
    memo = c["memo"].setdefault((shared, doors_open), {})
    return tsref.timed_goal_shape(c["ty"], c["st"], c["W"], c["H"], c["sched"][0] if shared else c["sched"], c["P"], rec["t"],
                                  rec["n"], rec["goal"], r["before"], r["after"], r["age"], r["init"], rec["reward"],
                                  rec["done"], c["pass_types"], flags | (nav_ref.DOORS_OPEN if doors_open else 0), scale,
                                  gamma, memo)


def fused(c, rec, gamma, scale, flags):
    """What a fused multiply-add would give for F: gamma * phi_after - phi_before rounded once."""
    r = c["roll"]
    db, da = tsref.goal_distances(c["ty"], c["st"], c["W"], c["H"], c["sched"], c["P"], rec["t"], rec["n"], rec["goal"],
                                  r["before"], r["after"], r["age"], r["init"], c["pass_types"], 0, c["memo"].setdefault((False, False), {}))
    pa, pb = shape_ref.phi(scale, np.where(da == U, 0, da)).astype(np.float64), shape_ref.phi(scale, np.where(db == U, 0, db))
    return (np.float64(np.float32(gamma)) * pa - pb.astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ sizes and periods
@pytest.mark.parametrize("P", [1, 2, 6, 16])
@pytest.mark.parametrize("W,H", [(5, 4), (17, 17), (32, 16), (32, 32)])
def test_every_size_and_period_equals_the_reference(W, H, P):
    c = case(W, H, P)
    assert nav().timed_goal_shape_floods(W, H, P) == floods(W, H, P)
    rec = records(c, 1041, W + P)                                     # two workgroups, a run across their boundary
    seen = set()
    for i, (flags, (gamma, scale)) in enumerate([(0, ARITH[0]), (ZT, ARITH[1])]):
        for shared in (False, True):
            want = ref(c, rec, gamma, scale, flags, shared)
            got = run(c, rec, gamma, scale, flags, off=(i, 2 * i + 1, 5 * i), shared=shared)
            assert all_same(got, want), (shared, [np.flatnonzero(bits(g) != bits(w))[:8] for g, w in zip(got, want)])
            seen |= set(want[2].tolist())
    assert seen == {0, 1}
    assert not got[2][BAD].any() and not got[1][BAD].any() and not np.signbit(got[1][BAD]).any()
    assert same(got[0][BAD], rec["reward"][BAD])                      # -0.0 and the NaN payloads as they came


def test_the_flood_counts_the_sizes_select():
    got = {(W, H, P): nav().timed_goal_shape_floods(W, H, P) for W, H in ((5, 4), (17, 17), (32, 16), (32, 32))
           for P in (1, 2, 6, 16)}
    assert [got[5, 4, P] for P in (1, 2, 6, 16)] == [8, 8, 8, 8] and [got[17, 17, P] for P in (1, 2, 6, 16)] == [8, 8, 8, 4]
    assert [got[32, 16, P] for P in (1, 2, 6, 16)] == [8, 8, 4, 2] and [got[32, 32, P] for P in (1, 2, 6, 16)] == [8, 8, 2, 1]


# ------------------------------------------------------------------------------------------------ record counts and order
@pytest.mark.parametrize("R", [0, 1, 1023, 1024, 1025, 2049])
def test_record_counts_in_any_order(R):
    c = case(17, 17, 6)
    rec = records(c, R, R)
    perm = np.random.default_rng(R + 1).permutation(R)
    shuffled = {k: v[perm] for k, v in rec.items()}
    for i, (flags, (gamma, scale)) in enumerate([(0, ARITH[1]), (ZT, ARITH[0]), (ZT, ARITH[1])]):
        want = ref(c, rec, gamma, scale, flags)
        got = run(c, rec, gamma, scale, flags, off=(i + 1, 3 - i, 7 * i + 1))
        assert all_same(got, want), [np.flatnonzero(bits(g) != bits(w))[:8] for g, w in zip(got, want)]
        again = run(c, shuffled, gamma, scale, flags, in_place=True)                  # a seeded shuffle, in place
        assert all(same(a, g[perm]) for a, g in zip(again, got))
    if R >= 1023:
        assert got[2].any() and not got[2].all()
        assert not same(fused(c, rec, *ARITH[1], 0)[want[2] != 0], ref(c, rec, *ARITH[1], 0)[1][want[2] != 0])   # an fma would show
    if R >= 16:
        bad = BAD + [R - 1, R - 2]
        assert not got[2][bad].any() and same(got[0][bad], rec["reward"][bad])
    if R > CHUNK + 40:
        k = slice(CHUNK - 8, CHUNK + 8)                               # one run across the workgroup boundary
        assert len(set(rec["n"][k].tolist())) == 1 and len({tuple(g) for g in np.floor(rec["goal"][k]).tolist()}) == 1


def test_outputs_absent_in_place_and_at_every_misalignment():
    c = case(32, 16, 6)
    rec = records(c, 1041, 2)
    gamma, scale = ARITH[1]
    want = ref(c, rec, gamma, scale, ZT)
    assert want[2].any() and not want[2].all()
    for absent in range(3):                                           # each nullable output absent in turn
        w = tuple(k != absent for k in range(3))
        got = run(c, rec, gamma, scale, ZT, want=w, off=(3, 1, 9))
        assert all(g is None if not k else same(g, x) for g, x, k in zip(got, want, w)), absent
    got = run(c, rec, gamma, scale, ZT, want=(False, True, True), with_reward=False)  # rec_reward NULL
    assert got[0] is None and same(got[1], want[1]) and same(got[2], want[2])
    for off_f in range(4):                                            # in place against out of place, at every alignment
        for in_place in (False, True):
            got = run(c, rec, gamma, scale, ZT, off=(off_f, (off_f + 1) % 4, 0), in_place=in_place)
            assert all_same(got, want), (off_f, in_place)
    for off_m in range(1, 16):                                        # the mask at every byte offset, the floats moving along
        got = run(c, rec, gamma, scale, ZT, off=(off_m % 4, (3 * off_m) % 4, off_m))
        assert all_same(got, want), off_m


def test_doors_and_a_padded_schedule_through_the_c_abi():
    from twoarmy_amd import _lib
    c = case(32, 16, 6)
    rec = records(c, 300, 4)
    gamma, scale = ARITH[1]
    assert (c["ty"] == 4).any() and (c["st"][c["ty"] == 4] != 0).any()                # there are closed doors
    want = ref(c, rec, gamma, scale, ZT, doors_open=True)
    assert all_same(run(c, rec, gamma, scale, ZT, doors_open=True), want)
    assert not same(want[1], ref(c, rec, gamma, scale, ZT)[1])
    # the C ABI with blocked_env_stride above P * height: the words between two envs' schedules are never read as schedule
    r, N, P, H, W, R = c["roll"], c["N"], c["P"], c["H"], c["W"], 300
    pad = np.full((N, P * H + 5), 0xFFFFFFFF, np.uint32)
    pad[:, :P * H] = c["sched"].reshape(N, -1)
    keep = [dev(x) for x in (c["ty"], c["st"], pad.view(np.int32), rec["t"], rec["n"], rec["goal"], rec["done"], rec["reward"],
                             r["before"], r["after"], r["age"], r["init"])]
    boxes = [Boxed(R, dt, o) for dt, o in zip((torch.float32, torch.float32, torch.uint8), (1, 2, 3))]
    p = [C.c_void_p(t.data_ptr()) for t in keep]
    rc = _lib.lib().mg_nav_timed_goal_shape(p[0], p[1], N, W, H, c["pass_types"], ZT, p[2], P * H + 5, P, p[3], p[4], p[5], p[6],
                                            p[7], R, p[8], p[9], p[10], p[11], r["T"], scale, gamma,
                                            *(C.c_void_p(b.view.data_ptr()) for b in boxes), None)
    torch.cuda.synchronize()
    assert rc == 0 and all(b.borders_intact() for b in boxes)
    assert all_same([host(b.view) for b in boxes], ref(c, rec, gamma, scale, ZT))


# ------------------------------------------------------------------------------------------------ the invariants
@pytest.mark.parametrize("W,H,P", [(5, 4, 2), (17, 17, 6), (32, 16, 16)])
def test_one_goal_per_env_equals_timed_field_then_shape(W, H, P):
    """Invariant (a), kernel to kernel: mg_nav_timed_field from the goal, then mg_nav_shape with that period."""
    c = case(W, H, P)
    r, N = c["roll"], c["N"]
    T = r["T"]
    rng = np.random.default_rng(W + P)
    gc = c["pool"][:, 0]
    gx, gy = (gc % W).astype(np.int32), (gc // W).astype(np.int32)
    sched = dev(c["sched"].view(np.int32))
    field = nav().timed_field(dev(c["ty"]), dev(c["st"]), W, H, sched, c["pass_types"], goal=(dev(gx), dev(gy)))[0]
    order = rng.permutation(T * N)
    order = order[np.argsort(order % N, kind="stable")]               # runs of one env, steps in any order
    t, n = (order // N).astype(np.int32), (order % N).astype(np.int32)
    reward = rng.standard_normal((T, N)).astype(np.float32)
    done = (rng.random((T, N)) < 0.2).astype(np.uint8)
    rec = dict(t=t, n=n, goal=np.stack([gy[n] + 0.5, gx[n] + 0.25], 1).astype(np.float32), done=done[t, n], reward=reward[t, n])
    for flags in (0, ZT):
        want = nav().shape(field, dev(r["before"]), dev(r["after"]), W, H, reward=dev(reward), age=dev(r["age"]),
                           init_pos=dev(r["init"]), done=dev(done), scale=0.01, gamma=0.99, zero_terminal=bool(flags))
        got = run(c, rec, 0.99, 0.01, flags)
        assert all(same(g, host(w)[t, n]) for g, w in zip(got, want))
        assert got[2].any()


@pytest.mark.parametrize("W,H", [(5, 4), (17, 17), (32, 32)])
def test_period_one_with_an_empty_schedule_equals_goal_shape(W, H):
    """Invariant (b), kernel to kernel."""
    c = case(W, H, 1)
    r = c["roll"]
    rec = records(c, 1041, 9)
    zero = torch.zeros((1, H), dtype=torch.int32, device=DEV)
    d = {k: dev(v) for k, v in rec.items()}
    for flags in (0, ZT):
        common = dict(reward=d["reward"], done=d["done"] if flags else None, pass_types=c["pass_types"], state=dev(c["st"]),
                      scale=0.01, gamma=0.99, zero_terminal=bool(flags))
        want = nav().goal_shape(dev(c["ty"]), d["t"], d["n"], d["goal"], dev(r["before"]), dev(r["after"]), W, H,
                                age=dev(r["age"]), init_pos=dev(r["init"]), **common)
        got = nav().timed_goal_shape(dev(c["ty"]), d["t"], d["n"], d["goal"], dev(r["before"]), dev(r["after"]), W, H, zero,
                                     dev(r["age"]), dev(r["init"]), **common)
        assert all(same(host(g), host(w)) for g, w in zip(got, want))
        assert host(got[2]).any()


@pytest.mark.parametrize("W,H,P", [(17, 17, 6), (32, 32, 16)])
def test_a_shaped_record_has_a_move_set_and_the_same_acting_distance(W, H, P):
    """Invariant (c), kernel to kernel: mask != 0 implies a non-empty move set of mg_nav_timed_goal_moves, whose acting_dist
    is the distance the shaping used -- read back from F where gamma = 0: F = -phi_before = scale * d exactly."""
    c = case(W, H, P)
    r = c["roll"]
    rec = records(c, 1041, 11)
    d = {k: dev(v) for k, v in rec.items()}
    sched = dev(c["sched"].view(np.int32))
    m, ad = nav().timed_goal_moves(dev(c["ty"]), d["t"], d["n"], d["goal"], dev(r["before"]), W, H, sched, dev(r["age"]),
                                   dev(r["init"]), c["pass_types"], state=dev(c["st"]))
    m, ad = host(m), host(ad.view(torch.int16)).astype(np.int64) & 0xFFFF
    for flags in (0, ZT):
        _, f, mask = run(c, rec, 0.0, 0.125, flags)
        assert mask.any() and (m[mask != 0] != 0).all()
        assert np.array_equal(f[mask != 0], 0.125 * ad[mask != 0].astype(np.float32))
        if flags:                                                     # a done record is shaped iff its acting state is reachable
            assert np.array_equal(mask[rec["done"] != 0] != 0, ad[rec["done"] != 0] != U)


# ------------------------------------------------------------------------------------------------ the longest flood
def test_serpentine_32x32_at_period_16():
    """A corridor that winds through all 32 rows, a blocker in it that is away in one phase of 16 only: distances far above
    255, one flood at a time (the image of 16 phases fills the LDS next to the staging)."""
    W = H = 32
    P = 16
    ty = np.ones((H, W), np.uint8)
    for y in range(1, H, 2):
        ty[y, :] = 2
        ty[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    sched = np.zeros((P, H), np.uint32)
    sched[1:, 16] = 1 << 5                                            # (5, 16) is free at phase 0 only
    ty = ty.reshape(1, -1)
    assert nav().timed_goal_shape_floods(W, H, P) == 1
    cells = np.flatnonzero(ty[0] == 1)
    rng = np.random.default_rng(3)
    T = 64
    cb = rng.choice(cells, T)
    ca = np.where(rng.random(T) < 0.5, cb, np.clip(cb + rng.choice([-1, 1, -W, W], T), 0, W * H - 1))
    before = np.stack([cb // W + 0.5, cb % W + 0.5], -1).astype(np.float32)[:, None]
    after = np.stack([ca // W + 0.5, ca % W + 0.5], -1).astype(np.float32)[:, None]
    age = rng.integers(0, 5 * P, (T, 1)).astype(np.int32)
    init = np.array([0.5, 0.5], np.float32)
    R = 600
    t = np.sort(rng.integers(0, T, R)).astype(np.int32)
    goals = np.array([(H - 2) * W, 0, 16 * W + 5])                    # either end, and the blocker's own cell
    g = goals[np.repeat(np.arange(3), R // 3)]
    rec = dict(t=t, n=np.zeros(R, np.int32), goal=np.stack([g // W + 0.5, g % W + 0.5], 1).astype(np.float32),
               done=(rng.random(R) < 0.1).astype(np.uint8), reward=rng.standard_normal(R).astype(np.float32))
    c = dict(W=W, H=H, N=1, P=P, ty=ty, st=None, sched=sched[None], memo={}, pass_types=nav_ref.PASS_DEFAULT,
             roll=dict(before=before, after=after, age=age, init=init, T=T))
    db, _ = tsref.goal_distances(ty, None, W, H, sched, P, rec["t"], rec["n"], rec["goal"], before, after, age, init,
                                 memo=c["memo"].setdefault((False, False), {}))
    assert db[db != U].max() > 255                                    # 16 rows of 32 cells: no distance for a byte
    for flags, (gamma, scale) in ((0, ARITH[1]), (ZT, ARITH[0])):
        want = ref(c, rec, gamma, scale, flags)
        assert all_same(run(c, rec, gamma, scale, flags, off=(1, 3, 5)), want)
        assert want[2].any() and not want[2].all()


# ------------------------------------------------------------------------------------------------ the point of the feature
def test_records_at_the_door_gap_get_the_timed_potential():
    """v6, records in row 9 (under the gap) and row 8 (the gap) whose goal (8, 6) lies beyond it: the static potential with
    the balls passable rewards the step into a ball, the timed one leaves it unshaped and rewards the wait."""
    ty = v6_planes(1)
    sched = nav().twoarmy_schedule(blocks=True).numpy().astype(np.int64)
    cells = [(x, y) for y in (9, 8) for x in range(6, 11)]
    elems = [(x, y, ax, ay, age) for x, y in cells for ax, ay in ((x, y), (x, y - 1)) for age in range(1, 7)]
    T = len(elems)
    before = np.array([[(y + 0.5, x + 0.5)] for x, y, _, _, _ in elems], np.float32)
    after = np.array([[(ay + 0.5, ax + 0.5)] for _, _, ax, ay, _ in elems], np.float32)
    age = np.array([[a] for *_, a in elems], np.int32)
    init = np.array([15.5, 1.5], np.float32)
    rec_t, rec_n = np.arange(T, dtype=np.int32), np.zeros(T, np.int32)
    goal = np.tile(np.array([[6.5, 8.5]], np.float32), (T, 1))
    reward = np.zeros(T, np.float32)
    gamma, scale = ARITH[1]
    want_t = tsref.timed_goal_shape(ty, None, 17, 17, sched, 6, rec_t, rec_n, goal, before, after, age, init, reward,
                                    pass_types=STATIC, scale=scale, gamma=gamma)
    want_s = shape_ref.goal_shape(ty, None, 17, 17, rec_t, rec_n, goal, before, after, reward, None, age, init, STATIC, 0,
                                  scale, gamma)
    # the reference alone shows the difference
    both = (want_t[2] != 0) & (want_s[2] != 0)
    assert want_s[2].all() and both.any() and (want_t[2] == 0).any()
    assert (bits(want_t[1])[both] != bits(want_s[1])[both]).any()
    into_ball = (want_t[2] == 0) & (after[:, 0, 0] < before[:, 0, 0])                 # a step up that the timed search refuses
    assert into_ball.any() and (want_s[1][into_ball] > 0).all()                       # ... and the static potential rewards
    # a wait that is progress (one transition nearer: about scale) is worth to the static potential what any wait is
    # (phi stays: (1 - gamma) * scale * d, a twentieth of it here)
    waits = both & (after[:, 0, 0] == before[:, 0, 0]) & (want_t[1] > 0.5 * scale)
    assert waits.any() and (want_s[1][waits] < 0.1 * scale).all()
    args = (dev(ty), dev(rec_t), dev(rec_n), dev(goal), dev(before), dev(after), 17, 17)
    got_t = nav().timed_goal_shape(*args, dev(sched.astype(np.int32)), dev(age), dev(init), reward=dev(reward), pass_types=STATIC,
                                   scale=scale, gamma=gamma)
    got_s = nav().goal_shape(*args, reward=dev(reward), pass_types=STATIC, age=dev(age), init_pos=dev(init), scale=scale,
                             gamma=gamma)
    assert all_same([host(g) for g in got_t], want_t) and all_same([host(g) for g in got_s], want_s)


# ------------------------------------------------------------------------------------------------ engine and trainer
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
def test_trainer_shapes_the_records_with_the_timed_potential_and_nothing_else(timed):
    N, T, scale = 8, 16, 0.05
    base, e0 = _trainer(N, T, 6)                                      # the same run without the switch
    shaped, e1 = _trainer(N, T, 6)
    base.enable_shaping(scale, hindsight=True, timed=timed)
    assert shaped.enable_shaping(scale, hindsight=True, timed=timed, hindsight_timed=True) == dict(
        scale=scale, hindsight=True, timed=timed, hindsight_timed=True)
    with pytest.raises(ValueError, match="needs hindsight=True"):
        shaped.enable_shaping(scale, hindsight=False, hindsight_timed=True)
    gamma = np.float32(shaped.agent.gamma)
    sched = nav().twoarmy_schedule(blocks=True).numpy().astype(np.int64)
    for u in range(2):
        for tr in (base, shaped):
            tr.collect()
            tr.shape_rewards()
        if u == 1:
            with pytest.raises(RuntimeError, match="relabel\\(\\) before shape_potential"):
                shaped.shape_potential(expect_her=True)               # the caller relabels this rollout, and has not yet
        base.relabel()
        shaped.relabel()
        h = {k: host(v) for k, v in shaped.her.items()}
        assert all(torch.equal(base.her[k], shaped.her[k]) for k in ("t", "n", "goal", "reward", "done"))
        R = len(h["t"])
        assert R > 0
        ty = shaped.engine.get_state()[0].reshape(N, 289)
        base.shape_potential(expect_her=True)
        shaped.shape_potential(expect_her=True)
        with pytest.raises(RuntimeError, match="ran already"):
            shaped.shape_potential()
        with pytest.raises(RuntimeError, match="relabel\\(\\) before shape_potential"):
            shaped.relabel()
        for k in ("reward", "reward_train", "shape_f", "shape_mask", "action", "pos", "age"):
            assert torch.equal(getattr(base, k), getattr(shaped, k)), (u, k)           # the rollout's half is untouched
        before, after = host(shaped.pos[3:3 + T]), host(shaped.pos[4:4 + T])
        age, init = host(shaped.age[:-1]), host(shaped.init_pos)
        zt = ZT if shaped.agent.use_done_mask else 0
        hwant = tsref.timed_goal_shape(ty, None, 17, 17, sched, 6, h["t"], h["n"], h["goal"], before, after, age, init,
                                       h["reward"], h["done"], STATIC, zt, scale, gamma)
        assert same(host(shaped.her["reward"]), hwant[0]) and same(host(shaped.her_shape_f), hwant[1])
        assert same(host(shaped.her_shape_mask), hwant[2]) and hwant[2].any()
        swant = shape_ref.goal_shape(ty, None, 17, 17, h["t"], h["n"], h["goal"], before, after, h["reward"], h["done"], age,
                                     init, STATIC, zt, scale, gamma)
        assert same(host(base.her["reward"]), swant[0]) and same(host(base.her_shape_mask), swant[2])
        ss = shaped.shaping_stats()
        assert set(ss) == {"mean", "unshaped", "her_mean", "her_unshaped"} and ss == pytest.approx(dict(
            base.shaping_stats(), her_mean=float(hwant[1][hwant[2] != 0].astype(np.float64).mean()),
            her_unshaped=1.0 - (hwant[2] != 0).mean()), rel=1e-9, abs=1e-12)
        # ppo_her_relabel's order against a shuffle of the same records: the same per-record outputs
        perm = np.random.default_rng(u).permutation(R)
        her = {k: dev(h[k][perm]) for k in ("t", "n", "goal", "done")}
        her["reward"] = dev(h["reward"][perm])
        got = shaped.engine.timed_goal_shape(her, shaped.pos[3:3 + T], shaped.pos[4:4 + T], shaped.age[:-1], shaped.init_pos,
                                             scale=scale, gamma=gamma, zero_terminal=bool(zt))
        assert all(same(host(g), w[perm]) for g, w in zip(got, hwant))
        for tr in (base, shaped):
            tr.carry_over()
            tr.her = None


def test_train_ppo_with_the_switch(capsys):
    from twoarmy_amd.soa import train_ppo
    tr = train_ppo.main(["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", "32", "--rollout_steps", "16", "--minibatch", "128",
                         "--updates", "2", "--k_epochs", "1", "--max_steps", "6", "--shaping_scale", "0.05", "--shaping_timed",
                         "--shaping_hindsight_timed", "--cuda", "cuda:0"])                # episodes end: there are records
    assert tr.env_steps == 2 * 16 * 32
    assert tr.shaping == dict(scale=0.05, hindsight=True, timed=True, hindsight_timed=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]
    assert len(lines) == 2 and all(re.search(r" her shaping mean -?\d+\.\d{4} her unshaped \d\.\d{4}$", ln) for ln in lines), lines
