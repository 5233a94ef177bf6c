"""Host-side checks of mg_nav_timed_goal_shape (include/minigrid_nav.h): the per-record reference (timed_goal_shape_ref.py)
against answers written out by hand and against the static reference it must reduce to, the flood count restated from the
header's byte count, the header against the ctypes table, every TW_E_ARG case of the launch (returned before anything is
launched: no device needed), and the argument errors of the trainer and the command line."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import nav_ref
import shape_ref
import timed_goal_moves_ref as tgref
import timed_goal_shape_ref as tsref
import timed_nav_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = tref.UNREACHABLE
ZT = tsref.ZERO_TERMINAL
W, H, P = 5, 4, 2
GOAL = (4, 1)                                                     # (x, y)


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def world():
    """5 x 4 of walls but for the corridor of row 1 and the cell (3, 0) above it.  The schedule blocks (2, 1) -- the middle of
    the corridor -- at phase 1, and (3, 0) at both phases."""
    ty = np.full((H, W), 2, np.uint8)
    ty[1, :] = 1
    ty[0, 3] = 1
    sched = np.zeros((P, H), np.uint32)
    sched[1, 1] = 1 << 2
    sched[:, 0] = 1 << 3
    return ty.reshape(1, -1), sched


def centre(x, y):
    return (y + 0.5, x + 0.5)                                     # positions are (y, x)


def test_the_fields_of_the_small_world():
    ty, sched = world()
    d = tgref.goal_field(ty[0], None, W, H, sched, P, GOAL[1] * W + GOAL[0]).reshape(P, H, W)
    assert d[0, 1].tolist() == [4, 4, 2, 1, 0]                    # from (1, 1) at phase 0 the only way on is to wait
    assert d[1, 1].tolist() == [5, 3, U, 1, 0]
    assert (np.delete(d, 1, axis=1) == U).all()                   # walls, and the cell that is blocked at every phase
    g = tgref.goal_field(ty[0], None, W, H, sched, P, 1 * W + 2).reshape(P, H, W)     # a goal that is blocked at phase 1
    assert g[0, 1].tolist() == [2, 2, 0, 2, 2] and g[1, 1].tolist() == [3, 1, U, 1, 3]  # beside it at phase 0: wait one
    assert (tgref.goal_field(ty[0], None, W, H, sched, P, 0 * W + 3) == U).all()       # a goal that is free at no phase


# (goal (x, y), acting (x, y), age, after (x, y), done) -> (F, mask) without the flag, with it;  scale = gamma = 0.5
KNOWN = [
    ((GOAL, (1, 1), 2, (1, 1), 0), (1.25, 1), (1.25, 1)),         # it must wait: 4 at phase 0 -> 3 at phase 1: 0.5 * -1.5 - -2
    ((GOAL, (1, 1), 3, (2, 1), 0), (1.0, 1), (1.0, 1)),           # ... and then goes: 3 at phase 1 -> 2 at phase 0
    ((GOAL, (1, 1), 2, (2, 1), 0), (0.0, 0), (0.0, 0)),           # the after cell is blocked at the next phase: unshaped
    ((GOAL, (1, 1), 2, (2, 1), 1), (0.0, 0), (2.0, 1)),           # ... unless the step was terminal: 0 - -2
    ((GOAL, (2, 1), 3, (3, 1), 0), (0.0, 0), (0.0, 0)),           # the acting cell is blocked at its phase
    ((GOAL, (2, 1), 3, (3, 1), 1), (0.0, 0), (0.0, 0)),           # ... terminal or not
    ((GOAL, (0, 1), 4, (0, 1), 1), (0.75, 1), (2.0, 1)),          # cut off: 4 -> 5: 0.5 * -2.5 - -2 / 0 - -2
    ((GOAL, (3, 1), 5, (4, 1), 1), (0.5, 1), (0.5, 1)),           # onto the goal: phi_after = 0 either way
    ((GOAL, (4, 1), 7, (4, 1), 0), (0.0, 1), (0.0, 1)),           # standing on the goal: shaped, F = 0
    ((GOAL, (4, 3), 0, (1, 1), 0), (1.25, 1), (1.25, 1)),         # age 0: init_pos (0, 1) acts at phase 0, 4 -> 3 at phase 1
    ((GOAL, (4, 3), -2, (1, 1), 0), (1.25, 1), (1.25, 1)),        # age < 0: the same, the after state's phase is 1
    ((GOAL, (1, 1), 2, None, 0), (0.0, 0), (0.0, 0)),             # after position outside the world
    ((GOAL, (1, 1), 2, None, 1), (0.0, 0), (2.0, 1)),
    (((2, 1), (1, 1), 1, (2, 1), 0), (0.5, 1), (0.5, 1)),         # a goal blocked at phase 1, entered at phase 0: 1 -> 0
    (((2, 1), (1, 1), 2, (2, 1), 0), (0.0, 0), (0.0, 0)),         # ... entered at phase 1: the ball moved onto the agent
    (((2, 1), (1, 1), 2, (1, 1), 0), (0.75, 1), (0.75, 1)),       # ... waited for instead: 2 -> 1: 0.5 * -0.5 - -1
    (((3, 0), (3, 1), 2, (3, 1), 0), (0.0, 0), (0.0, 0)),         # a goal blocked in all phases
    (((3, 0), (3, 1), 2, (3, 1), 1), (0.0, 0), (0.0, 0)),         # ... terminal or not: the acting state has no distance
    (((0, 0), (3, 1), 2, (3, 1), 1), (0.0, 0), (0.0, 0)),         # a goal on a wall
]


@pytest.mark.parametrize("flags", [0, ZT])
def test_known_answers(flags):
    ty, sched = world()
    R = len(KNOWN)
    rec_t, rec_n = np.arange(R), np.zeros(R, np.int64)
    goal = np.array([centre(*k[0][0]) for k in KNOWN], np.float32)
    before = np.array([[centre(*k[0][1])] for k in KNOWN], np.float32)
    age = np.array([[k[0][2]] for k in KNOWN], np.int32)
    after = np.array([[centre(*k[0][3]) if k[0][3] is not None else (np.nan, 1.0)] for k in KNOWN], np.float32)
    done = np.array([k[0][4] for k in KNOWN], np.uint8)
    reward = np.full(R, 0.25, np.float32)
    init = np.array(centre(0, 1), np.float32)
    out, f, mask = tsref.timed_goal_shape(ty, None, W, H, sched, P, rec_t, rec_n, goal, before, after, age, init, reward, done,
                                          flags=flags, scale=0.5, gamma=0.5)
    want = [k[2 if flags else 1] for k in KNOWN]
    assert f.dtype == np.float32 and out.dtype == np.float32 and mask.dtype == np.uint8
    assert f.tolist() == [w[0] for w in want] and mask.tolist() == [w[1] for w in want]
    assert out.tolist() == [0.25 + w[0] for w in want] and not np.signbit(f).any()
    assert tsref.timed_goal_shape(ty, None, W, H, sched, P, rec_t, rec_n, goal, before, after, age, init, None, done,
                                  flags=flags, scale=0.5, gamma=0.5)[0] is None
    perm = np.random.default_rng(1).permutation(R)                # the order of the records is immaterial
    again = tsref.timed_goal_shape(ty, None, W, H, sched, P, rec_t[perm], rec_n[perm], goal[perm], before, after, age, init,
                                   reward[perm], done[perm], flags=flags, scale=0.5, gamma=0.5)
    assert np.array_equal(again[1], f[perm]) and np.array_equal(again[2], mask[perm])


@pytest.mark.parametrize("Ww,Hh", [(1, 1), (1, 7), (9, 4), (17, 17)])
def test_period_one_with_an_empty_schedule_is_the_static_reference(Ww, Hh):
    """Invariant (b) on the host."""
    rng = np.random.default_rng(31 * Ww + Hh)
    N, T, R = 3, 6, 120
    ty, st = np.zeros((N, Ww * Hh), np.uint8), np.zeros((N, Ww * Hh), np.uint8)
    for n in range(N):
        ty[n], st[n] = nav_ref.random_world(rng, Ww, Hh, (0.0, 0.2)[n % 2])
    c = rng.integers(0, Ww * Hh, (2, T, N))
    before = np.stack([c[0] // Ww + 0.5, c[0] % Ww + 0.25], -1).astype(np.float32)
    after = np.stack([c[1] // Ww + 0.5, c[1] % Ww + 0.25], -1).astype(np.float32)
    after[2, 1] = (np.nan, 0.0)
    age = rng.integers(-1, 4, (T, N)).astype(np.int32)
    init = np.array([0.5, Ww - 0.5], np.float32)
    t, n = rng.integers(-1, T + 1, R), rng.integers(-1, N + 1, R)
    gc = rng.integers(0, Ww * Hh, R)
    goal = np.stack([gc // Ww + 0.5, gc % Ww + 0.5], 1).astype(np.float32)
    goal[::17] = (np.nan, 0.5)
    done = (rng.random(R) < 0.3).astype(np.uint8)
    reward = rng.standard_normal(R).astype(np.float32)
    zero = np.zeros((1, Hh), np.uint32)
    for flags in (0, ZT, nav_ref.DOORS_OPEN | ZT):
        for pass_types in (nav_ref.PASS_DEFAULT, nav_ref.PASS_DEFAULT | (1 << 6)):
            want = shape_ref.goal_shape(ty, st, Ww, Hh, t, n, goal, before, after, reward, done, age, init, pass_types, flags,
                                        0.01, 0.99)
            got = tsref.timed_goal_shape(ty, st, Ww, Hh, zero, 1, t, n, goal, before, after, age, init, reward, done, pass_types,
                                         flags, 0.01, 0.99)
            for g, w in zip(got, want):
                assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                                      w.view(np.uint32) if w.dtype == np.float32 else w)
    assert Ww * Hh < 30 or (got[2].any() and not got[2].all())


def test_a_shaped_record_has_the_move_set_of_its_acting_distance():
    """Invariant (c) on the host."""
    rng = np.random.default_rng(77)
    Ww, Hh, Pp, N, T, R = 7, 9, 6, 2, 12, 300
    ty = np.stack([nav_ref.random_world(rng, Ww, Hh, 0.2)[0] for _ in range(N)])
    sched = np.stack([tref.random_schedule(rng, Pp, Hh, 0.2) for _ in range(N)])
    c = rng.integers(0, Ww * Hh, (2, T, N))
    before = np.stack([c[0] // Ww + 0.5, c[0] % Ww + 0.5], -1).astype(np.float32)
    after = np.stack([c[1] // Ww + 0.5, c[1] % Ww + 0.5], -1).astype(np.float32)
    age = rng.integers(-1, 3 * Pp, (T, N)).astype(np.int32)
    init = np.array([0.5, 0.5], np.float32)
    t, n = rng.integers(0, T, R), rng.integers(0, N, R)
    gc = rng.integers(0, Ww * Hh, (N, 3))[n, rng.integers(0, 3, R)]
    goal = np.stack([gc // Ww + 0.5, gc % Ww + 0.5], 1).astype(np.float32)
    memo = {}
    db, _ = tsref.goal_distances(ty, None, Ww, Hh, sched, Pp, t, n, goal, before, after, age, init, memo=memo)
    mask = tsref.timed_goal_shape(ty, None, Ww, Hh, sched, Pp, t, n, goal, before, after, age, init, memo=memo)[2]
    m, d = tgref.timed_goal_moves(ty, None, Ww, Hh, sched, Pp, t, n, goal, before, age, init)
    assert mask.any() and not mask.all()
    assert (m[mask != 0] != 0).all() and np.array_equal(d.astype(np.int64), db)


# ------------------------------------------------------------------------------------------------ the flood count
def header():
    return open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()


def floods(Ww, Hh, Pp, fixed):
    """The formula of the header: the largest of 8, 4, 2, 1 whose images fit 64 KiB next to `fixed` bytes, else 1."""
    cells = (Ww * Hh + 7) & ~7
    return next((f for f in (8, 4, 2) if fixed + f * Pp * cells * 2 <= 65536), 1)


def test_flood_count_is_the_headers_formula():
    fixed = int(re.search(r"#define MG_NAV_TIMED_GOAL_SHAPE_LDS (\d+)", header()).group(1))
    assert 24 * 1024 < fixed < 28 * 1024                          # the staging of the move sets and of the three outputs
    for Ww, Hh in ((5, 4), (17, 17), (32, 16), (32, 32)):
        got = [nav().timed_goal_shape_floods(Ww, Hh, Pp) for Pp in range(1, 17)]
        assert got == [floods(Ww, Hh, Pp, fixed) for Pp in range(1, 17)], (Ww, Hh)
        assert set(got) <= {8, 4, 2, 1} and all(a >= b for a, b in zip(got, got[1:])), (Ww, Hh, got)
        assert all(g <= nav().timed_goal_floods(Ww, Hh, Pp + 1) for Pp, g in enumerate(got))      # the larger staging
    assert nav().timed_goal_shape_floods(32, 32, 16) == 1 and fixed + 16 * 1024 * 2 <= 65536      # one image always fits
    assert nav().timed_goal_shape_floods(17, 17, 6) == 8 and nav().timed_goal_shape_floods(5, 4, 16) == 8
    for bad in ((0, 5, 1), (5, 33, 1), (5, 5, 0), (5, 5, 17)):
        from twoarmy_amd import _lib
        assert _lib.lib().mg_nav_timed_goal_shape_floods(*bad) == -1, bad


# ------------------------------------------------------------------------------------------------ header and ctypes table
def test_header_arguments_are_the_ctypes_table():
    import twoarmy_amd
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    want = {"mg_nav_timed_goal_shape": "type state n_envs width height pass_types flags blocked blocked_env_stride period "
                                       "rec_t rec_n rec_goal rec_done rec_reward n_records pos_before pos_after age init_pos "
                                       "T scale gamma reward_out shaping mask stream",
            "mg_nav_timed_goal_shape_floods": "width height period"}
    for name, names in want.items():
        args = [a.strip() for a in re.search(r"\b%s\s*\((.*?)\);" % name, txt, re.S).group(1).split(",")]
        assert [re.search(r"(\w+)$", a).group(1) for a in args] == names.split(), name
        res, sig = twoarmy_amd._lib._SIGS[name]
        assert res is C.c_int and len(sig) == len(args) and name in twoarmy_amd._lib.exported_symbols()
        for a, c in zip(args, sig):
            is_ptr = "*" in a
            assert is_ptr == (c is twoarmy_amd._lib._vp), (name, a)
            if not is_ptr:
                assert {"int": "c_int", "int64_t": "c_long", "uint32_t": "c_uint", "float": "c_float"}[a.split()[0]] == c.__name__
    block = header()[header().index("mg_nav_goal_shape over (cell, phase)"):]
    for word in ("depends on record b alone", "(a)", "(b)", "(c)", "free at no phase", "a ball that moved onto the agent",
                 "in every phase in which it is free", "phase that follows", "bit for bit",
                 "MG_NAV_DOORS_OPEN | MG_NAV_SHAPE_ZERO_TERMINAL", "no atomics"):
        assert word in block, word


# ------------------------------------------------------------------------------------------------ argument rejection
def test_bad_arguments_are_rejected_before_any_launch():
    """Every TW_E_ARG case, on the host: the checks read no memory and come before the launch, so addresses inside a host
    buffer stand for the device arrays; n_records == 0 returns 0 and launches nothing either."""
    from twoarmy_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    v = lambda x: None if x is None else C.c_void_p(x)                                     # noqa: E731
    nan, inf = float("nan"), float("inf")

    def call(a):
        return lib.mg_nav_timed_goal_shape(v(a["type"]), v(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"],
                                           v(a["blocked"]), a["bstride"], a["P"], v(a["t"]), v(a["rn"]), v(a["goal"]),
                                           v(a["done"]), v(a["reward"]), a["R"], v(a["pb"]), v(a["pa"]), v(a["age"]),
                                           v(a["init"]), a["T"], a["scale"], a["gamma"], v(a["out"]), v(a["f"]), v(a["mask"]),
                                           None)

    good = dict(type=base, state=None, n=3, W=5, H=4, pass_types=nav_ref.PASS_DEFAULT, flags=ZT | 1, blocked=base + 64,
                bstride=0, P=2, t=base + 128, rn=base + 192, goal=base + 256, done=base + 320, reward=base + 384, R=0,
                pb=base + 448, pa=base + 456, age=base + 512, init=base + 576, T=2, scale=0.5, gamma=0.99, out=base + 640,
                f=base + 704, mask=base + 769)
    assert call(good) == 0 and call(dict(good, state=base + 832, bstride=8, flags=0, done=None, mask=None)) == 0
    assert call(dict(good, reward=None, out=None)) == 0 and call(dict(good, P=16, bstride=64, T=0)) == 0
    bad = [dict(type=None), dict(t=None), dict(rn=None), dict(goal=None), dict(pb=None), dict(pa=None),
           dict(age=None), dict(init=None), dict(age=None, init=None),                     # the age is the clock
           dict(n=0), dict(n=-1), dict(W=0), dict(H=0), dict(W=33), dict(H=33), dict(T=-1), dict(R=-1), dict(R=1 << 40),
           dict(pass_types=0x10000), dict(flags=4), dict(flags=8 | ZT), dict(flags=-1),    # unknown flag bits
           dict(P=0), dict(P=17), dict(P=-1), dict(blocked=None), dict(blocked=good["blocked"] + 2),
           dict(bstride=-1), dict(bstride=7), dict(P=3, bstride=11),                       # 0 < stride < P * height
           dict(pb=good["pb"] + 4), dict(pa=good["pa"] + 4), dict(t=good["t"] + 2), dict(rn=good["rn"] + 1),
           dict(goal=good["goal"] + 2), dict(age=good["age"] + 2), dict(init=good["init"] + 1),
           dict(reward=good["reward"] + 2), dict(out=good["out"] + 2), dict(f=good["f"] + 1),   # float arrays off 4 bytes
           dict(out=None, f=None, mask=None),                                              # no output
           dict(reward=None),                                                              # reward_out without rec_reward
           dict(done=None),                                                                # the terminal flag without rec_done
           dict(scale=nan), dict(scale=inf), dict(scale=-inf), dict(gamma=nan), dict(gamma=inf)]
    for kw in bad:
        for R in (0, 6):                                          # rejected whether or not there is anything to launch
            assert call(dict(good, R=R, **kw) if "R" not in kw else dict(good, **kw)) == -1, (kw, R)


# ------------------------------------------------------------------------------------------------ trainer and command line
def test_hindsight_timed_shaping_argument_errors_need_no_device():
    from twoarmy_amd.soa import train_ppo
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    for timed in (False, True):
        with pytest.raises(ValueError, match="hindsight_timed=True\\) needs hindsight=True"):
            VecPPOTrainer.enable_shaping(types.SimpleNamespace(), 0.1, hindsight=False, timed=timed, hindsight_timed=True)
    with pytest.raises(ValueError, match="booleans"):
        VecPPOTrainer.enable_shaping(types.SimpleNamespace(), 0.1, hindsight_timed=1)
    with pytest.raises(ValueError, match="positive finite"):
        VecPPOTrainer.enable_shaping(types.SimpleNamespace(), 0.0, hindsight_timed=True)
    with pytest.raises(SystemExit, match="--shaping_hindsight_timed needs --shaping_scale"):
        train_ppo.main(["--shaping_hindsight_timed"])
    with pytest.raises(SystemExit, match="not with --shaping_no_hindsight"):
        train_ppo.main(["--shaping_scale", "0.05", "--shaping_hindsight_timed", "--shaping_no_hindsight"])
    with pytest.raises(SystemExit, match="not with --shaping_no_hindsight"):
        train_ppo.main(["--shaping_scale", "0.05", "--shaping_timed", "--shaping_hindsight_timed", "--shaping_no_hindsight"])
    args = train_ppo.build_parser().parse_args(["--shaping_scale", "0.05", "--shaping_hindsight_timed"])
    assert args.shaping_hindsight_timed and not args.shaping_timed and not args.shaping_no_hindsight
    assert not train_ppo.build_parser().parse_args([]).shaping_hindsight_timed
    assert "--shaping_hindsight_timed" in train_ppo.__doc__ and "--shaping_hindsight_timed" in train_ppo.build_parser().format_help()
