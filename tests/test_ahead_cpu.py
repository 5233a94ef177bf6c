"""Host-side checks of the look-ahead of include/minigrid_nav.h: the numpy reference (ahead_ref.py) against labels written
out by hand, the header's invariants (a)-(d) on random worlds, ahead_bits / ahead_loss in float64 against a per-row loop and
autograd, the header's constants and signatures against the front end, and every TW_E_ARG case of the two entry points (the
checks read no memory and come before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ahead_ref
import nav_ref
import prior_ref
import timed_nav_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = nav_ref.UNREACHABLE
W, H = 5, 4
GOAL = (4, 1)                                                     # (x, y)
LEFT, RIGHT, UP, DOWN, SAME = 23, 25, 17, 31, 24                  # the bits of the five one-step displacements


def world():
    """5 x 4, empty but for one wall at (2, 1) (tests/test_shape_cpu.py):
        5 4 3 2 1
        6 5 U 1 0
        5 4 3 2 1
        6 5 4 3 2"""
    ty = np.ones((H, W), np.uint8)
    ty[1, 2] = 2
    return ty.reshape(-1)


def B(dy, dx):
    return 1 << ((dy + 3) * 7 + (dx + 3))


# (x, y) -> the labels at steps 1, 2, 3 and the distance
KNOWN = [
    ((3, 3), (B(-1, 0) | B(0, 1), B(-2, 0) | B(-1, 1), B(-2, 1)), 3),       # two optimal moves, which meet again at the goal
    ((3, 0), (B(0, 1) | B(1, 0), B(1, 1), B(1, 1)), 2),                     # 2 from the goal: absorbed at k = 3
    ((4, 1), (B(0, 0), B(0, 0), B(0, 0)), 0),                               # the goal itself
    ((2, 1), (0, 0, 0), U),                                                 # the wall: no state
    ((0, 3), (B(-1, 0) | B(0, 1), B(-1, 1) | B(0, 2), B(-1, 2) | B(0, 3)), 6),   # a corner: nothing leaves the world
    ((0, 0), (B(0, 1), B(0, 2), B(0, 3)), 5),                               # another: (0, 1) lies farther, not nearer
    ((4, 0), (B(1, 0), B(1, 0), B(1, 0)), 1),
]


def test_bit_positions():
    assert (B(0, -1), B(0, 1), B(-1, 0), B(1, 0), B(0, 0)) == tuple(1 << b for b in (LEFT, RIGHT, UP, DOWN, SAME))
    assert ahead_ref.bit_of(3, 3) == 48 and ahead_ref.bit_of(-3, -3) == 0


@pytest.mark.parametrize("k", [1, 2, 3])
def test_known_answers(k):
    dist = nav_ref.field(world(), None, W, H, goal=GOAL)["dist"][None]
    for (x, y), labels, d in KNOWN:
        assert ahead_ref.label(dist, W, H, y * W + x, 0, k) == (labels[k - 1], d), (x, y, k)
    pos = np.array([[(y + 0.5, x + 0.25)] for (x, y), _, _ in KNOWN] + [[(np.nan, 1.0)], [(4.0, 0.0)]], np.float32)
    lab, ad = ahead_ref.ahead(dist, pos, W, H, k)
    assert lab[:, 0].tolist() == [l[k - 1] for _, l, _ in KNOWN] + [0, 0]
    assert ad[:, 0].tolist() == [d for _, _, d in KNOWN] + [U, U]
    # the age rule: every element acts from init_pos = the cell (3, 3)
    lab, ad = ahead_ref.ahead(dist, pos, W, H, k, age=np.zeros((len(pos), 1), np.int32), init_pos=np.array([3.5, 3.5], np.float32))
    assert set(lab[:, 0].tolist()) == {KNOWN[0][1][k - 1]} and set(ad[:, 0].tolist()) == {3}


def test_waiting_is_the_only_optimal_move():
    """3 x 1, the goal at x = 2, the middle cell occupied at phase 1: from (0, phase 0) the agent can only wait."""
    ty = np.ones(3, np.uint8)
    blocked = np.array([[0], [1 << 1]], np.uint32)
    dist = timed_nav_ref.field(ty, None, 3, 1, blocked, 2, goal=(2, 0))["dist"]
    assert dist[0].tolist() == [3, 1, 0] and dist[1].tolist() == [2, U, 0]
    assert ahead_ref.label(dist, 3, 1, 0, 0, 1) == (B(0, 0), 3)
    assert ahead_ref.label(dist, 3, 1, 0, 0, 2) == (B(0, 1), 3)
    assert ahead_ref.label(dist, 3, 1, 0, 0, 3) == (B(0, 2), 3)
    assert ahead_ref.label(dist, 3, 1, 0, 1, 3) == (B(0, 2), 2)          # absorbed after two steps
    assert ahead_ref.label(dist, 3, 1, 1, 1, 1) == (0, U)                # not free at its phase
    assert ahead_ref.label(dist, 3, 1, 1, 0, 3) == (B(0, 1), 1)
    pos = np.array([[(0.5, 0.5)], [(0.5, 0.5)], [(0.5, 1.5)]], np.float32)
    age = np.array([[2], [5], [3]], np.int32)
    lab, ad = ahead_ref.ahead(dist[None], pos, 3, 1, 1, age=age, init_pos=np.zeros(2, np.float32))
    assert lab[:, 0].tolist() == [B(0, 0), B(0, 1), 0] and ad[:, 0].tolist() == [3, 2, U]


def random_case(i):
    """World i of the invariant tests: up to 9 x 9, walls at up to 25 %, P in {1, 2, 6}, a goal on an open cell."""
    rng = np.random.default_rng(1000 + i)
    w, h = int(rng.integers(1, 10)), int(rng.integers(1, 10))
    P = (1, 2, 6)[i % 3]
    ty, _ = nav_ref.random_world(rng, w, h, (0.0, 0.1, 0.25)[(i // 3) % 3], all_types=False)
    open_cells = np.flatnonzero(ty != 2)
    if open_cells.size == 0:
        ty[0] = 1
        open_cells = np.array([0])
    g = int(open_cells[rng.integers(0, open_cells.size)])
    if P == 1:
        dist = nav_ref.field(ty, None, w, h, goal=(g % w, g // w))["dist"][None]
    else:
        dist = timed_nav_ref.field(ty, None, w, h, timed_nav_ref.random_schedule(rng, P, h, 0.1), P, goal=(g % w, g // w))["dist"]
    return w, h, P, dist


def test_invariants_on_random_worlds():
    elements = labelled = 0
    one_step = {0: LEFT, 1: RIGHT, 2: UP, 3: DOWN, 4: SAME}
    for i in range(100):
        w, h, P, dist = random_case(i)
        moves1 = prior_ref.cell_moves(dist[0], w, h) if P == 1 else None
        for p in range(P):
            for c in range(w * h):
                labs = [ahead_ref.label(dist, w, h, c, p, k) for k in (1, 2, 3)]
                d = int(dist[p, c])
                elements += 1
                labelled += labs[2][0] != 0
                m = int(moves1[c]) if P == 1 else timed_nav_ref.move_set(dist, w, h, c, p)[0]
                assert labs[0][0] == sum(1 << one_step[b] for b in range(5) if (m >> b) & 1), (i, c, p)        # (a)
                for k, (lab, dd) in enumerate(labs, 1):
                    assert dd == d and (lab != 0) == (d != U) and lab >> 49 == 0                                  # (d)
                    cells = ahead_ref.cells_of(lab, c, w)
                    assert all(0 <= q < w * h and abs(q // w - c // w) + abs(q % w - c % w) <= k for q in cells)
                    if d != U and d >= k:
                        assert all(int(dist[(p + k) % P, q]) == d - k for q in cells), (i, c, p, k)              # (b)
                    if d != U and d < k:
                        assert all(int(dist[(p + d) % P, q]) == 0 for q in cells)
                    if k > 1 and d != U:                                                                         # (c)
                        union = 0
                        for q in ahead_ref.cells_of(labs[k - 2][0], c, w):
                            if d <= k - 1:                                   # a cell at distance 0 is carried over
                                step = [q]
                            else:
                                step = ahead_ref.cells_of(ahead_ref.label(dist, w, h, q, (p + k - 1) % P, 1)[0], q, w)
                            for s in step:
                                union |= 1 << ahead_ref.bit_of(s // w - c // w, s % w - c % w)
                        assert lab == union, (i, c, p, k)
    assert 2 * labelled >= elements, (labelled, elements)          # no test below passes on empty labels


# ------------------------------------------------------------------------------------------------ ahead_bits, ahead_loss
def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def loss_rows(p0, p1, labels, coef, n_valid):
    """The per-row loop of the definition, in Python floats."""
    import math
    eps = float(np.finfo(np.float32).eps)
    total, rows = 0.0, 0
    for b in range(len(labels)):
        if int(labels[b]) == 0 or (n_valid is not None and b >= n_valid):
            continue
        q0, q1 = p0[b] / p0[b].sum(), p1[b] / p1[b].sum()
        m = sum(q0[i] * q1[j] for i in range(7) for j in range(7) if (int(labels[b]) >> (i * 7 + j)) & 1)
        total += -math.log(min(max(m, eps), 1.0 - eps))
        rows += 1
    return coef * total / rows if rows else 0.0, rows


def random_labels(rng, n):
    lab = np.zeros(n, np.int64)
    for b in range(n):
        for bit in rng.choice(49, int(rng.integers(0, 5)), replace=False):
            lab[b] |= 1 << int(bit)
    return lab


def test_ahead_bits():
    rng = np.random.default_rng(5)
    lab = random_labels(rng, 40).reshape(8, 5)
    lab[0, 0] = (1 << 49) - 1
    got = nav().ahead_bits(torch.from_numpy(lab))
    assert got.dtype == torch.bool and got.shape == (8, 5, 7, 7)
    assert np.array_equal(got.numpy(), ahead_ref.bits(lab.astype(np.uint64)))
    assert got[0, 0].all() and bool(nav().ahead_bits(torch.tensor([1 << SAME]))[0, 3, 3])
    assert nav().AHEAD_SIDE == ahead_ref.SIDE and nav().AHEAD_MAX_STEPS == ahead_ref.MAX_STEPS


@pytest.mark.parametrize("n_valid", [None, 9, 0])
def test_ahead_loss_equals_the_row_loop(n_valid):
    rng = np.random.default_rng(6)
    Bn = 12
    p0, p1 = rng.random((Bn, 7)) + 0.01, rng.random((Bn, 7)) * 3 + 0.01        # any positive scale
    lab = random_labels(rng, Bn)
    lab[3] = 0
    lab[5] = (1 << 49) - 1                                                       # m = 1: clamped to 1 - eps
    want, rows = loss_rows(p0, p1, lab, 0.7, n_valid)
    term, stats = nav().ahead_loss(torch.from_numpy(p0), torch.from_numpy(p1), torch.from_numpy(lab), 0.7, n_valid)
    assert term.dtype == torch.float64 and int(stats["rows"]) == rows
    assert np.isclose(float(term), want, rtol=1e-12, atol=0.0)
    if n_valid == 0:
        assert float(term) == 0.0


def test_a_single_bit_label_is_the_heads_nll():
    rng = np.random.default_rng(7)
    Bn = 6
    p0, p1 = rng.random((Bn, 7)) + 0.05, rng.random((Bn, 7)) + 0.05
    p0, p1 = p0 / p0.sum(1, keepdims=True), p1 / p1.sum(1, keepdims=True)
    i, j = rng.integers(0, 7, Bn), rng.integers(0, 7, Bn)
    lab = torch.from_numpy((1 << (i * 7 + j)).astype(np.int64))
    t0, t1 = torch.from_numpy(p0), torch.from_numpy(p1)
    nll = (-torch.distributions.Categorical(probs=t0).log_prob(torch.from_numpy(i))
           - torch.distributions.Categorical(probs=t1).log_prob(torch.from_numpy(j))).mean()
    term, _ = nav().ahead_loss(t0, t1, lab, 1.0)
    assert np.isclose(float(term), float(nll), rtol=1e-12, atol=0.0)


def test_ahead_loss_gradients():
    rng = np.random.default_rng(8)
    p0 = torch.from_numpy(rng.random((5, 7)) + 0.1).requires_grad_()
    p1 = torch.from_numpy(rng.random((5, 7)) + 0.1).requires_grad_()
    lab = torch.from_numpy(random_labels(rng, 5))
    lab[1] = 0                                                      # an unlabelled row
    lab[0] |= 1 << SAME
    lab[2] |= 1 << LEFT
    lab[3] |= 1 << DOWN
    lab[4] |= 1                                                     # a padding row below: labelled, but past n_valid
    assert torch.autograd.gradcheck(lambda a, b: nav().ahead_loss(a, b, lab, 0.3, 4)[0], (p0, p1))
    term, _ = nav().ahead_loss(p0, p1, lab, 0.3, 4)
    term.backward()
    for g in (p0.grad, p1.grad):
        assert (g[1] == 0).all() and (g[4] == 0).all() and (g[0] != 0).any() and torch.isfinite(g).all()
    none, stats = nav().ahead_loss(p0.detach(), p1.detach(), torch.zeros(5, dtype=torch.int64), 0.3)
    assert float(none) == 0.0 and int(stats["rows"]) == 0


# ------------------------------------------------------------------------------------------------ header and ABI
def header():
    return open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()


def test_header_constants_and_signatures():
    import twoarmy_amd
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (MG_NAV_\w+) +(-?\w+)", header()) if re.match(r"-?(0x)?[0-9A-Fa-f]+$", v)}
    assert defs["MG_NAV_AHEAD_MAX_STEPS"] == nav().AHEAD_MAX_STEPS == 3
    assert defs["MG_NAV_AHEAD_SIDE"] == nav().AHEAD_SIDE == 7
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    want = {"mg_nav_ahead": "dist dist_pitch period n_envs width height pos age init_pos T steps ahead acting_dist stream",
            "mg_nav_goal_ahead": "type state n_envs width height pass_types flags rec_t rec_n rec_goal n_records pos age init_pos "
                                 "T steps ahead acting_dist stream"}
    for name, names in want.items():
        args = [a.strip() for a in re.search(r"\b%s\s*\((.*?)\);" % name, txt, re.S).group(1).split(",")]
        assert [re.search(r"(\w+)$", a).group(1) for a in args] == names.split(), name
        res, sig = twoarmy_amd._lib._SIGS[name]
        assert res is C.c_int and len(sig) == len(args) and name in twoarmy_amd._lib.exported_symbols()
        for a, c in zip(args, sig):
            is_ptr = "*" in a
            assert is_ptr == (c is twoarmy_amd._lib._vp), (name, a)
            if not is_ptr:
                assert {"int": "c_int", "int64_t": "c_long", "uint32_t": "c_uint"}[a.split()[0]] == c.__name__
    block = header()[header().index("---- Look-ahead"):]
    for word in ("(a)", "(b)", "(c)", "(d)", "max(d - j, 0)", "Manhattan radius", "Bit 24", "bits 49..63 are always 0",
                 "whether or not the cell is free at the next phase", "no atomics", "NaN included", "8-byte aligned"):
        assert word in block, word


def test_bad_arguments_are_rejected_before_any_launch():
    """Every TW_E_ARG case of both entry points, on the host: addresses inside a host buffer stand for the device arrays;
    T == 0 / n_records == 0 return 0 and launch nothing either."""
    from twoarmy_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    v = lambda x: None if x is None else C.c_void_p(x)                                     # noqa: E731

    def ahead(a):
        return lib.mg_nav_ahead(v(a["dist"]), a["pitch"], a["P"], a["n"], a["W"], a["H"], v(a["pos"]), v(a["age"]),
                                v(a["init"]), a["T"], a["steps"], v(a["ahead"]), v(a["ad"]), None)

    good = dict(dist=base, pitch=0, P=1, n=3, W=5, H=4, pos=base + 64, age=base + 128, init=base + 192, T=0, steps=3,
                ahead=base + 256, ad=base + 322)
    assert ahead(good) == 0 and ahead(dict(good, age=None, init=None, ad=None, pitch=24, steps=1, ahead=base + 264)) == 0
    assert ahead(dict(good, P=16)) == 0 and ahead(dict(good, P=2, steps=2)) == 0
    bad = [dict(dist=None), dict(pos=None), dict(ahead=None), dict(n=0), dict(n=-1), dict(T=-1), dict(W=0), dict(H=0),
           dict(W=33), dict(H=33), dict(pitch=19), dict(pitch=-1), dict(dist=base + 1), dict(ad=good["ad"] + 1),
           dict(pos=good["pos"] + 4), dict(age=good["age"] + 2), dict(init=good["init"] + 1), dict(init=None),
           dict(P=0), dict(P=17), dict(P=-1),
           dict(P=2, age=None, init=None), dict(P=2, age=None), dict(P=6, init=None),       # the age is the clock
           dict(steps=0), dict(steps=4), dict(steps=-1),
           dict(ahead=good["ahead"] + 4), dict(ahead=good["ahead"] + 2), dict(ahead=good["ahead"] + 1)]
    for kw in bad:
        for T in (0, 2):                                          # rejected whether or not there is anything to launch
            assert ahead(dict(good, T=T, **kw) if "T" not in kw else dict(good, **kw)) == -1, (kw, T)
    assert ahead(dict(good, n=1 << 20, T=1 << 20)) == -1                                   # T * n_envs >= 2^40

    def goal(a):
        return lib.mg_nav_goal_ahead(v(a["type"]), v(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"],
                                     v(a["t"]), v(a["rn"]), v(a["goal"]), a["R"], v(a["pos"]), v(a["age"]), v(a["init"]),
                                     a["T"], a["steps"], v(a["ahead"]), v(a["ad"]), None)

    good = dict(type=base, state=None, n=3, W=5, H=4, pass_types=nav_ref.PASS_DEFAULT, flags=1, t=base + 64, rn=base + 128,
                goal=base + 192, R=0, pos=base + 256, age=base + 320, init=base + 384, T=2, steps=3, ahead=base + 448,
                ad=base + 514)
    assert goal(good) == 0 and goal(dict(good, state=base + 600, flags=0, age=None, init=None, ad=None, steps=1, T=0)) == 0
    bad = [dict(type=None), dict(t=None), dict(rn=None), dict(goal=None), dict(pos=None), dict(ahead=None),
           dict(n=0), dict(n=-1), dict(W=0), dict(H=0), dict(W=33), dict(H=33), dict(W=-1),
           dict(pass_types=0x10000), dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(pos=good["pos"] + 4), dict(t=good["t"] + 2), dict(rn=good["rn"] + 1), dict(goal=good["goal"] + 2),
           dict(age=good["age"] + 2), dict(init=good["init"] + 1), dict(ad=good["ad"] + 1),
           dict(init=None), dict(T=-1), dict(R=-1), dict(R=1 << 40), dict(R=1 << 62),
           dict(steps=0), dict(steps=4), dict(steps=-1),
           dict(ahead=good["ahead"] + 4), dict(ahead=good["ahead"] + 2), dict(ahead=good["ahead"] + 1)]
    for kw in bad:
        for R in (0, 6):
            assert goal(dict(good, R=R, **kw) if "R" not in kw else dict(good, **kw)) == -1, (kw, R)


# ------------------------------------------------------------------------------------------------ trainer and command line
def test_orientation_prior_argument_errors_need_no_device():
    import types
    from twoarmy_amd.soa import train_ppo
    from twoarmy_amd.soa.soa_vec import VecSoATrainer
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite number >= 0"):
            VecSoATrainer.enable_orientation_prior(types.SimpleNamespace(), bad)
    for steps in (0, 4):
        with pytest.raises(ValueError, match="steps"):
            VecSoATrainer.enable_orientation_prior(types.SimpleNamespace(), 0.1, steps=steps)
    with pytest.raises(RuntimeError, match="before enable_orientation_prior"):
        VecSoATrainer.label_ahead(types.SimpleNamespace(orient_prior=None))
    with pytest.raises(RuntimeError, match="before enable_orientation_prior"):
        VecSoATrainer.orientation_prior_stats(types.SimpleNamespace(orient_prior=None))
    with pytest.raises(SystemExit, match="self-orientation agent only"):
        train_ppo.main(["--orient_prior_coef", "0.1"])
    with pytest.raises(SystemExit, match="self-orientation agent only"):
        train_ppo.main(["--orient_agreement"])
    with pytest.raises(SystemExit, match="self-orientation agent only"):
        train_ppo.main(["--orient_prior_coef", "0.1"], predictor=True)
    with pytest.raises(SystemExit, match="need --orient_prior_coef or --orient_agreement"):
        train_ppo.main(["--orient_prior_timed"], soa=True)
    with pytest.raises(SystemExit, match="finite number >= 0"):
        train_ppo.main(["--orient_prior_coef", "-1"], soa=True)
    with pytest.raises(SystemExit, match="1, 2 or 3"):
        train_ppo.main(["--orient_agreement", "--orient_prior_steps", "4"], soa=True)
    args = train_ppo.build_parser().parse_args(["--orient_prior_coef", "0.05", "--orient_prior_steps", "2",
                                                "--orient_prior_hindsight", "--orient_prior_every_state"])
    assert args.orient_prior_coef == 0.05 and args.orient_prior_steps == 2 and args.orient_prior_hindsight
    assert args.orient_prior_every_state and not args.orient_prior_timed and args.orient_prior_decay == 1.0
    d = train_ppo.build_parser().parse_args([])
    assert d.orient_prior_coef == 0.0 and d.orient_prior_steps == 3 and not d.orient_agreement
    st = {"labelled": 10, "agree": 0.25, "her_labelled": 0, "her_realised": None, "coef": 0.0}
    assert train_ppo.orient_fields(st, False) == " orient agree 0.250"
    assert train_ppo.orient_fields(st, True) == " orient agree 0.250 her realised -"
    assert train_ppo.orient_fields(dict(st, agree=None, her_realised=0.5), True) == " orient agree - her realised 0.500"
