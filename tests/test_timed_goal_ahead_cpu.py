"""Host-side checks of mg_nav_timed_goal_ahead (include/minigrid_nav.h): the per-record reference (timed_goal_ahead_ref.py)
against the header's invariants (a)-(d) and the references it must reduce to, the flood count restated from the header's
byte count, the header against the ctypes table, every TW_E_ARG case of the launch (returned before anything is launched: no
device needed), the trainer's and the command line's argument errors, and -- on the reference alone -- the conditions that
keep the GPU comparison on the same worlds from being vacuous."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import ahead_ref
import nav_ref
import timed_goal_ahead_ref as taref
import timed_nav_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = tref.UNREACHABLE
LEFT, RIGHT, UP, DOWN, SAME = 23, 25, 17, 31, 24                  # the bits of the five one-step displacements
WORLDS = ["5x4 P=1", "5x4 P=2", "5x4 P=16", "17x17 Twoarmy", "32x32 P=16"]


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def header():
    return open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()


def world(name):
    return taref.worlds()[name]


# ------------------------------------------------------------------------------------------------ the reference against itself
@pytest.mark.parametrize("name", WORLDS)
def test_one_goal_per_env_is_timed_field_then_ahead(name):
    """Invariant (a) on the host."""
    c = world(name)
    W, H, N, T = c["W"], c["H"], c["N"], c["T"]
    gc = np.array([c["pool"][n][0] for n in range(N)])
    dist = tref.fields(c["ty"], c["st"], W, H, c["sched"], c["P"], c["pass_types"], goal=(gc % W, gc // W))[0]
    order = np.random.default_rng(1).permutation(T * N)
    t, n = (order // N).astype(np.int32), (order % N).astype(np.int32)
    goal = np.stack([gc[n] // W + 0.5, gc[n] % W + 0.25], 1).astype(np.float32)
    for steps in (1, 2, 3):
        lab, ad = ahead_ref.ahead(dist, c["pos"], W, H, steps, c["age"], c["init"])
        got = taref.timed_goal_ahead(c, t, n, goal, steps)
        assert np.array_equal(got[0], lab[t, n]) and np.array_equal(got[1], ad[t, n])
        assert (got[0] != 0).any()


@pytest.mark.parametrize("name", ["5x4 P=1", "17x17 Twoarmy"])
def test_period_one_with_an_empty_schedule_is_goal_ahead(name):
    """Invariant (b) on the host."""
    c = world(name)
    still = dict(c, P=1, sched=np.zeros((1, c["H"]), np.uint32), memo={})
    rec = c["rec"]
    for steps in (1, 3):
        want = ahead_ref.goal_ahead(c["ty"], c["st"], c["W"], c["H"], rec["t"], rec["n"], rec["goal"], c["pos"], steps, c["age"],
                                    c["init"], pass_types=c["pass_types"])
        got = taref.timed_goal_ahead(still, rec["t"], rec["n"], rec["goal"], steps)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (got[0] != 0).any()


@pytest.mark.parametrize("name", WORLDS)
def test_one_step_is_the_move_set_and_a_label_means_a_distance(name):
    """Invariants (c) and (d) on the host."""
    c = world(name)
    rec = c["rec"]
    lab, ad = taref.want(c, 1)
    image = {0: LEFT, 1: RIGHT, 2: UP, 3: DOWN, 4: SAME}
    seen = 0
    for b in range(len(lab)):
        kind, field, ac, ph = taref.kind_of(c, rec["t"], rec["n"], rec["goal"], b)
        m, d = (0, U) if kind is not None else tref.move_set(field, c["W"], c["H"], ac, ph)
        assert int(lab[b]) == sum(1 << image[k] for k in range(5) if (m >> k) & 1) and int(ad[b]) == d, b
        seen |= m
    assert seen == 0x1F or name != "17x17 Twoarmy"                # every move and the wait, where the map has room for them
    for steps in (1, 2, 3):
        lab, ad = taref.want(c, steps)
        assert np.array_equal(lab != 0, ad != U) and not (lab >> np.uint64(49)).any()


@pytest.mark.parametrize("name", WORLDS)
def test_permuting_the_records_permutes_the_outputs(name):
    c = world(name)
    rec = c["rec"]
    perm = np.random.default_rng(5).permutation(len(rec["t"]))
    lab, ad = taref.want(c, 3)
    got = taref.timed_goal_ahead(c, rec["t"][perm], rec["n"][perm], rec["goal"][perm], 3)
    assert np.array_equal(got[0], lab[perm]) and np.array_equal(got[1], ad[perm])


# ------------------------------------------------------------------------------------------------ the GPU comparison is not vacuous
@pytest.mark.parametrize("name", WORLDS)
def test_the_worlds_of_the_gpu_test_show_what_they_must(name):
    c = world(name)
    rec = c["rec"]
    R = len(rec["t"])
    lab, ad = taref.want(c, 3)
    ad = ad.astype(np.int64)
    bits = np.array([bin(int(x)).count("1") for x in lab])
    assert (lab != 0).sum() * 2 >= R, (lab != 0).mean()
    assert (bits >= 2).sum() * 20 >= R, (bits >= 2).mean()
    lab1 = taref.want(c, 1)[0]
    # a wait: at one step the stay bit off the goal.  At P = 1 the move arrives in the row it left, where the cell's own
    # distance is d, never d - 1: no wait exists there by the header's rule, so that world cannot be asked for one.
    assert (((lab1 >> np.uint64(SAME)) & np.uint64(1) != 0) & (ad > 0) & (ad != U)).any() or c["P"] == 1, "no wait"
    assert (ad < 3).any()
    assert set(taref.kinds(c, rec)) == set(taref.KINDS) | {None}
    if name == "17x17 Twoarmy":
        static = ahead_ref.goal_ahead(c["ty"], None, 17, 17, rec["t"], rec["n"], rec["goal"], c["pos"], 3, c["age"], c["init"],
                                      pass_types=c["pass_types"])
        assert (static[0] != lab).any()                           # the reason the feature exists
        both = (static[0] != 0) & (lab != 0)
        assert (static[0][both] != lab[both]).any()               # ... among records both experts label, too
        for cut in (1024, 2048):                                  # a run lies across either workgroup boundary
            k = slice(cut - 1, cut + 1)
            assert len(set(rec["n"][k].tolist())) == 1 and len({tuple(g) for g in np.floor(rec["goal"][k]).tolist()}) == 1


# ------------------------------------------------------------------------------------------------ the host function
def floods(W, H, P):
    """The header's formula from the header's byte count."""
    fixed = int(re.search(r"#define MG_NAV_TIMED_GOAL_AHEAD_LDS (\d+)", header()).group(1))
    cells = (W * H + 7) & ~7
    return next((f for f in (8, 4, 2) if fixed + f * P * cells * 2 <= 65536), 1)


def test_the_flood_count_is_the_headers_formula():
    for W, H in ((5, 4), (17, 17), (32, 16), (32, 32)):
        for P in range(1, 17):
            assert nav().timed_goal_ahead_floods(W, H, P) == floods(W, H, P), (W, H, P)
    assert nav().timed_goal_ahead_floods(32, 32, 16) == 1
    assert nav().timed_goal_ahead_floods(17, 17, 6) == 8 and nav().timed_goal_ahead_floods(5, 4, 16) == 8
    from twoarmy_amd import _lib
    lib = _lib.lib()
    for W, H, P in ((0, 4, 2), (33, 4, 2), (5, 0, 2), (5, 33, 2), (5, 4, 0), (5, 4, 17)):
        assert lib.mg_nav_timed_goal_ahead_floods(W, H, P) == -1, (W, H, P)
        with pytest.raises(Exception):
            nav().timed_goal_ahead_floods(W, H, P)
    # the staging is the move sets' plus 8 KiB of labels: never more floods than mg_nav_timed_goal_moves runs
    assert all(nav().timed_goal_ahead_floods(32, H, P) <= nav().timed_goal_floods(32, H, P) for H in (16, 32) for P in range(1, 17))


# ------------------------------------------------------------------------------------------------ header and ABI
def test_header_signatures_and_parameter_names():
    import twoarmy_amd
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    want = {"mg_nav_timed_goal_ahead": "type state n_envs width height pass_types flags blocked blocked_env_stride period rec_t "
                                       "rec_n rec_goal n_records pos age init_pos T steps ahead acting_dist stream",
            "mg_nav_timed_goal_ahead_floods": "width height period"}
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
    # the records' part of the list is mg_nav_timed_goal_moves' with `steps` before the outputs
    moves = [re.search(r"(\w+)$", a.strip()).group(1)
             for a in re.search(r"\bmg_nav_timed_goal_moves\s*\((.*?)\);", txt, re.S).group(1).split(",")]
    assert moves[:18] == want["mg_nav_timed_goal_ahead"].split()[:18]
    defs = dict(re.findall(r"#define (MG_NAV_\w+) +(\d+)", header()))
    assert int(defs["MG_NAV_TIMED_GOAL_AHEAD_LDS"]) == int(defs["MG_NAV_TIMED_GOAL_SHAPE_LDS"]) - 11296 + 8192
    assert int(defs["MG_NAV_TIMED_GOAL_AHEAD_LDS"]) + 16 * 1024 * 2 <= 65536


def test_bad_arguments_are_rejected_before_any_launch():
    """Every TW_E_ARG case on the host: addresses inside a host buffer stand for the device arrays; n_records == 0 returns 0
    and launches nothing either."""
    from twoarmy_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    v = lambda x: None if x is None else C.c_void_p(x)                                     # noqa: E731

    def call(a):
        return lib.mg_nav_timed_goal_ahead(v(a["type"]), v(a["state"]), a["n"], a["W"], a["H"], a["pass_types"], a["flags"],
                                           v(a["blocked"]), a["bstride"], a["P"], v(a["t"]), v(a["rn"]), v(a["goal"]), a["R"],
                                           v(a["pos"]), v(a["age"]), v(a["init"]), a["T"], a["steps"], v(a["ahead"]), v(a["ad"]),
                                           None)

    good = dict(type=base, state=None, n=3, W=5, H=4, pass_types=nav_ref.PASS_DEFAULT, flags=1, blocked=base + 640, bstride=0,
                P=6, t=base + 64, rn=base + 128, goal=base + 192, R=0, pos=base + 256, age=base + 320, init=base + 384, T=2,
                steps=3, ahead=base + 448, ad=base + 514)
    assert call(good) == 0 and call(dict(good, state=base + 600, flags=0, ad=None, steps=1, T=0, bstride=24, ahead=base + 456)) == 0
    assert call(dict(good, P=1)) == 0 and call(dict(good, P=16, bstride=64)) == 0 and call(dict(good, steps=2)) == 0
    bad = [dict(ahead=good["ahead"] + 4), dict(ahead=good["ahead"] + 2), dict(ahead=good["ahead"] + 1), dict(ahead=None),
           dict(steps=0), dict(steps=4), dict(steps=-1),
           dict(age=None), dict(init=None), dict(age=None, init=None),
           dict(blocked=None), dict(blocked=good["blocked"] + 2),
           dict(bstride=23), dict(bstride=1), dict(bstride=-1), dict(P=16, bstride=63),
           dict(R=-1), dict(R=1 << 40), dict(R=1 << 62),
           dict(P=0), dict(P=17), dict(P=-1),
           dict(type=None), dict(t=None), dict(rn=None), dict(goal=None), dict(pos=None),
           dict(n=0), dict(n=-1), dict(W=0), dict(H=0), dict(W=33), dict(H=33), dict(W=-1),
           dict(pass_types=0x10000), dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(pos=good["pos"] + 4), dict(t=good["t"] + 2), dict(rn=good["rn"] + 1), dict(goal=good["goal"] + 2),
           dict(age=good["age"] + 2), dict(init=good["init"] + 1), dict(ad=good["ad"] + 1), dict(T=-1)]
    for kw in bad:
        for R in (0, 6):                                          # rejected whether or not there is anything to launch
            assert call(dict(good, R=R, **kw) if "R" not in kw else dict(good, **kw)) == -1, (kw, R)


# ------------------------------------------------------------------------------------------------ trainer and command line
def test_the_switch_needs_hindsight_labels():
    from twoarmy_amd.soa import train_ppo
    from twoarmy_amd.soa.soa_vec import VecSoATrainer
    with pytest.raises(ValueError, match="hindsight_timed=True needs hindsight=True"):
        VecSoATrainer.enable_orientation_prior(types.SimpleNamespace(), 0.1, hindsight_timed=True)
    with pytest.raises(SystemExit, match="--orient_prior_hindsight_timed needs --orient_prior_hindsight"):
        train_ppo.main(["--orient_prior_coef", "0.1", "--orient_prior_hindsight_timed"], soa=True)
    with pytest.raises(SystemExit, match="self-orientation agent only"):
        train_ppo.main(["--orient_prior_coef", "0.1", "--orient_prior_hindsight", "--orient_prior_hindsight_timed"])
    args = train_ppo.build_parser().parse_args(["--orient_prior_hindsight", "--orient_prior_hindsight_timed"])
    assert args.orient_prior_hindsight_timed and not train_ppo.build_parser().parse_args([]).orient_prior_hindsight_timed
