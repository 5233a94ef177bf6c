"""tests/bonus_episode_ref.py against traces written out by hand, the table sizes of ppo_bonus_episode_words, the layout
helpers, and the argument errors of BonusTracker(scope="episode") and train_ppo --bonus_scope / --bonus_form that are
raised before anything is launched.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bonus_episode_ref as er  # noqa: E402

F32 = np.float32


def trace(cells, done, **kw):
    """One env that steps onto cells[t] = (y, x), action 0, direction 0, reward 0; done[t] ends an episode."""
    T = len(cells)
    pos = np.array(cells, F32).reshape(T, 1, 2)
    d = np.array(done, np.uint8).reshape(T, 1)
    ref = er.EpisodeBonusRef(1, **kw)
    out = ref.scan(pos, None, np.zeros((T, 1), F32), d, np.zeros_like(d))
    return ref, out


def test_a_cell_revisited_inside_an_episode_pays_the_inverse_roots():
    ref, out = trace([(2, 3)] * 3, [0, 0, 0])
    assert list(out["count_state"][:, 0]) == [1, 2, 3]
    assert list(out["state"][:, 0]) == [F32(1.0), F32(1 / math.sqrt(2.0)), F32(1 / math.sqrt(3.0))]
    assert ref.table("state")[0, 2 * 17 + 3] == 3 and ref.table("state").sum() == 3


def test_the_same_cell_pays_one_again_after_a_done_and_the_done_step_is_paid_before_the_clear():
    #        episode 1 ............  | episode 2
    cells = [(2, 3), (2, 3), (2, 3), (2, 3), (5, 5), (2, 3)]
    done = [0, 0, 1, 0, 0, 0]
    ref, out = trace(cells, done)
    assert list(out["count_state"][:, 0]) == [1, 2, 3, 1, 1, 2]                 # the done step is the third visit
    assert out["state"][2, 0] == F32(1 / math.sqrt(3.0)) and out["state"][3, 0] == F32(1.0)
    assert ref.table("state")[0, 2 * 17 + 3] == 2 and ref.table("state")[0, 5 * 17 + 5] == 1
    assert ref.gen["state"] == [1]
    # truncated ends an episode as terminated does, and a done at every step pays 1 every time
    T = 4
    pos = np.full((T, 1, 2), 4.0, F32)
    z = np.zeros((T, 1), np.uint8)
    r = er.EpisodeBonusRef(1, ("state", "action"))
    out = r.scan(pos, None, np.zeros((T, 1), F32), z, np.ones_like(z))
    assert (out["state"] == 1).all() and (out["action"] == 1).all() and (out["reward"] == 2).all()
    assert r.table("state").sum() == 0 and r.table("action").sum() == 0 and r.gen["action"] == [4]


def test_first_pays_once_per_episode():
    cells = [(1, 1), (1, 2), (1, 1), (1, 1), (1, 1), (1, 2)]
    done = [0, 0, 0, 1, 0, 0]
    _, out = trace(cells, done, form="first", scale=0.25)
    assert list(out["state"][:, 0]) == [F32(0.25), F32(0.25), 0, 0, F32(0.25), F32(0.25)]
    assert list(out["count_state"][:, 0]) == [1, 1, 2, 3, 1, 1]


def test_keep_passes_the_reward_and_still_counts_and_invalid_steps_share_other_which_clears_too():
    pos = np.array([[[np.nan, 0]], [[0, 17]], [[2, 2]], [[2, 2]], [[-1, 0]]], F32)
    action = np.array([[0], [0], [7], [1], [0]])
    dirs = np.array([[0], [0], [0], [4], [0]])
    term = np.array([[0], [0], [0], [1], [0]], np.uint8)
    reward = np.full((5, 1), -0.01, F32)
    ref = er.EpisodeBonusRef(1, ("state", "action"))
    out = ref.scan(pos, action, reward, term, np.zeros_like(term), keep=term, dirs=dirs)
    assert list(out["count_state"][:, 0]) == [1, 2, 1, 2, 1] and list(out["count_action"][:, 0]) == [1, 2, 3, 4, 1]
    assert out["reward"][3, 0] == F32(-0.01) and out["reward"][2, 0] == F32((float(F32(-0.01)) + 1.0) + 1 / math.sqrt(3.0))
    assert ref.table("state")[0, -1] == 1 and ref.table("action")[0, -1] == 1 and ref.table("action").sum() == 1


def test_cutting_the_steps_anywhere_changes_nothing():
    rs = np.random.RandomState(3)
    T, N = 40, 3
    pos = rs.randint(0, 3, (T, N, 2)).astype(F32)
    action, dirs = rs.randint(0, 7, (T, N)), rs.randint(0, 4, (T, N))
    term, trunc = (rs.rand(T, N) < 0.1).astype(np.uint8), (rs.rand(T, N) < 0.1).astype(np.uint8)
    reward = rs.choice([-0.01, 0.9], (T, N)).astype(F32)
    whole = er.EpisodeBonusRef(N, er.KINDS)
    want = whole.scan(pos, action, reward, term, trunc, dirs=dirs)
    assert want["count_state"].max() > 2 and (term | trunc).sum() > 5
    cut = int(np.flatnonzero((term | trunc)[:, 0])[0]) + 1                       # directly behind a done step of env 0
    parts = er.EpisodeBonusRef(N, er.KINDS)
    got = [parts.scan(pos[s], action[s], reward[s], term[s], trunc[s], dirs=dirs[s]) for s in (slice(0, cut), slice(cut, T))]
    for k in want:
        assert np.array_equal(np.concatenate([g[k] for g in got]), want[k]), k
    assert all(np.array_equal(parts.table(k), whole.table(k)) and parts.gen[k] == whole.gen[k] for k in er.KINDS)


def test_a_count_stays_at_its_ceiling_and_the_generation_wraps():
    ref = er.EpisodeBonusRef(1, ("state",))
    start = np.zeros((1, 290), np.int64)
    start[0, 7] = er.COUNT_MAX - 1
    ref.preset("state", start, [255])
    pos = np.zeros((3, 1, 2), F32)
    pos[..., 1] = 7
    z = np.zeros((3, 1), np.uint8)
    out = ref.scan(pos, None, np.zeros((3, 1), F32), z, z)
    assert list(out["count_state"][:, 0]) == [er.COUNT_MAX] * 3 and ref.gen["state"] == [255]
    ref.scan(pos[:1], None, np.zeros((1, 1), F32), z[:1] + 1, z[:1])
    assert ref.gen["state"] == [0] and ref.table("state").sum() == 0


def test_layout_helpers_state_the_header():
    N, K = 3, 290
    counts = np.zeros((N, K), np.int64)
    counts[0, 5], counts[1, 289], counts[2, 0] = 4, er.COUNT_MAX, 1
    gen = np.array([0, 255, 9])
    stamp, old = np.full((N, K), 8), np.full((N, K), 77)
    stamp[0, :] = 0                                                               # env 0 is in generation 0: not stale
    tab = er.encode(counts, gen, stale=(stamp, old))
    assert tab.dtype == np.int32 and tab.size == er.words("state", N) == N * (K + 1)
    u = tab.view(np.uint32)
    assert u[5] == 4 and u[K + 289] == (255 << 24 | er.COUNT_MAX) and u[2 * K] == (9 << 24 | 1) and u[2 * K + 1] == (8 << 24 | 77)
    assert list(u[N * K:]) == [0, 255, 9]
    got, g, st = er.decode(tab, N)
    assert np.array_equal(got, counts) and np.array_equal(g, gen) and st[2, 1] == 8 and st[0, 1] == 0
    assert not er.decode(np.zeros(N * (K + 1), np.int32), N)[0].any()            # all-zero: nothing counted


def test_word_counts():
    import twoarmy_amd
    lib = twoarmy_amd._lib.lib()
    assert lib.ppo_bonus_episode_words(1, 17, 17, 7, 10) == 291 * 10 == er.words("state", 10)
    assert lib.ppo_bonus_episode_words(2, 17, 17, 7, 4096) == 8094 * 4096 == er.words("action", 4096)
    assert lib.ppo_bonus_episode_words(2, 32, 32, 8, 1) == 32770 and lib.ppo_bonus_episode_words(1, 1, 1, 1, 0) == 0
    for bad in [(0, 17, 17, 7, 1), (3, 17, 17, 7, 1), (1, 0, 17, 7, 1), (1, 17, 33, 7, 1), (2, 17, 17, 0, 1), (2, 17, 17, 9, 1),
                (1, 17, 17, 7, -1), (2, 32, 32, 8, 1 << 20)]:
        assert lib.ppo_bonus_episode_words(*bad) == -1, bad
    from twoarmy_amd import ppo_ops
    assert ppo_ops.bonus_episode_words("action", N=2) == 2 * 8094 and ppo_ops.BONUS_EPISODE_COUNT_BITS == er.COUNT_BITS
    assert ppo_ops.BONUS_FORMS == {"sqrt": 0, "first": 1}
    sig = twoarmy_amd._lib._SIGS["ppo_bonus_scan_episode"][1]
    assert len(sig) == 23 and len(twoarmy_amd._lib._SIGS["ppo_bonus_scan"][1]) == 22


def test_tracker_refuses_before_a_launch():
    import torch
    from twoarmy_amd.exploration import BonusTracker
    for scope in ("env", "shared"):
        with pytest.raises(ValueError, match="episode"):
            BonusTracker(2, "cpu", ("state",), scope, form="first")
    with pytest.raises(ValueError, match="form"):
        BonusTracker(2, "cpu", ("state",), "episode", form="novelty")
    tr = BonusTracker(2, "cpu", ("state", "action"), "episode", 0.5, form="first")
    assert tr.tables["state"].numel() == 2 * 291 and tr.tables["action"].numel() == 2 * 8094 and tr.form == "first"
    pos, z, r = torch.zeros((3, 2, 2)), torch.zeros((3, 2), dtype=torch.int32), torch.zeros((3, 2))
    flags = torch.zeros((3, 2), dtype=torch.uint8)
    for kw in ({}, dict(terminated=flags), dict(truncated=flags), dict(keep=flags)):
        with pytest.raises(ValueError, match="terminated= and truncated="):
            tr.account(pos, z, r, **kw)
    assert not tr.bonus and all(not t.any() for t in tr.tables.values())           # nothing was made or counted
    assert tr.read(per_env=True)["state"].shape == (2, 17, 17)


def test_train_ppo_takes_the_episode_flags_and_refuses_first_without_them():
    from twoarmy_amd.soa.train_ppo import build_parser, main
    base = vars(build_parser().parse_args([]))
    assert base["bonus_scope"] == "shared" and base["bonus_form"] == "sqrt" and base["bonus"] == "none"
    a = build_parser().parse_args(["--bonus", "state", "--bonus_scope", "episode", "--bonus_form", "first"])
    assert (a.bonus, a.bonus_scope, a.bonus_form) == ("state", "episode", "first")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--bonus_form", "always"])
    for argv in (["--bonus_form", "first"], ["--bonus", "state", "--bonus_scope", "env", "--bonus_form", "first"]):
        with pytest.raises(SystemExit, match="--bonus_form first needs --bonus_scope episode"):
            main(argv)
