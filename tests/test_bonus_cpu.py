"""tests/bonus_ref.py against the recording of the reference's own StateBonus / ActionBonus wrappers
(tests/golden/bonus.npz, tools/record_bonus_golden.py), the two scopes against each other and against the row-synchronous
definition, and the new train_ppo flags.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bonus_ref as br  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bonus.npz")
STACKS = (("state",), ("action",), ("state", "action"))


def golden():
    return np.load(GOLD)


def script_arrays(z, name):
    """(pos f32[S,1,2] (y, x), action, dir, reward f32, term) of a recorded script as ppo_bonus_scan takes them."""
    xy = z["xy_" + name]
    pos = np.stack([xy[:, 1], xy[:, 0]], -1).astype(np.float32)[:, None, :]
    col = lambda k, dt: z[k + "_" + name].astype(dt)[:, None]           # noqa: E731
    return pos, col("action", np.int64), col("dir", np.int64), col("reward", np.float32), col("term", np.uint8)


NAMES = [str(n) for n in np.load(GOLD)["script_names"]]


def test_recording_has_what_the_checks_need():
    z = golden()
    assert os.path.getsize(GOLD) < 100 * 1024
    assert sum(int(z["term_" + n].sum()) for n in NAMES) >= 1                      # a goal episode
    assert all(int((z["term_" + n] | z["trunc_" + n]).sum()) >= 2 for n in NAMES)   # counts persist across resets
    assert any((z["action_" + n] == 6).any() for n in NAMES)
    assert all(len(z["action_" + n]) <= 200 for n in NAMES)
    assert int(z["state_counts_still"][:, 2].max()) > 20                           # standing still: repeated keys


@pytest.mark.parametrize("scope", ["env", "shared"])
@pytest.mark.parametrize("name", NAMES)
def test_ref_reproduces_recorded_counts_and_bonuses(name, scope):
    z = golden()
    pos, action, dirs, reward, _ = script_arrays(z, name)
    for si, kinds in enumerate(STACKS):
        ref = br.BonusRef(1, kinds, scope)
        out = ref.scan(pos, action, reward, dirs=dirs)
        if "state" in kinds:
            want = np.zeros(17 * 17 + 1, np.int64)
            for x, y, c in z["state_counts_" + name]:
                want[y * 17 + x] = c
            assert np.array_equal(ref.tables["state"][0], want)
        if "action" in kinds:
            want = np.zeros(17 * 17 * 4 * 7 + 1, np.int64)
            for x, y, d, a, c in z["action_counts_" + name]:
                want[((y * 17 + x) * 4 + d) * 7 + a] = c
            assert np.array_equal(ref.tables["action"][0], want)
        # the recorded bonus is what the wrapper added to the bare reward: exactly float32(1 / sqrt(c)) of our count
        for k in kinds:
            c = out["count_" + k][:, 0]
            assert np.array_equal(out[k][:, 0], np.array([np.float32(1 / math.sqrt(int(v))) for v in c]))
        if len(kinds) == 1:
            k = kinds[0]
            rec_bonus = z["shaped_" + name][si] - z["reward_" + name]              # double: exact up to that subtraction
            assert np.allclose(rec_bonus, 1 / np.sqrt(out["count_" + k][:, 0]), rtol=0, atol=1e-15)
        # totals: the reference adds to the double -0.01, we to float32(-0.01): at most one float32 ulp apart
        rec = z["shaped_" + name][si]
        got = out["reward"][:, 0]
        ulp = np.spacing(np.abs(rec).astype(np.float32))
        assert (np.abs(got.astype(np.float64) - rec) <= ulp).all(), float(np.abs(got - rec).max())


def test_keep_mask_counts_but_passes_the_reward():
    z = golden()
    pos, action, dirs, reward, term = script_arrays(z, "blocked_goal")
    a = br.BonusRef(1, ("state", "action")).scan(pos, action, reward, dirs=dirs)
    ref = br.BonusRef(1, ("state", "action"))
    b = ref.scan(pos, action, reward, keep=term, dirs=dirs)
    assert term.any() and np.array_equal(b["reward"][term != 0], reward[term != 0])
    assert np.array_equal(b["reward"][term == 0], a["reward"][term == 0])
    assert np.array_equal(a["count_state"], b["count_state"]) and np.array_equal(a["count_action"], b["count_action"])


def random_walk(T, N, seed, width=17, height=17, n_actions=7, bad=0.05):
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(0, min(height, 3), (T, N)), rs.randint(0, min(width, 4), (T, N))], -1).astype(np.float32)
    action = rs.randint(0, n_actions, (T, N))
    dirs = rs.randint(0, 4, (T, N))
    m = rs.rand(T, N) < bad
    pos[m] = rs.choice([np.nan, np.inf, -1.0, 40.0], m.sum())[:, None]
    action[rs.rand(T, N) < bad] = n_actions
    dirs[rs.rand(T, N) < bad] = -1
    reward = rs.choice([-0.01, -0.1, 0.9], (T, N)).astype(np.float32)
    return pos, action, dirs, reward


def test_shared_equals_env_at_one_env():
    pos, action, dirs, reward = random_walk(90, 1, 3)
    a = br.BonusRef(1, ("state", "action"), "env", scale=0.25).scan(pos, action, reward, dirs=dirs)
    b = br.BonusRef(1, ("state", "action"), "shared", scale=0.25).scan(pos, action, reward, dirs=dirs)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_shared_is_the_row_synchronous_definition():
    pos, action, dirs, reward = random_walk(12, 9, 4)
    for kind in ("state", "action"):
        ref = br.BonusRef(9, (kind,), "shared")
        first = ref.scan(pos[:5], action[:5], reward[:5], dirs=dirs[:5])           # leaves a carry behind
        carry = {k: int(v) for k, v in enumerate(ref.tables[kind][0]) if v}
        out = ref.scan(pos[5:], action[5:], reward[5:], dirs=dirs[5:])
        keys = ref.keys(kind, pos[5:], action[5:], dirs[5:])
        assert np.array_equal(out["count_" + kind], br.shared_by_definition(keys, carry))
        assert first["count_" + kind].max() > 1
        same_row = keys[0][:, None] == keys[0][None, :]                            # one key in one row: one bonus
        assert (out[kind][0][:, None] == out[kind][0][None, :])[same_row].all()


def test_invalid_steps_share_one_slot():
    pos = np.array([[[np.nan, 0]], [[0, 17]], [[-1, 3]], [[2, 2]], [[2, 2]]], np.float32)
    action = np.array([[0], [0], [0], [7], [1]])
    dirs = np.array([[0], [0], [0], [0], [4]])
    ref = br.BonusRef(1, ("state", "action"))
    out = ref.scan(pos, action, np.zeros((5, 1), np.float32), dirs=dirs)
    assert list(out["count_state"][:, 0]) == [1, 2, 3, 1, 2] and list(out["count_action"][:, 0]) == [1, 2, 3, 4, 5]
    assert ref.tables["state"][0, -1] == 3 and ref.tables["action"][0, -1] == 5 and ref.tables["action"][0, :-1].sum() == 0


def test_train_ppo_parser_takes_the_bonus_flags_and_defaults_change_nothing():
    from twoarmy_amd.soa.train_ppo import build_parser
    base = vars(build_parser().parse_args([]))
    assert base["bonus"] == "none" and base["bonus_scope"] == "shared" and base["bonus_scale"] == 1.0
    assert base["bonus_dir"] is None
    a = build_parser().parse_args(["--bonus", "both", "--bonus_scope", "env", "--bonus_scale", "0.05", "--bonus_dir", "d"])
    assert (a.bonus, a.bonus_scope, a.bonus_scale, a.bonus_dir) == ("both", "env", 0.05, "d")
    for choice in ("none", "state", "action", "both"):
        assert build_parser().parse_args(["--bonus", choice]).bonus == choice
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--bonus", "curiosity"])
    new = {"bonus", "bonus_scope", "bonus_scale", "bonus_dir"}
    explicit = vars(build_parser().parse_args(["--bonus", "none"]))
    assert {k: v for k, v in explicit.items() if k not in new} == {k: v for k, v in base.items() if k not in new}
    assert base["visit_dir"] is None and base["num_envs"] == 4096 and base["her"] is True
