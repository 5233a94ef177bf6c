"""Reward normalisation, CPU side: the numpy restatement (tests/reward_norm_ref.py) against an independent statement of
the same quantity, its exact corners, and the header, the ctypes table and the train_ppo parser knowing the new names."""
import os
import re

import numpy as np
import pytest

import reward_norm_ref as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                                    # unit roundoff of float64


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


@pytest.mark.parametrize("T,N,gamma,dones", [(5, 65, 0.99, "mixed"), (7, 1000, 1.0, "none"), (4, 257, 0.5, "every"),
                                             (3, 1, 0.99, "last")])
def test_moments_against_numpy_over_the_explicit_return_sequence(T, N, gamma, dones):
    carry, stats = np.zeros(N), np.zeros(4)
    seq = []
    for r, te, tr in rn.case(T, N, dones):
        seq.append(rn.returns(r, te, tr, gamma, carry))
        carry, stats = rn.update(r, te, tr, gamma, carry, stats)
        assert np.array_equal(bits(carry), bits(np.where((te[-1] | tr[-1]) != 0, 0.0, seq[-1][-1])))
    G = np.concatenate(seq).reshape(-1)
    M, gmax = G.size, np.abs(G).max()
    assert stats[0] == M == 3 * T * N                                       # counts are exact
    # Bound.  Every Welford step and every merge rounds a handful of times on values no larger than 2 gmax, so it moves the
    # running mean by at most 4 U gmax; there are M steps and at most M merges: |mean - exact| <= 8 M U gmax (np.mean's
    # own pairwise error, (log2 M + 1) U gmax, is far inside it).  A mean off by dm moves each of the M products d * e,
    # each <= (2 gmax)^2, by at most 4 gmax dm, and each product and sum adds 4 U (2 gmax)^2 of its own: M2 is off by at
    # most M (4 gmax * 8 M U gmax + 16 U gmax^2), the variance M2 / M by at most (32 M + 16) U gmax^2 <= 64 M U gmax^2.
    # Relative to gmax and gmax^2 that is 8 M U and 64 M U: 1.9e-11 and 1.5e-10 at the largest case, M = 21 000.
    assert abs(stats[1] - np.mean(G)) <= 8 * M * U * gmax
    assert abs(stats[2] / stats[0] - np.var(G)) <= 64 * M * U * gmax * gmax
    assert np.array_equal(bits(stats[3]), bits(1.0 / np.sqrt(stats[2] / stats[0] + 1e-8)))


def test_gamma_zero_gives_the_moments_of_the_rewards_themselves():
    (r, te, tr), = rn.case(5, 65, "mixed")[:1]
    assert np.array_equal(bits(rn.returns(r, te, tr, 0.0, np.full(65, 3.5))), bits(r.astype(np.float64)))
    carry, stats = rn.update(r, te, tr, 0.0, np.full(65, 3.5), np.zeros(4))
    none = np.zeros_like(te)
    carry2, stats2 = rn.update(r, none, none, 0.0, np.zeros(65), np.zeros(4))          # neither flags nor carry matter
    assert np.array_equal(bits(stats), bits(stats2))
    assert np.array_equal(bits(carry2), bits(r[-1].astype(np.float64)))
    assert np.array_equal(bits(carry), bits(np.where((te[-1] | tr[-1]) != 0, 0.0, r[-1].astype(np.float64))))
    M, rmax = r.size, np.abs(r).max()
    assert stats[0] == M and abs(stats[1] - r.astype(np.float64).mean()) <= 8 * M * U * rmax
    assert abs(stats[2] / M - r.astype(np.float64).var()) <= 64 * M * U * rmax * rmax


def test_constant_returns_have_no_spread_exactly():
    T, N = 6, 37
    r = np.full((T, N), np.float32(0.2))
    none = np.zeros((T, N), np.uint8)
    carry, stats = rn.update(r, none, none, 0.0, np.zeros(N), np.zeros(4))
    carry, stats = rn.update(r, none, none, 0.0, carry, stats)
    assert stats[0] == 2 * T * N and stats[2] == 0.0 and np.array_equal(bits(stats[1]), bits(np.float64(np.float32(0.2))))
    assert np.array_equal(bits(stats[3]), bits(1.0 / np.sqrt(np.float64(1e-8)))) and stats[3] == pytest.approx(1e4)
    out = rn.apply(r, stats, 10.0)
    assert (out == np.float32(10.0)).all()                                           # 0.2 * 1e4, clamped


def test_merge_with_an_empty_operand_returns_the_others_bits():
    a = (np.float64(7.0), np.float64(-0.3), np.float64(1.25))
    odd_empty = (np.float64(0.0), np.float64(5.0), np.float64(9.0))                  # only the count says "empty"
    for e in (rn.EMPTY, odd_empty):
        assert rn.merge(a, e) is a and rn.merge(e, a) is a
    assert rn.merge(rn.EMPTY, rn.EMPTY) is rn.EMPTY
    assert rn.tree([]) is rn.EMPTY and rn.tree([a]) is a
    assert rn.scale_of(np.float64(0.0), np.float64(0.0)) == 1.0
    carry, stats = rn.update(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.uint8), 0.9,
                             np.ones(3), np.array([1.0, 2.0, 3.0, 4.0]))
    assert carry.tolist() == [1, 1, 1] and stats.tolist() == [1, 2, 3, 4]            # T == 0 changes nothing


def test_the_tree_over_five_is_the_hand_written_nesting():
    E, m = rn.EMPTY, rn.merge
    order_matters = 0
    for seed in range(16):
        rng = np.random.default_rng(seed)
        t = [(np.float64(n), np.float64(mu), np.float64(s)) for n, mu, s in
             zip(rng.integers(1, 9, 5), rng.standard_normal(5), rng.random(5))]
        want = m(m(m(t[0], t[1]), m(t[2], t[3])), m(m(t[4], E), E))
        got = rn.tree(t)
        assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))
        other = m(m(m(m(t[0], t[1]), t[2]), t[3]), t[4])                             # a left fold of the same five
        assert got[0] == other[0]
        order_matters += not all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, other))
    assert order_matters > 0                      # some of the sixteen sets round differently under the other order


def test_apply_is_one_float32_product_and_a_clamp():
    r = np.array([-0.9, -0.01, 0.2, 0.9, 0.0, -0.0, 3.0], np.float32)
    stats = np.array([10.0, 0.1, 2.5, 3.3333333333333335])
    s = np.float32(stats[3])
    assert np.array_equal(rn.apply(r, stats, 0.0).view(np.int32), (r * s).view(np.int32))
    assert np.array_equal(rn.apply(r, stats, np.inf).view(np.int32), (r * s).view(np.int32))
    got = rn.apply(r, stats, 1.5)
    assert got.max() == np.float32(1.5) and got.min() == np.float32(-1.5) and got[2] == np.float32(0.2) * s
    assert np.array_equal(rn.apply(r, np.zeros(4), 0.0).view(np.int32), r.view(np.int32))       # nothing seen: the bits stay


def test_header_ctypes_table_and_parser_know_the_new_names():
    txt = open(os.path.join(ROOT, "include", "twoarmy_ppo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    import twoarmy_amd
    from twoarmy_amd.soa import train_ppo
    arity = {}
    for name in ("ppo_reward_norm_workspace", "ppo_reward_norm_update", "ppo_reward_norm_apply"):
        m = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, code)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        arity[name] = len(params)
        assert name in twoarmy_amd._lib.exported_symbols(), name
        assert len(twoarmy_amd._lib._SIGS[name][1]) == len(params), name
        if name != "ppo_reward_norm_workspace":
            assert re.fullmatch(r"void\s*\*\s*stream", params[-1]), name
    assert arity == {"ppo_reward_norm_workspace": 1, "ppo_reward_norm_update": 10, "ppo_reward_norm_apply": 6}
    for formula in ("q = d / k", "mean = ma + (d * nb) / n", "(((d * d) * na) * nb) / n", "1.0 / sqrt(M2 / count + 1e-8)"):
        assert formula in txt, formula                                   # the formulas are normative text of the header
    p = train_ppo.build_parser()
    a = p.parse_args([])
    assert a.reward_norm is False and a.reward_norm_clip is None and a.reward_norm_no_hindsight is False
    a = p.parse_args(["--reward_norm", "--reward_norm_clip", "5", "--reward_norm_no_hindsight"])
    assert a.reward_norm and a.reward_norm_clip == 5.0 and a.reward_norm_no_hindsight
    from twoarmy_amd import exploration, ppo_ops
    assert all(hasattr(ppo_ops, f) for f in ("reward_norm_update", "reward_norm_apply", "reward_norm_read"))
    assert all(hasattr(exploration.RewardNormalizer, f)
               for f in ("update", "apply", "read", "state_dict", "load_state_dict", "reset"))
