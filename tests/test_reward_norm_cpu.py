"""Reward normalisation, CPU side: the numpy restatement (tests/reward_norm_ref.py) against an independent statement of
the same quantity, its exact corners, and the header, the ctypes table and the train_ppo parser knowing the new names.
For the GPU sweep over the fold's edges (rn.FOLD_EDGES): the level-wise tree and a slot-by-slot restatement of the kernel's
walk against rn.tree, and each named wrong walk differing in bits from it on the sweep's own inputs."""
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


# ------------------------------------------------------------------------------------------ the fold's edges (FOLD_EDGES)
def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def moments():
    """N -> [(k, mean, m2)]: the triples the scan hands the fold in every call of the GPU sweep's chains from a zero start
    (tests/test_reward_norm_gpu.py, fold_chains): mixed flags, and up to FOLD_SMALL no flags too, three calls each."""
    out = {}
    for N, _ in rn.FOLD_EDGES:
        out[N] = []
        for dones in ("mixed", "none") if N <= rn.FOLD_SMALL else ("mixed",):
            carry = np.zeros(N)
            for r, te, tr in rn.case(rn.FOLD_T, N, dones):
                carry, k, mean, m2 = rn.scan(r, te, tr, 0.99, carry)
                out[N].append((k, mean, m2))
    return out


def wave_tree(m, swapped=False):
    """rn_wave_tree of the kernel on the 64 triples a wavefront's lanes hold -> what the 64 lanes hold behind it (lane 0:
    the chunk's triple; a lane is overwritten at the levels at which it is a left operand, and keeps that)."""
    m = list(m)
    for level in range(6):
        w = 1 << level
        m = [(rn.merge(m[l + w], m[l]) if swapped else rn.merge(m[l], m[l + w])) if l % (2 * w) == 0 else m[l]
             for l in range(64)]
    return m


def left_fold(m):
    out = rn.EMPTY
    for x in m:
        out = rn.merge(out, x)
    return out


def walk(k, mean, m2, wrong=None, slow=False):
    """ppo_reward_norm_fold_kernel restated on the workspace's slots: pass p reads the `count` elements alive at stride
    64^p, a chunk of 64 per wavefront in turn (chunk c is wavefront c % 16's), and leaves each chunk's triple in the
    chunk's first slot.  `wrong` names one defect of a build the GPU sweep has to catch:
      "stale"     the per-chunk reset dropped: the empty lanes of a partial chunk keep what the wavefront's previous chunk
                  left in them
      "dropped"   chunks >= 16 of a pass never reach the next pass (the issue's statement of a loop that ends early)
      "unmerged"  what such a kernel computes: the chunk's first slot keeps its own element and the next pass reads that
      "stride"    stride = 64 from pass 1 on instead of 64^p
      "swapped"   right and left operand exchanged from level 12 (pass 2) on
      "leftfold1", "leftfold2"  a left fold of the chunk's elements instead of its tree, in pass 1 / from pass 2 on
    Passes a defect cannot touch go through rn.levels() (six levels at once) unless `slow`."""
    ws = [np.array(x, np.float64) for x in (k, mean, m2)]
    count, stride, p = len(k), 1, 0
    held = {}                                     # wavefront -> its lanes' registers, which outlive a chunk and a pass
    while True:
        chunks = -(-count // 64)
        read = 64 if wrong == "stride" and p >= 1 else stride
        plain = not slow and (wrong is None or (wrong in ("stride", "swapped", "leftfold2") and p < 2)
                              or (wrong == "leftfold1" and p != 1))
        if plain:
            res = rn.levels(*(x[::stride][:count] for x in ws), 6)
            for x, y in zip(ws, res):
                x[::64 * stride][:chunks] = y
        else:
            alive = chunks
            for c in range(chunks):
                if wrong in ("dropped", "unmerged") and c >= 16:
                    alive = 16 if wrong == "dropped" else chunks
                    continue
                lanes = [tuple(x[(c * 64 + l) * read] for x in ws) if c * 64 + l < count else
                         held[c % 16][l] if wrong == "stale" and c % 16 in held else rn.EMPTY for l in range(64)]
                if (wrong == "leftfold1" and p == 1) or (wrong == "leftfold2" and p >= 2):
                    lanes = [left_fold(lanes)] + lanes[1:]
                else:
                    lanes = wave_tree(lanes, swapped=wrong == "swapped" and p >= 2)
                held[c % 16] = lanes
                for x, y in zip(ws, lanes[0]):
                    x[c * 64 * read] = y
            chunks = alive
        if chunks == 1:
            return tuple(x[0] for x in ws)
        count, stride, p = chunks, stride * 64, p + 1


def test_the_levelwise_tree_and_the_kernels_walk_are_the_tree(moments):
    for N, _ in rn.FOLD_EDGES:
        for i, (k, mean, m2) in enumerate(moments[N][:2]):
            want = rn.tree([(k[j], mean[j], m2[j]) for j in range(N)])
            assert want[0] == rn.FOLD_T * N
            assert same(rn.tree_levelwise(k, mean, m2), want), N
            assert same(walk(k, mean, m2), want), N                           # 64-ary passes in place == the binary tree
            if N <= rn.FOLD_SMALL and i == 0:
                assert same(walk(k, mean, m2, slow=True), want), N           # and lane by lane, as the defects are modelled
    assert rn.tree_levelwise([], [], []) is rn.EMPTY and same(rn.tree_levelwise([2.0], [0.5], [0.25]), (2.0, 0.5, 0.25))
    odd = ([3.0, 0.0, 0.0, 2.0], [0.5, 7.0, 0.0, -1.0], [0.25, 9.0, 0.0, 4.0])    # empty operands that are not all-zero
    assert same(rn.tree_levelwise(*odd), rn.tree(list(zip(*odd))))
    r, te, tr = rn.case(rn.FOLD_T, 4097, "mixed")[1]
    a = rn.update(r, te, tr, 0.99, np.ones(4097), np.array([5.0, 0.1, 2.0, 0.0]))
    b = rn.update(r, te, tr, 0.99, np.ones(4097), np.array([5.0, 0.1, 2.0, 0.0]), levelwise=True)
    assert same(a, b)


# (defect, the sizes of FOLD_EDGES meant to catch it, whether every input there must tell).  The defective walk's triple
# differs in bits from the tree's on the very triples the GPU sweep hands the kernel, so a build with that defect cannot
# pass there.  Where only the rounding of one merge can tell (operands swapped: merge(a, b) and merge(b, a) are equal in
# exact arithmetic and round alike on about two inputs of three), some of a size's inputs must; the others tell on each.
DEFECTS = [("stale", (1025, 2049), True), ("dropped", (1025,), True), ("unmerged", (1088, 2049, 4095), True),
           ("stride", (4097,), True), ("swapped", (4097, 4160, 65537, 262145), False),
           ("leftfold1", (4096, 4097, 65537), False), ("leftfold2", (65537, 262145), False)]


@pytest.mark.parametrize("wrong,sizes,each", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_each_named_wrong_tree_differs_in_bits_at_its_sizes(moments, wrong, sizes, each):
    for N in sizes:
        told = []
        for k, mean, m2 in moments[N]:
            want, got = rn.tree_levelwise(k, mean, m2), walk(k, mean, m2, wrong)
            told.append(not same(got, want))
            if wrong in ("dropped", "stale"):
                assert got[0] != want[0]                                      # the count already differs
            if wrong in ("swapped", "leftfold1", "leftfold2"):
                assert got[0] == want[0]                                      # the same elements: only the rounding tells
        assert all(told) if each else any(told), (wrong, N, told)
    if wrong == "unmerged":                       # a one-element chunk IS its first slot: 1025 cannot tell, 1088 does
        assert all(same(walk(*m, wrong), rn.tree_levelwise(*m)) for m in moments[1025])
    if wrong == "leftfold2":                      # two elements in pass 2: their left fold is their tree; 16 are needed
        assert all(same(walk(*m, wrong), rn.tree_levelwise(*m)) for m in moments[4097] + moments[4160])


def test_the_scan_and_non_finite_cases_hold_what_they_are_meant_to():
    te, tr = rn.edge_flags(25, 65)
    done = (te | tr) != 0
    assert done[7, 0::2].all() and done[15, 0::2].all() and done[23, 0::2].all() and not done[7, 1::2].any()
    assert done[8, 1::2].all() and done[16, 1::2].all() and done[24, 1::2].all() and not done[8, 0::2].any()
    assert done.sum(0).max() == 3 and not done[[0, 6, 9, 14, 17, 22]].any()
    for t in (7, 8, 15, 16):
        assert (te[t] & tr[t]).any() and (te[t] & ~tr[t] & 1).any() and (tr[t] & ~te[t] & 1).any()
    te, tr = rn.edge_flags(8, 1)
    assert te[7, 0] and tr[7, 0] and te.sum() == 1                            # the single lane: both flags on the last row
    assert not rn.edge_flags(7, 65)[0].any()
    (r, te, tr), (r2, te2, tr2) = rn.nonfinite_case()
    assert np.isnan(r[rn.NF_NAN]) and r[rn.NF_PINF] == np.inf and r[rn.NF_NINF] == -np.inf
    assert (~np.isfinite(r)).sum() == 3 and np.isfinite(r2).all() and te[rn.NF_NINF] and rn.NF_PINF[0] == rn.BATCH
    with np.errstate(all="ignore"):
        c1, s1 = rn.update(r, te, tr, 0.99, np.zeros(rn.NF_N), np.zeros(4))
        c2, s2 = rn.update(r2, te2, tr2, 0.99, c1, s1)
    assert np.isnan(c1[5]) and c1[70] == np.inf and (~np.isfinite(c1)).sum() == 2      # the done step cleared env 129's
    assert np.isfinite(c2[5]) and c2[70] == np.inf and (~np.isfinite(c2)).sum() == 1   # and, in the second call, env 5's
    assert s1[0] == rn.NF_T * rn.NF_N and s2[0] == 2 * s1[0] and np.isnan(s1[1:]).all() and np.isnan(s2[1:]).all()
    clean = rn.update(np.where(np.isfinite(r), r, 0).astype(np.float32), te, tr, 0.99, np.zeros(rn.NF_N), np.zeros(4))[0]
    others = np.ones(rn.NF_N, bool)
    others[[5, 70, 129]] = False
    assert np.array_equal(bits(c1[others]), bits(clean[others]))              # the other envs' returns do not notice
    sp = rn.special_rewards(2049)
    assert np.isnan(sp).sum() >= 8 and np.isinf(sp).sum() >= 8 and (np.signbit(sp) & (sp == 0)).any() and np.isnan(sp[-1])
    assert ((sp != 0) & (np.abs(sp) < np.finfo(np.float32).tiny)).sum() >= 8  # denormals
    assert np.isfinite(rn.special_rewards(2049, nan=False)).sum() == 2049 - 8


def test_apply_with_a_nan_scale_clamps_to_minus_clip():
    """fminf(fmaxf(NaN, -c), c): fmaxf drops the NaN for -c, fminf keeps -c.  np.fmax / np.fmin are the same functions."""
    r = np.array([-0.9, 0.2, 0.0, 3.0], np.float32)
    stats = np.array([10.0, 0.1, 2.5, np.nan])
    assert (rn.apply(r, stats, 0.5) == np.float32(-0.5)).all() and np.isnan(rn.apply(r, stats, 0.0)).all()
    got = rn.apply(np.array([np.nan, np.inf, -np.inf, 1e-40], np.float32), np.array([10.0, 0.1, 2.5, 2.0]), 0.5)
    assert got.tolist() == [-0.5, 0.5, -0.5, np.float32(1e-40) * np.float32(2.0)]
    odd_empty = np.array([0.0, 5.0, 9.0, 123.0])
    assert np.array_equal(rn.apply(r, odd_empty, 0.0).view(np.int32), r.view(np.int32))


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
