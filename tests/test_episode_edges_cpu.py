"""Episode accounting at its edges, CPU side: the grid rule of include/twoarmy_ppo.h restated, and the bounds
tests/test_episode_kernels_edges_gpu.py holds ppo_episode_summary's return sum and score to (tests/episode_cases.py:
fold_bound, sum_bound) checked against higher-precision references on the very inputs that file uses.  Nothing here
is fitted to a device result."""
import fractions
import os
import re

import numpy as np
import pytest

import episode_cases as EC
import episode_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLD_SETS = list(EC.fold_sets())


def test_reference_grid_has_the_intended_boundaries():
    """Every M of the sweep sits where it was chosen to sit: 1 -> 2 workgroups, per_lane 1 -> 2, the cap, the first
    thread run longer than one batch of 8."""
    want = {1: (1, 1, 1, 1), 255: (1, 255, 1, 1), 256: (1, 256, 1, 1), 257: (1, 257, 2, 1), 2047: (1, 2047, 8, 1),
            2048: (1, 2048, 8, 1), 2049: (2, 1025, 5, 1), 131072: (64, 2048, 8, 1), 131073: (65, 2017, 8, 2),
            524288: (256, 2048, 8, 4), 524289: (256, 2049, 9, 4), 4097: (3, 1366, 6, 1)}
    assert set(EC.SWEEP_M) | {4097} == set(want)
    for M, w in want.items():
        g = EC.grid(M)
        assert (g["nblocks"], g["per_block"], g["per_thread"], g["per_lane"]) == w, M
        assert (g["per_thread"] > EC.BATCH) == (M == 524289), M              # only above the cap a thread's run loops
        assert g["nblocks"] * g["per_block"] >= M > (g["nblocks"] - 1) * g["per_block"]      # no workgroup without a share
    for M, (T, N) in list(EC.CAP_SHAPES.items()) + list(EC.ORDER_SHAPES.items()):
        assert T * N == M
    assert EC.CAP_SHAPES[524288] == (128, 4096)                              # the production rollout sits on the cap


def test_boundaries_cover_both_ends_of_every_share_and_of_empty_neighbours():
    for M in EC.SWEEP_M:
        g, idx = EC.grid(M), set(EC.boundaries(M).tolist())
        assert {0, M - 1} <= idx and max(idx) == M - 1 and min(idx) == 0
        for b in range(g["nblocks"]):
            lo, hi = EC.block_share(M, b)
            assert {lo, hi - 1} <= idx
        lo, hi = EC.thread_run(M, 0, 0)
        assert {lo, hi - 1} <= idx and hi - lo == min(g["per_thread"], M)
        # the runs tile the share in order, and a run that starts behind the share is empty
        b = g["nblocks"] - 1
        runs = [EC.thread_run(M, b, i) for i in range(EC.THREADS)]
        filled = [r for r in runs if r[0] < r[1]]
        assert filled[0][0] == EC.block_share(M, b)[0] and filled[-1][1] == M
        assert all(a[1] == c[0] for a, c in zip(filled, filled[1:]))
    assert EC.thread_run(524289, 0, 228)[0] > EC.block_share(524289, 0)[1]   # lo > block_hi: an empty run
    assert EC.thread_run(2049, 0, 205) == (1025, 1025)                       # lo == block_hi: another
    assert EC.thread_run(2049, 1, 204) == (2045, 2049)                       # a run cut by the end of the range


def test_cases_poison_what_must_not_be_read():
    for c in [EC.summary_case(M) for M in EC.SWEEP_M] + [EC.summary_case(4097, True)] + [EC.order_case(M) for M in EC.ORDER_SHAPES]:
        done = c["done"]
        assert np.array_equal(done, (c["term"] | c["trunc"]) != 0)
        assert np.isnan(c["ep_return"][~done]).all() and np.isfinite(c["ep_return"][done]).all()
        assert (c["ep_length"][~done] == EC.INT32_MIN).all() and (c["ep_length"][done] > 0).all()
        assert done[0] and done[-1]
    c = EC.summary_case(131073)
    assert (c["term"] & c["trunc"]).any() and (c["term"] > c["trunc"]).any() and (c["trunc"] > c["term"]).any()
    assert c["action"].min() == -1 and c["action"].max() == 8
    assert EC.summary_case(4097, True)["done"].all()
    assert 0 < EC.summary_case(524289)["done"].mean() < 0.01                 # a low density


@pytest.mark.parametrize("name,returns,keep,gain,score0", FOLD_SETS, ids=[s[0] for s in FOLD_SETS])
def test_float64_restatement_stays_within_the_bound(name, returns, keep, gain, score0):
    """The condition the GPU file relies on: the sequential float64 fold and sum it compares the device with lie within
    the bound of the exact (or long double) value, on every input set it uses."""
    E = len(returns)
    ref, kind = EC.fold_reference(returns, keep, gain, score0)
    if ref is None:
        pytest.skip(kind)
    assert (kind == "exact") == (E <= EC.EXACT_EPISODES)
    seq = EC.fold_seq(returns, keep, gain, score0)
    bound = EC.fold_bound(E, keep, gain, score0, returns)
    err = abs(fractions.Fraction(seq) - ref) if kind == "exact" else abs(float(np.longdouble(seq) - ref))
    print(name, "E", E, kind, "score", seq, "error", float(err), "bound", bound)
    assert err <= bound
    sref, skind = EC.sum_reference(returns)
    sseq = EC.sum_seq(returns)
    serr = abs(fractions.Fraction(sseq) - sref) if skind == "exact" else abs(float(np.longdouble(sseq) - sref))
    assert serr <= EC.sum_bound(E, returns)


def test_restatement_agrees_with_the_shared_folds():
    """episode_ref.episode_summary (what the GPU file compares with) is fold_seq / sum_seq on the case's returns."""
    for c, shape in ((EC.summary_case(2049), (1, 2049)), (EC.summary_case(2049), (2049, 1)), (EC.order_case(2049), (3, 683))):
        v = {k: c[k].reshape(shape) for k in ("ep_return", "ep_length", "term", "trunc", "reward")}
        w = ER.episode_summary(v["ep_return"], v["ep_length"], v["term"], v["trunc"], v["reward"], None, 5, 0.99, 0.01, EC.SCORE0)
        assert w["score"] == EC.fold_seq(c["returns"], 0.99, 0.01, EC.SCORE0)
        assert w["return_sum"] == EC.sum_seq(c["returns"]) and w["episodes"] == len(c["returns"])


@pytest.mark.parametrize("M", sorted(EC.ORDER_SHAPES))
def test_order_inputs_tell_the_orders_apart(M):
    """The strength of the "order matters" inputs: a column-major fold and a fold with two neighbouring workgroup shares
    exchanged lie outside the bound around the row-major fold, so a device result inside it has the right order."""
    c = EC.order_case(M)
    E, keep, gain = EC.ORDER_EPISODES, EC.ORDER_KEEP, EC.ORDER_GAIN
    row = EC.fold_seq(c["returns"], keep, gain, EC.SCORE0)
    bound = EC.fold_bound(E, keep, gain, EC.SCORE0, c["returns"])
    assert np.log10(np.abs(c["returns"]).max() / np.abs(c["returns"]).min()) > 9      # several orders of magnitude
    others = {"column-major": EC.column_major(c), "shares 0 and 1 exchanged": EC.swapped_shares(c, 0)}
    last = EC.grid(M)["nblocks"] - 2
    if last > 0:
        others["the last two shares exchanged"] = EC.swapped_shares(c, last)
    for what, returns in others.items():
        assert sorted(returns.tolist()) == sorted(c["returns"].tolist()) and not np.array_equal(returns, c["returns"])
        other = EC.fold_seq(returns, keep, gain, EC.SCORE0)
        print(M, what, other, "row-major", row, "bound", bound)
        assert abs(other - row) > 10 * bound, what
    # and any two neighbouring episodes exchanged
    for i in range(E - 1):
        r = c["returns"].copy()
        r[[i, i + 1]] = r[[i + 1, i]]
        assert abs(EC.fold_seq(r, keep, gain, EC.SCORE0) - row) > bound, i


def test_extreme_keep_and_gain_in_the_restatement():
    r = EC.summary_case(2049)["returns"]
    assert EC.fold_seq(r, 0.0, 1.0, EC.SCORE0) == r[-1] != 0.0
    assert EC.fold_seq(r, 1.0, 0.0, EC.SCORE0) == EC.SCORE0
    assert abs(EC.fold_seq(r, 1.0, 1.0, 0.0) - EC.sum_seq(r)) <= EC.sum_bound(len(r), r)


def test_header_states_the_rules_the_tests_rely_on():
    txt = open(os.path.join(ROOT, "include", "twoarmy_ppo.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", txt)
    for phrase in ("nblocks = min(ceil(M / 2048), 256)", "per_block = ceil(M / nblocks)", "per_thread = ceil(per_block / 256)",
                   "per_lane = ceil(nblocks / 64)", "T * N >= 2^40", "nothing is launched", "NULL counts as aligned",
                   "counted in no bin", "for k >= A is not written", "min and max ignore a NaN", "exactly +0.0"):
        assert phrase in flat, phrase
    assert flat.count("nothing is launched") >= 2 and flat.count("T * N >= 2^40") >= 3
