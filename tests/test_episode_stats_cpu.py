"""Episode accounting, CPU side: the numpy restatement (tests/episode_ref.py) is the reference's quantity, and the
header, the ctypes table and the train_ppo parser know the new names."""
import os
import re

import numpy as np

import episode_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# episode length <= max_steps = 50, |reward| <= 0.9, one float32 rounding per reward
RETURN_BOUND = 50 * 0.9 * 2.0 ** -24


def test_restatement_is_the_reference_bookkeeping_on_recorded_traces():
    """soa/train_ppo.py:124,136-141 (`ep_reward += reward`, `running_score = running_score * 0.99 + ep_reward * 0.01`)
    on the rewards the reference recorded, against the restatement on their float32 casts."""
    cols = ER.golden_columns()
    assert len(cols[6]) == 6 and len(cols[4]) == 10
    seen = {6: 0, 4: 0}
    for variant, columns in cols.items():
        for r64, term, trunc in columns:
            episodes, ref_score = ER.reference_loop(r64, term, trunc)
            r32 = r64.astype(np.float32).reshape(-1, 1)
            ep_ret, ep_len, carry_r, carry_l = ER.episode_scan(r32, term.reshape(-1, 1), trunc.reshape(-1, 1),
                                                               np.zeros(1), np.zeros(1, np.int32))
            done = np.nonzero(term | trunc)[0]
            assert done.tolist() == [t for t, _, _ in episodes]
            for t, ret, length in episodes:
                assert length <= 50
                assert ep_len[t, 0] == length
                assert abs(ep_ret[t, 0] - ret) <= RETURN_BOUND, (variant, t, ep_ret[t, 0], ret)
            # what is left after the last done step is the running episode's prefix
            tail = len(r64) - (done[-1] + 1)
            assert carry_l[0] == tail and abs(carry_r[0] - sum(float(x) for x in r64[len(r64) - tail:])) <= RETURN_BOUND
            s = ER.episode_summary(ep_ret, ep_len, term.reshape(-1, 1), trunc.reshape(-1, 1), r32)
            assert s["episodes"] == len(episodes) and s["successes"] == int(term.sum())
            assert s["length_sum"] == sum(e[2] for e in episodes) and s["max_length"] == max(e[2] for e in episodes)
            assert abs(s["score"] - ref_score) <= RETURN_BOUND, (s["score"], ref_score)
            assert sum(s["reward_hist"]) == len(r64) and s["reward_hist"][5] == 0      # only the five task rewards occur
            seen[variant] += len(episodes)
    assert seen == {6: 18, 4: 40}                                                    # 58 finished episodes in the file


def test_restatement_does_not_depend_on_the_cut():
    rng = np.random.default_rng(3)
    T, N = 90, 7
    r = rng.choice(np.array(ER.REWARD_VALUES, np.float32), size=(T, N))
    term = (rng.random((T, N)) < 0.04).astype(np.uint8)
    trunc = (rng.random((T, N)) < 0.02).astype(np.uint8)
    c0, l0 = rng.normal(size=N), rng.integers(0, 9, N).astype(np.int32)
    whole = ER.episode_scan(r, term, trunc, c0, l0)
    cr, cl, rets, lens, t = c0, l0, [], [], 0
    for step in (1, 7, 64, 18):
        a, b, cr, cl = ER.episode_scan(r[t:t + step], term[t:t + step], trunc[t:t + step], cr, cl)
        rets.append(a); lens.append(b); t += step
    assert t == T
    assert np.array_equal(np.concatenate(rets).view(np.int64), whole[0].view(np.int64))
    assert np.array_equal(np.concatenate(lens), whole[1])
    assert np.array_equal(cr.view(np.int64), whole[2].view(np.int64)) and np.array_equal(cl, whole[3])
    empty = ER.episode_summary(whole[0], whole[1], np.zeros_like(term), np.zeros_like(trunc), r, score=0.37)
    assert empty["episodes"] == 0 and empty["score"] == 0.37 and empty["min_return"] == np.inf and empty["max_return"] == -np.inf


def test_header_ctypes_table_and_parser_know_the_new_names():
    txt = open(os.path.join(ROOT, "include", "twoarmy_ppo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    import twoarmy_amd
    from twoarmy_amd.soa import train_ppo
    for name in ("ppo_episode_scan", "ppo_episode_summary", "ppo_episode_summary_workspace"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in twoarmy_amd._lib.exported_symbols(), name
    assert "train_ppo.py:124" in txt and "136-141" in txt                # the reference lines the kernels replace
    n_args = {k: len(twoarmy_amd._lib._SIGS[k][1]) for k in ("ppo_episode_scan", "ppo_episode_summary")}
    assert n_args == {"ppo_episode_scan": 10, "ppo_episode_summary": 17}
    p = train_ppo.build_parser()
    assert p.parse_args([]).score == "rollout"
    assert p.parse_args(["--score", "episode"]).score == "episode"
    assert p.parse_args([]).minibatch == 4096
    from twoarmy_amd import episode_stats, ppo_ops
    assert callable(ppo_ops.episode_scan) and callable(ppo_ops.episode_summary) and episode_stats.EpisodeTracker
