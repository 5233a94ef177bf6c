"""Update diagnostics without a GPU: identities of the float64 reference (update_stats_ref.py), the host read of the
accumulators (ppo_ops.update_stats_read), the KL stop rule, the cross-rank sum in a gloo group of two processes, and the
two flags of train_ppo's parser."""
import warnings

import numpy as np
import torch
import torch.distributed as dist

import update_stats_ref as ur
from test_dist_cpu import _init, _spawn


def _zero():
    return np.zeros(ur.WORDS)


def test_reference_k3_is_non_negative_and_counts_add_up():
    for B in (1, 257, 4099):
        p, a, old, adv, value, target = ur.inputs(B, B)
        s, R = ur.accumulate(_zero(), p, a, old, value, target)
        assert (R["k3"] >= 0).all() and s[3] >= 0 and s[0] == B and s[12] == 1
        assert s[10] == 2 * max(1, B // 16) if B > 1 else s[10] == 1           # the two planted blocks, nothing else
        assert 0 < s[4] < B or B == 1
        assert s[5] == np.abs(R["ratio"] - 1).max() and not s[13:].any()
        if B > 1:                                                               # one batch cut into two calls
            half, _ = ur.accumulate(_zero(), *(x[:B // 2] for x in (p, a, old, value, target)))
            both, _ = ur.accumulate(half, *(x[B // 2:] for x in (p, a, old, value, target)))
            assert both[12] == 2 and np.array_equal(both[[0, 4, 5, 10]], s[[0, 4, 5, 10]])
            assert np.allclose(both[:12], s[:12], rtol=1e-12, atol=0)


def test_reference_explained_variance_identities():
    """Dyadic targets whose mean is dyadic too: every sum below is exact in float64, so the identities hold exactly."""
    rs = np.random.RandomState(3)
    target = (rs.randint(-64, 65, 256) / 16.0).astype(np.float32)
    mean = np.float32(target.astype(np.float64).mean())
    assert float(mean) == target.astype(np.float64).mean()                      # 256 multiples of 1/16: the mean is exact
    p, a, old, adv, value, _ = ur.inputs(256, 5)
    s, _ = ur.accumulate(_zero(), p, a, old, target.copy(), target)
    assert ur.read(s)["explained_variance"] == 1.0 and s[8] == 0 and s[9] == 0
    s, _ = ur.accumulate(_zero(), p, a, old, np.full(256, mean, np.float32), target)
    assert ur.read(s)["explained_variance"] == 0.0 and s[8] == 0
    s, _ = ur.accumulate(_zero(), p, a, old, (-target).astype(np.float32), target)   # e = 2 t: Var(e) = 4 Var(t)
    assert ur.read(s)["explained_variance"] == -3.0


def test_reference_clip_frac_on_hand_built_rows():
    """Four rows of uniform probabilities acted with old log-probs that put the ratio at 0.85, 0.95, 1.05 and 1.2: with
    clip = 0.1 the first and the last are outside."""
    p = np.full((4, 5), 0.2, np.float32)
    a = np.zeros(4, np.int32)
    ratio = np.array([0.85, 0.95, 1.05, 1.2])
    old = (np.log(np.float64(np.float32(0.2)) / np.float64(np.float32(0.2) * 5)) - np.log(ratio)).astype(np.float32)
    z = np.zeros(4, np.float32)
    s, R = ur.accumulate(_zero(), p, a, old, z, z)
    assert np.allclose(R["ratio"], ratio, rtol=1e-6) and R["clipped"].tolist() == [True, False, False, True]
    d = ur.read(s)
    assert d["clip_frac"] == 0.5 and d["rows"] == 4 and d["saturated_frac"] == 0 and abs(d["top_mass"] - 0.2) < 1e-7
    assert abs(d["entropy"] - np.log(5)) < 1e-6 and abs(d["ratio_dev_max"] - 0.2) < 1e-6
    assert abs(d["approx_kl"] - ((ratio - 1) - np.log(ratio)).mean()) < 1e-6
    assert abs(d["approx_kl_k1"] + np.log(ratio).mean()) < 1e-6


def _read(s):
    from twoarmy_amd import ppo_ops
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # no warning, whatever the accumulators hold
        return ppo_ops.update_stats_read(s)


def test_update_stats_read_on_hand_made_accumulators():
    s = _zero()
    s[:13] = [4, 6.0, -0.2, 0.04, 1, 0.3, 8.0, 24.0, 2.0, 3.0, 2, 3.2, 2]
    s[13:] = 777.0                                                              # reserved: never read
    want = dict(rows=4.0, calls=2.0, entropy=1.5, approx_kl=0.01, approx_kl_k1=0.05, clip_frac=0.25, ratio_dev_max=0.3,
                explained_variance=1.0 - (3.0 / 4 - 0.25) / (24.0 / 4 - 4.0), saturated_frac=0.5, top_mass=0.8)
    for got in (_read(torch.tensor(s)), _read(s)):                              # a tensor on any device, or an array
        assert set(got) == set(want) and all(isinstance(v, float) for v in got.values())
        assert got == want and got == ur.read(s)
    # leading dimensions: arrays over them; rows == 0 -> every mean NaN, Var(t) == 0 -> explained_variance NaN
    flat = s.copy()
    flat[6:8] = [8.0, 16.0]                                                     # t = 2 four times: no variance
    got = _read(torch.tensor(np.stack([s, _zero(), flat]).reshape(3, 1, 16)))
    assert all(isinstance(v, np.ndarray) and v.shape == (3, 1) for v in got.values())
    assert got["rows"].ravel().tolist() == [4, 0, 4] and got["calls"].ravel().tolist() == [2, 0, 2]
    for k in ("entropy", "approx_kl", "approx_kl_k1", "clip_frac", "explained_variance", "saturated_frac", "top_mass"):
        assert got[k][0, 0] == want[k] and np.isnan(got[k][1, 0]), k
    assert got["ratio_dev_max"][1, 0] == 0 and np.isnan(got["explained_variance"][2, 0]) and got["entropy"][2, 0] == 1.5


def test_kl_stop_at_the_boundary():
    from twoarmy_amd.soa.ppo_vec import kl_stop
    assert not kl_stop(0.02 * 128, 128, 0.02 * 128 / 128)                       # equal to the target: go on
    assert kl_stop(np.nextafter(0.02 * 128, np.inf), 128, 0.02 * 128 / 128)
    assert not kl_stop(0.0, 128, 0.0) and kl_stop(1e-300, 128, 0.0)
    assert not kl_stop(5.0, 0, 0.0)                                             # nothing measured
    assert not kl_stop(1e6, 1, 1e9)


def _sum_worker(rank, world, port, q):
    twdist = _init(rank, world, port)
    got = twdist.sum_over_ranks([0.25 * (rank + 1), 100 + rank], "cpu")
    q.put((rank, got))
    dist.destroy_process_group()


def test_sum_over_ranks_in_a_gloo_group_of_two():
    res = _spawn(_sum_worker, 2)
    assert [r[1] for r in res] == [[0.75, 201.0], [0.75, 201.0]]                # every rank holds the same sums


def test_sum_over_ranks_without_a_group_returns_the_values():
    from twoarmy_amd.dist import sum_over_ranks
    assert sum_over_ranks([1, 2.5]) == [1.0, 2.5]


def test_parser_target_kl_implies_update_stats():
    from twoarmy_amd.soa.train_ppo import build_parser
    p = build_parser()
    d = p.parse_args([])
    assert d.update_stats is False and d.target_kl is None
    a = p.parse_args(["--target_kl", "0.02"])
    assert a.update_stats is True and a.target_kl == 0.02
    b = p.parse_args(["--update_stats"])
    assert b.update_stats is True and b.target_kl is None
    c = p.parse_args(["--target_kl", "0.5", "--update_stats"])
    assert c.update_stats is True and c.target_kl == 0.5
