"""Reward normalisation on the MI355X (csrc/reward_norm.hip; include/twoarmy_ppo.h, "Reward normalisation"):
ppo_reward_norm_update and ppo_reward_norm_apply bit for bit against tests/reward_norm_ref.py, every argument rule, the
stream protocol of tests/stream_util.py, and VecPPOTrainer with and without enable_reward_norm() over two rollouts of
8 envs x 16 steps (episodes of 10 steps, relabelling on).  The stream cases live here; see the note at STREAM_CASES.
Beyond rn.SHAPES: the fold at every N at which a wavefront takes another chunk or the walk another pass (rn.FOLD_EDGES),
the scan at every T around its batches of 8 rows with done steps where the batches meet, and non-finite rewards and
scales."""
import functools

import numpy as np
import pytest
import torch

import reward_norm_ref as rn
import test_streams_gpu as streams
from ppo_util import DEV, dev as _d, lib as _lib, ops as _ops, ptr as _P, rejected, stream as _stream
from stream_util import Case, host, same_bits

pytestmark = pytest.mark.gpu
FILL = -1234.5                                     # canary value: no reward, return or moment of these cases
PAD = 16                                           # canary elements on either side; 16 floats keep 16-byte alignment
F64, F32 = torch.float64, torch.float32


def guarded(n, dtype, offset=0):
    """(buffer, view of n elements inside it): PAD + offset canaries in front, PAD behind."""
    buf = torch.full((PAD + offset + n + PAD,), FILL, dtype=dtype, device=DEV)
    return buf, buf[PAD + offset:PAD + offset + n]


def intact(buf, n, offset=0):
    return bool((buf[:PAD + offset] == FILL).all()) and bool((buf[PAD + offset + n:] == FILL).all())


@functools.lru_cache(maxsize=None)
def start(N, zero):
    return rn.start_state(N, zero)


@functools.lru_cache(maxsize=None)
def reference(T, N, dones, gamma, zero):
    """(ret_carry, stats) after each of the three calls of the chain, computed once and read-only."""
    carry, stats = start(N, zero)
    out = []
    for r, te, tr in rn.case(T, N, dones):
        carry, stats = rn.update(r, te, tr, gamma, carry, stats)
        out.append((carry, stats))
    return out


def device_chain(T, N, dones, gamma, zero):
    """The same chain on the device, every in/out array between canaries -> [(ret_carry, stats)] on the host."""
    return device_calls(rn.case(T, N, dones), gamma, *start(N, zero))


def device_calls(rolls, gamma, c0, s0, nan_workspace=False):
    """One update per rollout of `rolls` from (c0, s0), every in/out array between canaries -> [(ret_carry, stats)] on the
    host.  nan_workspace: the workspace holds NaN before the first call, so that an entry read before it is written (the
    header: "every entry written before it is read") ends in the statistics."""
    N = c0.size
    cbuf, carry = guarded(N, F64)
    sbuf, stats = guarded(4, F64)
    wbuf, ws = guarded(_ops().reward_norm_workspace(N), F64)
    carry.copy_(_d(c0))
    stats.copy_(_d(s0))
    if nan_workspace:
        ws.fill_(float("nan"))
    out = []
    for r, te, tr in rolls:
        assert _ops().reward_norm_update(_d(r), _d(te), _d(tr), gamma, carry, stats, ws) is stats
        out.append((host(carry), host(stats)))
    assert intact(cbuf, N) and intact(sbuf, 4) and intact(wbuf, 3 * N)
    return out


def same_bits_or_nan(got, want):
    """Equal bits where `want` is no NaN, some NaN where it is one: a NaN's sign and payload are not the header's to fix."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(np.isnan(got[nan]).all()) \
        and same_bits(got[~nan], want[~nan])


# --------------------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("T,N", rn.SHAPES)
def test_update_equals_the_restatement_over_three_calls(T, N):
    assert _ops().reward_norm_workspace(N) == 3 * N
    for zero in (True, False):
        for dones in rn.DONES:
            for gamma in rn.GAMMAS:
                want = reference(T, N, dones, gamma, zero)
                got = device_chain(T, N, dones, gamma, zero)
                for i, ((gc, gs), (wc, ws)) in enumerate(zip(got, want)):
                    assert same_bits(gc, wc), ("ret_carry", T, N, zero, dones, gamma, i)
                    assert same_bits(gs, ws), ("stats", T, N, zero, dones, gamma, i, gs, ws)
                assert want[-1][1][0] == start(N, zero)[1][0] + 3 * T * N


def fold_chains(N):
    """(dones, zero) of the chains the sweep runs at N: every start and flag pattern up to FOLD_SMALL, one chain beyond."""
    return [(d, z) for z in (True, False) for d in ("mixed", "none")] if N <= rn.FOLD_SMALL else [("mixed", True)]


@functools.lru_cache(maxsize=None)
def fold_reference(N, dones, zero):
    """reference() with the tree taken level-wise (rn.tree_levelwise, equal to rn.tree at these sizes: the CPU file)."""
    carry, stats = start(N, zero)
    out = []
    for r, te, tr in rn.case(rn.FOLD_T, N, dones):
        carry, stats = rn.update(r, te, tr, 0.99, carry, stats, levelwise=True)
        out.append((carry, stats))
    return out


def check_chain(got, want, what):
    for i, ((gc, gs), (wc, ws)) in enumerate(zip(got, want)):
        assert same_bits(gc, wc), ("ret_carry", what, i)
        assert same_bits(gs, ws), ("stats", what, i, gs, ws)
    assert len(got) == len(want) == 3


@pytest.mark.parametrize("N", [n for n, _ in rn.FOLD_EDGES])
def test_fold_boundary_sweep(N):
    """The fold at every N at which it changes its path (rn.FOLD_EDGES names each edge): a wavefront's second and later
    chunks, partial and one-element chunks behind full ones, the third and fourth pass.  Three calls, a NaN-filled
    workspace."""
    assert _ops().reward_norm_workspace(N) == 3 * N
    for dones, zero in fold_chains(N):
        want = fold_reference(N, dones, zero)
        got = device_calls(rn.case(rn.FOLD_T, N, dones), 0.99, *start(N, zero), nan_workspace=True)
        check_chain(got, want, (N, dones, zero))
        assert want[-1][1][0] == got[-1][1][0] == start(N, zero)[1][0] + 3 * rn.FOLD_T * N      # the count is exact


@pytest.mark.parametrize("N", rn.SCAN_N)
@pytest.mark.parametrize("T", rn.SCAN_T)
def test_scan_batch_boundaries(T, N):
    """T around the scan's batches of 8 rows: a last batch of 1, 7 and 8 rows behind one and two whole ones, done steps on
    the last row of a batch and the first of the next (rn.edge_flags), and the longest carried chains (gamma 1, no flags)
    from a non-zero start."""
    c0, s0 = start(N, False)
    assert s0[0] > 0 and c0.any()
    for kind in rn.SCAN_KINDS:
        gamma = 0.99 if kind == "edge" else 1.0
        rolls = rn.scan_case(T, N, kind)
        want, carry, stats = [], c0, s0
        for r, te, tr in rolls:
            carry, stats = rn.update(r, te, tr, gamma, carry, stats)
            want.append((carry, stats))
        check_chain(device_calls(rolls, gamma, c0, s0, nan_workspace=True), want, (T, N, kind))
        assert want[-1][1][0] == s0[0] + 3 * T * N


def test_a_non_finite_reward_stays_with_its_env_and_its_episode():
    """The header: "a non-finite reward makes the statistics non-finite for good".  What else it does: nothing.  The other
    envs' returns and the count go on, and a done step clears a non-finite return like any other."""
    rolls = rn.nonfinite_case()
    zero = np.zeros(rn.NF_N), np.zeros(4)
    want, (carry, stats) = [], zero
    with np.errstate(all="ignore"):
        for r, te, tr in rolls:
            carry, stats = rn.update(r, te, tr, 0.99, carry, stats)
            want.append((carry, stats))
    got = device_calls(rolls, 0.99, *zero, nan_workspace=True)
    for i, ((gc, gs), (wc, ws)) in enumerate(zip(got, want)):
        assert same_bits_or_nan(gc, wc), ("ret_carry", i)                     # the infinities too, bit for bit
        assert np.array_equal(np.isfinite(gc), np.isfinite(wc))
        assert gs[0] == ws[0] == (i + 1) * rn.NF_T * rn.NF_N                  # the count is exact
        assert np.isnan(gs[1:]).all() and np.isnan(ws[1:]).all(), (i, gs)     # mean, M2 and scale: NaN, and they stay
    (c1, _), (c2, _) = got
    assert np.isnan(c1[5]) and c1[70] == np.inf and np.isfinite(c1[129]) and (~np.isfinite(c1)).sum() == 2
    assert np.isfinite(c2[5]) and c2[70] == np.inf and (~np.isfinite(c2)).sum() == 1


def test_the_cases_hold_what_they_are_meant_to():
    r, te, tr = rn.case(7, 1000, "mixed")[0]
    assert ((te & tr) != 0).any() and ((te | tr) == 0).any()                  # both flags on one step, and neither
    assert np.isin(r, rn.TASK_REWARDS).any() and not np.isin(r, rn.TASK_REWARDS).all()
    assert start(65, False)[1][0] > 0 and np.abs(start(65, False)[0]).max() > 0 and not start(65, True)[1].any()
    assert rn.case(5, 64, "first")[0][1][0].all() and not rn.case(5, 64, "first")[0][1][1:].any()
    assert rn.case(5, 64, "last")[0][2][4].all() and rn.case(5, 64, "every")[0][1].all() and not rn.case(5, 64, "none")[0][1].any()


def test_two_calls_on_equal_inputs_give_equal_bits():
    a, b = device_chain(7, 1000, "mixed", 0.99, False), device_chain(7, 1000, "mixed", 0.99, False)
    assert all(same_bits(x[0], y[0]) and same_bits(x[1], y[1]) for x, y in zip(a, b))
    r = _d(rn.rewards(np.random.default_rng(3), 1, 2049).reshape(-1))
    stats = _d(reference(5, 65, "mixed", 0.99, True)[-1][1])
    assert same_bits(host(_ops().reward_norm_apply(r, stats, 1.5)), host(_ops().reward_norm_apply(r, stats, 1.5)))


def test_read_and_the_normalizer_object():
    from twoarmy_amd.exploration import RewardNormalizer
    T, N = 5, 65
    want = reference(T, N, "mixed", 0.99, True)
    norm = RewardNormalizer(N, 0.99, 1.5, DEV)
    assert norm.read() == dict(count=0.0, mean=0.0, var=0.0, std=0.0, scale=1.0)
    rolls = rn.case(T, N, "mixed")
    for r, te, tr in rolls[:2]:
        norm.update(_d(r), _d(te), _d(tr))
    assert same_bits(host(norm.stats), want[1][1]) and same_bits(host(norm.ret_carry), want[1][0])
    got, s = norm.read(), want[1][1]
    assert got["count"] == s[0] == 2 * T * N and got["mean"] == s[1] and got["var"] == s[2] / s[0]
    assert got["std"] == (s[2] / s[0]) ** 0.5 and got["scale"] == s[3]
    assert same_bits(host(norm.apply(_d(rolls[2][0]))), rn.apply(rolls[2][0], s, 1.5))
    state = norm.state_dict()
    other = RewardNormalizer(N, 0.5, 0.0, DEV)
    other.load_state_dict(state)
    for m in (norm, other):                                                   # the copy continues with equal bits
        m.update(*(_d(x) for x in rolls[2]))
    assert other.gamma == 0.99 and other.clip == 1.5
    assert same_bits(host(other.stats), want[2][1]) and same_bits(host(norm.stats), want[2][1])
    assert same_bits(host(other.ret_carry), want[2][0])
    assert state["stats"].data_ptr() != norm.stats.data_ptr() and same_bits(host(state["stats"]), want[1][1])
    norm.reset()
    assert not host(norm.stats).any() and not host(norm.ret_carry).any()
    for bad in (dict(gamma=1.5), dict(gamma=float("nan")), dict(clip=float("nan"))):
        with pytest.raises(ValueError):
            RewardNormalizer(**{**dict(num_envs=N, gamma=0.9, clip=1.0, device=DEV), **bad})


# ---------------------------------------------------------------------------------------------------------- apply
CLIP = 0.5                                         # the task's +-0.9 times a scale near 1 lies outside it, 0.2 inside


@pytest.mark.parametrize("n", [1, 3, 4, 5, 2047, 2048, 2049])
def test_apply_equals_the_restatement_at_every_alignment(n):
    r_np = rn.rewards(np.random.default_rng(n), 1, n).reshape(-1)
    stats_np = reference(5, 65, "mixed", 0.99, True)[-1][1]
    stats, zero = _d(stats_np), torch.zeros(4, dtype=F64, device=DEV)
    scaled = rn.apply(r_np, stats_np, 0.0)
    if n >= 2047:
        assert scaled.max() > CLIP and scaled.min() < -CLIP                  # the clamp is active on both sides
    for off in range(4):                                                      # reward's floats past a 16-byte boundary
        for out_off in (off, (off + 1) % 4):
            for clip in (CLIP, 0.0, float("inf"), -1.0):
                rbuf, r = guarded(n, F32, off)
                obuf, out = guarded(n, F32, out_off)
                assert r.data_ptr() % 16 == 4 * off and out.data_ptr() % 16 == 4 * out_off
                r.copy_(_d(r_np))
                assert _ops().reward_norm_apply(r, stats, clip, out) is out
                want = rn.apply(r_np, stats_np, clip)
                assert same_bits(host(out), want), (n, off, out_off, clip)
                assert intact(obuf, n, out_off) and same_bits(host(r), r_np)
                assert _ops().reward_norm_apply(r, stats, clip, r) is r        # in place
                assert same_bits(host(r), want) and intact(rbuf, n, off), (n, off, clip)
        rbuf, r = guarded(n, F32, off)
        r.copy_(_d(r_np))
        fresh = _ops().reward_norm_apply(r, zero)                             # nothing seen, no clamp: the bits stay
        assert same_bits(host(fresh), r_np) and same_bits(host(_ops().reward_norm_apply(r, zero, 0.0, r)), r_np)
    assert not same_bits(rn.apply(r_np, stats_np, CLIP), r_np)
    shaped = _d(r_np.reshape(1, n))                                           # any shape goes in flat
    assert same_bits(host(_ops().reward_norm_apply(shaped, stats, CLIP)), rn.apply(r_np, stats_np, CLIP).reshape(1, n))


NAN_SCALE = np.array([10.0, 0.1, 2.5, np.nan])
ODD_EMPTY = np.array([0.0, 5.0, 9.0, 123.0])       # count 0 and the rest not: only the count says "nothing seen"


def applied(r_np, stats_np, clip):
    """apply into a guarded buffer -> the host copy; the input keeps its bits and the canaries theirs."""
    n = r_np.size
    r = _d(r_np)
    obuf, out = guarded(n, F32)
    assert _ops().reward_norm_apply(r, _d(stats_np), clip, out) is out
    assert intact(obuf, n) and same_bits(host(r), r_np)
    return host(out)


def test_apply_on_non_finite_rewards_and_a_non_finite_scale():
    n = 2049
    stats_np = reference(5, 65, "mixed", 0.99, True)[-1][1]
    special, no_nan = rn.special_rewards(n), rn.special_rewards(n, nan=False)
    for clip in (CLIP, 0.0):
        want = rn.apply(special, stats_np, clip)
        assert same_bits_or_nan(applied(special, stats_np, clip), want), clip
        assert np.isnan(want).sum() == (0 if clip else np.isnan(special).sum())      # the clamp turns a NaN into -clip
    assert (rn.apply(special, stats_np, CLIP)[np.isnan(special)] == np.float32(-CLIP)).all()
    tiny = (special != 0) & (np.abs(special) < np.finfo(np.float32).tiny)
    assert tiny.any() and (rn.apply(special, stats_np, 0.0)[tiny] != 0).all()         # denormals are not flushed
    plain = rn.rewards(np.random.default_rng(n), 1, n).reshape(-1)
    got = applied(plain, NAN_SCALE, CLIP)                                             # fminf(fmaxf(NaN, -c), c) = -c
    assert same_bits(got, rn.apply(plain, NAN_SCALE, CLIP)) and (got == np.float32(-CLIP)).all()
    got = applied(plain, NAN_SCALE, 0.0)
    assert same_bits_or_nan(got, rn.apply(plain, NAN_SCALE, 0.0)) and np.isnan(got).all()
    for clip in (0.0, float("inf")):                                                  # an odd empty: the bits stay
        assert same_bits(applied(no_nan, ODD_EMPTY, clip), no_nan) and same_bits(rn.apply(no_nan, ODD_EMPTY, clip), no_nan)
    assert same_bits(applied(no_nan, ODD_EMPTY, CLIP), rn.apply(no_nan, ODD_EMPTY, CLIP))


def test_update_from_an_odd_empty_returns_the_rollouts_triple_alone():
    T, N = 5, 65
    rolls = rn.case(T, N, "mixed")[:1]
    c0 = start(N, False)[0]
    (gc, gs), = device_calls(rolls, 0.99, c0, ODD_EMPTY, nan_workspace=True)
    (zc, zs), = device_calls(rolls, 0.99, c0, np.zeros(4))
    wc, ws = rn.update(*rolls[0], 0.99, c0, ODD_EMPTY)
    assert same_bits(gs, ws) and same_bits(gs, zs) and same_bits(gc, wc) and same_bits(gc, zc) and gs[0] == T * N


# ------------------------------------------------------------------------------------------------ argument rules
def test_update_rejections_launch_nothing():
    T, N = 5, 65
    r, te, tr = (_d(x) for x in rn.case(T, N, "mixed")[0])
    carry = torch.full((N + 2,), FILL, dtype=F64, device=DEV)
    stats = torch.full((6,), FILL, dtype=F64, device=DEV)
    ws = torch.full((3 * N + 2,), FILL, dtype=F64, device=DEV)
    canaries = [(carry, FILL), (stats, FILL), (ws, FILL)]
    good = dict(reward=_P(r), terminated=_P(te), truncated=_P(tr), T=T, N=N, gamma=0.99, ret_carry=_P(carry),
                stats=_P(stats), workspace=_P(ws))
    bad = [{k: None} for k in ("reward", "terminated", "truncated", "ret_carry", "stats", "workspace")]
    bad += [dict(T=-1), dict(N=0), dict(N=-1), dict(T=1 << 20, N=1 << 20), dict(T=1, N=715827883)]
    bad += [dict(ret_carry=_P(carry, 4)), dict(stats=_P(stats, 4)), dict(workspace=_P(ws, 4)), dict(stats=_P(stats, 1))]
    bad += [dict(gamma=g) for g in (-0.01, 1.01, float("nan"), float("inf"), -float("inf"))]
    for kw in bad:
        assert rejected("ppo_reward_norm_update", list({**good, **kw}.values()), canaries), kw
    assert _lib().ppo_reward_norm_update(*{**good, "T": 0}.values(), _stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((t == v).all()) for t, v in canaries)                     # T == 0: accepted, nothing launched
    assert _ops().reward_norm_update(r[:0], te[:0], tr[:0], 0.99, carry[:N], stats[:4], ws) is not None
    assert bool((carry == FILL).all()) and bool((stats == FILL).all())
    for n_bad in (0, -1, 715827883):
        assert _lib().ppo_reward_norm_workspace(n_bad) == -1
    for g in (0.0, 1.0):                                                      # the ends of the interval are inside it
        carry.zero_(); stats.zero_()
        assert _lib().ppo_reward_norm_update(*{**good, "gamma": g}.values(), _stream()) == 0
    torch.cuda.synchronize()
    assert float(stats[0]) == T * N


def test_apply_rejections_launch_nothing():
    n = 2049
    r = _d(rn.rewards(np.random.default_rng(1), 1, n).reshape(-1))
    stats = _d(reference(5, 65, "mixed", 0.99, True)[-1][1])
    out = torch.full((n + 8,), FILL, dtype=F32, device=DEV)
    canaries = [(out, FILL)]
    good = dict(reward=_P(r), n=n, stats=_P(stats), clip=CLIP, out=_P(out))
    bad = [{k: None} for k in ("reward", "stats", "out")]
    bad += [dict(n=-1), dict(n=1 << 40), dict(reward=_P(r, 2)), dict(out=_P(out, 1)), dict(out=_P(out, 2)),
            dict(stats=_P(stats, 4)), dict(clip=float("nan"))]
    for kw in bad:
        assert rejected("ppo_reward_norm_apply", list({**good, **kw}.values()), canaries), kw
    assert _lib().ppo_reward_norm_apply(*{**good, "n": 0}.values(), _stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == FILL).all())                                          # n == 0: accepted, nothing launched
    assert _ops().reward_norm_apply(r[:0], stats, CLIP).numel() == 0


# ------------------------------------------------------------------------------------------------ streams and capture
ST, SN, SAPPLY = 5, 65, 2049


def _update_case():
    def make(seed):
        r, te, tr = rn.case(ST, SN, "mixed", seed=seed + 1)[0]
        carry, stats = rn.start_state(SN, False, seed=seed)
        return streams.up(dict(reward=r, term=te, trunc=tr, ret_carry=carry, stats=stats))

    def call(b, o, ctx):
        _ops().reward_norm_update(b["reward"], b["term"], b["trunc"], 0.99, b["ret_carry"], b["stats"], o["workspace"])
        return dict(ret_carry=b["ret_carry"], stats=b["stats"])

    def ref(h):
        carry, stats = rn.update(h["reward"], h["term"], h["trunc"], 0.99, h["ret_carry"], h["stats"])
        return dict(ret_carry=carry, stats=stats)

    return Case("reward_norm_update", "scans", ["ppo_reward_norm_update"], make, call, ref=ref, state=("ret_carry", "stats"),
                outs=lambda: dict(workspace=torch.empty(3 * SN, dtype=F64, device=DEV)))


def _apply_case():
    def make(seed):
        r = rn.rewards(np.random.default_rng(seed + 20), 1, SAPPLY).reshape(-1)
        return streams.up(dict(reward=r, stats=rn.start_state(SN, False, seed=seed)[1]))

    def call(b, o, ctx):
        return dict(out=_ops().reward_norm_apply(b["reward"], b["stats"], CLIP, o["out"]))

    return Case("reward_norm_apply", "scans", ["ppo_reward_norm_apply"], make, call,
                ref=lambda h: dict(out=rn.apply(h["reward"], h["stats"], CLIP)),
                outs=lambda: dict(out=torch.empty(SAPPLY, dtype=F32, device=DEV)))


STREAM_CASES = [_update_case(), _apply_case()]
# test_streams_gpu's completeness check reads its module's CASES when it runs and wants a case for every prototype that
# takes a stream, and that file is not this change's to edit: a new list, as tests/test_her_select_gpu.py makes one, so
# that the parametrised tests over there keep the list they were given and these cases run once, here.
streams.CASES = streams.CASES + STREAM_CASES


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_eager_on_a_side_stream_behind_the_delay(case):
    streams.test_eager_on_a_side_stream(case)


@pytest.mark.parametrize("case", STREAM_CASES, ids=repr)
def test_captured_and_replayed_twice(case):
    streams.test_captured_and_replayed(case)


def test_a_captured_apply_scales_by_the_statistics_current_at_replay():
    r_np = rn.rewards(np.random.default_rng(4), 1, SAPPLY).reshape(-1)
    s1, s2 = reference(5, 65, "mixed", 0.99, True)[0][1], reference(5, 65, "every", 0.0, False)[-1][1]
    assert s1[3] != s2[3]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r, stats = _d(r_np), _d(s1)
        out = torch.full((SAPPLY,), float("nan"), dtype=F32, device=DEV)
        _ops().reward_norm_apply(r, stats, CLIP, out)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _ops().reward_norm_apply(r, stats, CLIP, out)
        out.fill_(float("nan"))
        g.replay()
        s.synchronize()
        first = host(out)
        stats.copy_(_d(s2))                                                   # only the device's statistics change
        out.fill_(float("nan"))
        g.replay()
        s.synchronize()
        second = host(out)
    torch.cuda.synchronize()
    assert same_bits(first, rn.apply(r_np, s1, CLIP)) and same_bits(second, rn.apply(r_np, s2, CLIP))
    assert not same_bits(first, second)


# ------------------------------------------------------------------------------------------------------------ trainer
TR_N, TR_T = 8, 16


def rollouts(norm=None, bonus=False, n_rollouts=2, inspect=None, after=None):
    """A seeded v6 trainer over n_rollouts rollouts and updates with relabelling on, the same draws for every call;
    inspect(tr, r) runs before the update of rollout r, after(tr, r) behind it and before carry_over().  -> the trainer
    (engine closed)."""
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(2)
    eng = TwoarmyEngine(6, TR_N, 17, seed=9981, max_steps=10)
    agent = PPO()
    agent.K_epochs = 1
    tr = VecPPOTrainer(agent, eng, rollout_steps=TR_T, minibatch=64, value_chunk=512)
    if bonus:
        tr.enable_bonus(("state",), "shared", 0.25)
    if norm is not None:
        tr.enable_reward_norm(**norm)
    for r in range(n_rollouts):
        tr.collect(uniforms=torch.rand(TR_T, TR_N, generator=torch.Generator().manual_seed(40 + r)).to(tr.device))
        if bonus:
            tr.shape_rewards()
        tr.relabel()
        tr.account_episodes()
        if inspect is not None:
            inspect(tr, r)
        torch.manual_seed(70 + r)                                             # the update's permutation
        tr.update()
        if after is not None:
            after(tr, r)
        tr.carry_over()
    eng.close()
    return tr


def nets(tr):
    return [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in (tr.agent.actor, tr.agent.critic)]


def same_nets(a, b):
    return all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in x)


def spy_on_gae(monkeypatch, calls):
    """Record the reward argument of every ppo_ops.gae call the trainer makes: (host copy, device address)."""
    from twoarmy_amd.soa import ppo_vec
    real = ppo_vec.ppo_ops.gae

    def gae(reward, *a, **kw):
        calls.append((host(reward).copy(), reward.data_ptr()))
        return real(reward, *a, **kw)
    monkeypatch.setattr(ppo_vec.ppo_ops, "gae", gae)


def test_without_the_enable_call_the_update_is_what_it_was(monkeypatch):
    """Two runs on the same draws: as it stands, and with the new front-end functions replaced by ones that raise and the
    rewards entering ppo_ops.gae recorded.  Equal parameters bit for bit, no new function reached, the rollout's own
    reward_train and the records' own reward handed to gae as they are, and no new state on the trainer."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)          # scoped: separate runs must agree bit for bit
    want = nets(rollouts())
    from twoarmy_amd import ppo_ops

    def never(*a, **kw):
        raise AssertionError("the reward normalisation ran without enable_reward_norm()")
    for f in ("reward_norm_update", "reward_norm_apply", "reward_norm_read"):
        monkeypatch.setattr(ppo_ops, f, never)
    calls, seen = [], []
    spy_on_gae(monkeypatch, calls)

    def inspect(tr, r):
        seen.append((tr.reward_train.data_ptr(), tr.her["reward"].data_ptr(), int(tr.her["t"].numel())))
    tr = rollouts(inspect=inspect)
    assert same_nets(nets(tr), want)
    assert tr.reward_norm is None and not hasattr(tr, "reward_scaled") and tr.reward_train is tr.reward
    assert len(calls) == 4 and all(h > 0 for _, _, h in seen)
    assert [c[1] for c in calls] == [p for a, b, _ in seen for p in (a, b)]   # the very tensors, no copy between


def test_with_it_targets_see_scaled_copies_and_everything_else_stays_raw(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    calls, raw, kept = [], [], {}
    spy_on_gae(monkeypatch, calls)
    clip = 2.0

    def inspect(tr, r):
        assert tr.reward_train is not tr.reward                               # the bonus stage made its own tensor
        raw.append(dict(reward=host(tr.reward).copy(), train=host(tr.reward_train).copy(), term=host(tr.term).copy(),
                        trunc=host(tr.trunc).copy(), her=host(tr.her["reward"]).copy(), done=host(tr.her["done"]).copy(),
                        her_tensor=tr.her["reward"]))
        if r == 1:
            kept["state"] = tr.reward_norm.state_dict()                       # as the first update left it

    def after(tr, r):
        w = raw[r]
        assert same_bits(host(tr.reward), w["reward"]) and same_bits(host(tr.reward_train), w["train"])
        assert same_bits(host(w["her_tensor"]), w["her"])                     # the records the update trained on: still raw
        w["scaled"] = host(tr.reward_scaled).copy()
        w["stats"], w["carry"] = host(tr.reward_norm.stats).copy(), host(tr.reward_norm.ret_carry).copy()
        if r == 1:                                                            # a state_dict round trip continues with equal bits
            from twoarmy_amd.exploration import RewardNormalizer
            twin = RewardNormalizer(TR_N, 0.5, 0.0, DEV)
            twin.load_state_dict(kept["state"])
            twin.update(tr.reward_train, tr.term, tr.trunc)
            assert same_bits(host(twin.stats), w["stats"]) and same_bits(host(twin.ret_carry), w["carry"])
            assert same_bits(host(twin.apply(tr.reward_train)), w["scaled"])

    tr = rollouts(dict(clip=clip, hindsight=True), bonus=True, inspect=inspect, after=after)
    gamma = tr.agent.gamma
    carry, stats = np.zeros(TR_N), np.zeros(4)
    assert len(calls) == 4
    for r, w in enumerate(raw):
        assert not same_bits(w["train"], w["reward"])                         # the bonus is in what gets normalised
        carry, stats = rn.update(w["train"], w["term"], w["trunc"], gamma, carry, stats)
        assert same_bits(w["stats"], stats) and same_bits(w["carry"], carry)  # once per collect(), from reward_train
        want = rn.apply(w["train"], stats, clip)
        assert same_bits(calls[2 * r][0], want) and same_bits(w["scaled"], want)
        hwant = rn.apply(w["her"], stats, clip)
        assert w["her"].size > 0 and same_bits(calls[2 * r + 1][0].reshape(-1), hwant)
        last = (w["done"] != 0) & (w["her"] == np.float32(0.9))
        assert last.any() and (hwant[last] == min(np.float32(0.9) * np.float32(stats[3]), np.float32(clip))).all()
        assert not same_bits(hwant, w["her"]) and not same_bits(want, w["train"])
    assert stats[0] == 2 * TR_T * TR_N and tr.reward_norm_stats()["count"] == stats[0]
    assert tr.reward_norm_stats()["std"] == (stats[2] / stats[0]) ** 0.5
    # the history window of the next relabel() holds the raw training reward, and the accounting the raw task reward
    assert same_bits(host(tr._hist[-1][3]), raw[1]["train"])


def test_the_accounting_does_not_see_the_scale_and_the_update_does():
    """One rollout with and without: the policy that acts is the same, so the episode accounting must be."""
    seen = []

    def inspect(tr, r):
        seen.append(tr.episode_stats())
    with_norm = nets(rollouts(dict(clip=10.0, hindsight=True), n_rollouts=1, inspect=inspect))
    plain = nets(rollouts(n_rollouts=1, inspect=inspect))
    for k in ("score", "mean_return", "min_return", "max_return", "reward_hist"):
        assert np.array_equal(np.asarray(seen[0][k]), np.asarray(seen[1][k])), k
    assert seen[0]["reward_hist"][5] == 0                                     # nothing but the task's five values
    assert not same_nets(with_norm, plain)


def test_hindsight_off_leaves_the_records_raw(monkeypatch):
    calls, raw = [], []
    spy_on_gae(monkeypatch, calls)

    def inspect(tr, r):
        raw.append((host(tr.reward_train).copy(), host(tr.her["reward"]).copy(), host(tr.term).copy(), host(tr.trunc).copy()))
    tr = rollouts(dict(clip=10.0, hindsight=False), n_rollouts=1, inspect=inspect)
    train, her, te, tru = raw[0]
    _, stats = rn.update(train, te, tru, tr.agent.gamma, np.zeros(TR_N), np.zeros(4))
    assert len(calls) == 2 and her.size > 0
    assert same_bits(calls[0][0], rn.apply(train, stats, 10.0)) and same_bits(calls[1][0].reshape(-1), her)


def test_enable_and_command_line_errors(capsys):
    from twoarmy_amd.soa import train_SoA, train_ppo
    tr = rollouts(n_rollouts=0)
    for kw in (dict(hindsight=1), dict(clip=float("nan"))):
        with pytest.raises(ValueError, match="enable_reward_norm"):
            tr.enable_reward_norm(**kw)
    for call in (tr.normalize_rewards, tr.reward_norm_stats):
        with pytest.raises(RuntimeError, match="enable_reward_norm"):
            call()
    args = ["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", "8", "--rollout_steps", "16", "--minibatch", "64",
            "--updates", "1", "--k_epochs", "1", "--max_steps", "10", "--cuda", "cuda:0"]
    for extra, msg in ((["--reward_norm_clip", "5"], "need --reward_norm"),
                       (["--reward_norm_no_hindsight"], "need --reward_norm"),
                       (["--reward_norm", "--reward_norm_clip", "-1"], "must be a number >= 0"),
                       (["--reward_norm", "--reward_norm_clip", "nan"], "must be a number >= 0"),
                       (["--reward_norm", "--gamma", "1.5"], "--gamma in"),):
        with pytest.raises(SystemExit, match=msg):
            train_ppo.main(args + extra)
    with pytest.raises(SystemExit, match="self-orientation"):
        train_SoA.main(args + ["--reward_norm"])
    tr = train_ppo.main(args + ["--reward_norm", "--reward_norm_clip", "inf", "--reward_norm_no_hindsight"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert " rstd " in line and tr.reward_norm.clip == float("inf") and tr._reward_norm_hindsight is False
    assert float(line.split(" rstd ")[1].split()[0]) == pytest.approx(tr.reward_norm_stats()["std"], abs=1e-6)
