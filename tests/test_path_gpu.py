"""mg_nav_path_scan and mg_nav_path_summary on the device (include/minigrid_nav.h, "Path efficiency") against
tests/path_ref.py, through the torch front end, the C ABI, PathTracker, VecPPOTrainer and train_ppo --path_stats.  Every
integer is compared exactly; the two float64 sums of the summary within the bound tests/test_episode_stats_gpu.py uses for
ppo_episode_summary's return sum."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import episode_cases as EC
import nav_ref
import path_ref
import timed_nav_ref as tref
from nav_util import Boxed, dev, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = nav_ref.UNREACHABLE
BALL = 1 << 6
CASES = [(5, 4, 3, 7, 1), (5, 5, 65, 9, 3), (17, 17, 8, 16, 6), (7, 6, 2, 5, 16)]      # (W, H, N, T, P)
DTYPES = (torch.uint16, torch.uint16, torch.int32, torch.int32)        # start, best, off, steps
EXACT = [0, 1, 2, 4, 5, 7, 8, 9]                                        # summary entries that are integers or a minimum


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def sum_bound(terms, total):
    """The bound test_episode_stats_gpu.py sets for ppo_episode_summary's return sum, |got - want| <= episodes * 2^-53 *
    (the sum of the absolute terms): a tree against a sequential sum of `terms` float64 numbers.  The terms here are
    quotients in [0, 1], so the sum of their absolute values is the sum itself."""
    return terms * 2.0 ** -53 * total


def check_summary(got, want):
    got = np.asarray(got, np.float64)
    print("summary", got.tolist(), "vs", want.tolist())
    assert np.array_equal(got[EXACT], want[EXACT])
    assert abs(got[3] - want[3]) <= sum_bound(want[1], want[3])         # SPL: one term per success among the rated
    assert abs(got[6] - want[6]) <= sum_bound(want[2], want[6])         # progress: one term per rated episode at most


# ------------------------------------------------------------------------------------------------ cases
_CASES = {}


def case(W, H, N, T, P):
    """Random worlds with a goal each, their field (static for P = 1, timed over a random schedule otherwise), and one
    rollout of random walks: positions on walls, outside the world and NaN, ages that follow the done flags from a running
    episode on (so they cross 0) with a few negative ones, at least two done steps per env, carries of running episodes."""
    key = (W, H, N, T, P)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * W + 100 * H + 10 * N + T + P)
    ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
    for n in range(N):
        ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.1, 0.2, 0.3)[n % 3])
    gc = np.array([rng.choice(np.flatnonzero(ty[n] == 1)) if (ty[n] == 1).any() else 0 for n in range(N)])
    goal = ((gc % W).astype(np.int32), (gc // W).astype(np.int32))
    if P == 1:
        dist = nav_ref.fields(ty, st, W, H, goal=goal)[0]
    else:
        sched = tref.random_schedule(rng, P, H, 0.1).astype(np.int64)
        dist = tref.fields(ty, st, W, H, sched, P, goal=goal)[0]
    assert (dist == U).any() and (dist != U).any()
    xy = np.stack([rng.integers(0, W, N), rng.integers(0, H, N)], 1)
    walk = np.zeros((T + 1, N, 2), np.float32)
    for t in range(T + 1):
        walk[t, :, 0], walk[t, :, 1] = xy[:, 1] + rng.choice([0.0, 0.5, 0.999], N), xy[:, 0] + rng.choice([0.0, 0.5, 0.999], N)
        xy = np.clip(xy + np.array([(-1, 0), (1, 0), (0, -1), (0, 1), (0, 0)])[rng.integers(0, 5, N)], -1, (W, H))
    before, after = walk[:-1].copy(), walk[1:].copy()
    M = T * N
    after.reshape(-1, 2)[0] = (np.nan, 0.5)
    before.reshape(-1, 2)[M // 3] = (np.nan, np.nan)
    after.reshape(-1, 2)[M // 2] = (0.5, np.inf)
    before.reshape(-1, 2)[M - 1] = (-0.25, 0.5)
    after.reshape(-1, 2)[M - 2] = (0.5, W + 3.0)
    done = rng.random((T, N)) < 0.15
    for n in range(N):
        done[rng.choice(T, 2, replace=False), n] = True                  # two done steps per env at least
    term = (done & (rng.random((T, N)) < 0.6)).astype(np.uint8)
    trunc = (done & ((term == 0) | (rng.random((T, N)) < 0.2))).astype(np.uint8)
    assert ((term | trunc) != 0).sum(0).min() >= 2 and (term & trunc).any() or M < 40
    age = np.zeros((T, N), np.int32)
    a = rng.integers(0, 5, N).astype(np.int32)
    for t in range(T):
        age[t] = a
        a = np.where(done[t], 0, a + 1)
    age.reshape(-1)[:: max(2, M // 5)] = -2
    init = np.array([H - 0.5, 0.25], np.float32)
    carry = (rng.integers(0, 40, N).astype(np.uint16), rng.integers(0, 40, N).astype(np.uint16),
             rng.integers(0, 9, N).astype(np.int32), rng.integers(0, 9, N).astype(np.int32))
    np.minimum(carry[1], carry[0], out=carry[1])                          # an episode never stands farther than it started
    carry[3][0] = 0                                                       # env 0: no episode is running
    carry[0][N - 1] = U                                                   # the last env runs an unrated episode
    carry[3][N - 1] = 3
    c = dict(W=W, H=H, N=N, T=T, P=P, dist=dist, before=before, after=after, term=term, trunc=trunc, age=age, init=init,
             carry=carry)
    c["want"] = path_ref.path_scan(dist, before, after, W, H, term, trunc, carry, age, init)
    for a in (dist, before, after, term, trunc, age) + carry + c["want"][0] + c["want"][1]:
        a.setflags(write=False)
    _CASES[key] = c
    return c


def device_field(c, pad):
    """The case's field on the device, dense or with `pad` elements of 0x5A5A behind every row -> (field, check)."""
    d = c["dist"]
    if not pad:
        return dev(d), lambda: True
    HW = c["W"] * c["H"]
    full = torch.full(d.shape[:-1] + (HW + pad,), 0x5A5A, dtype=torch.int16, device=DEV).view(torch.uint16)
    field = full[..., :HW]
    field.copy_(dev(d))
    return field, lambda: bool((host(full.view(torch.int16))[..., HW:] == 0x5A5A).all())


def run_scan(c, cuts, want_out=(True,) * 4, pad=0, with_age=True, carry=None):
    """path_scan over consecutive launches of the given lengths; carries and outputs in 0xA5 buffers at odd offsets whose
    borders are checked -> (host outputs, None where not asked for; host carries)."""
    N, T = c["N"], c["T"]
    assert sum(cuts) == T
    field, pad_ok = device_field(c, pad)
    cbox = [Boxed(N, dt, off) for dt, off in zip(DTYPES, (1, 3, 1, 2))]
    for b, v in zip(cbox, c["carry"] if carry is None else carry):
        b.view.copy_(dev(v))
    obox = [Boxed(T * N, dt, off, (T, N)) for dt, off in zip(DTYPES, (3, 1, 2, 1))]
    before, after, term, trunc, age = (dev(c[k]) for k in ("before", "after", "term", "trunc", "age"))
    init = dev(c["init"])
    t = 0
    for k in cuts:
        sl = slice(t, t + k)
        outs = tuple(b.view[sl] if w else False for b, w in zip(obox, want_out))
        got = nav().path_scan(field, before[sl], after[sl], c["W"], c["H"], term[sl], trunc[sl],
                              tuple(b.view for b in cbox), age=age[sl] if with_age else None,
                              init_pos=init if with_age else None, out=outs)
        assert all((g is None) == (not w) for g, w in zip(got, want_out))
        t += k
    torch.cuda.synchronize()
    assert all(b.borders_intact() for b in cbox + obox) and pad_ok()
    assert all(b.untouched() for b, w in zip(obox, want_out) if not w)
    return (tuple(host(b.view) if w else None for b, w in zip(obox, want_out)), tuple(host(b.view) for b in cbox))


def assert_scan(got, want, what):
    for g, w, name in zip(got[0] + got[1], want[0] + want[1], ("ep_start", "ep_best", "ep_off", "ep_steps",
                                                               "carry_start", "carry_best", "carry_off", "carry_steps")):
        if g is not None:
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:8])


# ------------------------------------------------------------------------------------------------ the scan
@pytest.mark.parametrize("W,H,N,T,P", CASES)
def test_scan_equals_the_restatement(W, H, N, T, P):
    c = case(W, H, N, T, P)
    want = c["want"]
    done = (c["term"] | c["trunc"]) != 0
    assert (want[0][2][done] > 0).any() and (want[0][0][done] == U).any() or N < 8      # off-path steps, unrated episodes
    for pad in (0, 3):                                                    # dist_pitch dense and W * H + 3
        assert_scan(run_scan(c, [T], pad=pad), want, ("one launch", pad))
        assert_scan(run_scan(c, [1] * T, pad=pad), want, ("T launches", pad))       # bit-equal, carries included
    assert_scan(run_scan(c, [T // 2, T - T // 2]), want, "two launches")
    for absent in range(4):                                               # each output NULL in turn
        w = tuple(k != absent for k in range(4))
        assert_scan(run_scan(c, [T], want_out=w), want, ("absent", absent))
    zero = path_ref.zero_carry(N)                                         # and from a reset: no episode is running
    assert_scan(run_scan(c, [T], carry=zero),
                path_ref.path_scan(c["dist"], c["before"], c["after"], W, H, c["term"], c["trunc"], zero, c["age"], c["init"]),
                "zero carries")


def test_scan_without_age_takes_the_positions_as_they_stand():
    c = case(5, 4, 3, 7, 1)
    want = path_ref.path_scan(c["dist"], c["before"], c["after"], 5, 4, c["term"], c["trunc"], c["carry"])
    assert_scan(run_scan(c, [7], with_age=False), want, "no age")
    assert not np.array_equal(want[0][0], c["want"][0][0]) or not np.array_equal(want[0][2], c["want"][0][2])


def test_scan_of_an_empty_rollout_launches_nothing():
    c = case(5, 4, 3, 7, 1)
    e, f = torch.empty((0, 3, 2), dtype=torch.float32, device=DEV), torch.empty((0, 3), dtype=torch.uint8, device=DEV)
    carry = tuple(dev(v) for v in c["carry"])
    out = nav().path_scan(dev(c["dist"]), e, e, 5, 4, f, f, carry)
    assert all(o.shape == (0, 3) and o.dtype == dt for o, dt in zip(out, DTYPES))
    assert all(np.array_equal(host(g), w) for g, w in zip(carry, c["carry"]))


# ------------------------------------------------------------------------------------------------ the summary
def episodes_for_summary(T, N, seed):
    """Scan outputs of a random rollout by the restatement: random distances, done flags, some unrated episodes."""
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 30, (T, N))
    da = np.where(rng.random((T, N)) < 0.6, np.maximum(db - 1, 0), db + rng.integers(0, 2, (T, N)))
    db[rng.random((T, N)) < 0.05] = U
    da[rng.random((T, N)) < 0.05] = U
    term = (rng.random((T, N)) < 0.05).astype(np.uint8)
    trunc = (rng.random((T, N)) < 0.04).astype(np.uint8)
    outs, _ = path_ref.scan_distances(db, da, term, trunc, path_ref.zero_carry(N))
    return outs, term, trunc


@pytest.mark.parametrize("T,N", [(1, 1), (7, 3), (300, 130), (2049, 4)], ids=["1x1", "7x3", "300x130", "2049x4"])
def test_summary_against_the_restatement(T, N):
    outs, term, trunc = episodes_for_summary(T, N, 7 * T + N)
    if T * N == 1:
        term[0, 0] = 1
    want = path_ref.path_summary(*outs, term, trunc)
    assert T * N < 100 or (want[0] > want[2] > want[1] > 0 and want[3] > 0 and want[6] > 0)
    words = nav().path_summary_workspace(T, N)
    assert words == 10 * min(256, -(-T * N // 2048))
    sbox, wbox = Boxed(10, torch.float64, 1), Boxed(words, torch.float64, 1)
    got = nav().path_summary(*(dev(o) for o in outs), dev(term), dev(trunc), summary=sbox.view, workspace=wbox.view)
    assert got is sbox.view
    check_summary(host(got), want)
    assert sbox.borders_intact() and wbox.borders_intact()
    again = nav().path_summary(*(dev(o) for o in outs), dev(term), dev(trunc))           # deterministic: the same bits
    assert np.array_equal(host(again).view(np.int64), host(got).view(np.int64))


def test_summary_of_a_rollout_without_a_done_step():
    T, N = 40, 130
    outs, term, _ = episodes_for_summary(T, N, 5)
    none = np.zeros((T, N), np.uint8)
    got = host(nav().path_summary(*(dev(o) for o in outs), dev(none), dev(none)))
    assert not got[:9].any() and got[9] == np.inf
    tr = nav().PathTracker(N, DEV, 5, 4)
    assert tr.read()["episodes"] == 0 and tr.read()["best_min"] == np.inf and tr.read()["spl"] is None


_SWEEP = {}


def sweep_case(M):
    """Flat scan outputs for M elements, made directly (no scan): done steps at a low random density and at both ends of
    every workgroup's share and of the whole range (the grid rule ppo_episode_summary documents, tests/episode_cases.py);
    some unrated episodes, best <= start.  The restatement's summary is computed once per M."""
    if M not in _SWEEP:
        rng = np.random.default_rng(900 + M)
        done = rng.random(M) < min(0.05, 1200.0 / M)
        done[EC.boundaries(M)] = True
        term = (done & (rng.random(M) < 0.6)).astype(np.uint8)
        trunc = (done & ((term == 0) | (rng.random(M) < 0.2))).astype(np.uint8)
        start = rng.integers(0, 40, M).astype(np.uint16)
        start[rng.random(M) < 0.05] = U
        best = np.where(start == U, U, rng.integers(0, 40, M) % (start.astype(np.int64) + 1)).astype(np.uint16)
        outs = (start, best, rng.integers(0, 50, M).astype(np.int32), rng.integers(1, 51, M).astype(np.int32))
        want = path_ref.path_summary(*(o.reshape(1, M) for o in outs), term.reshape(1, M), trunc.reshape(1, M))
        _SWEEP[M] = (outs, term, trunc, want)
    return _SWEEP[M]


@pytest.mark.parametrize("M", EC.PATH_SWEEP_M)
def test_summary_at_every_grid_boundary(M):
    """1 -> 2 workgroups, 64 -> 65 partials, the 256-workgroup cap and the first thread run longer than 8 elements, each
    as [1][M] and [M][1], the workspace of exactly the queried size and filled with NaN."""
    outs, term, trunc, want = sweep_case(M)
    g = EC.grid(M)
    assert want[0] >= 2 * g["nblocks"] - 1 and want[0] > want[2] > want[1] > 0 and want[3] > 0 and want[6] > 0
    for T, N in ((1, M), (M, 1)):
        words = nav().path_summary_workspace(T, N)
        assert words == 10 * g["nblocks"]
        sbox, wbox = Boxed(10, torch.float64, 1), Boxed(words, torch.float64, 1)
        wbox.view.fill_(float("nan"))
        got = nav().path_summary(*(dev(o).view(T, N) for o in outs), dev(term).view(T, N), dev(trunc).view(T, N),
                                 summary=sbox.view, workspace=wbox.view)
        check_summary(host(got), want)
        assert sbox.borders_intact() and wbox.borders_intact() and not np.isnan(host(wbox.view)).any()


# ------------------------------------------------------------------------------------------------ the tracker
@pytest.mark.parametrize("W,H,N,T,P", [CASES[1], CASES[0]])
def test_tracker_carries_episodes_across_rollouts(W, H, N, T, P):
    c = case(W, H, N, T, P)
    tr = nav().PathTracker(N, DEV, W, H, period=P)
    carry = path_ref.zero_carry(N)
    args = [dev(c[k]) for k in ("dist", "before", "after", "term", "trunc", "age", "init")]
    for k in range(2):                                                    # the same rollout twice: the second continues
        tr.account(*args)
        outs, carry = path_ref.path_scan(c["dist"], c["before"], c["after"], W, H, c["term"], c["trunc"], carry, c["age"],
                                         c["init"])
        assert all(np.array_equal(host(g), w) for g, w in zip(tr.steps, outs)), k
        assert all(np.array_equal(host(g), w) for g, w in zip(tr.carry, carry)), k
        want = path_ref.path_summary(*outs, c["term"], c["trunc"])
        check_summary(host(tr.summary), want)
        st = tr.read()
        assert [st[name] for name in path_ref.SUMMARY][:3] == want[:3].tolist() and st["off_sum"] == want[7]
        for name, w in path_ref.derived(want).items():
            assert (st[name] is None and w is None) or abs(st[name] - w) <= 1e-12, name
    tr.reset()
    assert not any(host(x).any() for x in tr.carry)


# ------------------------------------------------------------------------------------------------ argument rejection
def test_bad_arguments_launch_nothing():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    v = lambda x: None if x is None else C.c_void_p(x)                                     # noqa: E731
    W, H, N, T = 5, 4, 3, 2
    dist = torch.zeros((N, 2, W * H + 1), dtype=torch.int16, device=DEV)
    pos = torch.zeros((T + 1, N, 2), dtype=torch.float32, device=DEV)
    age = torch.ones((T + 1, N), dtype=torch.int32, device=DEV)
    init = torch.zeros(4, dtype=torch.float32, device=DEV)
    flags = torch.ones(T * N + 1, dtype=torch.uint8, device=DEV)
    carries = [Boxed(N + 2, dt) for dt in DTYPES]
    outs = [Boxed(T * N + 2, dt) for dt in DTYPES]
    summ, work = Boxed(12, torch.float64), Boxed(12, torch.float64)
    cs, cb, co, ck = (b.view.data_ptr() for b in carries)
    es, eb, eo, ek = (b.view.data_ptr() for b in outs)

    def scan(a):
        return lib.mg_nav_path_scan(v(a["dist"]), a["pitch"], a["P"], a["n"], a["W"], a["H"], v(a["pb"]), v(a["pa"]),
                                    v(a["age"]), v(a["init"]), v(a["term"]), v(a["trunc"]), a["T"], v(a["cs"]), v(a["cb"]),
                                    v(a["co"]), v(a["ck"]), v(a["es"]), v(a["eb"]), v(a["eo"]), v(a["ek"]), None)

    def summary(a):
        return lib.mg_nav_path_summary(v(a["es"]), v(a["eb"]), v(a["eo"]), v(a["ek"]), v(a["term"]), v(a["trunc"]), a["T"],
                                       a["n"], v(a["summary"]), v(a["work"]), None)

    good = dict(dist=dist.data_ptr(), pitch=0, P=1, n=N, W=W, H=H, pb=pos.data_ptr(), pa=pos.data_ptr() + 8 * N,
                age=age.data_ptr(), init=init.data_ptr(), term=flags.data_ptr(), trunc=flags.data_ptr() + 1, T=T, cs=cs, cb=cb,
                co=co, ck=ck, es=es, eb=eb, eo=eo, ek=ek, summary=summ.view.data_ptr(), work=work.view.data_ptr())
    bad_scan = [dict(dist=None), dict(dist=good["dist"] + 1), dict(pitch=-1), dict(pitch=W * H - 1),      # mg_nav_shape's
                dict(P=0), dict(P=17), dict(P=-1), dict(P=2, age=None, init=None), dict(P=2, age=None),
                dict(pb=None), dict(pa=None), dict(n=0), dict(n=-1), dict(W=0), dict(H=0), dict(W=33), dict(H=33),
                dict(T=-1), dict(pb=good["pb"] + 4), dict(pa=good["pa"] + 4), dict(age=good["age"] + 2),
                dict(init=good["init"] + 1), dict(init=None), dict(T=1 << 30, n=1 << 10),
                dict(term=None), dict(trunc=None),                                                       # NULL flags
                dict(cs=None), dict(cb=None), dict(co=None), dict(ck=None),                              # NULL carries
                dict(cs=cs + 1), dict(cb=cb + 1), dict(co=co + 2), dict(ck=ck + 1),                      # misaligned carries
                dict(es=es + 1), dict(eb=eb + 1), dict(eo=eo + 2), dict(ek=ek + 3),                      # misaligned outputs
                dict(es=None, eb=None, eo=None, ek=None)]                                                # no output
    for kw in bad_scan:
        assert scan(dict(good, **kw)) == -1, kw
    bad_summary = [dict(es=None), dict(eb=None), dict(eo=None), dict(ek=None), dict(term=None), dict(trunc=None),
                   dict(summary=None), dict(work=None), dict(T=0), dict(T=-1), dict(n=0), dict(T=1 << 30, n=1 << 10),
                   dict(es=es + 1), dict(eb=eb + 1), dict(eo=eo + 2), dict(ek=ek + 2), dict(summary=good["summary"] + 4),
                   dict(work=good["work"] + 4)]
    for kw in bad_summary:
        assert summary(dict(good, **kw)) == -1, kw
    assert lib.mg_nav_path_summary_workspace(0, 8) == -1 and lib.mg_nav_path_summary_workspace(8, -1) == -1
    assert lib.mg_nav_path_summary_workspace(1 << 30, 1 << 10) == -1
    assert scan(dict(good, T=0)) == 0                                     # nothing to do: ok, no launch
    torch.cuda.synchronize()
    assert all(b.untouched() for b in carries + outs + [summ, work])
    # and the good calls launch: from zeroed carries every step stands on cell 0 of an all-zero field, at distance 0, and
    # ends an episode of its own, one step long and off path (no step at distance 0 is on path)
    for b in carries:
        b.view.view(torch.int16 if b.view.dtype == torch.uint16 else torch.int32).zero_()
    assert scan(good) == 0 and summary(good) == 0
    assert scan(dict(good, P=2, pitch=W * H + 1, es=None, eo=None, ek=ek + 4)) == 0
    torch.cuda.synchronize()
    assert all(b.borders_intact() for b in carries + outs + [summ, work])
    assert host(outs[3].view)[:T * N + 1].tolist() == [1] * (T * N + 1) and host(outs[2].view)[:T * N].tolist() == [1] * (T * N)
    assert not host(outs[0].view)[:T * N].any() and not host(carries[3].view)[:N].any()
    assert host(summ.view)[:10].tolist() == [T * N, T * N, T * N, 0.0, 0, 0, 0.0, T * N, T * N, 0]


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer(N, T, max_steps=50, seed=5):
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(seed)
    eng = TwoarmyEngine(6, N, 17, seed=9981, max_steps=max_steps)
    agent = PPO()
    agent.to(eng.device).use_nhwc()
    return VecPPOTrainer(agent, eng, rollout_steps=T, minibatch=64, value_chunk=64), eng


@pytest.mark.parametrize("timed", [False, True], ids=["static", "timed"])
def test_trainer_accounts_paths_across_rollouts(timed):
    N, T = 8, 16
    tr, eng = _trainer(N, T, max_steps=11)                                # short episodes: several end in every rollout
    with pytest.raises(RuntimeError, match="account_paths"):
        tr.path_stats()
    carry = path_ref.zero_carry(N)
    seen = 0
    for u in range(2):
        tr.collect()
        assert tr.paths is None or u == 1
        tr.account_paths(timed=timed)
        field = host(tr.timed_field if timed else tr.nav_field)
        assert field.shape == ((N, 6, 289) if timed else (N, 289)) and (tr.timed_field is None) == (not timed)
        ty = eng.get_state()[0].reshape(N, 289)                           # the field is the map as the rollout left it
        if timed:
            sched = nav().twoarmy_schedule(blocks=True).numpy().astype(np.int64)
            assert np.array_equal(field, tref.fields(ty, None, 17, 17, sched, 6, nav_ref.PASS_DEFAULT | BALL)[0])
        else:
            assert np.array_equal(field, nav_ref.fields(ty, None, 17, 17, nav_ref.PASS_DEFAULT | BALL)[0])
        before, after = host(tr.pos[3:3 + T]), host(tr.pos[4:4 + T])
        term, trunc = host(tr.term), host(tr.trunc)
        outs, carry = path_ref.path_scan(field, before, after, 17, 17, term, trunc, carry, host(tr.age[:-1]),
                                         host(tr.init_pos))
        assert all(np.array_equal(host(g), w) for g, w in zip(tr.paths.steps, outs)), u
        assert all(np.array_equal(host(g), w) for g, w in zip(tr.paths.carry, carry)), u
        want = path_ref.path_summary(*outs, term, trunc)
        st = tr.path_stats()
        check_summary([st[k] for k in path_ref.SUMMARY], want)
        for name, w in path_ref.derived(want).items():
            assert (st[name] is None and w is None) or abs(st[name] - w) <= 1e-12, name
        done = (term | trunc) != 0
        assert want[0] == done.sum() >= N and want[2] > 0
        if u == 1:                                                        # episodes that began in the first rollout end here
            assert (outs[3][done] > np.nonzero(done)[0] + 1).any()
        seen += int(want[0])
        tr.carry_over()
    with pytest.raises(RuntimeError, match="one tracker"):
        tr.account_paths(timed=not timed)
    assert seen >= 2 * N
    eng.close()


def test_one_timed_field_serves_the_prior_the_shaping_and_the_paths(monkeypatch):
    """enable_prior(timed=True), enable_shaping(timed=True) and account_paths(timed=True) on one trainer: after one rollout
    every consumer's outputs are bit for bit those of a trainer with that feature alone (same seed, same uniforms), the
    trainer holds exactly one uint16[N, 6, 289] buffer, and the front end's launches show one mg_nav_timed_field for the
    rollout."""
    N, T = 8, 16
    names = []
    real = nav().call
    monkeypatch.setattr(nav(), "call", lambda name, *args: (names.append(name), real(name, *args))[1])
    uni = torch.rand(T, N, generator=torch.Generator().manual_seed(40)).to(DEV)

    def run(prior, shaping, paths):
        tr, eng = _trainer(N, T, max_steps=11)
        if prior:
            tr.enable_prior(0.5, timed=True)
        if shaping:
            tr.enable_shaping(0.05, hindsight=False, timed=True)
        del names[:]
        tr.collect(uniforms=uni)
        tr.shape_rewards()
        if prior:
            tr.label_expert()
        if shaping:
            tr.shape_potential()
        if paths:
            tr.account_paths(timed=True)
        torch.cuda.synchronize()
        eng.close()
        return tr, names.count("mg_nav_timed_field")

    (both, n_all), (prior, n_p), (shaped, n_s), (paths, n_a) = run(1, 1, 1), run(1, 0, 0), run(0, 1, 0), run(0, 0, 1)
    assert (n_all, n_p, n_s, n_a) == (1, 1, 1, 1)
    for other in (prior, shaped, paths):
        for k in ("pos", "age", "reward", "term", "trunc"):
            assert np.array_equal(host(getattr(both, k)), host(getattr(other, k))), k
    for k in ("expert_moves", "expert_dist"):
        assert np.array_equal(host(getattr(both, k)), host(getattr(prior, k))), k
    for k in ("shape_f", "shape_mask", "reward_train"):
        assert np.array_equal(host(getattr(both, k)).view(np.uint8), host(getattr(shaped, k)).view(np.uint8)), k
    assert host(both.shape_mask).any() and host(both.expert_moves).any()
    assert np.array_equal(host(both.paths.summary).view(np.uint64), host(paths.paths.summary).view(np.uint64))
    assert all(np.array_equal(host(a), host(b)) for a, b in zip(both.paths.steps, paths.paths.steps))
    assert host(both.paths.summary)[0] > 0
    fields = [v for v in vars(both).values()
              if torch.is_tensor(v) and v.dtype == torch.uint16 and tuple(v.shape) == (N, 6, 289)]
    assert len(fields) == 1 and fields[0] is both.timed_field
    for other in (prior, shaped, paths):
        assert np.array_equal(host(both.timed_field), host(other.timed_field))


def test_an_env_driven_by_the_timed_expert_reaches_spl_one():
    """The trainer's rollout with the policy replaced by the timed expert's action for the state as it stands (policy index
    4 = the env's `done` = wait): every step is on path in the timed field, every episode ends in success after exactly
    its start distance, across rollout boundaries."""
    N, T = 8, 16
    tr, eng = _trainer(N, T)
    logp = torch.zeros(N, dtype=torch.float32, device=DEV)

    def expert(*args, **kwargs):
        a = eng.timed_field(want_field=False)[2]
        return torch.where((a < 0) | (a > 3), 4, a).to(torch.int32), logp

    tr.agent.act_batch = expert
    episodes = 0
    for u in range(4):                                                    # 64 steps: the reset lies 24 .. 49 steps from the goal
        tr.collect()
        tr.account_paths(timed=True)
        st = tr.path_stats()
        print("rollout", u, st)
        assert st["off_sum"] == 0 and not tr.trunc.any()
        if st["episodes"]:
            assert st["successes"] == st["rated"] == st["episodes"] and st["spl"] == 1.0 and st["progress"] == 1.0
            assert st["steps_sum"] == st["start_sum"] and st["best_min"] == 0 and st["off_path_rate"] == 0.0
        episodes += st["episodes"]
        tr.carry_over()
    assert episodes >= N
    eng.close()


ENTRY_ARGS = ["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", "8", "--rollout_steps", "16", "--minibatch", "32",
              "--k_epochs", "1", "--updates", "1", "--max_steps", "11", "--cuda", "cuda:0"]


def test_train_ppo_path_stats_appends_fields_and_leaves_the_update_alone(capsys, monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # scoped: separate runs must agree bit for bit
    from twoarmy_amd.soa import train_ppo
    runs = [train_ppo.main(ENTRY_ARGS + extra) for extra in ([], ["--path_stats"], ["--path_stats", "--path_stats_timed"])]
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]
    assert len(lines) == 3
    opt = r"(?:-?\d+\.\d{4}|-)"
    tail = r" spl %s progress %s off_path %s$" % (opt, opt, opt)
    assert not re.search(r" spl ", lines[0]) and re.search(tail, lines[1]) and re.search(tail, lines[2])
    losses = [re.search(r"action_loss (\S+) value_loss (\S+)", ln).groups() for ln in lines]
    assert losses[0] == losses[1] == losses[2]
    strip = lambda ln: re.sub(r"rollout \S+ \(\S+ env-steps/s/rank\) update \S+ ", "", ln)              # noqa: E731
    assert strip(lines[1]).startswith(strip(lines[0])) and strip(lines[2]).startswith(strip(lines[0]))
    plain, static, timed = runs
    assert plain.paths is None and plain.timed_field is None and plain.nav_field is None            # no launch, no tensor
    assert static.paths.period == 1 and static.timed_field is None and timed.paths.period == 6
    for other in (static, timed):                                         # the update itself: every parameter bit for bit
        for net in ("actor", "critic"):
            for p, q in zip(getattr(plain.agent, net).parameters(), getattr(other.agent, net).parameters()):
                assert torch.equal(p, q)
    st = static.path_stats()
    assert st["episodes"] == int(((static.term | static.trunc) != 0).sum()) > 0
    with pytest.raises(SystemExit):
        train_ppo.main(ENTRY_ARGS + ["--path_stats_timed"])
