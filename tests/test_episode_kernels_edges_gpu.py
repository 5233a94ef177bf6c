"""ppo_episode_scan and ppo_episode_summary (include/twoarmy_ppo.h) at their edges on the MI355X: every boundary of the
scan's prefetch and of the summary's grid, the order of the fold, every action count, what is written and what is read,
and every argument rule.  Inputs, references and bounds come from tests/episode_cases.py; the bounds are derived and
checked on the CPU in tests/test_episode_edges_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import episode_cases as EC
import episode_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                                                        # guard elements on either side
NAN_SENTINEL = 0x7FF800005A5A5A5A                              # a quiet NaN with a payload
SENTINEL = {torch.float64: NAN_SENTINEL, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A}
RAW = {torch.float64: torch.int64, torch.int64: torch.int64, torch.int32: torch.int32}


def ops():
    from twoarmy_amd import ppo_ops
    return ppo_ops


def dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(DEV)          # a copy: the shared cases are read-only


def host(t):
    return t.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


class Guarded:
    """`n` elements of `dtype` with PAD elements before and behind them, the whole buffer filled with the sentinel."""

    def __init__(self, n, dtype, shape=None):
        self.n, self.s = n, SENTINEL[dtype]
        self.raw = torch.full((n + 2 * PAD,), self.s, dtype=RAW[dtype], device=DEV)
        self.view = self.raw[PAD:PAD + n].view(dtype).view(shape if shape is not None else (n,))

    def intact(self):
        r = host(self.raw)
        return bool((r[:PAD] == self.s).all() and (r[PAD + self.n:] == self.s).all())

    def untouched(self):
        return bool((host(self.raw) == self.s).all())

    def kept(self, lo):
        """Elements lo .. n-1 of the array itself still hold the sentinel."""
        return bool((host(self.raw)[PAD + lo:PAD + self.n] == self.s).all())


# ------------------------------------------------------------------------------------------------------------ the scan
def run_scan(c, want_return=True, want_length=True, carry=None):
    """One launch of ppo_episode_scan on the rollout `c`, every writable array guarded -> host (ep_return, ep_length,
    carry_return, carry_length), None for an output that was not asked for."""
    from twoarmy_amd import _marshal
    T, N = c["reward"].shape
    cr, cl = Guarded(N, torch.float64), Guarded(N, torch.int32)
    cr.view.copy_(dev(c["carry_return"] if carry is None else carry[0]))
    cl.view.copy_(dev(c["carry_length"] if carry is None else carry[1]))
    er, el = Guarded(T * N, torch.float64, (T, N)), Guarded(T * N, torch.int32, (T, N))
    r, term, trunc = dev(c["reward"]), dev(c["term"]), dev(c["trunc"])         # named: they live until the synchronise
    _marshal.call("ppo_episode_scan", r, _marshal.ptr(r, torch.float32), _marshal.ptr(term, torch.uint8),
                  _marshal.ptr(trunc, torch.uint8), T, N, _marshal.ptr(cr.view), _marshal.ptr(cl.view),
                  _marshal.ptr(er.view if want_return else None), _marshal.ptr(el.view if want_length else None))
    torch.cuda.synchronize()
    assert cr.intact() and cl.intact() and er.intact() and el.intact()
    assert (want_return or er.untouched()) and (want_length or el.untouched())
    return (host(er.view) if want_return else None, host(el.view) if want_length else None, host(cr.view), host(cl.view))


def assert_scan(got, want, what=None):
    if got[0] is not None:
        assert np.array_equal(bits(got[0]), bits(want[0])), what
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(bits(got[2]), bits(want[2])) and np.array_equal(got[3], want[3]), what


def scan_want(c, carry=None):
    return ER.episode_scan(c["reward"], c["term"], c["trunc"], *(carry or (c["carry_return"], c["carry_length"])))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 129])
def test_scan_shape_sweep(N):
    """Every T around the 8-row prefetch, as ONE launch with non-zero carries; outputs absent in turn at three shapes."""
    for T in (1, 7, 8, 9, 15, 16, 17, 25):
        c = EC.rollout(T, N, 100 * T + N)
        want = scan_want(c)
        assert c["carry_length"].all() and c["carry_return"].all()
        assert_scan(run_scan(c), want, (T, N))
        if (T, N) in ((9, 65), (17, 1), (16, 64)):
            for wr, wl in ((True, False), (False, True), (False, False)):
                got = run_scan(c, wr, wl)
                assert (got[0] is None) == (not wr) and (got[1] is None) == (not wl)
                assert_scan(got, want, (T, N, wr, wl))


@pytest.mark.parametrize("place", ["first", "last", "every", "none"])
def test_scan_flag_placement(place):
    T, N = 17, 65
    base = EC.rollout(T, N, 31)
    for kind in ("terminated", "truncated", "both"):
        flags = np.zeros((T, N), np.uint8)
        if place != "none":
            flags[{"first": 0, "last": T - 1, "every": slice(None)}[place]] = 1
        c = dict(base, term=flags if kind != "truncated" else np.zeros_like(flags),
                 trunc=flags if kind != "terminated" else np.zeros_like(flags))
        want = scan_want(c)
        got = run_scan(c)
        assert_scan(got, want, (place, kind))
        if place == "every":
            assert np.array_equal(bits(got[0][1:]), bits(c["reward"][1:].astype(np.float64))) and (got[1][1:] == 1).all()
        if place in ("last", "every"):
            assert not got[3].any() and np.array_equal(bits(got[2]), bits(np.zeros(N)))       # restarted from +0.0
        if place == "none":
            assert np.array_equal(got[3], c["carry_length"] + T)


def test_scan_writes_inside_its_arrays_only():
    """N = 65, T = 9: the second workgroup holds one env and the prefetch runs one row past a full batch; run_scan checks
    the guards of all four writable arrays, here with the outputs present and absent."""
    c = EC.rollout(9, 65, 77)
    want = scan_want(c)
    for wr, wl in ((True, True), (False, False)):
        assert_scan(run_scan(c, wr, wl), want)


def test_scan_confines_a_non_finite_reward_to_its_episode():
    T, N = 25, 65
    base = EC.rollout(T, N, 9)
    term, trunc, r = base["term"].copy(), base["trunc"].copy(), base["reward"].copy()
    nan_env, inf_env = 3, 64                                     # the second one alone in its workgroup
    term[:11, nan_env] = trunc[:11, nan_env] = 0
    term[10, nan_env] = 1
    term[:13, inf_env] = trunc[:13, inf_env] = 0
    trunc[12, inf_env] = 1
    clean = dict(base, term=term, trunc=trunc)
    r[4, nan_env] = np.nan
    r[2, inf_env], r[6, inf_env] = np.inf, -np.inf
    dirty = dict(clean, reward=r)
    a, b = run_scan(clean), run_scan(dirty)
    with np.errstate(invalid="ignore"):                          # inf - inf in the restatement
        assert_scan(b, scan_want(dirty))
    others = np.setdiff1d(np.arange(N), [nan_env, inf_env])
    assert np.array_equal(bits(a[0][:, others]), bits(b[0][:, others])) and np.array_equal(a[1], b[1])
    assert np.array_equal(bits(a[2][others]), bits(b[2][others])) and np.array_equal(a[3], b[3])
    assert np.isnan(b[0][4:11, nan_env]).all() and np.isfinite(b[0][:4, nan_env]).all()
    assert (b[0][2:6, inf_env] == np.inf).all() and np.isnan(b[0][6:13, inf_env]).all()
    for env, t0 in ((nan_env, 11), (inf_env, 13)):               # the next episode: the same steps from zero carries
        tail = dict(reward=r[t0:], term=term[t0:], trunc=trunc[t0:])
        fresh = run_scan(tail, carry=(np.zeros(N), np.zeros(N, np.int32)))
        assert np.isfinite(b[0][t0:, env]).all()
        assert np.array_equal(bits(b[0][t0:, env]), bits(fresh[0][:, env])) and np.array_equal(b[1][t0:, env], fresh[1][:, env])
        assert bits(b[2][env:env + 1]) == bits(fresh[2][env:env + 1]) and b[3][env] == fresh[3][env]


# --------------------------------------------------------------------------------------------------------- the summary
@functools.lru_cache(maxsize=None)
def _device_inputs(key):
    c = EC.order_case(key[1]) if key[0] == "order" else EC.summary_case(*key[1:])
    return {k: dev(c[k]) for k in ("ep_return", "ep_length", "term", "trunc", "reward", "action")}


def run_summary(key, T, N, A=5, keep=0.99, gain=0.01, score0=EC.SCORE0, with_action=True, workspace="nan", edit=None):
    """One call of ppo_episode_summary on a shared case viewed as [T][N]: every output guarded, action_hist a 7-entry
    sentinel buffer, the workspace of exactly the queried size and filled with NaN (or zeros) -> host results."""
    d = dict(_device_inputs(key))
    if edit:
        d.update(edit)
    v = {k: (None if t is None else t.view(T, N)) for k, t in d.items()}
    words = ops().episode_summary_workspace(T, N)
    assert words == 24 * EC.grid(T * N)["nblocks"]
    summ, ah, rh = Guarded(8, torch.float64), Guarded(7, torch.int64), Guarded(6, torch.int64)
    ws, sc = Guarded(words, torch.float64), Guarded(1, torch.float64)
    ws.view.fill_(float("nan") if workspace == "nan" else 0.0)
    if score0 is not None:
        sc.view.fill_(score0)
    ops().episode_summary(v["ep_return"], v["ep_length"], v["term"], v["trunc"], v["reward"],
                          v["action"] if with_action else None, A, keep, gain, sc.view if score0 is not None else None,
                          summ.view, ah.view[:A], rh.view, ws.view)
    torch.cuda.synchronize()
    assert all(g.intact() for g in (summ, ah, rh, ws, sc)) and ah.kept(A)
    assert score0 is not None or sc.untouched()
    return dict(summary=host(summ.view), action_hist=host(ah.view[:A]).tolist(), reward_hist=host(rh.view).tolist(),
                score=None if score0 is None else float(host(sc.view)[0]), workspace=host(ws.view))


@functools.lru_cache(maxsize=None)
def summary_want(key, A=5, keep=0.99, gain=0.01, score0=EC.SCORE0, with_action=True):
    """The sequential restatement; the row-major order of [1][M], [M][1] and every other [T][N] of one case is the same."""
    c = EC.order_case(key[1]) if key[0] == "order" else EC.summary_case(*key[1:])
    f = lambda a: a.reshape(1, -1)                                                          # noqa: E731
    return ER.episode_summary(f(c["ep_return"]), f(c["ep_length"]), f(c["term"]), f(c["trunc"]), f(c["reward"]),
                              f(c["action"]) if with_action and c["action"] is not None else None, A, keep, gain,
                              0.0 if score0 is None else score0)


def check_summary(got, want, returns, keep=0.99, gain=0.01, score0=EC.SCORE0):
    s, E = got["summary"], want["episodes"]
    print("episodes", E, "return_sum", s[3], "vs", want["return_sum"], "score", got["score"], "vs", want["score"])
    assert E == len(returns)
    assert [s[0], s[1], s[2], s[6], s[7]] == [E, want["successes"], want["truncated"], want["length_sum"], want["max_length"]]
    assert bits(s[4:6]).tolist() == bits([want["min_return"], want["max_return"]]).tolist()
    assert got["action_hist"] == want["action_hist"] and got["reward_hist"] == want["reward_hist"]
    assert abs(s[3] - want["return_sum"]) <= EC.sum_bound(E, returns)
    if got["score"] is not None:
        assert abs(got["score"] - want["score"]) <= EC.fold_bound(E, keep, gain, score0, returns)


@pytest.mark.parametrize("M", EC.SWEEP_M)
def test_summary_boundary_sweep(M):
    """Every grid boundary as [1][M] and [M][1] (and the two cap sizes in 2-D), done steps at both ends of every
    workgroup share, of thread runs and of the range; NaN returns and INT32_MIN lengths wherever no episode ends."""
    key = ("sweep", M)
    c, want = EC.summary_case(M), summary_want(key)
    assert want["episodes"] >= min(M, 2) and sum(want["reward_hist"]) == M and (want["reward_hist"][5] > 0 or M == 1)
    for T, N in [(1, M), (M, 1)] + ([EC.CAP_SHAPES[M]] if M in EC.CAP_SHAPES else []):
        check_summary(run_summary(key, T, N), want, c["returns"])


def test_summary_with_every_step_done():
    key = ("sweep", 4097, True)
    want = summary_want(key)
    assert want["episodes"] == 4097
    check_summary(run_summary(key, 17, 241), want, EC.summary_case(4097, True)["returns"])


@pytest.mark.parametrize("M", sorted(EC.ORDER_SHAPES))
def test_summary_order_matters(M):
    """keep = 0.5, gain = 1, returns over eleven orders of magnitude: the device lies within the bound of the row-major
    fold, and the column-major fold and the folds with two neighbouring shares exchanged lie far outside it."""
    c = EC.order_case(M)
    keep, gain, E = EC.ORDER_KEEP, EC.ORDER_GAIN, EC.ORDER_EPISODES
    key = ("order", M)
    want = summary_want(key, 5, keep, gain)
    got = run_summary(key, c["T"], c["N"], 5, keep, gain, with_action=False)
    check_summary(got, want, c["returns"], keep, gain)
    bound = EC.fold_bound(E, keep, gain, EC.SCORE0, c["returns"])
    others = [EC.column_major(c), EC.swapped_shares(c, 0)]
    if EC.grid(M)["nblocks"] > 2:
        others.append(EC.swapped_shares(c, EC.grid(M)["nblocks"] - 2))
    for returns in others:
        wrong = EC.fold_seq(returns, keep, gain, EC.SCORE0)
        print("wrong order", wrong, "row-major", want["score"], "device", got["score"], "bound", bound)
        assert abs(wrong - want["score"]) > 10 * bound and abs(wrong - got["score"]) > bound


@pytest.mark.parametrize("keep,gain", EC.KEEP_GAIN)
def test_summary_extreme_keep_and_gain(keep, gain):
    key, c = ("sweep", 2049), EC.summary_case(2049)
    want = summary_want(key, 5, keep, gain)
    got = run_summary(key, 3, 683, 5, keep, gain)
    check_summary(got, want, c["returns"], keep, gain)
    if keep == 0.0:
        assert bits([got["score"]])[0] == bits([gain * c["returns"][-1]])[0]                 # the last return alone
    if (keep, gain) == (1.0, 0.0):
        assert bits([got["score"]])[0] == bits([EC.SCORE0])[0]


@pytest.mark.parametrize("A", EC.ACTION_COUNTS)
def test_summary_every_action_count(A):
    """Actions from [-1, 8]: the first A bins are bincount's, the rest is counted nowhere, action_hist[A..6] keeps its
    sentinel (run_summary), and nothing else moves with A."""
    key, c = ("sweep", 2049), EC.summary_case(2049)
    want = summary_want(key, A)
    got = run_summary(key, 1, 2049, A)
    check_summary(got, want, c["returns"])
    a = c["action"]
    assert got["action_hist"] == np.bincount(a[(a >= 0) & (a < A)], minlength=A).tolist()
    assert sum(got["action_hist"]) < a.size and (a == -1).any() and (a == 8).any() and (a == A).any()
    assert np.array_equal(bits(got["summary"]), bits(run_summary(key, 1, 2049, 5)["summary"]))


def test_summary_optional_and_degenerate_inputs():
    key, c = ("sweep", 2049), EC.summary_case(2049)
    full = run_summary(key, 1, 2049)
    bare = run_summary(key, 1, 2049, with_action=False, score0=None)                       # action = NULL, score = NULL
    assert bare["action_hist"] == [0] * 5 and bare["score"] is None
    assert np.array_equal(bits(bare["summary"]), bits(full["summary"])) and bare["reward_hist"] == full["reward_hist"]
    none = torch.zeros(2049, dtype=torch.uint8, device=DEV)                                # no done step at all
    score0 = float(np.float64(0.1) / 3)
    got = run_summary(key, 1, 2049, score0=score0, edit=dict(term=none, trunc=none))
    s = got["summary"]
    assert bits([got["score"]])[0] == bits([score0])[0]
    assert s[4] == np.inf and s[5] == -np.inf and not s[[0, 1, 2, 3, 6, 7]].any()
    assert got["reward_hist"] == full["reward_hist"] and got["action_hist"] == full["action_hist"]


@pytest.mark.parametrize("M", [2049, 131073, 524289])
def test_summary_is_deterministic_and_needs_no_workspace_contents(M):
    key = ("sweep", M)
    a = run_summary(key, 1, M, workspace="nan")
    b = run_summary(key, 1, M, workspace="zero")
    assert np.array_equal(bits(a["summary"]), bits(b["summary"])) and bits([a["score"]])[0] == bits([b["score"]])[0]
    assert a["action_hist"] == b["action_hist"] and a["reward_hist"] == b["reward_hist"]
    assert np.array_equal(bits(a["workspace"]), bits(b["workspace"]))                        # every word was written


def test_summary_with_a_non_finite_return():
    """One NaN among the finite returns: counts, lengths and histograms as without it, min and max ignore it, the return
    sum and the score take it."""
    key, c = ("sweep", 131073), EC.summary_case(131073)
    clean = run_summary(key, 1, 131073)
    where = int(np.flatnonzero(c["done"])[len(c["returns"]) // 2])
    r = c["ep_return"].copy()
    r[where] = np.nan
    got = run_summary(key, 1, 131073, edit=dict(ep_return=dev(r)))
    assert np.array_equal(got["summary"][[0, 1, 2, 6, 7]], clean["summary"][[0, 1, 2, 6, 7]])
    assert got["action_hist"] == clean["action_hist"] and got["reward_hist"] == clean["reward_hist"]
    rest = np.delete(c["returns"], len(c["returns"]) // 2)
    assert bits(got["summary"][4:6]).tolist() == bits([rest.min(), rest.max()]).tolist()
    assert np.isnan(got["summary"][3]) and np.isnan(got["score"])


# ---------------------------------------------------------------------------------------------------------- rejections
def test_episode_rejections_launch_nothing():
    """Every TW_E_ARG case of the two entries through the raw C ABI: the code comes back, and after a synchronise every
    byte of every buffer still holds its sentinel.  T * N = 2^40 and the misaligned pointers are safe to pass only
    because the call returns before any launch -- which the size query, host code alone, shows first."""
    from twoarmy_amd import _lib, _marshal
    lib = _lib.lib()
    assert lib.ppo_episode_summary_workspace(1 << 20, 1 << 20) == -1 and lib.ppo_episode_summary_workspace(1 << 20, (1 << 20) - 1) > 0
    T, N, A = 4, 8, 5
    M = T * N
    size = dict(reward=4 * M, term=M, trunc=M, action=4 * M, carry_return=8 * N, carry_length=4 * N, ep_return=8 * M,
                ep_length=4 * M, score=8, summary=64, action_hist=56, reward_hist=48,
                workspace=8 * lib.ppo_episode_summary_workspace(T, N))
    offset, total = {}, 64
    for k, n in size.items():                                   # 64-byte aligned, at least 64 sentinel bytes between
        offset[k] = total
        total += (n + 63) // 64 * 64 + 64
    pool = torch.full((total,), 0x5A, dtype=torch.uint8, device=DEV)
    assert pool.data_ptr() % 64 == 0
    good = {k: pool.data_ptr() + o for k, o in offset.items()}
    good.update(T=T, N=N, A=A)
    v = lambda x: None if x is None else C.c_void_p(x)                                      # noqa: E731

    def scan(a):
        rc = lib.ppo_episode_scan(v(a["reward"]), v(a["term"]), v(a["trunc"]), a["T"], a["N"], v(a["carry_return"]),
                                  v(a["carry_length"]), v(a["ep_return"]), v(a["ep_length"]), _marshal.stream(pool))
        torch.cuda.synchronize()
        return rc

    def summary(a):
        rc = lib.ppo_episode_summary(v(a["ep_return"]), v(a["ep_length"]), v(a["term"]), v(a["trunc"]), v(a["reward"]),
                                     v(a["action"]), a["A"], a["T"], a["N"], 0.99, 0.01, v(a["score"]), v(a["summary"]),
                                     v(a["action_hist"]), v(a["reward_hist"]), v(a["workspace"]), _marshal.stream(pool))
        torch.cuda.synchronize()
        return rc

    off = lambda *ks, by: [{k: good[k] + by} for k in ks]                                   # noqa: E731
    shape = [dict(T=0), dict(T=-1), dict(N=0), dict(N=-1), dict(T=1 << 20, N=1 << 20)]
    bad_scan = [{k: None} for k in ("reward", "term", "trunc", "carry_return", "carry_length")] + shape
    bad_scan += off("carry_return", "ep_return", by=4) + off("reward", "carry_length", "ep_length", by=2)
    bad_summary = [{k: None} for k in ("ep_return", "ep_length", "term", "trunc", "reward", "summary", "reward_hist",
                                       "workspace")] + shape + [dict(A=1), dict(A=6), dict(A=8)]
    bad_summary += off("ep_return", "score", "summary", "workspace", "action_hist", "reward_hist", by=4)
    bad_summary += off("reward", "ep_length", "action", by=2)
    for fn, cases in ((scan, bad_scan), (summary, bad_summary)):
        for kw in cases:
            assert fn(dict(good, **kw)) == -1, (fn.__name__, kw)
            assert bool((pool == 0x5A).all()), (fn.__name__, kw)
    # the unmodified calls, and the nullable pointers NULL, are accepted and write inside their arrays only
    assert scan(good) == 0 and scan(dict(good, ep_return=None, ep_length=None)) == 0
    assert summary(good) == 0 and summary(dict(good, action=None, score=None, action_hist=None)) == 0
    p = host(pool)
    outputs = ("carry_return", "carry_length", "ep_return", "ep_length", "score", "summary", "reward_hist", "workspace")
    inside = np.zeros(total, bool)
    for k in outputs:
        inside[offset[k]:offset[k] + size[k]] = True
        assert (p[offset[k]:offset[k] + size[k]] != 0x5A).any(), k
    inside[offset["action_hist"]:offset["action_hist"] + 8 * A] = True
    assert (p[~inside] == 0x5A).all()


# ---------------------------------------------------------------------------------------------------------- the tracker
def test_tracker_follows_a_changing_rollout_length():
    """account() with T = 128, 1, 128 and then one step in the 1-D form: the per-step outputs and carries are the scan's
    restatement over the concatenation bit for bit, the summary of each call is the restatement's, the score runs on
    from call to call within the sum of the calls' bounds, and the buffers are re-sized when T changes."""
    from twoarmy_amd.episode_stats import EpisodeTracker
    c, N = EC.tracker_case(), EC.TRACKER_N
    tr = EpisodeTracker(N, DEV)
    t, score, slack = 0, 0.0, 0.0
    for call, k in enumerate(EC.TRACKER_CUTS):
        sl = slice(t, t + k)
        args = [dev(c[name][sl]) for name in ("reward", "term", "trunc", "action")]
        if call == len(EC.TRACKER_CUTS) - 1:
            args = [a.view(-1) for a in args]
            assert k == 1 and args[0].dim() == 1
        tr.account(*args)
        assert tr.ep_return.shape == tr.ep_length.shape == (k, N)
        assert tr._workspace.numel() == ops().episode_summary_workspace(k, N)
        assert np.array_equal(bits(host(tr.ep_return)), bits(c["ep_return"][sl])) and np.array_equal(host(tr.ep_length), c["ep_length"][sl])
        want = ER.episode_summary(c["ep_return"][sl], c["ep_length"][sl], c["term"][sl], c["trunc"][sl], c["reward"][sl],
                                  c["action"][sl], 5, 0.99, 0.01, score)
        returns = EC.tracker_returns()[call]
        assert want["episodes"] == len(returns) > 0
        slack += EC.fold_bound(len(returns), 0.99, 0.01, score, returns)
        score = want["score"]
        st = tr.read()
        print("call", call, "T", k, "episodes", st["episodes"], "score", st["score"], "vs", score, "slack", slack)
        assert [st[f] for f in ("episodes", "successes", "truncated", "length_sum", "max_length")] == \
               [want[f] for f in ("episodes", "successes", "truncated", "length_sum", "max_length")]
        assert st["min_return"] == want["min_return"] and st["max_return"] == want["max_return"]
        assert st["action_hist"] == want["action_hist"] and st["reward_hist"] == want["reward_hist"]
        assert abs(st["return_sum"] - want["return_sum"]) <= EC.sum_bound(len(returns), returns)
        assert abs(st["score"] - score) <= slack
        t += k
    assert np.array_equal(bits(host(tr.carry_return)), bits(c["end_return"])) and np.array_equal(host(tr.carry_length), c["end_length"])
