"""Replay-side PPO kernels (csrc/ppo_kernels.hip: ppo_her_relabel[_window], ppo_gather_stack[_u8], ppo_age_scan,
ppo_decoder_frames) at their edges: episode lengths around HER_MAX_LEN and `skip`, episodes across the kernel's 64-step
chunks, Philox counters that wrap, ragged batches, every age around the episode start, odd pitches, the ABI's NULL /
range rejections.  Index kernels are compared bit for bit with the CPU oracles; the decoder with float64 under a derived
rounding bound (tests/replay_ref.py).  Every rejected call is refused on the host before anything is launched."""
import numpy as np
import pytest
import torch

import her_oracle
import ppo_oracle as po
import replay_ref as rr
from ppo_util import DEV, TW_E_ARG, dev as _d, lib as _lib, ops as _ops, ptr as _P, stream as _stream

pytestmark = pytest.mark.gpu
KEYS = ("counts", "t", "n", "goal", "reward", "done")


# ====================================================================================================== hindsight
def _device_relabel(roll, choices=None, **kw):
    got = _ops().her_relabel(_d(roll["pos"]), _d(roll["terminated"]), _d(roll["truncated"]), _d(roll["age0"]),
                             _d(roll["reward"]), None if choices is None else _d(choices), **kw)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _oracle(roll, choices=None, **kw):
    return her_oracle.relabel(roll["pos"], roll["terminated"], roll["truncated"], roll["age0"], roll["reward"],
                              choices=choices, **kw)


def _assert_same(got, want, what=""):
    for k in KEYS:
        assert rr.same_bits(got[k], want[k]), (what, k, got[k].shape, want[k].shape)


@pytest.fixture(scope="module", params=["int", "frac"])
def sweep(request):
    return rr.synthetic_rollout(rr.SWEEP_SEED, rr.SWEEP_T, rr.SWEEP_N, request.param)


@pytest.mark.parametrize("source", ["philox", "choices"])
def test_her_sweep_equals_oracle(sweep, source):
    choices = rr.sweep_choices(rr.SWEEP_SEED, rr.SWEEP_T, rr.SWEEP_N) if source == "choices" else None
    sizes = {}
    for max_goals in (0, 1, 2, 3, 4):
        for skip in (0, 1, 4):
            kw = dict(seed=rr.SWEEP_SEED, env_id0=3, step0=11, max_goals=max_goals, skip=skip)
            want = _oracle(sweep, choices, **kw)
            _assert_same(_device_relabel(sweep, choices, **kw), want, (max_goals, skip))
            sizes[max_goals, skip] = want["t"].size
    assert all(sizes[0, s] == 0 for s in (0, 1, 4)) and sizes[4, 0] >= 1000 and sizes[1, 4] > 0
    assert sizes[4, 0] > sizes[2, 0] > sizes[1, 0]


def test_her_philox_counters_wrap_and_seed_high_word(sweep):
    """env_id0 + n wraps at n = 16, step0 + t1 at t1 = 256; the seed's high word is the second Philox key word."""
    kw = dict(seed=0x0123456789ABCDEF, env_id0=0xFFFFFFF0, step0=0xFFFFFF00)
    want = _oracle(sweep, **kw)
    assert ((want["n"] > 16) & (want["t"] > 256)).any() and ((want["n"] < 16) & (want["t"] < 256)).any()
    _assert_same(_device_relabel(sweep, **kw), want)
    low = _oracle(sweep, seed=0x89ABCDEF, env_id0=0xFFFFFFF0, step0=0xFFFFFF00)
    assert not (low["t"].size == want["t"].size and np.array_equal(low["goal"], want["goal"]))     # k1 matters


def _distinct(T):
    """T positions that are pairwise different: every step is a first visit."""
    t = np.arange(T, dtype=np.float32)
    return np.stack([np.floor(t / 8) - 2, (t % 8) * np.float32(0.5) - 1], 1)


def test_her_single_step_rollout_launches_once(monkeypatch):
    """T = 1 with a done: one record, index 0, never a goal -> H = 0, no emit launch, empty outputs."""
    lib = _lib()
    calls = []
    real = lib.ppo_her_relabel_window
    monkeypatch.setattr(lib, "ppo_her_relabel_window", lambda *a: calls.append(a[13]) or real(*a))
    roll = rr.single_env(1, [(0, 0)])
    got = _device_relabel(roll, seed=5)
    assert len(calls) == 1 and calls[0] is None                     # the counts-only pass (offsets == NULL) alone
    _assert_same(got, _oracle(roll, seed=5))
    assert got["t"].size == 0 and got["goal"].shape == (0, 2) and got["counts"].tolist() == [0]


@pytest.mark.parametrize("T,s0", [(64, 0), (65, 1), (94, 30), (200, 100)])
def test_her_64_step_episode_aligned_shifted_straddling(T, s0):
    """All 64 lanes live; [0, 63] sits in one chunk of the c0 loop, [1, 64] and [30, 93] end in the next one."""
    for mode, pos in (("distinct", _distinct(T)), ("int", None), ("frac", None)):
        roll = rr.single_env(T, [(s0, s0 + 63)], pos=pos, seed=T, mode=mode if pos is None else "int")
        for skip in (0, 4, 63):
            want = _oracle(roll, seed=21, skip=skip)
            _assert_same(_device_relabel(roll, seed=21, skip=skip), want, (mode, skip))
            if mode == "distinct" and skip < 63:
                assert (want["t"] >= s0).any() and want["t"].max() <= s0 + 63    # ([0, s0 - 1] is an episode too)
        # with distinct positions record 63 (lane 63) is a candidate: picked explicitly it relabels all 64 steps
        if mode == "distinct":
            ch = np.full((T, 1, 4), -1, np.int32)
            fv = her_oracle.first_visit(roll["pos"][s0:s0 + 64, 0])
            ch[s0 + 63, 0, 0] = int(np.flatnonzero(fv == 63)[0])
            want = _oracle(roll, choices=ch)
            assert want["t"].tolist() == list(range(s0, s0 + 64)) and want["done"].tolist() == [0] * 63 + [1]
            _assert_same(_device_relabel(roll, choices=ch), want)


def test_her_65_step_episode_is_dropped_the_next_one_kept():
    roll = rr.single_env(70, [(0, 64), (65, 69)], pos=_distinct(70))
    want = _oracle(roll, seed=2)
    assert want["t"].size > 0 and want["t"].min() >= 65
    _assert_same(_device_relabel(roll, seed=2), want)
    # and an episode running since before the rollout (age0 != 0) followed by a 64-step one
    roll = rr.single_env(70, [(6, 69)], pos=_distinct(70), age0=60)
    want = _oracle(roll, seed=2)
    assert want["t"].size > 0 and want["t"].min() >= 6
    _assert_same(_device_relabel(roll, seed=2), want)


@pytest.mark.parametrize("skip", [1, 4, 63])
def test_her_episodes_of_skip_and_skip_plus_one_steps(skip):
    """An episode of `skip` steps offers no candidate; one of skip + 1 steps offers only the first of them, which is never
    a goal; one of skip + 2 steps is the shortest that yields records."""
    if skip == 63:
        eps = [(0, 62), (63, 126)]
    else:
        eps = [(0, skip - 1), (skip, 2 * skip), (2 * skip + 1, 3 * skip + 2)]
    T = eps[-1][1] + 1
    roll = rr.single_env(T, eps, pos=_distinct(T))
    for max_goals in (1, 4):
        want = _oracle(roll, seed=8, skip=skip, max_goals=max_goals)
        _assert_same(_device_relabel(roll, seed=8, skip=skip, max_goals=max_goals), want)
        if skip == 63:
            assert want["t"].size == 0
        elif max_goals == 4:                        # both candidates are picked; one pick may be the excluded first one
            assert want["t"].size == skip + 2 and want["t"].min() == eps[-1][0] and want["done"].tolist()[-1] == 1
        else:
            assert want["t"].size in (0, skip + 2)


def test_her_nothing_to_relabel():
    # all positions equal: one unique entry, index 0
    roll = rr.single_env(40, [(0, 19), (20, 39)], pos=np.tile(np.float32([2.0, -0.0]), (40, 1)))
    roll["pos"][::2, 0, 1] = 0.0                                     # +0.0 and -0.0 alternate: still ONE position
    got = _device_relabel(roll, seed=3)
    _assert_same(got, _oracle(roll, seed=3))
    assert got["t"].size == 0
    # an episode that began before the rollout and does not end in it
    roll = rr.single_env(70, [], age0=5)
    got = _device_relabel(roll, seed=3)
    _assert_same(got, _oracle(roll, seed=3))
    assert got["t"].size == 0
    # ... and one that began before it and ends in it, with nothing after
    roll = rr.single_env(70, [], age0=5)
    roll["truncated"][69, 0] = 1
    got = _device_relabel(roll, seed=3)
    _assert_same(got, _oracle(roll, seed=3))
    assert got["t"].size == 0


def test_her_reads_no_flags_past_the_rollout():
    """T = 70 is no multiple of the 64-step chunk: the lanes of the last chunk that lie past T must not look at the done
    flags.  Here the rollout is the head of larger buffers whose next 64 rows are all done, so a lane that did look
    would see episodes ending past the rollout and the counts would differ."""
    T, N = 70, 3
    roll = rr.synthetic_rollout(5, T, N, "int")
    big = {}
    for k in ("pos", "terminated", "truncated", "reward"):
        x = roll[k]
        tail = np.ones((64,) + x.shape[1:], x.dtype)
        big[k] = _d(np.concatenate([x, tail]))
    got = _ops().her_relabel(big["pos"][:T], big["terminated"][:T], big["truncated"][:T], _d(roll["age0"]),
                             big["reward"][:T], seed=4)
    want = _oracle(roll, seed=4)
    assert want["t"].size > 0
    _assert_same({k: v.cpu().numpy() for k, v in got.items()}, want)


# ------------------------------------------------------------------------------------------------ raw ABI
CANARY_I, CANARY_F, CANARY_B = -7, 123.0, 0xAB


class _HerCall:
    """Device buffers of one raw ppo_her_relabel_window call, outputs prefilled with canaries."""

    def __init__(self, roll, rows):
        self.roll = roll
        self.T, self.N = roll["terminated"].shape
        self.inp = [_d(roll[k]) for k in ("pos", "terminated", "truncated", "age0", "reward")]
        self.counts = torch.full((self.N,), CANARY_I, dtype=torch.int32, device=DEV)
        self.t = torch.full((rows,), CANARY_I, dtype=torch.int32, device=DEV)
        self.n = torch.full((rows,), CANARY_I, dtype=torch.int32, device=DEV)
        self.goal = torch.full((rows, 2), CANARY_F, dtype=torch.float32, device=DEV)
        self.reward = torch.full((rows,), CANARY_F, dtype=torch.float32, device=DEV)
        self.done = torch.full((rows,), CANARY_B, dtype=torch.uint8, device=DEV)

    def __call__(self, offsets=None, counts=True, seed=77, max_goals=4, skip=0, T=None, N=None, null=()):
        """null: names among pos/terminated/truncated/age0/reward (inputs) and t/n/goal/reward_out/done (outputs)."""
        names = ("pos", "terminated", "truncated", "age0", "reward")
        inp = [None if k in null else _P(x) for k, x in zip(names, self.inp)]
        outs = [None if k in null else _P(x) for k, x in zip(("t", "n", "goal", "reward_out", "done"),
                                                             (self.t, self.n, self.goal, self.reward, self.done))]
        if offsets is None:
            outs = [None] * 5 if not null else outs
        rc = _lib().ppo_her_relabel_window(*inp, None, seed, 2, 9, self.T if T is None else T, self.N if N is None else N,
                                           max_goals, skip, _P(offsets), _P(self.counts) if counts else None, *outs,
                                           _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self, counts=True):
        ok = bool((self.t == CANARY_I).all() and (self.n == CANARY_I).all() and (self.goal == CANARY_F).all()
                  and (self.reward == CANARY_F).all() and (self.done == CANARY_B).all())
        return ok and (not counts or bool((self.counts == CANARY_I).all()))


def test_her_abi_two_passes_null_counts_and_gapped_offsets():
    roll = rr.synthetic_rollout(11, 150, 9, "frac")
    want = _oracle(roll, seed=77, env_id0=2, step0=9)
    H, N, GAP = int(want["t"].size), 9, 3
    assert H > 100 and (want["counts"] > 0).sum() >= 5
    call = _HerCall(roll, H + GAP * N + 8)
    assert call(offsets=None) == 0                                            # counts-only pass
    assert call.untouched(counts=False) and np.array_equal(call.counts.cpu().numpy(), want["counts"])
    excl = np.cumsum(want["counts"]) - want["counts"]
    offs = (excl + GAP * np.arange(N)).astype(np.int64)
    for with_counts in (True, False):                                         # counts == NULL with offsets is accepted
        call = _HerCall(roll, H + GAP * N + 8)
        assert call(offsets=_d(offs), counts=with_counts) == 0
        cnt = call.counts.cpu().numpy()
        assert np.array_equal(cnt, want["counts"]) if with_counts else (cnt == CANARY_I).all()
        got = {k: getattr(call, k).cpu().numpy() for k in ("t", "n", "goal", "reward", "done")}
        written = np.zeros(H + GAP * N + 8, bool)
        for n in range(N):
            a, b, c = int(offs[n]), int(excl[n]), int(want["counts"][n])
            written[a:a + c] = True
            for k in got:
                assert rr.same_bits(got[k][a:a + c], want[k][b:b + c]), (n, k)
        assert written.sum() == H and not written[-8:].any()
        gap = ~written                                                        # the gaps and the rows past the end
        assert (got["t"][gap] == CANARY_I).all() and (got["n"][gap] == CANARY_I).all()
        assert (got["goal"][gap] == CANARY_F).all() and (got["reward"][gap] == CANARY_F).all()
        assert (got["done"][gap] == CANARY_B).all()


def test_her_abi_rejections_launch_nothing():
    roll = rr.synthetic_rollout(11, 150, 9, "int")
    counts = _oracle(roll, seed=77, env_id0=2, step0=9)["counts"].astype(np.int64)
    rows = int(counts.sum()) + 8
    offs = _d(np.cumsum(counts) - counts)
    call = _HerCall(roll, rows)
    assert call(offsets=offs) == 0 and not call.untouched()                   # the accepted call does write
    call = _HerCall(roll, rows)
    bad = [dict(max_goals=-1), dict(max_goals=5), dict(skip=-1), dict(skip=64), dict(T=0), dict(N=0), dict(T=-1), dict(N=-1)]
    bad += [dict(null=(k,)) for k in ("pos", "terminated", "truncated", "age0", "reward")]
    for kw in bad:
        for o in (None, offs):
            assert call(offsets=o, **kw) == TW_E_ARG, kw
            assert call.untouched(), kw
    assert call(offsets=None, counts=False) == TW_E_ARG and call.untouched()  # neither offsets nor counts
    for k in ("t", "n", "goal", "reward_out", "done"):                        # offsets with an output pointer missing
        assert call(offsets=offs, null=(k,)) == TW_E_ARG, k
        assert call.untouched(), k
    # ppo_her_relabel is the skip = 0 entry of the same function
    inp = [_P(x) for x in call.inp]
    rc = _lib().ppo_her_relabel(*inp, None, 77, 2, 9, 150, 9, 5, None, _P(call.counts), None, None, None, None, None, _stream())
    torch.cuda.synchronize()
    assert rc == TW_E_ARG and call.untouched()
    rc = _lib().ppo_her_relabel(*inp, None, 77, 2, 9, 150, 9, 4, None, _P(call.counts), None, None, None, None, None, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(call.counts.cpu().numpy(), _oracle(roll, seed=77, env_id0=2, step0=9)["counts"])


# ------------------------------------------------------------------------------------------------ trainer level
def _trainer(N, T, **eng_kw):
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(4)
    eng = TwoarmyEngine(4, N, 17, **eng_kw)
    return eng, VecPPOTrainer(PPO(), eng, rollout_steps=T, minibatch=512, value_chunk=512)


def test_trainer_relabels_over_a_window_of_four_earlier_rollouts():
    """rollout_steps = 16 against 50-step episodes: relabel() looks back over ceil(49 / 16) = 4 earlier rollouts.  After
    EVERY rollout it equals the oracle run over all steps so far from age0 = 0, cut to the current rollout -- after the
    sixth over all 96 steps, cut to t >= 80.

    All envs start together and an untrained policy rarely ends an episode before its 50-step limit, so the episode ends
    sit at t = 49 and t = 99: the sixth rollout [80, 95] may hold none, and its comparison is then one of empty records.
    The fourth rollout [48, 63] (window still growing: 3 earlier rollouts) and the seventh [96, 111] (window full, the
    two oldest rollouts already dropped from it) hold them, from episodes that began three rollouts back; hence seven
    rollouts, and the look-back assertion on those two."""
    N, T, R = 48, 16, 7
    eng, tr = _trainer(N, T)
    assert tr._hist.maxlen == 4
    parts, kept, oldest = [], [], []
    for r in range(R):
        tr.collect()
        parts.append([x.cpu().numpy().copy() for x in (tr.pos[4:4 + T], tr.term, tr.trunc, tr.reward)])
        got = {k: v.cpu().numpy() for k, v in tr.relabel().items()}
        tr.her = None
        assert len(tr._hist) == min(r, 4)
        pos, term, trunc, rew = (np.concatenate([p[i] for p in parts]) for i in range(4))
        want = her_oracle.relabel(pos, term, trunc, np.zeros(N, np.int32), rew, seed=tr.her_seed, env_id0=eng.env_id0,
                                  step0=0)
        back = T * r
        keep = want["t"] >= back
        for k in ("n", "goal", "reward", "done"):
            assert rr.same_bits(got[k], want[k][keep]), (r, k)
        assert rr.same_bits(got["t"], want["t"][keep] - back), r
        assert rr.same_bits(got["counts"], np.bincount(want["n"][keep], minlength=N).astype(np.int32)), r
        # where the oldest episode with a kept record began: walk back from the record to the step after the last done
        done = (term | trunc) != 0
        first = back + T
        for t, n in set(zip(want["t"][keep].tolist(), want["n"][keep].tolist())):
            s = t
            while s > 0 and not done[s - 1, n]:
                s -= 1
            first = min(first, s)
        kept.append(int(keep.sum()))
        oldest.append(first)
        tr.carry_over()
    print("records per rollout:", kept, "oldest episode start per rollout:", oldest)
    # some kept record belongs to an episode that began at least two rollouts back -- also with the window full
    far = [r for r in range(R) if kept[r] > 0 and oldest[r] < T * (r - 1)]
    assert far and max(far) >= 5, (kept, oldest)
    eng.close()


def test_trainer_relabels_64_step_episodes():
    N, T = 32, 130
    eng, tr = _trainer(N, T, max_steps=64)
    tr.collect()
    got = {k: v.cpu().numpy() for k, v in tr.relabel().items()}
    term, trunc = tr.term.cpu().numpy(), tr.trunc.cpu().numpy()
    want = her_oracle.relabel(tr.pos[4:4 + T].cpu().numpy(), term, trunc, np.zeros(N, np.int32), tr.reward.cpu().numpy(),
                              seed=tr.her_seed, env_id0=eng.env_id0, step0=0)
    _assert_same(got, want)
    # an episode truncated at max_steps = 64 was relabelled: records of an env whose first done is at t = 63
    first_done = np.argmax((term | trunc) != 0, 0)
    full = np.flatnonzero((first_done == 63) & (trunc[63] != 0))
    assert full.size > 0 and np.isin(want["n"][want["t"] <= 63], full).any()
    eng.close()


def test_trainer_refuses_episodes_longer_than_64_steps():
    eng, tr = _trainer(8, 16, max_steps=65)
    with pytest.raises(ValueError):
        tr.relabel()
    eng.close()


# ====================================================================================================== gather
LUT = np.array([0.9, -0.9, -0.5, 0.3], np.float32)
G_N, G_K = 7, 12
AGES, KS = tuple(range(-3, 7)), (3, 4, 11)
COMBOS = [(a, k) for a in AGES for k in KS]
PAD_F, PAD_U8, OUT_CANARY = 777.0, 200, -55.5


def _gather_inputs(kind, pitch, seed):
    """frames [K][N][pitch] with the pad columns holding a value no output may show; float values for the oracle."""
    rs = np.random.RandomState(seed)
    if kind == "u8":
        codes = rs.randint(0, 4, size=(G_K, G_N, 289)).astype(np.uint8)
        buf = np.full((G_K, G_N, pitch), PAD_U8, np.uint8)
        buf[..., :289] = codes
        values = LUT[codes]
    else:
        values = rs.randn(G_K, G_N, 289).astype(np.float32)
        buf = np.full((G_K, G_N, pitch), PAD_F, np.float32)
        buf[..., :289] = values
    return dict(buf=buf, values=values, pos=rs.randn(G_K, G_N, 2).astype(np.float32),
                init_frame=rs.randn(289).astype(np.float32), init_pos=rs.randn(2).astype(np.float32))


def _gather_call(kind, buf, pitch, pos_frames, k_idx, n_idx, age, init_frame, init_pos, B, out, pos_out):
    fn = _lib().ppo_gather_stack_u8 if kind == "u8" else _lib().ppo_gather_stack
    rc = fn(_P(buf), pitch, _P(pos_frames), G_N, _P(k_idx), _P(n_idx), _P(age), _P(init_frame), _P(init_pos), B, _P(out),
            _P(pos_out), _stream())
    torch.cuda.synchronize()
    return rc


def _samples(B, seed):
    """B samples cycling through every (age, k); three more valid entries follow them in the index arrays, so that a
    kernel that walked one sample too far would still read valid indices -- and be caught by the canary row."""
    order = np.random.RandomState(seed).permutation(len(COMBOS))
    idx = [COMBOS[order[i % len(COMBOS)]] for i in range(B + 3)]
    age = np.array([a for a, _ in idx], np.int32)
    k = np.array([k for _, k in idx], np.int32)
    n = (np.arange(B + 3) % G_N).astype(np.int32)
    return k, n, age


@pytest.mark.parametrize("kind,pitch", [("f32", 289), ("f32", 292), ("f32", 304), ("u8", 289), ("u8", 304), ("u8", 305)])
def test_gather_stack_ragged_batches_pitches_and_null_pos(kind, pitch):
    g = _gather_inputs(kind, pitch, pitch)
    dbuf, dpos, dif, dip = _d(g["buf"]), _d(g["pos"]), _d(g["init_frame"]), _d(g["init_pos"])
    for B in (1, 2, 3, 5, 257):
        k, n, age = _samples(B, B)
        want, want_pos = po.gather_stack(g["values"], g["pos"], k[:B], n[:B], age[:B], g["init_frame"], g["init_pos"])
        for with_pos in (True, False):
            out = torch.full((B + 4, 4, 289), OUT_CANARY, dtype=torch.float32, device=DEV)
            pos_out = torch.full((B + 4, 4, 2), OUT_CANARY, dtype=torch.float32, device=DEV)
            rc = _gather_call(kind, dbuf, pitch, dpos if with_pos else None, _d(k), _d(n), _d(age), dif,
                              dip if with_pos else None, B, out, pos_out if with_pos else None)
            assert rc == 0
            o, p = out.cpu().numpy(), pos_out.cpu().numpy()
            assert rr.same_bits(o[:B], want), (B, with_pos)
            assert (o[B:] == np.float32(OUT_CANARY)).all(), (B, with_pos)          # the row after out[B-1] and beyond
            if with_pos:
                assert rr.same_bits(p[:B], want_pos) and (p[B:] == np.float32(OUT_CANARY)).all(), B
            else:
                assert (p == np.float32(OUT_CANARY)).all()
    if kind == "u8":                                                   # the expansion is the LUT, exactly
        assert set(np.unique(want[age[:B] >= 4]).tolist()) <= set(LUT.tolist())


def _poison_groups():
    """Every (age, k) once, env = index % N, split into groups in which no sample reads a row another one poisons."""
    groups = []
    for i, (age, k) in enumerate(COMBOS):
        n = i % G_N
        poison = {(k - back, n) for back in range(4) if age - back <= 0}
        reads = {(k - back, n) for back in range(4) if age - back > 0}
        for grp in groups:
            if not (poison & grp["reads"]) and not (reads & grp["poison"]):
                break
        else:
            grp = dict(samples=[], poison=set(), reads=set())
            groups.append(grp)
        grp["samples"].append((k, n, age))
        grp["poison"] |= poison
        grp["reads"] |= reads
    return groups


def test_gather_stack_never_reads_across_the_episode_start():
    """Every age -3 .. 6 with k = 3 (slot 0 reads row 0), 4 and 11.  Each frame and position row the contract replaces by
    the reset frame is NaN: an off-by-one in `age - back <= 0` shows as a NaN, which random data would hide."""
    groups = _poison_groups()
    assert sum(len(g["samples"]) for g in groups) == len(COMBOS) and sum(len(g["poison"]) for g in groups) >= 48
    for pitch in (289, 292):
        g = _gather_inputs("f32", pitch, 5)
        for grp in groups:
            buf, pos = g["buf"].copy(), g["pos"].copy()
            for row, n in grp["poison"]:
                buf[row, n] = np.nan
                pos[row, n] = np.nan
            k, n, age = (np.array(x, np.int32) for x in zip(*grp["samples"]))
            B = len(k)
            out = torch.full((B + 1, 4, 289), OUT_CANARY, dtype=torch.float32, device=DEV)
            pos_out = torch.full((B + 1, 4, 2), OUT_CANARY, dtype=torch.float32, device=DEV)
            pad = np.full(3, 3, np.int32)                              # valid index entries past the batch (see _samples)
            rc = _gather_call("f32", _d(buf), pitch, _d(pos), _d(np.concatenate([k, pad])), _d(np.concatenate([n, pad * 0])),
                              _d(np.concatenate([age, pad * 0])), _d(g["init_frame"]), _d(g["init_pos"]), B, out, pos_out)
            assert rc == 0
            o, p = out.cpu().numpy(), pos_out.cpu().numpy()
            assert not np.isnan(o).any() and not np.isnan(p).any(), grp["samples"]
            want, want_pos = po.gather_stack(g["values"], g["pos"], k, n, age, g["init_frame"], g["init_pos"])
            assert rr.same_bits(o[:B], want) and rr.same_bits(p[:B], want_pos)
            assert (o[B] == np.float32(OUT_CANARY)).all() and (p[B] == np.float32(OUT_CANARY)).all()
            for b in range(B):                                         # what "replaced" means, stated without the oracle
                for j in range(4):
                    if age[b] - (3 - j) <= 0:
                        assert rr.same_bits(o[b, j], g["init_frame"]) and rr.same_bits(p[b, j], g["init_pos"])


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_gather_stack_rejections_launch_nothing(kind):
    g = _gather_inputs(kind, 292, 1)
    k, n, age = _samples(5, 1)
    a = dict(buf=_d(g["buf"]), pos_frames=_d(g["pos"]), k_idx=_d(k), n_idx=_d(n), age=_d(age),
             init_frame=_d(g["init_frame"]), init_pos=_d(g["init_pos"]))
    out = torch.full((6, 4, 289), OUT_CANARY, dtype=torch.float32, device=DEV)
    pos_out = torch.full((6, 4, 2), OUT_CANARY, dtype=torch.float32, device=DEV)

    def call(pitch=292, B=5, out_=out, pos_out_=pos_out, **over):
        b = dict(a, **over)
        return _gather_call(kind, b["buf"], pitch, b["pos_frames"], b["k_idx"], b["n_idx"], b["age"], b["init_frame"],
                            b["init_pos"], B, out_, pos_out_)

    bad = [dict(pitch=288), dict(pitch=0), dict(B=0), dict(B=-1), dict(out_=None), dict(pos_frames=None), dict(init_pos=None)]
    bad += [{key: None} for key in ("buf", "k_idx", "n_idx", "age", "init_frame")]
    for kw in bad:
        assert call(**kw) == TW_E_ARG, kw
        assert bool((out == OUT_CANARY).all()) and bool((pos_out == OUT_CANARY).all()), kw
    assert call() == 0 and not bool((out[:5] == OUT_CANARY).any())                # the same call, accepted, writes
    assert call(pos_frames=None, init_pos=None, pos_out_=None) == 0               # no positions wanted: both may be NULL


# ====================================================================================================== age scan
@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("T", [1, 64, 65])
def test_age_scan_equals_the_recurrence(T, N):
    rs = np.random.RandomState(1000 * T + N)
    term = (rs.rand(T, N) < 0.15).astype(np.uint8)
    trunc = (rs.rand(T, N) < 0.15).astype(np.uint8)
    both = rs.rand(T, N) < 0.1
    term[both], trunc[both] = 1, 1
    age0 = np.where(rs.rand(N) < 0.5, rs.randint(0, 2 ** 30 + 1, N), 0).astype(np.int32)
    age0[-1] = 2 ** 30
    want = np.empty((T + 1, N), np.int32)
    want[0] = age0
    for t in range(T):
        want[t + 1] = np.where((term[t] | trunc[t]) != 0, 0, want[t] + 1)
    buf = torch.full((T + 2, N), CANARY_I, dtype=torch.int32, device=DEV)      # one canary row behind age[T]
    dterm, dtrunc, dage0 = _d(term), _d(trunc), _d(age0)
    rc = _lib().ppo_age_scan(_P(dterm), _P(dtrunc), _P(dage0), T, N, _P(buf), _stream())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert rc == 0 and rr.same_bits(got[:T + 1], want) and (got[T + 1] == CANARY_I).all()
    assert rr.same_bits(_ops().age_scan(_d(term), _d(trunc), _d(age0)).cpu().numpy(), want)
    if T > 1 and N > 1:
        assert both.any() and want.max() >= 2 ** 30


def test_age_scan_rejections_launch_nothing():
    T, N = 5, 9
    term, trunc = (torch.zeros((T, N), dtype=torch.uint8, device=DEV) for _ in range(2))
    age0 = torch.zeros(N, dtype=torch.int32, device=DEV)
    age = torch.full((T + 1, N), CANARY_I, dtype=torch.int32, device=DEV)
    for args in ((None, trunc, age0, T, N, age), (term, None, age0, T, N, age), (term, trunc, None, T, N, age),
                 (term, trunc, age0, T, N, None), (term, trunc, age0, 0, N, age), (term, trunc, age0, T, 0, age),
                 (term, trunc, age0, -1, N, age), (term, trunc, age0, T, -1, age)):
        a = [_P(x) if isinstance(x, torch.Tensor) or x is None else x for x in args]
        assert _lib().ppo_age_scan(*a, _stream()) == TW_E_ARG
        torch.cuda.synchronize()
        assert bool((age == CANARY_I).all())


# ====================================================================================================== decoder
DEC_FRAMES = (1, 513, 1031)          # one block; the first grid-stride wrap (grid = 512); two wraps and a remainder


@pytest.fixture(scope="module")
def decoder_cases():
    """Per scale: latents, float64 reference and bound for 1031 frames, evaluated once; the smaller frame counts are
    prefixes (a frame's value does not depend on the batch it sits in)."""
    w = rr.decoder_weights(3)
    cases = {}
    for scale in (0.2, 1.0, 3.0):
        z = rr.decoder_latents(int(scale * 10), max(DEC_FRAMES), scale)
        cases[scale] = (z, rr.decoder_f64(z, w), rr.decoder_bound(z, w))
    return w, cases


def _decode(z, w):
    dw = {k: v.to(DEV) for k, v in w.items()}
    return _ops().decoder_frames(z.to(DEV), dw["w1"], dw["b1"], dw["w2"], dw["b2"], dw["w3"], dw["b3"]).cpu().double()


@pytest.mark.parametrize("n_frames", DEC_FRAMES)
def test_decoder_within_the_fp32_rounding_bound_of_float64(decoder_cases, n_frames):
    """|kernel - float64| <= 280 * 2^-24 * A3 for every element (replay_ref.decoder_bound).  The float64 side unfolds
    nothing: it runs the three transposed convolutions and the pooling, so the host's kfold folding is under test too."""
    w, cases = decoder_cases
    worst = 0.0
    for scale, (z, want, bound) in cases.items():
        got = _decode(z[:n_frames], w)
        assert got.shape == (n_frames, 289) and bool(torch.isfinite(got).all())
        ratio = (got - want[:n_frames]).abs() / bound[:n_frames]
        worst = max(worst, float(ratio.max()))
        print("decoder n_frames=%d scale=%g: max |err| / bound = %.2e (max |err| %.3e, max |want| %.3e)"
              % (n_frames, scale, float(ratio.max()), float((got - want[:n_frames]).abs().max()), float(want.abs().max())))
        assert bool((ratio <= 1.0).all()), (n_frames, scale, float(ratio.max()))
    assert worst > 0.0                                                  # fp32 does differ from float64 somewhere


def test_decoder_on_the_sensitivity_input():
    """The input on which tests/test_replay_edges_cpu.py shows that a single tap off by 1e-3 leaves the bound."""
    from test_replay_edges_cpu import sensitivity_input
    w, z, _ = sensitivity_input()
    ratio = (_decode(z, w) - rr.decoder_f64(z, w)).abs() / rr.decoder_bound(z, w)
    print("decoder sensitivity input: max |err| / bound = %.2e" % float(ratio.max()))
    assert bool((ratio <= 1.0).all()), float(ratio.max())


def test_decoder_rejections_launch_nothing():
    w = {k: v.to(DEV) for k, v in rr.decoder_weights(3).items()}
    kfold = _ops().fold_decoder_tail(w["w3"])
    z = rr.decoder_latents(1, 2, 1.0).to(DEV)
    out = torch.full((3, 289), OUT_CANARY, dtype=torch.float32, device=DEV)
    ptrs = dict(z=z, w1=w["w1"], b1=w["b1"], w2=w["w2"], b2=w["b2"], kfold=kfold, frames=out)

    def call(n=2, **over):
        p = dict(ptrs, **over)
        rc = _lib().ppo_decoder_frames(_P(p["z"]), n, _P(p["w1"]), _P(p["b1"]), _P(p["w2"]), _P(p["b2"]), _P(p["kfold"]), 0.25,
                                       _P(p["frames"]), _stream())
        torch.cuda.synchronize()
        return rc

    for kw in [dict(n=0), dict(n=-1)] + [{k: None} for k in ptrs]:
        assert call(**kw) == TW_E_ARG, kw
        assert bool((out == OUT_CANARY).all()), kw
    assert call() == 0
    o = out.cpu()
    assert not bool((o[:2] == OUT_CANARY).any()) and bool((o[2] == OUT_CANARY).all())
    # b3 is the constant the ABI adds to every cell
    w0 = {k: v.cpu() for k, v in w.items()}
    w0["b3"] = torch.tensor([0.25])
    want = rr.decoder_f64(z.cpu(), w0)
    assert bool(((o[:2].double() - want).abs() <= rr.decoder_bound(z.cpu(), w0)).all())
