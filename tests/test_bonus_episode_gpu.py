"""ppo_bonus_scan_episode (csrc/exploration_bonus.hip) bit for bit against tests/bonus_episode_ref.py: outputs, and the
tables read by the layout the header documents (stamped words, a generation per env); raw table bits where two runs of
the kernel are compared, and bonus_scan's env scope where no episode ends.  Then every front end:
BonusTracker(scope="episode"), VecPPOTrainer.enable_bonus on a real engine, train_ppo --bonus_scope episode.  Side streams
and graph capture: the entry's row in tests/test_streams_gpu.py."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bonus_episode_ref as er
from test_bonus_cpu import random_walk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {1: ("state",), 2: ("action",), 3: ("state", "action")}
FORMS = ("sqrt", "first")
SHAPES = [(1, 1), (7, 3), (256, 2), (257, 65), (513, 5)]       # across the 256-step chunk and the 64-lane wavefront


def dev(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt).contiguous()


class Run:
    """Tables and arguments of one configuration; scan() launches the kernel on a slice of steps."""

    def __init__(self, N, mask, form="sqrt", scale=1.0, width=17, height=17, n_actions=7):
        from twoarmy_amd import ppo_ops
        self.ops, self.N, self.mask, self.form, self.scale = ppo_ops, N, mask, form, scale
        self.geom = dict(width=width, height=height, n_actions=n_actions)
        self.tab = {k: torch.zeros(ppo_ops.bonus_episode_words(k, width, height, n_actions, N), dtype=torch.int32,
                                   device=DEV) for k in KINDS[mask]}

    def scan(self, pos, action, dirs, reward, term, trunc, keep=None, outs=(True, True, True), reward_out=None):
        """outs: which of bonus_state / bonus_action / reward_out are passed; reward_out="alias": reward itself."""
        T, N = pos.shape[:2]
        mk = lambda want: torch.full((T, N), -7.0, dtype=torch.float32, device=DEV) if want else None      # noqa: E731
        bs, ba = mk(outs[0] and self.mask & 1), mk(outs[1] and self.mask & 2)
        r = dev(reward, torch.float32)
        ro = r if reward_out == "alias" else mk(outs[2])
        self.ops.bonus_scan_episode(dev(pos, torch.float32), dev(action, torch.int32), r, dev(term, torch.uint8),
                                    dev(trunc, torch.uint8), self.tab.get("state"), self.tab.get("action"), self.form,
                                    self.scale, keep=dev(keep, torch.uint8), dir=dev(dirs, torch.int32), bonus_state=bs,
                                    bonus_action=ba, reward_out=ro, **self.geom)
        f = lambda t: None if t is None else t.cpu().numpy()                                                 # noqa: E731
        return {"state": f(bs), "action": f(ba), "reward": f(ro)}

    def raw(self):
        return {k: t.cpu().numpy() for k, t in self.tab.items()}

    def preset(self, kind, words):
        self.tab[kind].copy_(torch.from_numpy(words).to(DEV))


def same(got, want, mask):
    for k in KINDS[mask] + ("reward",):
        assert got[k] is not None and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


def same_tables(run, ref):
    """The device tables, read as the header lays them out, hold the restatement's running counts and generations."""
    for k, words in run.raw().items():
        counts, gen, _ = er.decode(words, run.N)
        assert np.array_equal(counts, ref.table(k)), k
        assert list(gen) == ref.gen[k], k


@functools.lru_cache(maxsize=None)
def walk(T, N, seed=11, p_done=0.05):
    """A random walk with random done flags; column 0 never ends an episode and column 1 ends one at every step."""
    pos, action, dirs, reward = random_walk(T, N, seed)
    rs = np.random.RandomState(seed + 100)
    term, trunc = (rs.rand(T, N) < p_done).astype(np.uint8), (rs.rand(T, N) < p_done).astype(np.uint8)
    if N > 1:
        term[:, 0] = trunc[:, 0] = 0
        term[:, 1], trunc[:, 1] = np.arange(T) % 2, (np.arange(T) + 1) % 2
    return pos, action, dirs, reward, term, trunc


@functools.lru_cache(maxsize=None)
def walk_ref(T, N, mask, form, scale=1.0, keep_seed=None, seed=11):
    """The restatement of walk(T, N) from empty tables, computed once and shared; nobody changes what it returns."""
    pos, action, dirs, reward, term, trunc = walk(T, N, seed)
    keep = None if keep_seed is None else (np.random.RandomState(keep_seed).rand(T, N) < 0.3).astype(np.uint8)
    ref = er.EpisodeBonusRef(N, KINDS[mask], scale, form)
    return ref.scan(pos, action, reward, term, trunc, keep=keep, dirs=dirs), ref, keep


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("T,N", SHAPES)
def test_random_walks_every_kind_mask_and_form(T, N):
    pos, action, dirs, reward, term, trunc = walk(T, N)
    if T > 1:
        assert (term | trunc).any() and (N == 1 or ((term | trunc)[:, 1].all() and not (term | trunc)[:, 0].any()))
    for form in FORMS:
        for mask in (1, 2, 3):
            want, ref, _ = walk_ref(T, N, mask, form)
            run = Run(N, mask, form)
            same(run.scan(pos, action, dirs, reward, term, trunc), want, mask)
            same_tables(run, ref)
    if T >= 256:
        c = walk_ref(T, N, 3, "sqrt")[0]["count_state"]
        assert c[:, 0].max() > 20 and (N == 1 or (c[:, 1] == 1).all())          # counts build up, and clear at every step


def test_a_done_on_either_side_of_the_chunk_boundary():
    """Episode ends at steps 254 .. 257 of a 300-step call (one env each, and one env with all four): the clear falls in
    front of, on and behind the boundary between the first LDS chunk (steps 0 .. 255) and the second."""
    T, N = 300, 5
    pos, action, dirs, reward = random_walk(T, N, 21)
    term, trunc = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
    for n, t in enumerate((254, 255, 256, 257)):
        (term if n % 2 else trunc)[t, n] = 1
        term[t, 4] = 1
    for form in FORMS:
        ref = er.EpisodeBonusRef(N, KINDS[3], 1.0, form)
        want = ref.scan(pos, action, reward, term, trunc, dirs=dirs)
        run = Run(N, 3, form)
        same(run.scan(pos, action, dirs, reward, term, trunc), want, 3)
        same_tables(run, ref)
        assert ref.gen["state"] == [1, 1, 1, 1, 4]
    c = want["count_state"]
    assert c[250:254].max() > 10 and all(c[t + 1, n] == 1 for n, t in enumerate((254, 255, 256, 257)))


# ------------------------------------------------------------------------------------------------ 2. cuts
def run_cuts(cuts, data, N, form="sqrt", start=None):
    pos, action, dirs, reward, term, trunc = data
    run, parts, t0 = Run(N, 3, form), [], 0
    for k, words in (start or {}).items():
        run.preset(k, words)
    for c in cuts:
        sl = slice(t0, t0 + c)
        parts.append(run.scan(pos[sl], action[sl], dirs[sl], reward[sl], term[sl], trunc[sl]))
        t0 += c
    assert t0 == pos.shape[0]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}, run


def same_bits_as(whole, whole_run, got, run, what):
    same(got, whole, 3)
    for k, words in whole_run.raw().items():
        assert np.array_equal(words, run.raw()[k]), (what, k)                   # the raw words: stamps included


@pytest.mark.parametrize("form", FORMS)
def test_result_does_not_depend_on_how_steps_are_cut_into_launches(form):
    """One call of T steps against every two-way split and against T calls of one step: equal bits in the outputs and in
    the tables.  Column 1 ends an episode at every step, so every split lies directly behind a done step of it."""
    T, N = 40, 5
    data = walk(T, N)
    want, ref, _ = walk_ref(T, N, 3, form)
    whole, whole_run = run_cuts([T], data, N, form)
    same(whole, want, 3)
    same_tables(whole_run, ref)
    done = data[4] | data[5]
    assert any(done[c - 1, 2:].any() for c in range(1, T)) and any(not done[c - 1, 2:].any() for c in range(1, T))
    for c in range(1, T):
        got, run = run_cuts([c, T - c], data, N, form)
        same_bits_as(whole, whole_run, got, run, c)
    got, run = run_cuts([1] * T, data, N, form)
    same_bits_as(whole, whole_run, got, run, "step by step")


def test_cuts_around_the_chunk_boundary_and_behind_a_done_step_there():
    T, N = 300, 5
    pos, action, dirs, reward = random_walk(T, N, 21)
    term, trunc = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
    for n, t in enumerate((254, 255, 256, 257)):
        term[t, n] = 1
    trunc[100, 4] = trunc[256, 4] = 1
    data = (pos, action, dirs, reward, term, trunc)
    whole, whole_run = run_cuts([T], data, N)
    ref = er.EpisodeBonusRef(N, KINDS[3])
    same(whole, ref.scan(pos, action, reward, term, trunc, dirs=dirs), 3)
    for cuts in ([255, 45], [256, 44], [257, 43], [258, 42], [101, 199], [1, 256, 43], [44, 256]):
        got, run = run_cuts(cuts, data, N)
        same_bits_as(whole, whole_run, got, run, cuts)
        same_tables(run, ref)


# ------------------------------------------------------------------------------------------------ 3. the generation
def test_a_table_at_the_last_generation_wraps_exactly():
    """Tables preset to generation 255 (and a few envs shortly before it), with running counts and with words left over
    from an earlier generation, run over two and more episode ends: the step from 255 to 0 clears the span for real."""
    T, N = 300, 70
    pos, action, dirs, reward, term, trunc = (a.copy() for a in walk(T, N, 31, 0.01))
    term[10, 2:] = 1
    trunc[280, 2:] = 1                                                           # two ends for every env but column 0
    rs = np.random.RandomState(4)
    gen0 = np.full(N, 255)
    gen0[5:9] = [254, 253, 0, 128]
    start, refs = {}, er.EpisodeBonusRef(N, KINDS[3])
    for k in KINDS[3]:
        K = er.n_keys(k)
        counts = np.where(rs.rand(N, K) < 0.02, rs.randint(1, 9, (N, K)), 0)
        cells = [y * 17 + x for y in range(3) for x in range(4)]                 # the cells the walk stands on
        mine = cells if k == "state" else [c * 28 + s for c in cells for s in range(28)]
        counts[:, mine] = rs.randint(0, 5, (N, len(mine)))
        stale = (np.full((N, K), 200), rs.randint(1, 99, (N, K)))                # generation 200: long over
        start[k] = er.encode(counts, gen0, stale)
        back, g, st = er.decode(start[k], N)
        assert np.array_equal(back, counts) and np.array_equal(g, gen0) and (st == 200).sum() > N * K // 2
        refs.preset(k, counts, gen0)
    data = (pos, action, dirs, reward, term, trunc)
    whole, whole_run = run_cuts([T], data, N, start=start)
    want = refs.scan(pos, action, reward, term, trunc, dirs=dirs)
    same(whole, want, 3)
    same_tables(whole_run, refs)
    ends = (term | trunc).sum(0)
    assert ends[0] == 0 and ends[1] == T and (ends[2:] >= 2).all()
    assert want["count_state"][:10, 2:].max() > 5                                # the preset counts were carried ...
    for k, words in whole_run.raw().items():
        _, gen, stamp = er.decode(words, N)
        assert np.array_equal(gen, (gen0 + ends) % 256)
        wrapped = gen0 + ends >= 256
        assert wrapped[1:6].all() and not wrapped[[0, 7, 8]].any() and wrapped.sum() >= N - 4
        assert (stamp[wrapped] <= gen[wrapped, None]).all() and not (stamp[wrapped] == 200).any()   # ... and no old word is left
        assert (stamp[0] == 200).sum() > 100                                     # no end: nothing was cleared
    for cuts in ([11, 289], [10, 290], [256, 44], [1] * 12 + [288]):             # behind the wrapping done, in front of it
        got, run = run_cuts(cuts, data, N, start=start)
        same_bits_as(whole, whole_run, got, run, cuts)


def test_a_count_stays_at_its_ceiling():
    N, K = 2, er.n_keys("state")
    counts = np.zeros((N, K), np.int64)
    counts[0, 7], counts[1, 7] = er.COUNT_MAX - 2, er.COUNT_MAX
    run = Run(N, 1)
    run.preset("state", er.encode(counts, [3, 255]))
    pos = np.zeros((4, N, 2), np.float32)
    pos[..., 1] = 7
    z = np.zeros((4, N), np.uint8)
    got = run.scan(pos, None, None, np.zeros((4, N), np.float32), z, z)
    ref = er.EpisodeBonusRef(N, ("state",))
    ref.preset("state", counts, [3, 255])
    want = ref.scan(pos, None, np.zeros((4, N), np.float32), z, z)
    same(got, want, 1)
    same_tables(run, ref)
    assert list(want["count_state"][:, 0]) == [er.COUNT_MAX - 1] + [er.COUNT_MAX] * 3
    assert list(er.decode(run.raw()["state"], N)[1]) == [3, 255]                  # the ceiling does not reach the stamp


# ------------------------------------------------------------------------------------------------ 4. edges
def test_invalid_steps_count_in_other_and_other_clears_too():
    bad = [np.nan, np.inf, -np.inf, -1.0, 17.0, 1e9, -1e-9]
    pos = np.array([[[v, 2.0]] for v in bad] + [[[2.0, v]] for v in bad] + [[[-0.0, -0.0]], [[16.9, 16.5]]], np.float32)
    T = len(pos)
    action, dirs = np.zeros((T, 1), np.int64), np.zeros((T, 1), np.int64)
    extra_a = np.array([[7], [-1], [1 << 30], [0], [0], [0]])
    extra_d = np.array([[0], [0], [0], [4], [-1], [-(1 << 31)]])
    pos = np.concatenate([pos, np.full((6, 1, 2), 4.0, np.float32)])
    action, dirs = np.concatenate([action, extra_a]), np.concatenate([dirs, extra_d])
    T = len(pos)
    reward = np.full((T, 1), -0.01, np.float32)
    term, trunc = np.zeros((T, 1), np.uint8), np.zeros((T, 1), np.uint8)
    term[4], trunc[17] = 1, 1
    run, ref = Run(1, 3), er.EpisodeBonusRef(1, KINDS[3])
    got = run.scan(pos, action, dirs, reward, term, trunc)
    want = ref.scan(pos, action, reward, term, trunc, dirs=dirs)
    same(got, want, 3)
    same_tables(run, ref)
    assert list(want["count_state"][:7, 0]) == [1, 2, 3, 4, 5, 1, 2]            # other builds up, clears, builds up
    assert list(want["count_action"][16:, 0]) == [10, 11, 1, 2, 3, 4]
    assert ref.table("state")[0, -1] == 0 and ref.table("state")[0, 4 * 17 + 4] == 4 and ref.table("action")[0, -1] == 4


@pytest.mark.parametrize("form", FORMS)
def test_keep_mask_null_outputs_aliasing_and_direction_forms(form):
    T, N = 65, 63
    pos, action, dirs, reward, term, trunc = walk(T, N)
    want, ref, keep = walk_ref(T, N, 3, form, 0.5, keep_seed=2)
    assert keep.any() and not keep.all()
    run = Run(N, 3, form, 0.5)
    got = run.scan(pos, action, dirs, reward, term, trunc, keep=keep)
    same(got, want, 3)
    assert np.array_equal(got["reward"][keep != 0], reward[keep != 0])
    plain = walk_ref(T, N, 3, form, 0.5)[0]                                       # keep protects reward_out and nothing else
    assert all(np.array_equal(want[k], plain[k]) for k in ("state", "action", "count_state", "count_action"))
    raw = run.raw()
    for outs in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:                 # every NULL combination
        run = Run(N, 3, form, 0.5)
        got = run.scan(pos, action, dirs, reward, term, trunc, keep=keep, outs=outs)
        for k, on in zip(("state", "action", "reward"), outs):
            assert (got[k] is None) if not on else np.array_equal(got[k], want[k]), (outs, k)
        assert all(np.array_equal(run.raw()[k], raw[k]) for k in raw), outs
    run = Run(N, 3, form, 0.5)
    got = run.scan(pos, action, dirs, reward, term, trunc, keep=keep, reward_out="alias")
    assert np.array_equal(got["reward"], want["reward"])
    # one direction per env (t-stride 0) == the same direction repeated over [T][N]; no directions == all zero
    per_env = dirs[0].copy()
    a = Run(N, 2, form).scan(pos, action, per_env, reward, term, trunc)
    b = Run(N, 2, form).scan(pos, action, np.broadcast_to(per_env, (T, N)), reward, term, trunc)
    c = Run(N, 2, form).scan(pos, action, None, reward, term, trunc)
    d = Run(N, 2, form).scan(pos, action, np.zeros((T, N), np.int64), reward, term, trunc)
    r = er.EpisodeBonusRef(N, ("action",), 1.0, form).scan(pos, action, reward, term, trunc, dirs=per_env)
    assert np.array_equal(a["action"], b["action"]) and np.array_equal(a["action"], r["action"])
    assert np.array_equal(c["action"], d["action"]) and not np.array_equal(a["action"], c["action"])


def test_directions_read_where_they_live():
    """dir_ptr = (address, stride_t, stride_n): a column of a wider record array, as the engine's records are read."""
    from twoarmy_amd import ppo_ops
    T, N = 9, 5
    pos, action, dirs, reward, term, trunc = walk(T, N)
    rec = torch.full((T, N, 3), -9, dtype=torch.int32, device=DEV)
    rec[:, :, 1] = dev(dirs, torch.int32)
    run = Run(N, 2)
    ba = torch.empty((T, N), device=DEV)
    ppo_ops.bonus_scan_episode(dev(pos, torch.float32), dev(action, torch.int32), None, dev(term, torch.uint8),
                               dev(trunc, torch.uint8), None, run.tab["action"], dir_ptr=(rec.data_ptr() + 4, 3 * N, 3),
                               bonus_action=ba)
    assert np.array_equal(ba.cpu().numpy(), walk_ref(T, N, 2, "sqrt")[0]["action"])


def test_another_grid_and_action_count():
    w, h, na = 5, 7, 3
    T, N = 20, 70
    pos, action, dirs, reward = random_walk(T, N, 11, w, h, na)
    rs = np.random.RandomState(9)
    pos[..., 0] = np.where(np.isfinite(pos[..., 0]), rs.randint(-1, h + 1, (T, N)), pos[..., 0])    # the whole grid and its rim
    pos[..., 1] = np.where(np.isfinite(pos[..., 1]), rs.randint(-1, w + 1, (T, N)), pos[..., 1])
    term, trunc = (rs.rand(T, N) < 0.1).astype(np.uint8), (rs.rand(T, N) < 0.1).astype(np.uint8)
    ref = er.EpisodeBonusRef(N, KINDS[3], 1.0, "sqrt", w, h, na)
    want = ref.scan(pos, action, reward, term, trunc, dirs=dirs)
    run = Run(N, 3, "sqrt", 1.0, w, h, na)
    same(run.scan(pos, action, dirs, reward, term, trunc), want, 3)
    same_tables(run, ref)


def test_nothing_outside_the_tables_and_outputs_is_written():
    from twoarmy_amd import ppo_ops
    T, N, G = 9, 5, 4096
    pos, action, dirs, reward, term, trunc = walk(T, N)
    term = term.copy()
    term[4] = 1                                                                  # generation 255: these ends clear for real
    words = {k: ppo_ops.bonus_episode_words(k, 17, 17, 7, N) for k in KINDS[3]}
    guarded = {k: torch.full((2 * G + 4 * n,), 0xA5, dtype=torch.uint8, device=DEV) for k, n in words.items()}
    outs = {k: torch.full((2 * G + 4 * T * N,), 0xA5, dtype=torch.uint8, device=DEV) for k in ("bs", "ba", "ro")}
    tab = {k: guarded[k][G:G + 4 * n].view(torch.int32) for k, n in words.items()}
    ref = er.EpisodeBonusRef(N, KINDS[3])
    for k in tab:
        tab[k].copy_(torch.from_numpy(er.encode(np.zeros((N, er.n_keys(k)), np.int64), [255] * N)).to(DEV))
        ref.preset(k, np.zeros((N, er.n_keys(k)), np.int64), [255] * N)
    o = {k: t[G:G + 4 * T * N].view(torch.float32).view(T, N) for k, t in outs.items()}
    ppo_ops.bonus_scan_episode(dev(pos, torch.float32), dev(action, torch.int32), dev(reward, torch.float32),
                               dev(term, torch.uint8), dev(trunc, torch.uint8), tab["state"], tab["action"],
                               dir=dev(dirs, torch.int32), bonus_state=o["bs"], bonus_action=o["ba"], reward_out=o["ro"])
    want = ref.scan(pos, action, reward, term, trunc, dirs=dirs)
    same({"state": o["bs"].cpu().numpy(), "action": o["ba"].cpu().numpy(), "reward": o["ro"].cpu().numpy()}, want, 3)
    for k, n in words.items():
        g = guarded[k].cpu().numpy()
        assert (g[:G] == 0xA5).all() and (g[G + 4 * n:] == 0xA5).all(), k
        counts, gen, _ = er.decode(tab[k].cpu().numpy(), N)
        assert np.array_equal(counts, ref.table(k)) and list(gen) == ref.gen[k]
    for k, t in outs.items():
        g = t.cpu().numpy()
        assert (g[:G] == 0xA5).all() and (g[G + 4 * T * N:] == 0xA5).all(), k


def test_bad_arguments_are_refused_and_change_nothing():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    T, N = 2, 3
    pos = torch.zeros((T, N, 2), device=DEV)
    act = torch.zeros((T, N), dtype=torch.int32, device=DEV)
    rew = torch.zeros((T, N), device=DEV)
    flag = torch.zeros((T, N), dtype=torch.uint8, device=DEV)
    st = torch.zeros(291 * N, dtype=torch.int32, device=DEV)
    at = torch.zeros(8094 * N, dtype=torch.int32, device=DEV)
    bs = torch.full((T, N), -7.0, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                 # noqa: E731
    good = dict(pos=p(pos), action=p(act), dir=None, st=0, sn=0, reward=p(rew), keep=None, term=p(flag), trunc=p(flag), T=T,
                N=N, w=17, h=17, na=7, mask=3, form=0, scale=1.0, stab=p(st), atab=p(at), bs=p(bs), ba=None, ro=p(rew),
                stream=None)
    call = lambda **kw: lib.ppo_bonus_scan_episode(*{**good, **kw}.values())      # noqa: E731
    bad = [dict(pos=None), dict(pos=C.c_void_p(pos.data_ptr() + 4)), dict(stab=None), dict(atab=None), dict(action=None),
           dict(mask=0), dict(mask=4), dict(w=0), dict(h=33), dict(na=0), dict(na=9), dict(T=-1), dict(N=-1),
           dict(reward=None), dict(dir=p(act), st=-1), dict(dir=p(act), sn=-1), dict(stab=C.c_void_p(st.data_ptr() + 4)),
           dict(atab=C.c_void_p(at.data_ptr() + 4)), dict(T=1 << 16, N=1 << 15), dict(w=32, h=32, na=8, N=1 << 20),
           dict(term=None), dict(trunc=None), dict(term=None, trunc=None), dict(form=2), dict(form=-1)]
    torch.cuda.synchronize()
    before = tuple(t.clone() for t in (st, at, rew, bs))
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(T=0) == 0 and call(N=0) == 0                                      # nothing to do: nothing launched
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (st, at, rew, bs)))
    assert call() == 0 and call(form=1) == 0
    assert call(mask=1, atab=None, action=None) == 0 and call(mask=2, stab=None, bs=None) == 0
    assert call(reward=None, ro=None) == 0
    torch.cuda.synchronize()
    assert _lib.lib().tw_last_hip_error() == 0 and (bs != -7).all() and st.any() and at.any()


# ------------------------------------------------------------------------------------------------ 5. the env scope
@pytest.mark.parametrize("T,N", [(1, 1), (257, 3), (513, 65)])      # one step, a chunk boundary, two chunks and 65 envs
@pytest.mark.parametrize("mask", (1, 2, 3))
def test_without_an_episode_end_it_is_the_env_scope(T, N, mask):
    """No step flagged done, form "sqrt", fresh tables: bonus_scan(scope="env") bit for bit in every output, its counts
    in the decoded tables, and every generation word 0."""
    from twoarmy_amd import ppo_ops
    pos, action, dirs, reward = walk(T, N, 11, 0.0)[:4]
    none = np.zeros((T, N), np.uint8)
    keep = (np.random.RandomState(5).rand(T, N) < 0.3).astype(np.uint8)
    run = Run(N, mask, "sqrt", 0.5)
    got = run.scan(pos, action, dirs, reward, none, none, keep=keep)
    tab = {k: torch.zeros(ppo_ops.bonus_table_words(k, "env", N=N), dtype=torch.int32, device=DEV) for k in KINDS[mask]}
    out = {k: torch.full((T, N), -7.0, device=DEV) for k in KINDS[mask] + ("reward",)}
    ppo_ops.bonus_scan(dev(pos, torch.float32), dev(action, torch.int32), dev(reward, torch.float32), tab.get("state"),
                       tab.get("action"), "env", 0.5, keep=dev(keep, torch.uint8), dir=dev(dirs, torch.int32),
                       bonus_state=out.get("state"), bonus_action=out.get("action"), reward_out=out["reward"])
    same(got, {k: t.cpu().numpy() for k, t in out.items()}, mask)
    for k, words in run.raw().items():
        counts, gen, _ = er.decode(words, N)
        assert np.array_equal(counts, (tab[k].cpu().numpy().astype(np.int64) & 0xFFFFFFFF).reshape(N, -1)), k
        assert counts.sum() == T * N and not gen.any(), k


# ------------------------------------------------------------------------------------------------ 6. front ends
def _trainer(form, kinds=("state", "action")):
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(3)
    eng = TwoarmyEngine(6, 8, 17, seed=9981)
    agent = PPO()
    agent.K_epochs = 1
    tr = VecPPOTrainer(agent, eng, rollout_steps=16, minibatch=128)
    if form:
        tr.enable_bonus(kinds, "episode", 0.25, form)
    return tr, eng


@pytest.mark.parametrize("form", FORMS)
def test_tracker_and_trainer_on_the_real_engine(form):
    """8 envs x 64 steps (4 rollouts of 16; episodes of 50 steps end inside): reward_train is the restatement run on the
    trainer's own pos, action, term and trunc, and the tracker reads back the running episodes' counts."""
    tr, eng = _trainer(form)
    plain, eng2 = _trainer(None)
    try:
        assert tr.bonus.scope == "episode" and tr.bonus.form == form
        ref = er.EpisodeBonusRef(8, KINDS[3], 0.25, form)
        ends = 0
        for u in range(4):
            tr.collect(); plain.collect()
            assert plain.reward_train is plain.reward and plain.shape_rewards() is plain.reward     # the flag off
            shaped = tr.shape_rewards()
            assert shaped is tr.reward_train and shaped is not tr.reward
            assert torch.equal(tr.reward, plain.reward) and torch.equal(tr.action, plain.action)      # same rollout
            term, trunc = tr.term.cpu().numpy(), tr.trunc.cpu().numpy()
            want = ref.scan(tr.pos[4:20].cpu().numpy(), tr.env_actions().cpu().numpy(), tr.reward.cpu().numpy(), term, trunc,
                            keep=term, dirs=tr.dir.cpu().numpy())
            assert np.array_equal(shaped.cpu().numpy().view(np.uint32), want["reward"].view(np.uint32)), u
            for k in KINDS[3]:
                assert np.array_equal(tr.bonus.bonus[k].cpu().numpy(), want[k]), (u, k)
            ends += int((term | trunc).sum())
            pe = tr.bonus.read(per_env=True)
            st, ac = ref.table("state"), ref.table("action")
            assert np.array_equal(pe["state"], st[:, :-1].reshape(8, 17, 17)) and np.array_equal(pe["other"]["state"], st[:, -1])
            assert np.array_equal(pe["action"], ac[:, :-1].reshape(8, 17, 17, 4, 7).transpose(0, 3, 4, 1, 2))
            assert np.array_equal(tr.bonus.read()["state"], st[:, :-1].sum(0).reshape(17, 17))
            tr.carry_over(); plain.carry_over()
        assert ends >= 8                                            # every env finished an episode: the counts did clear
        assert ref.table("state").sum() < 64 * 8 - 8 * 30
        bs = tr.bonus_stats()
        assert bs["mean"] > 0 and set(bs["mean_by_kind"]) == set(KINDS[3])
        tr.bonus.reset_counts()
        assert tr.bonus.read()["state"].sum() == 0 and not any(t.any() for t in tr.bonus.tables.values())
    finally:
        eng.close(); eng2.close()


def test_tracker_takes_one_step_and_refuses_missing_flags_on_the_device():
    from twoarmy_amd.exploration import BonusTracker
    T, N = 12, 6
    pos, action, dirs, reward, term, trunc = walk(T, N)
    tr = BonusTracker(N, DEV, "state", "episode", 2.0, form="first")
    ref = er.EpisodeBonusRef(N, ("state",), 2.0, "first")
    for t in range(T):                                                           # one step per call: [N, 2], [N]
        out = tr.account(dev(pos[t], torch.float32), dev(action[t], torch.int32), dev(reward[t], torch.float32),
                         terminated=dev(term[t], torch.uint8), truncated=dev(trunc[t], torch.uint8))
        want = ref.scan(pos[t:t + 1], action[t:t + 1], reward[t:t + 1], term[t:t + 1], trunc[t:t + 1])
        assert out.shape == (N,) and np.array_equal(out.cpu().numpy(), want["reward"][0])
    assert np.array_equal(tr.read(per_env=True)["state"], ref.table("state")[:, :-1].reshape(N, 17, 17))
    before = {k: t.clone() for k, t in tr.tables.items()}
    with pytest.raises(ValueError):
        tr.account(dev(pos, torch.float32), dev(action, torch.int32), dev(reward, torch.float32), dev(term, torch.uint8))
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], tr.tables[k]) for k in before)


def test_train_ppo_in_a_child_process_prints_the_bonus_fields():
    argv = ["--env", "MiniGrid-twoarmy-17x17-v6", "--updates", "1", "--num_envs", "8", "--rollout_steps", "32", "--minibatch",
            "256", "--k_epochs", "1", "--cuda", "cuda:0", "--bonus", "state", "--bonus_scope", "episode"]
    p = subprocess.run([sys.executable, "-m", "twoarmy_amd.soa.train_ppo"] + argv, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("update ")]
    assert len(lines) == 1, p.stdout[-2000:]
    m = re.search(r" bonus mean (\d+\.\d{4})$", lines[0])
    assert m and 0 < float(m.group(1)) <= 1.0, lines[0]
