"""ppo_bonus_scan (csrc/exploration_bonus.hip) bit for bit against tests/bonus_ref.py, and through every front end:
BonusTracker, the StateBonus / ActionBonus facade on a real engine against the recording of the reference's wrappers
(tests/golden/bonus.npz), VecPPOTrainer.shape_rewards and train_ppo --bonus."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import bonus_ref as br
from test_bonus_cpu import NAMES, STACKS, golden, random_walk, script_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = {1: ("state",), 2: ("action",), 3: ("state", "action")}


def dev(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dt).contiguous()


class Run:
    """Tables and arguments of one configuration; scan() launches the kernel on a slice of steps."""

    def __init__(self, N, mask, scope, scale=1.0, width=17, height=17, n_actions=7):
        from twoarmy_amd import ppo_ops
        self.ops, self.N, self.mask, self.scope, self.scale = ppo_ops, N, mask, scope, scale
        self.geom = dict(width=width, height=height, n_actions=n_actions)
        self.tab = {k: torch.zeros(ppo_ops.bonus_table_words(k, scope, width, height, n_actions, N), dtype=torch.int32,
                                   device=DEV) for k in KINDS[mask]}

    def scan(self, pos, action, dirs, reward, keep=None, outs=(True, True, True), reward_out=None):
        """outs: which of bonus_state / bonus_action / reward_out are passed; reward_out="alias": reward itself."""
        T, N = pos.shape[:2]
        mk = lambda want: torch.full((T, N), -7.0, dtype=torch.float32, device=DEV) if want else None      # noqa: E731
        bs, ba = mk(outs[0] and self.mask & 1), mk(outs[1] and self.mask & 2)
        r = dev(reward, torch.float32)
        ro = r if reward_out == "alias" else mk(outs[2])
        self.ops.bonus_scan(dev(pos, torch.float32), dev(action, torch.int32), r, self.tab.get("state"),
                            self.tab.get("action"), self.scope, self.scale, keep=dev(keep, torch.uint8),
                            dir=dev(dirs, torch.int32), bonus_state=bs, bonus_action=ba, reward_out=ro, **self.geom)
        f = lambda t: None if t is None else t.cpu().numpy()                                                 # noqa: E731
        return {"state": f(bs), "action": f(ba), "reward": f(ro)}

    def tables(self):
        out = {}
        for k, t in self.tab.items():
            if self.scope == "env":
                out[k] = (t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).reshape(self.N, -1)
            else:
                out[k] = t.view(torch.int64).cpu().numpy().reshape(1, -1)
        return out


def same(got, want, mask):
    for k in KINDS[mask] + ("reward",):
        assert got[k] is not None and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


@functools.lru_cache(maxsize=None)
def walk(T, N, seed=11, width=17, height=17, n_actions=7):
    return random_walk(T, N, seed, width, height, n_actions)


@functools.lru_cache(maxsize=None)
def walk_ref(T, N, mask, scope, scale=1.0, width=17, height=17, n_actions=7, keep_seed=None):
    pos, action, dirs, reward = walk(T, N, 11, width, height, n_actions)
    keep = None if keep_seed is None else (np.random.RandomState(keep_seed).rand(T, N) < 0.3).astype(np.uint8)
    ref = br.BonusRef(N, KINDS[mask], scope, scale, width, height, n_actions)
    return ref.scan(pos, action, reward, keep=keep, dirs=dirs), ref.tables, keep


# ------------------------------------------------------------------------------------------------ 1. golden
@pytest.mark.parametrize("scope", ["env", "shared"])
@pytest.mark.parametrize("name", NAMES)
def test_golden_scripts_through_the_kernel(name, scope):
    z = golden()
    pos, action, dirs, reward, _ = script_arrays(z, name)
    for si, kinds in enumerate(STACKS):
        mask = sum({"state": 1, "action": 2}[k] for k in kinds)
        run = Run(1, mask, scope)
        got = run.scan(pos, action, dirs, reward)
        ref = br.BonusRef(1, kinds, scope)
        same(got, ref.scan(pos, action, reward, dirs=dirs), mask)
        tabs = run.tables()
        if "state" in kinds:
            want = np.zeros(290, np.int64)
            for x, y, c in z["state_counts_" + name]:
                want[y * 17 + x] = c
            assert np.array_equal(tabs["state"][0], want)
        if "action" in kinds:
            want = np.zeros(289 * 28 + 1, np.int64)
            for x, y, d, a, c in z["action_counts_" + name]:
                want[((y * 17 + x) * 4 + d) * 7 + a] = c
            assert np.array_equal(tabs["action"][0], want)
        rec = z["shaped_" + name][si]
        assert (np.abs(got["reward"][:, 0].astype(np.float64) - rec) <= np.spacing(np.abs(rec).astype(np.float32))).all()


@pytest.mark.parametrize("name", NAMES)
def test_facade_wrappers_on_a_real_engine_reproduce_the_recording(name):
    from twoarmy_amd.gym_minigrid.envs.twoarmy import Twoarmy_v6
    from twoarmy_amd.gym_minigrid.wrappers import ActionBonus, StateBonus
    z = golden()
    eid = int(z["meta_" + name][1])
    want_s = {(int(x), int(y)): int(c) for x, y, c in z["state_counts_" + name]}
    want_a = {((int(x), int(y)), int(d), int(a)): int(c) for x, y, d, a, c in z["action_counts_" + name]}
    pos, action, dirs, reward, _ = script_arrays(z, name)
    for si, make in enumerate((lambda e: StateBonus(e), lambda e: ActionBonus(e), lambda e: ActionBonus(StateBonus(e)))):
        base = Twoarmy_v6(agent_view_size=17, tile_size=17, seed=9981, env_id=eid)
        env = make(base)
        try:
            got, t = [], 0
            for op in z["ops_" + name]:
                if op == -1:
                    env.reset()
                    continue
                _, r, term, trunc, _ = env.step(int(op))
                assert (base.agent_pos, base.agent_dir) == (tuple(z["xy_" + name][t]), int(z["dir_" + name][t])), t
                assert (term, trunc) == (bool(z["term_" + name][t]), bool(z["trunc_" + name][t]))
                got.append(r)
                t += 1
            got = np.array(got, np.float64)
            if si == 0:
                assert env.counts == want_s
                ref = br.BonusRef(1, ("state",)).scan(pos, action, reward, dirs=dirs)["reward"]
            elif si == 1:
                assert env.counts == want_a
                ref = br.BonusRef(1, ("action",)).scan(pos, action, reward, dirs=dirs)["reward"]
            else:                                  # stacked wrappers: the inner one's float32 reward is the outer one's input
                assert env.counts == want_a and env.env.counts == want_s
                inner = br.BonusRef(1, ("state",)).scan(pos, action, reward, dirs=dirs)["reward"]
                ref = br.BonusRef(1, ("action",)).scan(pos, action, inner, dirs=dirs)["reward"]
            assert np.array_equal(got.astype(np.float32), ref[:, 0])
            if si < 2:
                rec = z["shaped_" + name][si]
                assert (np.abs(got - rec) <= np.spacing(np.abs(rec).astype(np.float32))).all()
        finally:
            base.close()


# ------------------------------------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("N", [1, 63, 65, 130])
@pytest.mark.parametrize("T", [1, 3, 64, 65, 130])
def test_random_walks_every_kind_mask_and_scope(T, N):
    pos, action, dirs, reward = walk(T, N)
    for scope in ("env", "shared"):
        for mask in (1, 2, 3):
            want, tabs, _ = walk_ref(T, N, mask, scope)
            run = Run(N, mask, scope)
            same(run.scan(pos, action, dirs, reward), want, mask)
            got = run.tables()
            for k in KINDS[mask]:
                assert np.array_equal(got[k], tabs[k]), (scope, mask, k)


def test_chunk_boundary_of_the_env_scope():
    """More steps than one LDS chunk (256): the second chunk gathers what the first stored."""
    T, N = 300, 3
    pos, action, dirs, reward = walk(T, N)
    want, tabs, _ = walk_ref(T, N, 3, "env")
    run = Run(N, 3, "env")
    same(run.scan(pos, action, dirs, reward), want, 3)
    assert all(np.array_equal(run.tables()[k], tabs[k]) for k in KINDS[3])


# ------------------------------------------------------------------------------------------------ 3. cuts
@pytest.mark.parametrize("scope", ["env", "shared"])
def test_result_does_not_depend_on_how_steps_are_cut_into_launches(scope):
    T, N = 130, 65
    pos, action, dirs, reward = walk(T, N)
    want, tabs, _ = walk_ref(T, N, 3, scope)
    for cuts in ([130], [1] * 130, [7, 64, 59]):
        run, parts, t0 = Run(N, 3, scope), [], 0
        for c in cuts:
            sl = slice(t0, t0 + c)
            parts.append(run.scan(pos[sl], action[sl], dirs[sl], reward[sl]))
            t0 += c
        got = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        same(got, want, 3)
        assert all(np.array_equal(run.tables()[k], tabs[k]) for k in KINDS[3]), cuts


# ------------------------------------------------------------------------------------------------ 4. concentration
def test_all_envs_on_one_cell_and_one_env_that_never_moves():
    T, N = 5, 130
    pos = np.full((T, N, 2), 3.0, np.float32)
    zeros = np.zeros((T, N), np.int64)
    run = Run(N, 3, "shared")
    got = run.scan(pos, zeros, zeros, np.zeros((T, N), np.float32))
    for t in range(T):
        b = np.float32(1.0 / np.sqrt(float(130 * (t + 1))))
        assert (got["state"][t] == b).all() and (got["action"][t] == b).all()
    assert run.tables()["state"][0, 3 * 17 + 3] == 650 and run.tables()["state"].sum() == 650
    T, N = 130, 1
    pos = np.full((T, N, 2), 5.0, np.float32)
    zeros = np.zeros((T, N), np.int64)
    run = Run(N, 3, "env")
    got = run.scan(pos, zeros, zeros, np.zeros((T, N), np.float32))
    want = (1.0 / np.sqrt(np.arange(1, 131, dtype=np.float64))).astype(np.float32)
    assert np.array_equal(got["state"][:, 0], want) and np.array_equal(got["action"][:, 0], want)
    assert run.tables()["action"][0, ((5 * 17 + 5) * 4) * 7] == 130


# ------------------------------------------------------------------------------------------------ 5. 1 / sqrt(c)
def expected_bonus(c, scale):
    return (np.float64(scale) * (1.0 / np.sqrt(c.astype(np.float64)))).astype(np.float32)


@pytest.mark.parametrize("scale", [1.0, 0.3])
def test_inverse_square_root_of_every_count_up_to_2_pow_20_env_scope(scale):
    """A 1 x 1 grid has two slots per env; env n starts from count n (a few from large counts up to 2^31 - 2) and takes
    one step, so count n + 1 is evaluated for every n < 2^20."""
    N = 1 << 20
    before = np.arange(N, dtype=np.int64)
    before[-8:] = [(1 << 31) - 3, (1 << 31) - 1 - 2, (1 << 30) + 12345, 3037000499, (1 << 24), (1 << 24) + 1, 4194303999,
                   (1 << 32) - 2]
    run = Run(N, 1, "env", scale, 1, 1, 1)
    tab = np.zeros((N, 2), np.int64)
    tab[:, 0] = before
    run.tab["state"].copy_(torch.from_numpy(tab.astype(np.uint32).view(np.int32).reshape(-1)).to(DEV))
    got = run.scan(np.zeros((1, N, 2), np.float32), None, None, np.zeros((1, N), np.float32), outs=(True, False, False))
    assert np.array_equal(got["state"][0], expected_bonus(before + 1, scale))
    assert np.array_equal(run.tables()["state"][:, 0], before + 1) and not run.tables()["state"][:, 1].any()


@pytest.mark.parametrize("scale", [1.0, 0.3])
def test_inverse_square_root_of_large_counts_shared_scope(scale):
    K = 32 * 32 * 4 * 8
    rs = np.random.RandomState(5)
    before = rs.randint(0, 1 << 40, K, dtype=np.int64)
    before[:6] = [0, (1 << 40) - 1, (1 << 31) - 2, (1 << 32), (1 << 32) - 1, (1 << 35) + 7]
    run = Run(K, 2, "shared", scale, 32, 32, 8)
    run.tab["action"].view(torch.int64)[:K] = torch.from_numpy(before).to(DEV)
    k = np.arange(K)
    cell, d, a = k // 32, (k // 8) % 4, k % 8
    pos = np.stack([cell // 32, cell % 32], -1).astype(np.float32)[None]
    got = run.scan(pos, a[None], d[None], np.zeros((1, K), np.float32), outs=(False, True, False))
    assert np.array_equal(got["action"][0], expected_bonus(before + 1, scale))
    assert np.array_equal(run.tables()["action"][0, :K], before + 1) and run.tables()["action"][0, K] == 0


# ------------------------------------------------------------------------------------------------ 6. edges
def test_invalid_positions_directions_and_actions_take_the_other_slot_only():
    bad = [np.nan, np.inf, -np.inf, -1.0, 17.0, 1e9, -1e-9]
    pos = np.array([[[v, 2.0]] for v in bad] + [[[2.0, v]] for v in bad] + [[[-0.0, -0.0]], [[16.9, 16.5]]], np.float32)
    T = len(pos)
    action = np.zeros((T, 1), np.int64)
    dirs = np.zeros((T, 1), np.int64)
    extra_a = np.array([[7], [-1], [1 << 30], [0], [0], [0]])
    extra_d = np.array([[0], [0], [0], [4], [-1], [-(1 << 31)]])
    pos = np.concatenate([pos, np.full((6, 1, 2), 4.0, np.float32)])
    action, dirs = np.concatenate([action, extra_a]), np.concatenate([dirs, extra_d])
    reward = np.full((T + 6, 1), -0.01, np.float32)
    for scope in ("env", "shared"):
        run = Run(1, 3, scope)
        got = run.scan(pos, action, dirs, reward)
        ref = br.BonusRef(1, ("state", "action"), scope)
        same(got, ref.scan(pos, action, reward, dirs=dirs), 3)
        tabs = run.tables()
        assert tabs["state"][0, -1] == 14 and tabs["state"][0, 0] == 1 and tabs["state"][0, 16 * 17 + 16] == 1
        assert tabs["action"][0, -1] == 20 and tabs["action"][0].sum() == T + 6
        assert all(np.array_equal(tabs[k], ref.tables[k]) for k in tabs)


@pytest.mark.parametrize("scope", ["env", "shared"])
def test_keep_mask_null_outputs_aliasing_and_direction_forms(scope):
    T, N = 65, 63
    pos, action, dirs, reward = walk(T, N)
    want, tabs, keep = walk_ref(T, N, 3, scope, 0.5, keep_seed=2)
    assert keep.any() and not keep.all()
    run = Run(N, 3, scope, 0.5)
    got = run.scan(pos, action, dirs, reward, keep=keep)
    same(got, want, 3)
    assert np.array_equal(got["reward"][keep != 0], reward[keep != 0])
    for outs in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:                 # every NULL combination
        run = Run(N, 3, scope, 0.5)
        got = run.scan(pos, action, dirs, reward, keep=keep, outs=outs)
        for k, on in zip(("state", "action", "reward"), outs):
            assert (got[k] is None) if not on else np.array_equal(got[k], want[k]), (outs, k)
        assert all(np.array_equal(run.tables()[k], tabs[k]) for k in tabs), outs
    run = Run(N, 3, scope, 0.5)
    got = run.scan(pos, action, dirs, reward, keep=keep, reward_out="alias")
    assert np.array_equal(got["reward"], want["reward"])
    # one direction per env (t-stride 0) == the same direction repeated over [T][N]; no directions == all zero
    per_env = dirs[0].copy()
    a = Run(N, 2, scope).scan(pos, action, per_env, reward)
    b = Run(N, 2, scope).scan(pos, action, np.broadcast_to(per_env, (T, N)), reward)
    c = Run(N, 2, scope).scan(pos, action, None, reward)
    d = Run(N, 2, scope).scan(pos, action, np.zeros((T, N), np.int64), reward)
    ref = br.BonusRef(N, ("action",), scope).scan(pos, action, reward, dirs=per_env)
    assert np.array_equal(a["action"], b["action"]) and np.array_equal(a["action"], ref["action"])
    assert np.array_equal(c["action"], d["action"]) and not np.array_equal(a["action"], c["action"])


@pytest.mark.parametrize("geom", [(5, 7, 7), (32, 32, 1), (32, 32, 8), (7, 5, 3)])
def test_other_grids_and_action_counts(geom):
    w, h, na = geom
    T, N = 20, 70
    pos, action, dirs, reward = walk(T, N, 11, w, h, na)
    rs = np.random.RandomState(9)
    pos[..., 0] = np.where(np.isfinite(pos[..., 0]), rs.randint(-1, h + 1, (T, N)), pos[..., 0])    # the whole grid and its rim
    pos[..., 1] = np.where(np.isfinite(pos[..., 1]), rs.randint(-1, w + 1, (T, N)), pos[..., 1])
    for scope in ("env", "shared"):
        ref = br.BonusRef(N, ("state", "action"), scope, 1.0, w, h, na)
        want = ref.scan(pos, action, reward, dirs=dirs)
        run = Run(N, 3, scope, 1.0, w, h, na)
        same(run.scan(pos, action, dirs, reward), want, 3)
        assert all(np.array_equal(run.tables()[k], ref.tables[k]) for k in ref.tables)


@pytest.mark.parametrize("scope", ["env", "shared"])
def test_nothing_outside_the_tables_is_written(scope):
    from twoarmy_amd import ppo_ops
    T, N, G = 9, 5, 4096
    pos, action, dirs, reward = walk(T, N)
    words = {k: ppo_ops.bonus_table_words(k, scope, 17, 17, 7, N) for k in ("state", "action")}
    guarded = {k: torch.full((2 * G + 4 * n,), 0xA5, dtype=torch.uint8, device=DEV) for k, n in words.items()}
    run = Run(N, 3, scope)
    for k, n in words.items():
        run.tab[k] = guarded[k][G:G + 4 * n].view(torch.int32)
        run.tab[k].zero_()
    want, tabs, _ = walk_ref(T, N, 3, scope)
    same(run.scan(pos, action, dirs, reward), want, 3)
    for k, n in words.items():
        g = guarded[k].cpu().numpy()
        assert (g[:G] == 0xA5).all() and (g[G + 4 * n:] == 0xA5).all(), k
        assert np.array_equal(run.tables()[k], tabs[k])


def test_bad_arguments_are_rejected_and_sizes_are_what_the_header_says():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    assert lib.ppo_bonus_table_words(1, 0, 17, 17, 7, 10) == 290 * 10
    assert lib.ppo_bonus_table_words(2, 0, 17, 17, 7, 4096) == 8093 * 4096        # 133 MB of action counts at 4096 envs
    assert lib.ppo_bonus_table_words(1, 1, 17, 17, 7, 4096) == 2 * 290
    assert lib.ppo_bonus_table_words(2, 1, 32, 32, 8, 1) == 2 * 32769
    assert lib.ppo_bonus_workspace_bytes(3, 1, 128, 17, 17, 7) == 4 * 128 * (290 + 8093)
    assert lib.ppo_bonus_workspace_bytes(2, 0, 128, 17, 17, 7) == 0
    for bad in [(0, 0, 17, 17, 7, 1), (3, 0, 17, 17, 7, 1), (1, 2, 17, 17, 7, 1), (1, 0, 0, 17, 7, 1), (1, 0, 17, 33, 7, 1),
                (2, 0, 17, 17, 0, 1), (2, 0, 17, 17, 9, 1), (1, 0, 17, 17, 7, -1), (2, 0, 32, 32, 8, 1 << 20)]:
        assert lib.ppo_bonus_table_words(*bad) == -1, bad
    assert lib.ppo_bonus_workspace_bytes(0, 1, 4, 17, 17, 7) == -1 and lib.ppo_bonus_workspace_bytes(1, 1, -1, 17, 17, 7) == -1
    T, N = 2, 3
    pos = torch.zeros((T, N, 2), device=DEV)
    act = torch.zeros((T, N), dtype=torch.int32, device=DEV)
    rew = torch.zeros((T, N), device=DEV)
    st = torch.zeros(290 * N, dtype=torch.int32, device=DEV)
    at = torch.zeros(8093 * N, dtype=torch.int32, device=DEV)
    ws = torch.zeros(T * (290 + 8093), dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                 # noqa: E731
    good = dict(pos=p(pos), action=p(act), dir=None, st=0, sn=0, reward=p(rew), keep=None, T=T, N=N, w=17, h=17, na=7,
                mask=3, scope=0, scale=1.0, stab=p(st), atab=p(at), bs=None, ba=None, ro=p(rew), ws=p(ws), stream=None)
    call = lambda **kw: lib.ppo_bonus_scan(*{**good, **kw}.values())             # noqa: E731
    assert call() == 0 and call(scope=1) == 0
    assert call(T=0) == 0 and call(N=0) == 0
    bad = [dict(pos=None), dict(pos=C.c_void_p(pos.data_ptr() + 4)), dict(stab=None), dict(atab=None), dict(action=None),
           dict(mask=0), dict(mask=4), dict(scope=2), dict(scope=-1), dict(w=0), dict(h=33), dict(na=0), dict(na=9),
           dict(T=-1), dict(N=-1), dict(reward=None), dict(scope=1, ws=None), dict(dir=p(act), st=-1), dict(dir=p(act), sn=-1),
           dict(stab=C.c_void_p(st.data_ptr() + 4)), dict(T=1 << 16, N=1 << 15)]
    torch.cuda.synchronize()
    before = (st.clone(), at.clone(), rew.clone())
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (st, at, rew)))
    assert call(mask=1, atab=None, action=None) == 0 and call(mask=2, stab=None) == 0 and call(reward=None, ro=None) == 0
    torch.cuda.synchronize()


def test_tracker_reads_back_maps_and_resets():
    from twoarmy_amd.exploration import BonusTracker
    T, N = 33, 20
    pos, action, dirs, reward = walk(T, N)
    for scope in ("env", "shared"):
        tr = BonusTracker(N, DEV, ("action", "state"), scope, 2.0)
        out = tr.account(dev(pos, torch.float32), dev(action, torch.int32), dev(reward, torch.float32),
                         dir=dev(dirs, torch.int32))
        ref = br.BonusRef(N, ("state", "action"), scope, 2.0)
        want = ref.scan(pos, action, reward, dirs=dirs)
        assert np.array_equal(out.cpu().numpy(), want["reward"])
        assert np.array_equal(tr.bonus["state"].cpu().numpy(), want["state"])
        r = tr.read()
        st, ac = ref.tables["state"].sum(0), ref.tables["action"].sum(0)
        assert np.array_equal(r["state"], st[:-1].reshape(17, 17)) and r["other"] == {"state": st[-1], "action": ac[-1]}
        assert np.array_equal(r["action"], ac[:-1].reshape(17, 17, 4, 7).transpose(2, 3, 0, 1))
        assert r["state"].sum() + r["other"]["state"] == T * N
        if scope == "env":
            pe = tr.read(per_env=True)
            assert np.array_equal(pe["state"], ref.tables["state"][:, :-1].reshape(N, 17, 17))
        one = tr.account(dev(pos[0], torch.float32), dev(action[0], torch.int32), dev(reward[0], torch.float32),
                         dir=dev(dirs[0], torch.int32))                                     # one step: [N]
        assert one.shape == (N,) and np.array_equal(one.cpu().numpy(), ref.scan(pos[:1], action[:1], reward[:1],
                                                                              dirs=dirs[:1])["reward"][0])
        tr.reset_counts()
        assert tr.read()["state"].sum() == 0


def test_vec_env_returns_the_shaped_reward():
    from twoarmy_amd.vecenv import TwoarmyVecEnv
    from twoarmy_amd._lib import FIELDS
    N = 65
    env = TwoarmyVecEnv("MiniGrid-twoarmy-17x17-v6", num_envs=N, state_bonus=True, action_bonus=True, bonus_scope="shared",
                        bonus_scale=0.5)
    try:
        env.reset()
        ref = br.BonusRef(N, ("state", "action"), "shared", 0.5)
        rs = np.random.RandomState(1)
        for _ in range(12):
            a = rs.randint(0, 5, N)
            _, r, term, trunc, info = env.step(torch.from_numpy(a))
            d = env.engine.get_state()[2][:, FIELDS["DIR"]]
            ext = info["reward_extrinsic"].cpu().numpy()
            want = ref.scan(env.agent_yx.cpu().numpy()[None], np.where(a == 4, 6, a)[None], ext[None], dirs=d[None])
            assert np.array_equal(r.cpu().numpy(), want["reward"][0])
            assert (r.cpu().numpy() > ext).all()
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ 7. trainer
def _trainer(bonus, her_goal_run=False):
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(3)
    eng = TwoarmyEngine(6, 64, 17, seed=9981)
    agent = PPO()
    agent.K_epochs = 1
    tr = VecPPOTrainer(agent, eng, rollout_steps=16, minibatch=256)
    if bonus:
        tr.enable_bonus(("state", "action"), bonus, 0.25)
    return tr, eng


@pytest.mark.parametrize("scope", ["env", "shared"])
def test_trainer_shapes_its_own_tensors_and_hindsight_records_carry_them(scope):
    tr, eng = _trainer(scope)
    plain, eng2 = _trainer(None)
    try:
        ref = br.BonusRef(64, ("state", "action"), scope, 0.25)
        seen = 0
        for u in range(5):                                  # 80 steps: episodes of 50 steps end inside, counts carry over
            tr.collect(); plain.collect()
            assert plain.reward_train is plain.reward and plain.shape_rewards() is plain.reward
            shaped = tr.shape_rewards()
            assert shaped is tr.reward_train and shaped is not tr.reward
            assert torch.equal(tr.reward, plain.reward) and torch.equal(tr.action, plain.action)      # same rollout
            want = ref.scan(tr.pos[4:20].cpu().numpy(), tr.env_actions().cpu().numpy(), tr.reward.cpu().numpy(),
                            keep=tr.term.cpu().numpy(), dirs=tr.dir.cpu().numpy())
            assert np.array_equal(shaped.cpu().numpy(), want["reward"]), u
            assert (tr.dir.cpu().numpy() >= 0).all() and (tr.dir.cpu().numpy() < 4).all()
            h = tr.relabel()
            tr.account_episodes(); plain.account_episodes()
            a, b = tr.episode_stats(), plain.episode_stats()
            # mean_neg_logp is no episode statistic: it averages the actor's log-probabilities, which two separate forward
            # passes of two trainers reproduce only to rounding
            assert abs(a.pop("mean_neg_logp") - b.pop("mean_neg_logp")) < 1e-5
            assert a == b and tr.stats() == plain.stats() and tr.running_score(0.0) == plain.running_score(0.0)
            assert a["reward_hist"][-1] == 0                # every accounted reward is one of the env's own values
            if h["t"].numel():
                seen += 1
                t, n, done = h["t"].long(), h["n"].long(), h["done"] != 0
                assert done.any() and (h["reward"][done] == 0.9).all()
                assert torch.equal(h["reward"][~done], tr.reward_train[t[~done], n[~done]])
                assert (h["reward"][~done] > tr.reward[t[~done], n[~done]]).all()
                adv, target = tr.compute_targets()
                assert torch.isfinite(adv).all() and adv.numel() == 16 * 64 + h["t"].numel()
            tr.her = None
            tr.carry_over(); plain.carry_over()
        assert seen > 0
        bs = tr.bonus_stats()
        assert bs["state"].sum() + bs["other"]["state"] == 80 * 64 and bs["mean"] > 0
        tab = ref.tables["state"].sum(0)
        assert np.array_equal(bs["state"], tab[:-1].reshape(17, 17))
    finally:
        eng.close(); eng2.close()


ARGS = ["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", "64", "--rollout_steps", "16", "--minibatch", "256",
        "--updates", "2", "--k_epochs", "1", "--cuda", "cuda:0"]


def _lines(capsys):
    return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]


def test_train_ppo_logs_the_bonus_and_is_unchanged_without_it(tmp_path, capsys):
    """--bonus none (the default, tests/test_bonus_cpu.py) makes no tracker, trains on the reward tensor itself and logs
    the line as it was; --bonus both appends `bonus mean` behind the same fields and writes the count maps."""
    import os
    from twoarmy_amd.soa import train_ppo
    b = train_ppo.main(ARGS + ["--bonus", "none"])
    none = _lines(capsys)
    d = str(tmp_path / "bonus")
    c = train_ppo.main(ARGS + ["--bonus", "both", "--bonus_dir", d])
    both = _lines(capsys)
    assert len(none) == len(both) == 2
    assert b.bonus is None and b.reward_train is b.reward and b.dir is None
    assert " bonus mean" not in none[0] and none[0].startswith("update 0: rollout ")
    assert re.search(r" rewards \[[\d ]+\]$", none[0])                              # the line ends where it always did
    blank = lambda ln: re.sub(r"-?\d+(?:\.\d+)?|(?<=[ /])-(?=[ /])", "#", ln)       # noqa: E731
    for ln_n, ln_b in zip(none, both):
        m = re.search(r" bonus mean (\d+\.\d{4})$", ln_b)
        assert m and float(m.group(1)) > 0
        assert blank(ln_b[:m.start()]) == blank(ln_n)                               # the same fields in front of it
    # the first rollout precedes any update: extrinsic fields are equal with and without shaping
    ext = lambda ln: re.search(r"episodes \d+ successes \d+ mean_r \S+", ln).group(0)  # noqa: E731
    assert ext(none[0]) == ext(both[0])
    assert sorted(os.listdir(d)) == ["bonus_000000_rank0.npz", "bonus_000001_rank0.npz"]
    z = np.load(os.path.join(d, "bonus_000001_rank0.npz"))
    assert z["state"].shape == (17, 17) and z["action"].shape == (4, 7, 17, 17)
    assert z["state"].sum() + z["other_state"] == 2 * 16 * 64 == z["action"].sum() + z["other_action"]
    assert c.reward_train is not c.reward
