"""The shortest-path prior on hindsight records: VecPPOTrainer.enable_prior(hindsight=True) labels relabel()'s records
under their own goals (mg_nav_goal_moves on the engine's planes) and update() trains on those labels; the statistics and
the command line around it.  64 envs, 16-step rollouts, episodes of 12 steps so that every rollout ends some."""
import re

import numpy as np
import pytest
import torch

import goal_moves_ref
import nav_ref
import prior_ref
from nav_util import host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = nav_ref.UNREACHABLE
N, T, MAX_STEPS, MB = 64, 16, 12, 512
STATIC = nav_ref.PASS_DEFAULT | (1 << 6)


def _trainer(variant, state=None):
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(5)
    eng = TwoarmyEngine(variant, N, 17, seed=9981, max_steps=MAX_STEPS)
    agent = PPO()
    agent.K_epochs = 1
    if state is not None:
        agent.actor.load_state_dict(state[0]); agent.critic.load_state_dict(state[1])
    agent.to(eng.device).use_nhwc()
    return VecPPOTrainer(agent, eng, rollout_steps=T, minibatch=MB, value_chunk=MB), eng


def _state(tr):
    return ({k: v.clone() for k, v in tr.agent.actor.state_dict().items()},
            {k: v.clone() for k, v in tr.agent.critic.state_dict().items()})


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.parameters(), b.parameters()))


def _perm(total, seed):
    """Whole minibatches only: every distinct batch size costs a convolution search."""
    return torch.randperm(total, generator=torch.Generator().manual_seed(seed))[:total // MB * MB]


@pytest.mark.parametrize("variant", [6, 4])
def test_labels_statistics_and_update(variant, monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # scoped: two updates must agree bit for bit
    plain, e0 = _trainer(variant)
    state = _state(plain)
    hind, e1 = _trainer(variant, state)
    plain.enable_prior(0.5)
    hind.enable_prior(0.5, hindsight=True)
    assert plain.prior["hindsight"] is False and hind.prior["hindsight"] is True and hind.her_moves is None
    for u in range(2):                          # the second rollout relabels over a window of two; `hind` alone goes there
        for tr in (plain, hind)[u:]:
            tr.collect()
            tr.relabel()
        h = hind.her
        R = int(h["t"].numel())
        assert R > 0                                                      # the test cannot pass empty
        if u == 0:                                                        # one start: the same rollout, the same records
            assert all(torch.equal(h[k], plain.her[k]) for k in ("t", "n", "goal"))
        hind.label_expert()
        hind.her = dict(h)                                                # records that were not labelled: another relabel()
        with pytest.raises(RuntimeError, match="label_expert"):
            hind.update(permutations=[_perm(T * N + R, u)])
        hind.her = h
        assert hind.her_moves.shape == (R,) and hind.her_moves.dtype == torch.uint8 and hind.her_dist.shape == (R,)

        # the labels against the host reference on the engine's planes and the acting positions
        ty = host(e1.plane_views()[0])
        t, n, goal = host(h["t"]), host(h["n"]), host(h["goal"])
        pos, age, init = host(hind.pos[3:3 + T]), host(hind.age[:-1]), host(hind.init_pos)
        want_m, want_d = goal_moves_ref.goal_moves(ty, None, 17, 17, t, n, goal, pos, age, init, pass_types=STATIC)
        m, d = host(hind.her_moves), host(hind.her_dist).view(np.uint16)
        assert np.array_equal(m, want_m) and np.array_equal(d, want_d)
        assert (m != 0).any()

        # what the records are: a done record's goal is the position its step reached
        done = host(h["done"]) != 0
        assert done.any() and np.isin(d[done], (0, 1, U)).all(), sorted(set(d[done].tolist()))
        # inside a run (consecutive steps of one env under one goal) the agent moves one cell per step
        di = d.astype(np.int64)
        run = (n[1:] == n[:-1]) & (t[1:] == t[:-1] + 1) & (goal[1:] == goal[:-1]).all(-1)
        both = run & (di[1:] != U) & (di[:-1] != U)
        assert both.any() and (di[:-1][both] - di[1:][both] <= 1).all()

        # the statistics against numpy
        ps = hind.prior_stats()
        act = host(hind.action)[t, n]
        pm = prior_ref.to_policy_mask(want_m, 5).astype(np.int64)
        lab = pm != 0
        hit = ((pm >> act) & 1) != 0
        assert ps["her_labelled"] == int(lab.sum()) and ps["her_agree"] == (hit & lab).sum() / lab.sum()
        assert 0 < ps["her_agree"] <= 1 and "her_opt_mass" not in ps
        if u == 1:
            break
        plain.label_expert()
        pp = plain.prior_stats()
        assert plain.her_moves is None and plain.her_dist is None
        assert pp["her_labelled"] is None and pp["her_agree"] is None
        assert all(ps[k] == pp[k] for k in ("agree", "opt_mass", "labelled", "coef"))

        # the updates from one start: the critic does not see the prior, the actor sees the hindsight labels
        perm = _perm(T * N + R, 10)
        assert (perm >= T * N).any()
        lp, lh = plain.update(permutations=[perm]), hind.update(permutations=[perm])
        assert torch.equal(lp[1], lh[1]) and _same(plain.agent.critic, hind.agent.critic)
        assert not _same(plain.agent.actor, hind.agent.actor)
        assert hind.her is None
        hind.carry_over()
    e0.close(); e1.close()


def test_hindsight_without_relabelling_is_the_plain_prior(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    plain, e0 = _trainer(6)
    hind, e1 = _trainer(6, _state(plain))
    plain.enable_prior(0.5)
    hind.enable_prior(0.5, hindsight=True)
    for tr in (plain, hind):
        tr.collect()
    with pytest.raises(RuntimeError, match="label_expert"):
        hind.update(permutations=[_perm(T * N, 0)])                       # update() without label_expert()
    for tr in (plain, hind):
        tr.label_expert()
    assert hind.her is None and hind.her_moves is None
    ps = hind.prior_stats()
    assert ps["her_labelled"] is None and ps["her_agree"] is None
    perm = _perm(T * N, 1)
    lp, lh = plain.update(permutations=[perm]), hind.update(permutations=[perm])
    assert torch.equal(lp[0], lh[0]) and torch.equal(lp[1], lh[1])
    assert _same(plain.agent.actor, hind.agent.actor) and _same(plain.agent.critic, hind.agent.critic)
    e0.close(); e1.close()


ARGS = ["--env", "MiniGrid-twoarmy-17x17-v4", "--num_envs", str(N), "--rollout_steps", str(T), "--minibatch", str(MB),
        "--k_epochs", "1", "--updates", "1", "--max_steps", str(MAX_STEPS)]


def test_train_ppo_appends_her_agree_only_when_asked(capsys):
    from twoarmy_amd.soa import train_ppo
    lines = lambda: [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]     # noqa: E731
    with pytest.raises(SystemExit):
        train_ppo.main(ARGS + ["--prior_hindsight"])                      # needs --prior_coef or --expert_agreement
    lines()
    a = train_ppo.main(ARGS + ["--prior_coef", "0.1"])
    old = lines()
    b = train_ppo.main(ARGS + ["--prior_coef", "0.1", "--prior_hindsight"])
    new = lines()
    assert len(old) == len(new) == 1
    pat = r" expert agree (\d\.\d{3}) opt_mass (\d\.\d{3})"
    mo, mn = re.search(pat + "$", old[0]), re.search(pat + r" her agree (\d\.\d{3})$", new[0])
    assert mo and mn and "her agree" not in old[0]
    assert int(re.search(r" her_records (\d+) ", new[0]).group(1)) > 0
    assert mo.groups() == mn.groups()[:2]                                 # the first rollout precedes any update
    blank = lambda ln: re.sub(r"-?\d+(?:\.\d+)?|(?<=[ /])-(?=[ /])", "#", ln)       # noqa: E731
    assert blank(new[0][:mn.end(2)]) == blank(old[0])                     # the old format, byte for byte, then the new field
    assert a.prior["hindsight"] is False and a.her_moves is None and b.prior["hindsight"] is True
