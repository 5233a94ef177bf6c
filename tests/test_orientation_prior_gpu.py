"""The look-ahead prior of the orientation head in the SoA trainer: 8 envs x 16 steps of v6 (episodes of 10 steps, so that
they end inside a rollout) over two rollouts with relabelling on.  The seeded policy reaches no goal, so the episodes of the
even envs are declared successes after relabel(): the sample set then holds rollout samples and hindsight samples."""
import numpy as np
import pytest
import torch

import ahead_ref
import nav_ref
import timed_nav_ref
from test_soa_cpu import seeded_agent

pytestmark = pytest.mark.gpu
N, T = 8, 16
BALL = 1 << 6
PASS = nav_ref.PASS_DEFAULT | BALL


def rollouts(prior=None, n_rollouts=2, inspect=None):
    """A trainer run over n_rollouts rollouts and updates, the same draws for every call; inspect(tr, r) runs after the
    labels of rollout r are made and before its update.  -> the trainer (engine closed)."""
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.soa_vec import VecSoATrainer
    eng = TwoarmyEngine(6, N, 17, seed=9981, max_steps=10)
    agent = seeded_agent()
    agent.K_epochs = agent.K_epochs_pre_agent_position = 1
    tr = VecSoATrainer(agent, eng, rollout_steps=T, minibatch=64, value_chunk=512)
    if prior is not None:
        tr.enable_orientation_prior(**prior)
    for r in range(n_rollouts):
        uni = torch.rand(T + 1, N, 3, generator=torch.Generator().manual_seed(40 + r)).to(tr.device)
        tr.collect(uniforms=uni)
        tr.relabel()
        tr.term[:, ::2] |= tr.trunc[:, ::2]                          # the even envs "reach the goal"
        if prior is not None:
            tr.label_ahead()
        if inspect is not None:
            inspect(tr, r)
        torch.manual_seed(70 + r)                                      # the permutations of both learners
        tr.update()
        tr.carry_over()
    eng.close()
    return tr


def nets(tr):
    ag = tr.agent
    return [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
            for m in (ag.actor, ag.critic, ag.agent_position_preditor)]


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


_BASE = {}


def base(n_rollouts):
    if n_rollouts not in _BASE:
        _BASE[n_rollouts] = nets(rollouts(n_rollouts=n_rollouts))
    return _BASE[n_rollouts]


@pytest.mark.parametrize("timed", [False, True])
def test_labels_and_statistics_against_the_reference(timed):
    seen = {}

    def inspect(tr, r):
        ty = tr.engine.plane_views()[0].cpu().numpy()
        pos, age = tr.pos[3:3 + T].cpu().numpy(), tr.age[:-1].cpu().numpy()
        init = tr.init_pos.cpu().numpy()
        if timed:
            from twoarmy_amd import minigrid_nav as nav
            blocked = nav.twoarmy_schedule(blocks=True).numpy().view(np.uint32)
            dist = timed_nav_ref.fields(ty, None, 17, 17, blocked, 6, PASS)[0]
            # the trainer's one timed field: label_ahead() reads the buffer every timed feature shares
            fields = [v for v in vars(tr).values()
                      if torch.is_tensor(v) and v.dtype == torch.uint16 and tuple(v.shape) == (N, 6, 289)]
            assert len(fields) == 1 and fields[0] is tr.timed_field and tr._timed_field_at == tr.env_steps
            assert np.array_equal(tr.timed_field.cpu().numpy().view(np.uint16), dist)
        else:
            dist = nav_ref.fields(ty, None, 17, 17, PASS)[0]
        want = ahead_ref.ahead(dist, pos, 17, 17, 3, age, init)
        lab = tr.expert_ahead.cpu().numpy().view(np.uint64)
        assert np.array_equal(lab, want[0]) and np.array_equal(tr.ahead_dist.cpu().numpy().view(np.uint16), want[1])
        assert (want[0] != 0).mean() > 0.5
        h = {k: tr.her[k].cpu().numpy() for k in ("t", "n", "goal", "done")}
        assert h["t"].size > 0 and tr._her_ahead_of is tr.her
        hw = ahead_ref.goal_ahead(ty, None, 17, 17, h["t"], h["n"], h["goal"], pos, 3, age, init, pass_types=PASS)
        hl = tr.her_ahead.cpu().numpy().view(np.uint64)
        assert np.array_equal(hl, hw[0]) and np.array_equal(tr.her_ahead_dist.cpu().numpy().view(np.uint16), hw[1])
        # a done record acts at most one move from its goal (the state AFTER its step): its label is the one bit of that
        # displacement -- bit 24 alone only where the agent stood on the goal cell already, which a moving agent's done
        # records do not (measured on this rollout pair: 0 of 18 and 0 of 34 done records)
        acting = np.where((age <= 0)[..., None], init, pos)[h["t"], h["n"]]
        dy = np.floor(h["goal"][:, 0]) - np.floor(acting[:, 0])
        dx = np.floor(h["goal"][:, 1]) - np.floor(acting[:, 1])
        done = h["done"] != 0
        assert done.any() and (np.abs(dy[done]) + np.abs(dx[done]) <= 1).all()
        bit = ((dy + 3) * 7 + dx + 3).astype(np.int64)
        assert (hl[done] == (np.uint64(1) << bit[done].astype(np.uint64))).all()
        still = done & (dy == 0) & (dx == 0)
        assert (hl[still] == 1 << 24).all()
        # statistics against numpy
        st = tr.orientation_prior_stats()
        fut = tr.future[:T].cpu().numpy().astype(np.int64) + 3
        on = want[0] != 0
        hit = ((want[0] >> (fut[..., 0] * 7 + fut[..., 1]).astype(np.uint64)) & np.uint64(1)) != 0
        assert st["labelled"] == int(on.sum()) and st["agree"] == pytest.approx((hit & on).sum() / on.sum(), abs=1e-12)
        ot, on_, og, disp = tr.orientation_samples()
        ns = tr._n_success_samples
        rec = tr._her_sample_rec.cpu().numpy()
        d = disp[ns:].cpu().numpy().astype(np.int64) + 3
        hon = hl[rec] != 0
        hhit = ((hl[rec] >> (d[:, 0] * 7 + d[:, 1]).astype(np.uint64)) & np.uint64(1)) != 0
        assert ns > 0 and rec.size > 0 and st["her_labelled"] == int(hon.sum())
        assert st["her_realised"] == pytest.approx((hhit & hon).sum() / hon.sum(), abs=1e-12)
        assert st["coef"] == pytest.approx(0.5 * 0.5 ** r)
        seen[r] = True

    tr = rollouts(dict(coef=0.5, decay=0.5, timed=timed, hindsight=True), inspect=inspect)
    assert seen == {0: True, 1: True} and tr.orient_prior["updates"] == 2
    # the replay FIFO carries labels
    assert len(tr._replay) > 0 and all(e["ahead"].dtype == torch.int64 and e["ahead"].shape[0] == e["disp"].shape[0]
                                       for e in tr._replay)
    assert any(bool((e["ahead"] != 0).any()) for e in tr._replay)


def test_the_prior_changes_the_orientation_head_only(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # scoped: separate runs must agree bit for bit
    # one update: the policy of the NEXT rollout is conditioned on draws from the changed head, so only the first update
    # can leave the actor and the critic bit for bit
    a, c, o = base(1)
    pa, pc, po = nets(rollouts(dict(coef=0.5, hindsight=True), n_rollouts=1))
    assert same(a, pa) and same(c, pc) and not same(o, po)
    a, c, o = base(2)
    for kw in (dict(coef=0.0), dict(coef=0.0, hindsight=True, timed=True)):   # label and report only: every bit the old one
        za, zc, zo = nets(rollouts(kw))
        assert same(a, za) and same(c, zc) and same(o, zo)
    assert not hasattr(rollouts(None, n_rollouts=1), "expert_ahead")          # without the enable call nothing new appears


def test_every_state_adds_the_other_steps_as_prior_only_rows():
    from twoarmy_amd.soa.agent.Self_orientation_agent import self_orinetation_agent as Agent
    counts = {}

    def inspect(tr, r):
        ot, on, og, disp = tr.orientation_samples()
        _, success = tr._episode_ends()
        rows = tr._prior_rows(ot, on, og, disp)
        counts[r] = (ot.numel(), rows[0].numel(), int((~success).sum()), rows)
        assert rows[0].numel() == ot.numel() + int((~success).sum()) == ot.numel() + tr._n_prior_only
        nll = rows[5]
        assert int(nll.sum()) == ot.numel() and not bool(nll[ot.numel():].any())
        assert torch.equal(rows[4][ot.numel():], tr.expert_ahead[~success])          # labelled under the env's goal
        # the NLL of a minibatch is over its NLL rows only: the value without the prior-only rows
        g = torch.Generator().manual_seed(3)
        B = rows[0].numel()
        p0 = (torch.rand(B, 7, generator=g) + 0.1).to(tr.device)
        p1 = (torch.rand(B, 7, generator=g) + 0.1).to(tr.device)
        p0, p1 = p0 / p0.sum(1, keepdim=True), p1 / p1.sum(1, keepdim=True)
        k = ot.numel()
        with_rows = Agent.orientation_nll(p0.double(), p1.double(), rows[3], None, nll)
        alone = Agent.orientation_nll(p0[:k].double(), p1[:k].double(), disp)
        assert float(with_rows) == pytest.approx(float(alone), rel=1e-12)

    tr = rollouts(dict(coef=0.5, every_state=True), n_rollouts=1, inspect=inspect)
    assert counts[0][1] > counts[0][0] > 0 and tr.orient_prior["every_state"]


def test_real_minibatches_mix_rollout_replay_and_padding_rows():
    """update_orientation itself, second rollout (the FIFO then holds the first one's successes), every_state on: every
    orientation_step is intercepted, and the NLL it would compute on the head's own probabilities must be the NLL of the
    rows that carry one -- rollout samples and replayed samples -- taken alone; prior-only and padding rows carry none,
    padding rows no label either."""
    from twoarmy_amd.soa.agent.Self_orientation_agent import self_orinetation_agent as Agent
    calls = []

    def inspect(tr, r):
        if r != 1:
            return
        ag = tr.agent
        real = ag.orientation_step
        ot, _, _, _ = tr.orientation_samples()
        _, success = tr._episode_ends()
        n_eps = int(torch.unique(tr._success_key).numel())
        rep = tr.replay_samples(n_eps)
        tr._expect = (ot.numel(), int((~success).sum()), 0 if rep is None else int(rep["disp"].shape[0]))

        def step(x8, p4, goal, disp, n_valid=None, ahead=None, prior_coef=0.0, nll_rows=None):
            B = disp.shape[0]
            nv = B if n_valid is None else n_valid
            assert ahead is not None and ahead.shape == (B,) and nll_rows is not None and nll_rows.shape == (B,)
            assert prior_coef == pytest.approx(0.5) and not bool(nll_rows[nv:].any()) and not bool((ahead[nv:] != 0).any())
            with torch.no_grad():
                p0, p1 = ag.orient_probs(x8, p4, goal)
                got = Agent.orientation_nll(p0.double(), p1.double(), disp, n_valid, nll_rows)
                m = nll_rows.clone()
                alone = Agent.orientation_nll(p0[m].double(), p1[m].double(), disp[m]) if bool(m.any()) else None
            if alone is not None:
                assert float(got) == pytest.approx(float(alone), rel=1e-12)
            calls.append((B, nv, int(nll_rows.sum()), int((ahead != 0).sum())))
            return real(x8, p4, goal, disp, n_valid, ahead=ahead, prior_coef=prior_coef, nll_rows=nll_rows)
        ag.orientation_step = step

    tr = rollouts(dict(coef=0.5, every_state=True), n_rollouts=2, inspect=inspect)
    n_samples, n_prior_only, n_rep = tr._expect
    assert n_samples > 0 and n_prior_only > 0 and n_rep > 0                     # all three kinds of rows were there
    assert sum(c[1] for c in calls) == n_samples + n_prior_only + n_rep         # one epoch: every row once
    assert sum(c[2] for c in calls) == n_samples + n_rep                        # the NLL rows: samples and replay
    assert any(c[0] > c[1] for c in calls) and all(c[0] >= 64 for c in calls)   # a padded minibatch
    assert sum(c[3] for c in calls) > 0


def test_command_line(capsys):
    from twoarmy_amd.soa import train_SoA, train_ppo
    args = ["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", "8", "--rollout_steps", "16", "--minibatch", "64",
            "--updates", "1", "--k_epochs", "1", "--k_epochs_orientation", "1", "--max_steps", "10", "--cuda", "cuda:0"]
    tr = train_SoA.main(args + ["--orient_agreement", "--orient_prior_hindsight"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert " orient agree " in line and " her realised " in line and tr.orient_prior["coef"] == 0.0
    with pytest.raises(SystemExit, match="self-orientation agent only"):
        train_ppo.main(args + ["--orient_agreement"])
