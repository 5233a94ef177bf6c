"""ppo_loss_fwd_bwd_stats (csrc/ppo_kernels.hip): the loss outputs bit for bit against ppo_loss_fwd_bwd_masked, the
accumulators against the float64 statement of update_stats_ref.py within float32 rounding bounds derived next to them,
accumulation, padding, determinism, every argument rule, and the trainer's wiring with the KL stop.  The entry's two
stream checks are a case of the table in test_streams_gpu.py.  The shapes are the smallest that reach every edge: one row, one workgroup less and more than
full, padding across workgroups, and 66 workgroups (more partials than the final pass has lanes)."""
import numpy as np
import pytest
import torch

import update_stats_ref as ur
from ppo_util import DEV, accepted, dev as _dev, lib as _lib, lib_module as _libmod, ops as _ops, ptr as _P
from stream_util import host, same_bits

pytestmark = pytest.mark.gpu
EPS32 = ur.EPS32
CLIP, ENT = ur.CLIP, ur.ENT
SHAPES = [(1, 1), (255, 255), (256, 256), (257, 257), (768, 257), (600, 1)]       # (B, n_valid)
BIG = (16641, 16641)                                                              # 65 workgroups and one row


def _raw(name, x, n_valid, stats=None, sws=None):
    """One raw call of `name` on device copies of the inputs x -> (losses, grad_probs, grad_value) as host arrays."""
    p, a, old, adv, value, target = (_dev(t) for t in x)
    B = len(a)
    nb = (B + 255) // 256
    outs = [torch.full((n,), np.nan, device=DEV) for n in (2, B * 5, B, 2 * nb)]
    args = [_P(t) for t in (p, a, old, adv, value, target)] + [B, n_valid, 5, CLIP, ENT] + [_P(o) for o in outs]
    if stats is not None:
        args += [_P(stats), _P(sws)]
    assert accepted(name, args)
    return [host(o) for o in outs[:3]]


def _stats_call(x, n_valid, stats):
    """The stats entry on x into the device row `stats`, its workspace NaN-filled: every entry is written before it is read."""
    sws = torch.full((_lib().ppo_loss_stats_workspace(len(x[1])),), np.nan, dtype=torch.float64, device=DEV)
    return _raw("ppo_loss_fwd_bwd_stats", x, n_valid, stats, sws)


def _zeros():
    return torch.zeros(ur.WORDS, dtype=torch.float64, device=DEV)


_inputs = {}


def _x(B):
    if B not in _inputs:
        _inputs[B] = ur.inputs(B, 7000 + B)
    return _inputs[B]


# ------------------------------------------------------------------------------------------------ the loss outputs
@pytest.mark.parametrize("B,n_valid", SHAPES)
def test_loss_outputs_equal_the_masked_entry_bit_for_bit(B, n_valid):
    x = _x(B)
    want = _raw("ppo_loss_fwd_bwd_masked", x, n_valid)
    got = _stats_call(x, n_valid, _zeros())
    for g, w, name in zip(got, want, ("losses", "grad_probs", "grad_value")):
        assert not np.isnan(w).any() and same_bits(g, w), name


# ------------------------------------------------------------------------------------------------ the accumulators
@pytest.mark.parametrize("B,n_valid", SHAPES + [BIG])
def test_accumulators_vs_float64_reference(B, n_valid):
    x = _x(B)
    stats = _zeros()
    _stats_call(x, n_valid, stats)
    got = host(stats)
    want, R = ur.accumulate(np.zeros(ur.WORDS), x[0], x[1], x[2], x[4], x[5], CLIP, n_valid)
    bound = ur._bounds(x, R, n_valid)
    err = np.abs(got - want)
    print("B %d n_valid %d: err / bound %s" % (B, n_valid, " ".join(
        "%d:%.3g" % (i, err[i] / bound[i]) for i in range(13) if bound[i] > 0)))
    for i in (0, 4, 10, 12):
        assert got[i] == want[i], (ur.NAMES[i], got[i], want[i])
    assert want[0] == n_valid and want[12] == 1 and not got[13:].any()
    assert (err <= bound).all(), [(ur.NAMES[i], err[i], bound[i]) for i in range(13) if err[i] > bound[i]]
    assert got[3] >= 0 and (n_valid < 16 or 0 < got[4] < n_valid)


def test_two_calls_on_the_halves_against_one_call_on_the_whole():
    x = _x(512)
    whole, halves = _zeros(), _zeros()
    _stats_call(x, 512, whole)
    _stats_call([t[:256] for t in x], 256, halves)
    _stats_call([t[256:] for t in x], 256, halves)
    w, h = host(whole), host(halves)
    assert np.array_equal(w[[0, 4, 5, 10]], h[[0, 4, 5, 10]]) and (w[12], h[12]) == (1, 2)
    sums = [1, 2, 3, 6, 7, 8, 9, 11]
    assert (np.abs(w[sums] - h[sums]) <= 1e-12 * np.abs(w[sums])).all(), (w, h)


def test_a_call_adds_to_a_non_zero_row_and_leaves_the_reserved_entries():
    x = _x(257)
    fresh = _zeros()
    _stats_call(x, 257, fresh)
    one = host(fresh)
    start = np.array([3, 1.5, -0.25, 0.125, 2, 1e-3, 4.0, 8.0, -2.0, 16.0, 1, 0.75, 5, -77.0, -77.0, -77.0])
    row = _dev(start.copy())
    _stats_call(x, 257, row)
    got = host(row)
    assert np.array_equal(got[13:], start[13:])                                  # the sentinels
    assert np.array_equal(got[[0, 4, 10, 12]], start[[0, 4, 10, 12]] + one[[0, 4, 10, 12]])
    assert got[5] == max(start[5], one[5]) == one[5]
    sums = [1, 2, 3, 6, 7, 8, 9, 11]
    assert np.array_equal(got[sums], start[sums] + one[sums])                    # one double addition each
    high = _dev(np.where(np.arange(16) == 5, 1e6, 0.0))                          # a maximum above the batch's stays
    _stats_call(x, 257, high)
    assert host(high)[5] == 1e6


def test_padding_leaves_equal_bits_in_all_sixteen_entries():
    x = _x(768)
    padded, plain = _dev(np.full(16, 0.5)), _dev(np.full(16, 0.5))
    _stats_call(x, 257, padded)
    _stats_call([t[:257] for t in x], 257, plain)
    assert same_bits(host(padded), host(plain))
    big, cut = _zeros(), _zeros()                                                # 66 workgroups of padding around one
    xb = _x(BIG[0])
    _stats_call(xb, 255, big)
    _stats_call([t[:255] for t in xb], 255, cut)
    assert same_bits(host(big), host(cut))


def test_the_same_call_twice_gives_equal_bits():
    xb = _x(BIG[0])
    a, b = _zeros(), _zeros()
    la = _stats_call(xb, BIG[1], a)
    lb = _stats_call(xb, BIG[1], b)
    assert same_bits(host(a), host(b)) and all(same_bits(u, v) for u, v in zip(la, lb))


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections_launch_nothing():
    """Every rule violated alone by a raw call: TW_E_ARG through the checked launch path, and after a synchronise losses,
    gradients and stats still hold their sentinels.  The same call with the rule kept is accepted and writes."""
    from test_ppo_kernels_edges_gpu import CANARY, _each_rejected, _fill
    B, A = 3, 5
    probs = torch.full((B, A), 0.2, device=DEV)
    action = torch.zeros(B, dtype=torch.int32, device=DEV)
    old, adv, value, target = (torch.full((B,), v, device=DEV) for v in (-1.6, 1.0, 0.5, 0.0))
    outs = [_fill(2), _fill(B * A), _fill(B), _fill(2), _fill(16, torch.float64), _fill(12, torch.float64)]
    good = [_P(t) for t in (probs, action, old, adv, value, target)] + [B, B, A, 0.1, 0.01] + [_P(o) for o in outs]
    bad = [(i, None) for i in (0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 15, 16)]         # 15: stats, 16: stats_workspace
    bad += [(15, _P(outs[4], 4)), (16, _P(outs[5], 4))]                            # off 8-byte alignment
    bad += [(8, 7), (8, 4), (7, 0), (7, B + 1), (6, 0)]
    _each_rejected("ppo_loss_fwd_bwd_stats", good, bad, outs)
    assert host(outs[4])[12] == CANARY + 1 and host(outs[4])[13] == CANARY         # the accepted call ADDS; reserved intact
    assert _lib().ppo_loss_stats_workspace(0) < 0 and _lib().ppo_loss_stats_workspace(-5) < 0
    assert [_lib().ppo_loss_stats_workspace(b) for b in (1, 256, 257, 16641)] == [12, 12, 24, 66 * 12]
    with pytest.raises(_libmod().TwoarmyLibraryError):                             # the front end raises what the C call returns
        _ops().ppo_losses(probs.repeat(1, 2)[:, :7].contiguous().requires_grad_(), value.view(-1, 1).requires_grad_(),
                          action, old, adv, target, stats=_zeros())
    with pytest.raises(AssertionError):
        _ops().ppo_losses(probs.requires_grad_(), value.view(-1, 1).requires_grad_(), action, old, adv, target,
                          stats=torch.zeros(8, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ front end
def test_front_end_accumulates_into_a_row_of_a_larger_tensor_and_caches_its_workspace():
    from twoarmy_amd import ppo_ops
    x = _x(600)
    p, a, old, adv, value, target = (_dev(t) for t in x)
    table = torch.zeros((3, 16), dtype=torch.float64, device=DEV)

    def run(stats):
        tp, tv = p.clone().requires_grad_(True), value.clone().view(-1, 1).requires_grad_(True)
        al, vl = ppo_ops.ppo_losses(tp, tv, a, old, adv, target, clip=CLIP, ent_coef=ENT, n_valid=257, stats=stats)
        gp, gv = torch.autograd.grad(al + vl, (tp, tv))
        return [host(t) for t in (al.detach(), vl.detach(), gp, gv)]

    plain, with_stats = run(None), run(table[1])
    ws = ppo_ops._stats_workspace(p.device, 600)
    again = run(table[1])
    assert ppo_ops._stats_workspace(p.device, 600) is ws and ws.numel() == 3 * 12   # made once per (device, B)
    assert all(same_bits(u, v) and same_bits(u, w) for u, v, w in zip(plain, with_stats, again))
    t = host(table)
    assert not t[0].any() and not t[2].any() and t[1, 0] == 2 * 257 and t[1, 12] == 2
    d = ppo_ops.update_stats_read(table)                                           # the one host read, here of a device tensor
    want = ur.read(ur.accumulate(np.zeros(16), x[0], x[1], x[2], x[4], x[5], CLIP, 257)[0])
    for k in ("entropy", "approx_kl", "clip_frac", "explained_variance", "saturated_frac", "top_mass"):
        assert np.isnan(d[k][0]) and abs(d[k][1] - want[k]) <= 1e-5 * max(1.0, abs(want[k])), k


# ------------------------------------------------------------------------------------------------ trainer
N_ENVS, T_STEPS, MB, K = 8, 16, 64, 3
SAMPLES = N_ENVS * T_STEPS


def _trainer(state=None, k_epochs=K):
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(5)
    eng = TwoarmyEngine(6, N_ENVS, 17, seed=9981)
    agent = PPO()
    agent.K_epochs = k_epochs
    if state is not None:
        agent.actor.load_state_dict(state[0]); agent.critic.load_state_dict(state[1])
    agent.to(eng.device).use_nhwc()
    return VecPPOTrainer(agent, eng, rollout_steps=T_STEPS, minibatch=MB), eng


def _params(tr):
    return [p.detach().clone() for net in (tr.agent.actor, tr.agent.critic) for p in net.parameters()]


def _run(tr, uniforms, perms):
    tr.collect(uniforms=uniforms)
    return tr.update(permutations=perms)


@pytest.fixture(scope="module")
def trainer_runs():
    """One start, one rollout (fixed uniforms), one update (fixed permutations) for five trainers: plain K = 3, with the
    diagnostics, with target_kl = 0, with target_kl = 1e9, and plain K = 1.  MIOpen's deterministic kernels for all of
    them: two updates must agree bit for bit."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        first, e0 = _trainer()
        state = ({k: v.clone() for k, v in first.agent.actor.state_dict().items()},
                 {k: v.clone() for k, v in first.agent.critic.state_dict().items()})
        uniforms = torch.rand(T_STEPS, N_ENVS, generator=torch.Generator().manual_seed(40)).to(first.device)
        perms = [torch.randperm(SAMPLES, generator=torch.Generator().manual_seed(u)) for u in range(K)]
        out, engines = {}, []
        for name, k_epochs, enable in (("plain", K, None), ("stats", K, {}), ("stop", K, dict(target_kl=0.0)),
                                       ("never", K, dict(target_kl=1e9)), ("one", 1, None)):
            tr, eng = (first, e0) if name == "plain" else _trainer(state, k_epochs)
            engines.append(eng)
            snaps = []
            if enable is not None:
                tr.enable_update_stats(**enable)
                step = tr.agent.minibatch_step_x

                def spy(*a, _step=step, _tr=tr, _snaps=snaps, **kw):               # the row after every optimiser step
                    res = _step(*a, **kw)
                    _snaps.append(_tr.agent.stats_row.clone())
                    return res
                tr.agent.minibatch_step_x = spy
            losses = _run(tr, uniforms, perms)
            out[name] = dict(tr=tr, losses=[host(x) for x in losses], params=[host(p) for p in _params(tr)],
                             snaps=[host(s) for s in snaps], logp=host(tr.logp))
        yield out
        for e in engines:
            e.close()
    finally:
        torch.backends.cudnn.deterministic = was


def _same_params(a, b):
    return all(same_bits(u, v) for u, v in zip(a["params"], b["params"]))


def test_trainer_with_diagnostics_trains_the_same_bits(trainer_runs):
    plain, st = trainer_runs["plain"], trainer_runs["stats"]
    assert all(same_bits(u, v) for u, v in zip(plain["losses"], st["losses"])) and _same_params(plain, st)
    assert plain["tr"].update_diag is None and plain["tr"].agent.stats_row is None and st["tr"].agent.stats_row is None
    assert set(plain["tr"].stats()) == {"env_steps", "episodes", "successes", "mean_reward"}
    us = st["tr"].update_stats()
    per = us["per_epoch"]
    assert us["epochs_run"] == K and per["rows"].tolist() == [SAMPLES] * K and per["calls"].tolist() == [SAMPLES // MB] * K
    assert np.isfinite(per["approx_kl"]).all() and (per["approx_kl"] >= 0).all()
    assert all(us[k] == per[k][K - 1] for k in per) and st["tr"].stats()["approx_kl"] == us["approx_kl"]
    assert 0 < us["entropy"] <= np.log(5) + 1e-6 and 0 <= us["clip_frac"] <= 1 and us["explained_variance"] <= 1
    # epoch 0, first minibatch: no optimiser step has changed the policy yet, so the ratio is 1 up to the float32 error
    # of logp and expf, rel = 8 * 2^-23 * (1 + |logp| + |old|) with logp = old = the rollout's log-probabilities
    first = st["snaps"][0]
    rel = 8 * EPS32 * (1 + 2 * np.abs(st["logp"]).max())
    print("first minibatch: ratio_dev_max %.3g, rel %.3g; approx_kl per epoch %s" % (first[5], rel, per["approx_kl"]))
    assert first[0] == MB and first[12] == 1
    assert first[5] <= rel, (first[5], rel)


def test_target_kl_zero_stops_after_the_first_epoch(trainer_runs):
    stop, one = trainer_runs["stop"], trainer_runs["one"]
    us = stop["tr"].update_stats()
    assert us["epochs_run"] == 1 and us["approx_kl"] > 0
    rows = host(stop["tr"].update_diag["stats"])
    assert rows[0, 0] == SAMPLES and not rows[1:].any()
    assert np.isnan(us["per_epoch"]["entropy"][1:]).all()
    assert _same_params(stop, one) and all(same_bits(u, v) for u, v in zip(stop["losses"], one["losses"]))
    assert len(stop["snaps"]) == SAMPLES // MB


def test_target_kl_out_of_reach_runs_every_epoch(trainer_runs):
    never, st = trainer_runs["never"], trainer_runs["stats"]
    assert never["tr"].update_stats()["epochs_run"] == K and _same_params(never, st)
    assert same_bits(host(never["tr"].update_diag["stats"]), host(st["tr"].update_diag["stats"]))


# ------------------------------------------------------------------------------------------------ CLI
ARGS = ["--env", "MiniGrid-twoarmy-17x17-v6", "--num_envs", "8", "--rollout_steps", "8", "--minibatch", "32",
        "--k_epochs", "2", "--updates", "1"]


def test_train_ppo_appends_the_diagnostics_only_when_asked(capsys):
    import re
    from twoarmy_amd.soa import train_ppo
    lines = lambda: [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]     # noqa: E731
    a = train_ppo.main(ARGS)
    none = lines()
    b = train_ppo.main(ARGS + ["--target_kl", "0.02"])
    asked = lines()
    assert len(none) == len(asked) == 1 and a.update_diag is None and b.update_diag["target_kl"] == 0.02
    assert re.search(r" rewards \[[\d ]+\]$", none[0]) and " ent " not in none[0]        # the line ends where it always did
    m = re.search(r" ent (\d\.\d{4}) kl (\d\.\d{6}) clipfrac (\d\.\d{4}) ev (-?\d+\.\d{4}) epochs ([12])$", asked[0])
    assert m, asked[0]
    assert not any(k.startswith("diag/") for k in a.agent.writer.scalars)
    logged = b.agent.writer.scalars
    assert {k for k in logged if k.startswith("diag/")} == {"diag/entropy", "diag/approx_kl", "diag/clip_frac",
                                                            "diag/explained_variance", "diag/epochs_run"}
    assert logged["diag/epochs_run"][0] == (0, float(m.group(5)))
