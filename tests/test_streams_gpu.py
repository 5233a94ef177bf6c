"""Every launch entry point on a side stream and under graph capture ("Streams and capture").

Part A: the call is made on a side stream behind a delay, its inputs copied in on that stream over a valid decoy; any
launch that went to another stream has then read the decoy or an unwritten workspace.  Part B: the call is captured on
a side stream and replayed twice on new inputs.  Both compare with the same call on the default stream bit for bit, and
with the CPU restatement of the op where the case names one.  The protocol is tests/stream_util.py; this file is the
table."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import bonus_episode_ref
import bonus_ref
import episode_ref
import gae_runs_ref as gr
import nav_ref
import obs_ref
import path_ref
import render_ref
import replay_ref
import timed_goal_ahead_ref as taref
import update_stats_ref as ur
import visit_ref
from nav_util import u16_full
from test_bonus_episode_gpu import walk as episode_walk
from stream_util import (DEV, ENQUEUE_MS, Case, check_against_ref, check_same, dev, expected_sequence, hip_error, host,
                         rng, run_captured, run_default, run_side, same_bits)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U8, I32 = np.float32, np.uint8, np.int32
CHUNK = 1024                          # records per workgroup of the record kernels (NAV_GOAL_ELEMS)


def ops():
    from twoarmy_amd import ppo_ops
    return ppo_ops


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def M():
    from twoarmy_amd import _marshal
    return _marshal


def pick(d, *keys):
    return {k: d[k] for k in keys}


def unchanged(x, y, keys):
    """The names among `keys` whose arrays are equal in the results x and y: what a case's `also` expects to be empty."""
    return [k for k in keys if np.array_equal(x[k], y[k])]


def probs(r, B, A):
    p = r.random((B, A)).astype(np.float64) + 0.05
    return (p / p.sum(1, keepdims=True)).astype(F32)


# ------------------------------------------------------------------------------------------------ rollouts and worlds
@functools.lru_cache(maxsize=None)
def rollout_np(seed, T, N, W, H):
    """A valid synthetic rollout: positions inside the grid, sparse flags, the engine's reward values, policy actions."""
    r = rng(seed, 1)

    def pos():
        yx = np.stack([r.integers(0, H, (T, N)), r.integers(0, W, (T, N))], -1)
        return (yx + r.choice([0.0, 0.25, 0.5], (T, N, 2))).astype(F32)
    return dict(pos_b=pos(), pos_a=pos(), term=(r.random((T, N)) < 0.15).astype(U8), trunc=(r.random((T, N)) < 0.1).astype(U8),
                reward=r.choice(np.array(episode_ref.REWARD_VALUES, F32), (T, N)).astype(F32),
                action=r.integers(0, 5, (T, N)).astype(I32), dirs=r.integers(0, 4, (T, N)).astype(I32),
                age=r.integers(0, 10, (T, N)).astype(I32), init_pos=np.array([1.0, 1.0], F32),
                keep=(r.random((T, N)) < 0.2).astype(U8))


@functools.lru_cache(maxsize=None)
def world_np(seed, N, W, H):
    """N valid worlds: empty cells, walls, one goal; colours of the palette; an agent inside the grid."""
    r = rng(seed, 2)
    ty = np.where(r.random((N, W * H)) < 0.2, 2, 1).astype(U8)
    ty[np.arange(N), r.integers(0, W * H, N)] = 8
    co = np.where(ty == 1, 0, r.integers(0, 6, (N, W * H))).astype(U8)
    return dict(ty=ty, co=co, st=np.zeros((N, W * H), U8), ax=r.integers(0, W, N).astype(I32),
                ay=r.integers(0, H, N).astype(I32), ad=r.integers(0, 4, N).astype(I32))


def up(d):
    return {k: dev(v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------- PPO math
CASES = []
T, N = 3, 65


def _gae_make(seed):
    r = rng(seed)
    return up(dict(reward=r.standard_normal((T, N)).astype(F32), value=r.standard_normal((T, N)).astype(F32),
                   next_value=r.standard_normal((T, N)).astype(F32), done=(r.random((T, N)) < 0.2).astype(U8)))


def _gae_call(b, o, ctx):
    adv, target, ret = ops().gae(b["reward"], b["value"], b["next_value"], b["done"], gamma=0.99, lam=0.95, use_done_mask=True)
    return dict(adv=adv, target=target, ret=ret)


def _gae_ref(h):
    import ppo_oracle as po
    return dict(zip(("adv", "target", "ret"), po.gae(h["reward"], h["value"], h["next_value"], h["done"], 0.99, 0.95, True)))


GAE = Case("gae", "ppo", ["ppo_gae"], _gae_make, _gae_call, ref=_gae_ref,
           tol={k: (1e-5, 1e-5) for k in ("adv", "target", "ret")})      # test_ppo_gpu's tolerance of the lam > 0 scan
CASES.append(GAE)


def _adv_ref(h):
    import ppo_oracle as po
    return dict(adv=po.adv_norm(h["adv"]))


ADV_NORM = Case("adv_norm_", "ppo", ["ppo_adv_norm"], lambda seed: up(dict(adv=rng(seed).standard_normal((257, 3)).astype(F32))),
                lambda b, o, ctx: dict(adv=ops().adv_norm_(b["adv"])), ref=_adv_ref, tol=dict(adv=(1e-5, 1e-6)))
CASES.append(ADV_NORM)


def _sample_make(seed):
    r = rng(seed)
    return up(dict(probs=probs(r, N, 5), uniforms=r.random(N).astype(F32), offset=np.array([r.integers(0, 1000)], np.int64)))


def _sample_raw(b, o, ctx):
    m = M()
    m.call("ppo_sample", b["probs"], m.ptr(b["probs"]), N, 5, m.ptr(b["uniforms"]), 7, 3, m.ptr(o["action"]), m.ptr(o["logp"]))
    return dict(o)


CASES.append(Case("sample(offset_dev)", "ppo", ["ppo_sample_dev"], _sample_make,
                  lambda b, o, ctx: dict(zip(("action", "logp"), ops().sample(b["probs"], b["uniforms"], seed=7, offset=3,
                                                                              offset_dev=b["offset"]))),
                  note="default-stream run only"))
CASES.append(Case("ppo_sample (C ABI)", "ppo", ["ppo_sample"], _sample_make, _sample_raw,
                  outs=lambda: dict(action=torch.empty(N, dtype=torch.int32, device=DEV), logp=torch.empty(N, device=DEV)),
                  note="default-stream run only; no front end"))

B2 = 257                              # two workgroups of the two-stage reductions


def _loss_make(seed):
    r = rng(seed)
    return up(dict(probs=probs(r, B2, 5), value=r.standard_normal(B2).astype(F32), action=r.integers(0, 5, B2).astype(I32),
                   old_logp=np.log(probs(r, B2, 5)[:, 0]).astype(F32), adv=r.standard_normal(B2).astype(F32),
                   target_v=r.standard_normal(B2).astype(F32), moves=r.integers(0, 32, B2).astype(U8)))


def _losses_call(b, o, ctx):
    p, v = b["probs"].detach().requires_grad_(), b["value"].detach().requires_grad_()
    al, vl = ops().ppo_losses(p, v, b["action"], b["old_logp"], b["adv"], b["target_v"], n_valid=250)
    return dict(action_loss=al.detach(), value_loss=vl.detach(), grad_probs=al.grad_fn.saved_tensors[0],
                grad_value=vl.grad_fn.saved_tensors[0])


def _losses_raw(b, o, ctx):
    m = M()
    m.call("ppo_loss_fwd_bwd", b["probs"], m.ptr(b["probs"]), m.ptr(b["action"]), m.ptr(b["old_logp"]), m.ptr(b["adv"]),
           m.ptr(b["value"]), m.ptr(b["target_v"]), B2, 5, 0.1, 0.01, m.ptr(o["losses"]), m.ptr(o["grad_probs"]),
           m.ptr(o["grad_value"]), m.ptr(o["workspace"]))
    return pick(o, "losses", "grad_probs", "grad_value")


def _prior_call(b, o, ctx):
    p = b["probs"].detach().requires_grad_()
    loss, (out, counts) = ops().prior_loss(p, b["moves"], 0.5, n_valid=250)
    return dict(loss=loss.detach(), out=out, counts=counts, grad_probs=loss.grad_fn.saved_tensors[0])


def _losses_ref(h):
    import ppo_oracle as po
    v = slice(0, 250)                                       # n_valid = 250: the means run over the real rows
    al, vl = po.losses(h["probs"][v], h["action"][v], h["old_logp"][v], h["adv"][v], h["value"][v], h["target_v"][v])
    return dict(action_loss=np.float32(al), value_loss=np.float32(vl), _atol=dict(action_loss=1e-5, value_loss=1e-5))


CASES.append(Case("ppo_losses", "ppo", ["ppo_loss_fwd_bwd_masked"], _loss_make, _losses_call, ref=_losses_ref))  # test_ppo_gpu's 1e-5
CASES.append(Case("ppo_loss_fwd_bwd (C ABI)", "ppo", ["ppo_loss_fwd_bwd"], _loss_make, _losses_raw,
                  outs=lambda: dict(losses=torch.empty(2, device=DEV), grad_probs=torch.empty((B2, 5), device=DEV),
                                    grad_value=torch.empty(B2, device=DEV), workspace=torch.empty(4, device=DEV)),
                  note="default-stream run only; no front end"))
CASES.append(Case("prior_loss", "ppo", ["ppo_prior_loss_fwd_bwd"], _loss_make, _prior_call, note="default-stream run only"))


def _lstm_make(seed):
    r = rng(seed)
    return up(dict(gates=r.standard_normal((3, 32)).astype(F32), xin=r.standard_normal((3, 2, 32)).astype(F32),
                   bias=r.standard_normal(32).astype(F32), c=r.standard_normal((3, 8)).astype(F32)))


CASES.append(Case("lstm_cell_", "ppo", ["ppo_lstm_cell"], _lstm_make,
                  lambda b, o, ctx: dict(h=ops().lstm_cell_(b["gates"], b["c"], gates_b=b["xin"][:, 1], bias=b["bias"]), c=b["c"]),
                  note="default-stream run only"))


def _epi_make(seed):
    r = rng(seed)
    cl = torch.channels_last
    return dict(x=dev(r.standard_normal((2, 4, 12, 12)).astype(F32)).contiguous(memory_format=cl),
                w=dev((r.standard_normal((8, 4, 3, 3)) * 0.2).astype(F32)).contiguous(memory_format=cl),
                bias=dev(r.standard_normal(8).astype(F32)),
                gy=dev(r.standard_normal((2, 8, 10, 10)).astype(F32)).contiguous(memory_format=cl))


def _epi_call(b, o, ctx):
    w, bias = b["w"].detach().requires_grad_(), b["bias"].detach().requires_grad_()
    y = ops().conv_bias_relu(b["x"], w, bias, (1, 1))
    _, gb = torch.autograd.grad(y, (w, bias), b["gy"])    # the weight gradient is MIOpen's, and not the same bits run to run
    return dict(y=y.detach(), gb=gb)


def _relu_bwd_raw(b, o, ctx):
    m, cl = M(), torch.channels_last
    m.call("ppo_relu_bwd_bias_grad_nhwc", b["gy"], m.ptr(b["gy"], None, cl), m.ptr(b["y"], None, cl), m.ptr(o["gx"], None, cl),
           m.ptr(o["partial"]), 200, 8)
    return dict(o)


def _relu_bwd_outs():
    blocks = M().query("ppo_relu_bwd_bias_grad_nhwc_blocks", 200, 8)
    return dict(gx=torch.empty((2, 8, 10, 10), device=DEV).contiguous(memory_format=torch.channels_last),
                partial=torch.empty((blocks, 8), device=DEV))


CASES.append(Case("conv_bias_relu fwd+bwd", "ppo", ["ppo_bias_relu_nhwc", "ppo_relu_bwd_bias_grad_nhwc"], _epi_make, _epi_call,
                  note="default-stream run only"))
CASES.append(Case("relu_bwd_bias_grad (C ABI)", "ppo", ["ppo_relu_bwd_bias_grad_nhwc"],
                  lambda seed: dict(gy=_epi_make(seed)["gy"], y=_epi_make(seed + 10)["gy"].relu()), _relu_bwd_raw, outs=_relu_bwd_outs,
                  note="default-stream run only; through the C ABI, so that the masked gradient itself is compared, which the "
                       "front end hands to MIOpen"))


def _conv1_make(F):
    def make(seed):
        r = rng(seed, F)
        return dict(frames=dev(r.standard_normal((2, F, 289)).astype(F32)), w=dev((r.standard_normal((64, F, 4, 4)) * 0.1).astype(F32)),
                    bias=dev(r.standard_normal(64).astype(F32)),
                    gy=dev(r.standard_normal((2, 64, 33, 33)).astype(F32)).contiguous(memory_format=torch.channels_last))
    return make


def _conv1_call(b, o, ctx):
    w, bias = b["w"].detach().requires_grad_(), b["bias"].detach().requires_grad_()
    y = ops().conv1_up4_bias_relu(b["frames"], w, bias)
    gw, gb = torch.autograd.grad(y, (w, bias), b["gy"])
    return dict(y=y.detach(), gw=gw, gb=gb)


for _F in (4, 8):
    CASES.append(Case("conv1_up4_bias_relu fwd+bwd F=%d" % _F, "ppo", ["ppo_conv1_up4_bias_relu", "ppo_conv1_up4_bwd"],
                      _conv1_make(_F), _conv1_call, note="default-stream run only"))
CASES.append(Case("conv1_up4_bias_relu_infer", "ppo", ["ppo_conv1_up4_bias_relu_c"], _conv1_make(4),
                  lambda b, o, ctx: dict(y=ops().conv1_up4_bias_relu_infer(b["frames"], b["w"], b["bias"])),
                  note="default-stream run only"))

B_STATS, NV_STATS = 600, 257


def _stats_case():
    """stream_util's protocol on the front end: every seed draws its own minibatch (seed 0 is the decoy); `stats` is state
    the call updates in place, carried across the warm-up and the replays."""
    def make(seed):
        p, a, old, adv, value, target = ur.inputs(B_STATS, 8100 + seed)
        return dict(up(dict(probs=p, action=a, old_logp=old, adv=adv, value=value, target_v=target)),
                    stats=torch.zeros(16, dtype=torch.float64, device=DEV))

    def call(b, o, ctx):
        p, v = b["probs"].detach().requires_grad_(), b["value"].detach().requires_grad_()
        al, vl = ops().ppo_losses(p, v, b["action"], b["old_logp"], b["adv"], b["target_v"], clip=ur.CLIP, ent_coef=ur.ENT,
                                  n_valid=NV_STATS, stats=b["stats"])
        return dict(action_loss=al.detach(), value_loss=vl.detach(), grad_probs=al.grad_fn.saved_tensors[0],
                    grad_value=vl.grad_fn.saved_tensors[0], stats=b["stats"])

    def ref(h):
        x = (h["probs"], h["action"], h["old_logp"], h["adv"], h["value"], h["target_v"])
        want, R = ur.accumulate(h["stats"], x[0], x[1], x[2], x[4], x[5], ur.CLIP, NV_STATS)
        return dict(stats=want, _atol=dict(stats=ur._bounds(x, R, NV_STATS)))

    def also(part, x, y):
        if part == "A":                                        # the decoy has another answer everywhere
            assert not unchanged(x, y, x) and x["stats"][12] == 1
            return
        # the row is carried: the eager warm-up is call 1, so the two replays added exactly two calls and two batches of rows
        assert [x["stats"][12], y["stats"][12]] == [2, 3] and [x["stats"][0], y["stats"][0]] == [2 * NV_STATS, 3 * NV_STATS]
        assert not unchanged(x, y, ["grad_probs"])

    return Case("ppo_losses(stats=)", "ppo", ["ppo_loss_fwd_bwd_stats"], make, call, ref=ref, state=("stats",), also=also)


H_RUNS = 5000                                                      # three workgroups: reduce, carry pass, apply


def _arrays_differ(part, x, y):
    """Both parts: every output with more than one element differs, from the decoy's and between the replays."""
    assert not unchanged(x, y, [k for k in x if x[k].size > 1])


def _runs_case():
    def make(seed):
        t, n, goal, done = gr._records(H_RUNS, 50 + seed)
        return dict(up(dict(t=t, n=n, goal=goal, done=done)), broken=torch.zeros(1, dtype=torch.int32, device=DEV))

    def call(b, o, ctx):
        return dict(run_end=ops().run_ends(b["t"], b["n"], b["goal"], b["done"], b["broken"]), broken=b["broken"])

    def ref(h):
        end, broken = gr.run_ends(h["t"], h["n"], h["goal"], h["done"])
        return dict(run_end=end, broken=h["broken"] + np.int32(broken))

    return Case("run_ends", "ppo", ["ppo_run_ends"], make, call, ref=ref, state=("broken",), also=_arrays_differ)


def _gae_runs_case():
    def make(seed):
        r, v, nv = gr.inputs(H_RUNS, 60 + seed)
        end = gr.pattern("her", H_RUNS, 60 + seed)
        return up(dict(reward=r, value=v, next_value=nv, done=gr.dones(end, seed), run_end=end))

    def call(b, o, ctx):
        adv, target, ret = ops().gae_runs(b["reward"], b["value"], b["next_value"], b["done"], b["run_end"], 0.99, 0.95, True)
        return dict(adv=adv, target=target, ret=ret)

    def ref(h):
        a64, _, r64, S, L = gr.gae_runs64(h["reward"], h["value"], h["next_value"], h["done"], h["run_end"], 0.99, 0.95, True)
        bound = gr._k(L, H_RUNS) * gr.EPS32 * S
        return dict(adv=a64, ret=r64, target=gr.one_step32(h["reward"], h["value"], h["next_value"], h["done"], 0.99, True)[0],
                    _atol=dict(adv=bound, ret=bound + gr.EPS32 * (S + np.abs(h["value"]))))

    return Case("gae_runs", "ppo", ["ppo_gae_runs"], make, call, ref=ref, also=_arrays_differ)


CASES += [_stats_case(), _runs_case(), _gae_runs_case()]

# --------------------------------------------------------------------------------------------------------- replay


def _dec_make(seed):
    w = replay_ref.decoder_weights(seed)
    return dict({k: v.to(DEV) for k, v in w.items()}, z=replay_ref.decoder_latents(seed, 3, 1.0).to(DEV))


CASES.append(Case("decoder_frames", "replay", ["ppo_decoder_frames"], _dec_make,
                  lambda b, o, ctx: dict(frames=ops().decoder_frames(b["z"], *(b[k] for k in ("w1", "b1", "w2", "b2", "w3", "b3")))),
                  note="default-stream run only"))
K_, B_ = 7, 5


def _gather_make(u8):
    def make(seed):
        r = rng(seed, int(u8))
        fr = r.integers(0, 4, (K_, N, 304)).astype(U8) if u8 else r.random((K_, N, 292)).astype(F32)
        return up(dict(buf=fr, posf=r.random((K_, N, 2)).astype(F32), k_idx=r.integers(3, K_, B_).astype(I32),
                       n_idx=r.integers(0, N, B_).astype(I32), age=r.integers(0, 6, B_).astype(I32),
                       init_f=r.random(289).astype(F32), init_p=np.array([15.0, 3.0], F32)))
    return make


def _gather_call(b, o, ctx):
    out, pos = ops().gather_stack(b["buf"][..., :289], b["posf"], b["k_idx"], b["n_idx"], b["age"], b["init_f"], b["init_p"])
    return dict(out=out, pos=pos)


def _gather_ref(h):
    import ppo_oracle as po
    return dict(zip(("out", "pos"), po.gather_stack(h["buf"][..., :289], h["posf"], h["k_idx"], h["n_idx"], h["age"],
                                                    h["init_f"], h["init_p"])))


CASES.append(Case("gather_stack f32", "replay", ["ppo_gather_stack"], _gather_make(False), _gather_call, ref=_gather_ref))
CASES.append(Case("gather_stack u8", "replay", ["ppo_gather_stack_u8"], _gather_make(True), _gather_call,
                  note="default-stream run only"))

HER_T, HER_G = 5, 4
HER_ROOM = 2 * HER_T * HER_G          # output slots per env: more than an env can emit, so no input can overrun them


def _her_make(seed):
    d = rollout_np(seed, HER_T, N, 17, 17)
    return up(dict(pos=d["pos_a"], term=d["term"], trunc=d["trunc"], age0=d["age"][0], reward=d["reward"],
                   offsets=HER_ROOM * np.arange(N, dtype=np.int64)))


def _her_outs():
    H = N * HER_ROOM
    return dict(counts=torch.empty(N, dtype=torch.int32, device=DEV), t=torch.empty(H, dtype=torch.int32, device=DEV),
                n=torch.empty(H, dtype=torch.int32, device=DEV), goal=torch.empty((H, 2), device=DEV),
                reward=torch.empty(H, device=DEV), done=torch.empty(H, dtype=torch.uint8, device=DEV))


def _her_call(fn, emit):
    def call(b, o, ctx):
        m = M()
        skip = [0] if fn == "ppo_her_relabel_window" else []
        outs = [m.ptr(o[k]) if emit else None for k in ("t", "n", "goal", "reward", "done")]
        offsets = b["offsets"] if emit else None
        m.call(fn, b["pos"], m.ptr(b["pos"]), m.ptr(b["term"]), m.ptr(b["trunc"]), m.ptr(b["age0"]), m.ptr(b["reward"]), None,
               11, 0, 0, HER_T, N, HER_G, *skip, m.ptr(offsets), m.ptr(o["counts"]), *outs)
        return dict(o) if emit else dict(counts=o["counts"])
    return call


_HER_NOTE = ("default-stream run only; through the C ABI: her_relabel reads the record count back between its two "
             "launches, so each launch is a case of its own with room for every record an env can emit")
CASES.append(Case("her_relabel count pass", "replay", ["ppo_her_relabel"], _her_make, _her_call("ppo_her_relabel", False),
                  outs=_her_outs, note=_HER_NOTE))
CASES.append(Case("her_relabel emit pass", "replay", ["ppo_her_relabel"], _her_make, _her_call("ppo_her_relabel", True),
                  outs=_her_outs, note=_HER_NOTE))
CASES.append(Case("her_relabel_window count pass", "replay", ["ppo_her_relabel_window"], _her_make,
                  _her_call("ppo_her_relabel_window", False), outs=_her_outs, note=_HER_NOTE))
CASES.append(Case("her_relabel_window emit pass", "replay", ["ppo_her_relabel_window"], _her_make,
                  _her_call("ppo_her_relabel_window", True), outs=_her_outs, note=_HER_NOTE))

# ---------------------------------------------------------------------------------------------------------- scans


def _roll_make(*keys, T=T, extra=None):
    def make(seed):
        b = up(pick(rollout_np(seed, T, N, 17, 17), *keys))
        b.update(extra(seed) if extra else {})
        return b
    return make


def _age_ref(h):
    age = np.zeros((T + 1, N), I32)
    age[0] = h["age0"]
    for t in range(T):
        age[t + 1] = np.where((h["term"][t] | h["trunc"][t]) != 0, 0, age[t] + 1)
    return dict(age=age)


CASES.append(Case("age_scan", "scans", ["ppo_age_scan"],
                  _roll_make("term", "trunc", extra=lambda seed: dict(age0=dev(rng(seed).integers(0, 9, N).astype(I32)))),
                  lambda b, o, ctx: dict(age=ops().age_scan(b["term"], b["trunc"], b["age0"])), ref=_age_ref))


def _epscan_call(b, o, ctx):
    ops().episode_scan(b["reward"], b["term"], b["trunc"], b["carry_return"], b["carry_length"], out=(o["ep_return"], o["ep_length"]))
    return dict(o, carry_return=b["carry_return"], carry_length=b["carry_length"])


def _epscan_ref(h):
    return dict(zip(("ep_return", "ep_length", "carry_return", "carry_length"),
                    episode_ref.episode_scan(h["reward"], h["term"], h["trunc"], h["carry_return"], h["carry_length"])))


CASES.append(Case("episode_scan", "scans", ["ppo_episode_scan"],
                  _roll_make("reward", "term", "trunc", extra=lambda seed: dict(
                      carry_return=dev(rng(seed).choice([0.0, -0.01, 0.89], N)), carry_length=dev(rng(seed).integers(0, 9, N).astype(I32)))),
                  _epscan_call, outs=lambda: dict(ep_return=torch.empty((T, N), dtype=torch.float64, device=DEV),
                                                  ep_length=torch.empty((T, N), dtype=torch.int32, device=DEV)),
                  ref=_epscan_ref, state=("carry_return", "carry_length")))
TS = 5                                # the two summaries: T = 5, N = 65


def _summary_make(seed):
    d = rollout_np(seed, TS, N, 17, 17)
    er, el, _, _ = episode_ref.episode_scan(d["reward"], d["term"], d["trunc"], np.zeros(N), np.zeros(N, I32))
    return up(dict(pick(d, "term", "trunc", "reward", "action"), ep_return=er, ep_length=el, score=np.array([0.25 * seed])))


def _summary_call(b, o, ctx):
    ops().episode_summary(b["ep_return"], b["ep_length"], b["term"], b["trunc"], b["reward"], action=b["action"], score=b["score"],
                          summary=o["summary"], action_hist=o["action_hist"], reward_hist=o["reward_hist"], workspace=o["workspace"])
    return dict(pick(o, "summary", "action_hist", "reward_hist"), score=b["score"])


def _summary_outs():
    return dict(summary=torch.empty(8, dtype=torch.float64, device=DEV), action_hist=torch.empty(5, dtype=torch.int64, device=DEV),
                reward_hist=torch.empty(6, dtype=torch.int64, device=DEV),
                workspace=torch.empty(ops().episode_summary_workspace(TS, N), dtype=torch.float64, device=DEV))


def _summary_ref(h):
    w = episode_ref.episode_summary(h["ep_return"], h["ep_length"], h["term"], h["trunc"], h["reward"], action=h["action"],
                                    score=float(h["score"][0]))
    summary = np.array([w["episodes"], w["successes"], w["truncated"], w["return_sum"], w["min_return"], w["max_return"],
                        w["length_sum"], w["max_length"]], np.float64)
    bound = np.zeros(8)
    bound[3] = w["episodes"] * 2.0 ** -53 * w["abs_return_sum"]          # test_episode_stats_gpu's bounds, and its SCORE_TOL
    return dict(summary=summary, score=np.array([w["score"]]), action_hist=np.array(w["action_hist"]),
                reward_hist=np.array(w["reward_hist"]), _atol=dict(summary=bound, score=1e-12))


CASES.append(Case("episode_summary", "scans", ["ppo_episode_summary"], _summary_make, _summary_call, outs=_summary_outs,
                  state=("score",), ref=_summary_ref))


def _vscan_call(b, o, ctx):
    first, cells = ops().visit_scan(b["pos_a"], b["term"], b["trunc"], b["carry"])
    return dict(first=first, cells=cells, carry=b["carry"])


def _vscan_ref(h):
    first, cells, seen = visit_ref.visit_scan(h["pos_a"], h["term"], h["trunc"], 17, 17, visit_ref.carry_to_sets(h["carry"], N, 17, 17))
    return dict(first=first, cells=cells, carry=visit_ref.sets_to_carry(seen, 17, 17).view(I32))


def _vscan_carry(seed):
    r = rng(seed, 3)
    seen = [set(r.integers(0, 289, 4).tolist()) for _ in range(N)]
    return dict(carry=dev(visit_ref.sets_to_carry(seen, 17, 17).view(I32)))


CASES.append(Case("visit_scan", "scans", ["ppo_visit_scan"], _roll_make("pos_a", "term", "trunc", extra=_vscan_carry), _vscan_call,
                  ref=_vscan_ref, state=("carry",)))
CASES.append(Case("visit_hist", "scans", ["ppo_visit_hist"],
                  _roll_make("pos_a", "keep", extra=lambda seed: dict(counts=dev(rng(seed).integers(0, 50, 290)))),
                  lambda b, o, ctx: dict(counts=ops().visit_hist(b["pos_a"], b["counts"], mask=b["keep"])),
                  ref=lambda h: dict(counts=visit_ref.visit_hist(h["pos_a"], 17, 17, mask=h["keep"], counts=h["counts"])),
                  state=("counts",)))

# -------------------------------------------------------------------------------------------------------- bonuses
NA = 7


def _bonus_case(scope):
    def make(seed):
        b = up(pick(rollout_np(seed, T, N, 17, 17), "pos_a", "action", "reward", "keep", "dirs"))
        for k in ("state", "action"):
            b["table_" + k] = torch.zeros(ops().bonus_table_words(k, scope, 17, 17, NA, N), dtype=torch.int32, device=DEV)
        return b

    def outs():
        o = {k: torch.empty((T, N), device=DEV) for k in ("bonus_state", "bonus_action", "reward_out")}
        if scope == "shared":
            o["workspace"] = torch.empty(max(1, ops().bonus_workspace_bytes(3, scope, T, 17, 17, NA) // 4), dtype=torch.int32, device=DEV)
        return o

    def call(b, o, ctx):
        ops().bonus_scan(b["pos_a"], b["action"], b["reward"], b["table_state"], b["table_action"], scope=scope, scale=0.5,
                         n_actions=NA, keep=b["keep"], dir=b["dirs"], bonus_state=o["bonus_state"], bonus_action=o["bonus_action"],
                         reward_out=o["reward_out"], workspace=o.get("workspace"))
        return dict(pick(o, "bonus_state", "bonus_action", "reward_out"), table_state=b["table_state"], table_action=b["table_action"])

    def ref(h):
        r = bonus_ref.BonusRef(N, ("state", "action"), scope, 0.5, 17, 17, NA)
        for k in ("state", "action"):                       # the device layouts, as test_bonus_gpu.Run.tables reads them
            t = h["table_" + k]
            r.tables[k] = (t.astype(np.int64) & 0xFFFFFFFF).reshape(N, -1) if scope == "env" else t.view(np.int64).reshape(1, -1).copy()
        w = r.scan(h["pos_a"], h["action"], h["reward"], keep=h["keep"], dirs=h["dirs"])
        tabs = {k: (r.tables[k].astype(I32).reshape(-1) if scope == "env" else r.tables[k].reshape(-1).view(I32)) for k in r.tables}
        return dict(bonus_state=w["state"], bonus_action=w["action"], reward_out=w["reward"], table_state=tabs["state"],
                    table_action=tabs["action"])
    return Case("bonus_scan scope=%s" % scope, "bonuses", ["ppo_bonus_scan"], make, call, outs=outs, ref=ref,
                state=("table_state", "table_action"))


BT, BN = 40, 70                      # the episodic scan: column 1 of episode_walk ends an episode at every step


def _episode_tables(words):
    """Stamped words -> what they mean: the running episodes' counts, then the generations."""
    counts, gen, _ = bonus_episode_ref.decode(words, BN)
    return np.concatenate([counts.reshape(-1), gen])


def _bonus_episode_case():
    def make(seed):
        pos, action, dirs, reward, term, trunc = episode_walk(BT, BN, 50 + seed)
        b = up(dict(pos=pos, action=action.astype(I32), dirs=dirs.astype(I32), reward=reward, term=term, trunc=trunc,
                    keep=(rng(seed).random((BT, BN)) < 0.3).astype(U8)))
        for k in ("state", "action"):
            b["table_" + k] = torch.zeros(ops().bonus_episode_words(k, N=BN), dtype=torch.int32, device=DEV)
        return b

    def call(b, o, ctx):
        ops().bonus_scan_episode(b["pos"], b["action"], b["reward"], b["term"], b["trunc"], b["table_state"], b["table_action"],
                                 scale=0.5, keep=b["keep"], dir=b["dirs"], bonus_state=o["bonus_state"],
                                 bonus_action=o["bonus_action"], reward_out=o["reward_out"])
        return dict(o, table_state=b["table_state"], table_action=b["table_action"])

    def ref(h):
        r = bonus_episode_ref.EpisodeBonusRef(BN, ("state", "action"), 0.5)
        for k in r.kinds:
            counts, gen, _ = bonus_episode_ref.decode(h["table_" + k], BN)
            r.preset(k, counts, gen)
        w = r.scan(h["pos"], h["action"], h["reward"], h["term"], h["trunc"], keep=h["keep"], dirs=h["dirs"])
        tabs = {k: np.concatenate([r.table(k).reshape(-1), r.gen[k]]) for k in r.kinds}
        return dict(bonus_state=w["state"], bonus_action=w["action"], reward_out=w["reward"], table_state=tabs["state"],
                    table_action=tabs["action"])

    def also(part, x, y):
        if part == "A":                                        # the decoy has another answer everywhere
            assert not unchanged(x, y, x)
            return
        for k in ("table_state", "table_action"):              # the tables are carried: 40 more episode ends per call
            gens = [bonus_episode_ref.decode(r[k], BN)[1] for r in (x, y)]
            assert [g[1] for g in gens] == [2 * BT, 3 * BT] and not gens[1][0]

    return Case("bonus_scan_episode", "bonuses", ["ppo_bonus_scan_episode"], make, call, ref=ref, also=also,
                outs=lambda: {k: torch.empty((BT, BN), device=DEV) for k in ("bonus_state", "bonus_action", "reward_out")},
                state=("table_state", "table_action"),
                read=lambda k, a: _episode_tables(a) if k.startswith("table_") else a)


BONUS_EPISODE = _bonus_episode_case()
CASES += [_bonus_case("env"), _bonus_case("shared"), BONUS_EPISODE]

# ----------------------------------------------------------------------------------------------------- navigation
R_ = CHUNK + 1


def nav_set(seed, Nn, W, H, P, Tn=T):
    """Everything a shortest-path case may take for one seed: planes, agent, schedule, a rollout, records, and the fields
    of these worlds (made by the library on the default stream before the protocol starts)."""
    r = rng(seed, 4)
    w, d = world_np(seed, Nn, W, H), rollout_np(seed, Tn, Nn, W, H)
    b = up(dict(w, **d))
    b["blocked"] = dev(((r.random((P, H, W)) < 0.15) * (1 << np.arange(W))).sum(-1).astype(I32))
    b["clock"] = dev(r.integers(0, 20, Nn).astype(I32))
    b["rt"], b["rn"] = dev(r.integers(0, Tn, R_).astype(I32)), dev(r.integers(0, Nn, R_).astype(I32))
    b["rgoal"] = dev(np.stack([r.integers(0, H, R_), r.integers(0, W, R_)], -1).astype(F32) + np.float32(0.25))
    b["rreward"], b["rdone"] = dev(r.standard_normal(R_).astype(F32)), dev((r.random(R_) < 0.2).astype(U8))
    b["done"] = b["term"] | b["trunc"]
    b["dist"] = nav().distance_field(b["ty"], b["st"], W, H, want_error=False)[0]
    b["tdist"] = nav().timed_field(b["ty"], b["st"], W, H, b["blocked"], want_error=False)[0]
    return b


def _nav_case(name, fns, keys, call, Nn=N, W=17, H=17, P=6, Tn=T, ref=None, state=(), extra=None, outs=None, note=None):
    def make(seed):
        b = pick(nav_set(seed, Nn, W, H, P, Tn), *keys)
        b.update(extra(seed, b) if extra else {})
        return b
    CASES.append(Case("%s %dx%d N=%d P=%d" % (name, W, H, Nn, P), "navigation", fns, make,
                      lambda b, o, ctx: call(b, o, W, H), ref=(lambda h: ref(h, W, H)) if ref else None, state=state, outs=outs,
                      note=note))


def _named(names, vals):
    return {k: v for k, v in zip(names, vals) if v is not None}


def _field_ref(h, W, H):
    return _named(("dist", "agent_dist", "agent_action", "error"),
                  nav_ref.fields(h["ty"], h["st"], W, H, agent=(h["ax"], h["ay"]))[:4])


REC = ("ty", "st", "rt", "rn", "rgoal", "pos_b", "age", "init_pos")
for _N, _W, _H in ((3, 5, 9), (N, 17, 17)):
    _nav_case("distance_field", ["mg_nav_field"], ("ty", "st", "ax", "ay"), Nn=_N, W=_W, H=_H, P=1, ref=_field_ref,
              call=lambda b, o, W, H: _named(("dist", "agent_dist", "agent_action", "error"),
                                             nav().distance_field(b["ty"], b["st"], W, H, agent=(b["ax"], b["ay"]))))
    for _P in (1, 6):
        _nav_case("timed_field", ["mg_nav_timed_field"], ("ty", "st", "ax", "ay", "blocked", "clock"), Nn=_N, W=_W, H=_H, P=_P,
                  note="default-stream run only",
                  call=lambda b, o, W, H: _named(("dist", "agent_dist", "agent_action", "error"),
                                                 nav().timed_field(b["ty"], b["st"], W, H, b["blocked"], agent=(b["ax"], b["ay"]),
                                                                   clock=b["clock"])))
_only = dict(note="default-stream run only")
_nav_case("lookup", ["mg_nav_lookup"], ("dist", "pos_a"), P=1, **_only,
          call=lambda b, o, W, H: dict(d=nav().lookup(b["dist"], b["pos_a"], W, H)))
_nav_case("optimal_moves", ["mg_nav_optimal_moves"], ("dist", "pos_b", "age", "init_pos"), P=1, **_only,
          call=lambda b, o, W, H: _named(("moves", "dist"), nav().optimal_moves(b["dist"], b["pos_b"], W, H, b["age"], b["init_pos"])))
_nav_case("timed_moves", ["mg_nav_timed_moves"], ("tdist", "pos_b", "age", "init_pos"), **_only,
          call=lambda b, o, W, H: _named(("moves", "dist"), nav().timed_moves(b["tdist"], b["pos_b"], W, H, b["age"], b["init_pos"])))
_nav_case("goal_moves", ["mg_nav_goal_moves"], REC, P=1, **_only,
          call=lambda b, o, W, H: _named(("moves", "dist"), nav().goal_moves(b["ty"], b["rt"], b["rn"], b["rgoal"], b["pos_b"], W, H,
                                                                             age=b["age"], init_pos=b["init_pos"], state=b["st"])))
_nav_case("goal_ahead", ["mg_nav_goal_ahead"], REC, P=1, **_only,
          call=lambda b, o, W, H: _named(("labels", "dist"), nav().goal_ahead(b["ty"], b["rt"], b["rn"], b["rgoal"], b["pos_b"], W, H,
                                                                              age=b["age"], init_pos=b["init_pos"], state=b["st"])))
_nav_case("goal_shape", ["mg_nav_goal_shape"], REC + ("pos_a", "rreward", "rdone"), P=1, **_only,
          call=lambda b, o, W, H: _named(("out", "f", "mask"), nav().goal_shape(
              b["ty"], b["rt"], b["rn"], b["rgoal"], b["pos_b"], b["pos_a"], W, H, reward=b["rreward"], done=b["rdone"], age=b["age"],
              init_pos=b["init_pos"], state=b["st"], zero_terminal=True)))
for _P in (1, 6):
    _nav_case("timed_goal_moves", ["mg_nav_timed_goal_moves"], REC + ("blocked",), P=_P, **_only,
              call=lambda b, o, W, H: _named(("moves", "dist"), nav().timed_goal_moves(
                  b["ty"], b["rt"], b["rn"], b["rgoal"], b["pos_b"], W, H, b["blocked"], b["age"], b["init_pos"], state=b["st"])))
    _nav_case("timed_goal_shape", ["mg_nav_timed_goal_shape"], REC + ("blocked", "pos_a", "rreward", "rdone"), P=_P, **_only,
              call=lambda b, o, W, H: _named(("out", "f", "mask"), nav().timed_goal_shape(
                  b["ty"], b["rt"], b["rn"], b["rgoal"], b["pos_b"], b["pos_a"], W, H, b["blocked"], b["age"], b["init_pos"],
                  reward=b["rreward"], done=b["rdone"], state=b["st"], zero_terminal=True)))
    _f = "dist" if _P == 1 else "tdist"
    _nav_case("shape", ["mg_nav_shape"], (_f, "pos_b", "pos_a", "reward", "age", "init_pos", "done"), P=_P, **_only,
              call=lambda b, o, W, H, f=_f: _named(("out", "f", "mask"), nav().shape(
                  b[f], b["pos_b"], b["pos_a"], W, H, reward=b["reward"], age=b["age"], init_pos=b["init_pos"], done=b["done"],
                  zero_terminal=True)))
    _nav_case("ahead", ["mg_nav_ahead"], (_f, "pos_b", "age", "init_pos"), P=_P, **_only,
              call=lambda b, o, W, H, f=_f: _named(("labels", "dist"), nav().ahead(b[f], b["pos_b"], W, H, age=b["age"],
                                                                                   init_pos=b["init_pos"])))

    def _pscan_call(b, o, W, H, f=_f):
        carry = tuple(b["carry%d" % i] for i in range(4))
        outs = nav().path_scan(b[f], b["pos_b"], b["pos_a"], W, H, b["term"], b["trunc"], carry, age=b["age"], init_pos=b["init_pos"])
        return dict(_named(("ep_start", "ep_best", "ep_off", "ep_steps"), outs), **{"carry%d" % i: c for i, c in enumerate(carry)})

    def _pscan_carry(seed, b, f=_f):
        """Carries of episodes that are running: those an earlier rollout of the same worlds leaves (made on the device)."""
        z16 = lambda: torch.zeros(N, dtype=torch.int16, device=DEV).view(torch.uint16)        # noqa: E731
        carry = (z16(), z16(), torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV))
        e = up(rollout_np(seed + 10, T, N, 17, 17))
        nav().path_scan(b[f], e["pos_b"], e["pos_a"], 17, 17, e["term"], e["trunc"], carry, age=e["age"], init_pos=e["init_pos"])
        return {"carry%d" % i: c for i, c in enumerate(carry)}

    def _pscan_ref(h, W, H, f=_f):
        outs, carry = path_ref.path_scan(h[f], h["pos_b"], h["pos_a"], W, H, h["term"], h["trunc"],
                                         tuple(h["carry%d" % i] for i in range(4)), h["age"], h["init_pos"])
        return dict(zip(("ep_start", "ep_best", "ep_off", "ep_steps", "carry0", "carry1", "carry2", "carry3"), outs + tuple(carry)))
    _nav_case("path_scan", ["mg_nav_path_scan"], (_f, "pos_b", "pos_a", "term", "trunc", "age", "init_pos"), P=_P,
              call=_pscan_call, extra=_pscan_carry, ref=_pscan_ref, state=("carry0", "carry1", "carry2", "carry3"))


def _psum_extra(seed, b):
    z16 = lambda: torch.zeros(N, dtype=torch.int16, device=DEV).view(torch.uint16)            # noqa: E731
    carry = (z16(), z16(), torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV))
    outs = nav().path_scan(b["dist"], b["pos_b"], b["pos_a"], 17, 17, b["term"], b["trunc"], carry)
    return dict(zip(("ep_start", "ep_best", "ep_off", "ep_steps"), outs))


def _psum_call(b, o, W, H):
    nav().path_summary(b["ep_start"], b["ep_best"], b["ep_off"], b["ep_steps"], b["term"], b["trunc"], summary=o["summary"],
                       workspace=o["workspace"])
    return dict(summary=o["summary"])


def _psum_ref(h, W, H):
    w = path_ref.path_summary(h["ep_start"], h["ep_best"], h["ep_off"], h["ep_steps"], h["term"], h["trunc"])
    bound = np.zeros(10)                                     # test_path_gpu.check_summary: exact but the two quotient sums
    bound[3], bound[6] = w[1] * 2.0 ** -53 * w[3], w[2] * 2.0 ** -53 * w[6]
    return dict(summary=w, _atol=dict(summary=bound))


_nav_case("path_summary", ["mg_nav_path_summary"], ("dist", "pos_b", "pos_a", "term", "trunc"), P=1, Tn=TS, ref=_psum_ref, call=_psum_call,
          extra=_psum_extra, outs=lambda: dict(summary=torch.empty(10, dtype=torch.float64, device=DEV),
                                               workspace=torch.empty(nav().path_summary_workspace(TS, N), dtype=torch.float64, device=DEV)))


def _timed_goal_ahead_case():
    """The 17 x 17 world under stream_util's protocol: every seed draws its own records, rollout and clocks (seed 0 is the
    decoy), so a launch on the wrong stream, or a replay that kept the captured inputs, reads another answer."""
    R = 1100
    sets = {}

    def world_of(seed):
        if seed not in sets:
            base = taref.twoarmy()
            rng = np.random.default_rng(900 + seed)
            c = dict(base, memo={})
            free = np.stack([np.asarray(base["ty"][n] != 2).reshape(17, 17) for n in range(base["N"])])
            c["pos"] = taref._walk(rng, free, 17, 17, base["T"], base["N"], [(5 + 2 * n, 9 + (n + seed) % 2) for n in range(base["N"])])
            c["age"] = taref._clocks(rng, base["T"], base["N"], base["P"])
            c["rec"] = taref._records_of_runs(rng, c, R, 40)
            sets[seed] = c
        return sets[seed]

    def make(seed):
        c = world_of(seed)
        b = dict(ty=c["ty"], sched=c["sched"].view(np.int32), pos=c["pos"], age=c["age"], init=c["init"], rt=c["rec"]["t"],
                 rn=c["rec"]["n"], rgoal=c["rec"]["goal"])
        return up({k: np.array(v) for k, v in b.items()})      # copies: the shared world is read-only (nav_util.dev)

    def call(b, o, ctx):
        nav().timed_goal_ahead(b["ty"], b["rt"], b["rn"], b["rgoal"], b["pos"], 17, 17, b["sched"], b["age"], b["init"],
                               pass_types=taref.STATIC, out=o["labels"], dist_out=o["dist"])
        return dict(labels=o["labels"], dist=o["dist"])

    def ref(h):
        c = dict(taref.twoarmy(), memo={}, pos=h["pos"], age=h["age"], init=h["init"])
        lab, ad = taref.timed_goal_ahead(c, h["rt"], h["rn"], h["rgoal"], 3)
        return dict(labels=lab.view(np.int64), dist=ad)

    def also(part, x, y):
        if part == "A":                                        # the decoy has another answer
            assert len(unchanged(x, y, x)) < len(x)
        else:
            assert not unchanged(x, y, ["labels"])

    return Case("timed_goal_ahead 17x17 N=4 P=6", "navigation", ["mg_nav_timed_goal_ahead"], make, call, ref=ref, also=also,
                outs=lambda: dict(labels=torch.empty(R, dtype=torch.int64, device=DEV), dist=u16_full(R)))


CASES.append(_timed_goal_ahead_case())

# -------------------------------------------------------------------------------------------- observation wrappers


def _obs_cases(Nn, W, H):
    from twoarmy_amd import minigrid_obs as mo
    tag = " %dx%d N=%d" % (W, H, Nn)

    def wmake(*keys, extra=None):
        def make(seed):
            b = up(pick(world_np(seed, Nn, W, H), *keys))
            b.update(extra(seed) if extra else {})
            return b
        return make

    def image(seed):
        r = rng(seed, 5)
        return dict(image=dev(np.stack([r.integers(0, 11, (Nn, 7, 7)), r.integers(0, 6, (Nn, 7, 7)), r.integers(0, 3, (Nn, 7, 7))],
                                       -1).astype(U8)), tail=dev(r.integers(0, 2, 28).astype(F32)))
    agent = ("ax", "ay", "ad")
    out = [
        Case("onehot" + tag, "obs", ["mg_obs_onehot"], wmake(extra=image),
             lambda b, o, ctx: dict(zip(("out", "error"), mo.onehot(b["image"], want_error=True))),
             ref=lambda h: dict(zip(("out", "error"), obs_ref.onehot(h["image"])))),
        Case("flat_obs" + tag, "obs", ["mg_obs_flat"], wmake(extra=image),
             lambda b, o, ctx: dict(out=mo.flat_obs(b["image"], b["tail"])), ref=lambda h: dict(out=obs_ref.flat(h["image"], h["tail"]))),
        Case("full_obs" + tag, "obs", ["mg_obs_full"], wmake("ty", "co", "st", *agent),
             lambda b, o, ctx: dict(zip(("out", "error"), mo.full_obs(b["ty"], b["co"], b["st"], W, H, b["ax"], b["ay"], b["ad"],
                                                                      want_error=True))),
             ref=lambda h: dict(zip(("out", "error"), obs_ref.full(h["ty"], h["co"], h["st"], W, H, h["ax"], h["ay"], h["ad"])))),
        Case("symbolic_obs" + tag, "obs", ["mg_obs_symbolic"], wmake("ty"),
             lambda b, o, ctx: dict(out=mo.symbolic_obs(b["ty"], W, H)), ref=lambda h: dict(out=obs_ref.symbolic(h["ty"], W, H))),
        Case("goal_index" + tag, "obs", ["mg_obs_goal_index"], wmake("ty"),
             lambda b, o, ctx: dict(out=mo.goal_index(b["ty"], W, H)), ref=lambda h: dict(out=obs_ref.goal_index(h["ty"], W, H))),
    ]

    def gd_make(seed):
        w = world_np(seed, Nn, W, H)
        return up(dict(pick(w, "ax", "ay"), k=obs_ref.goal_index(w["ty"], W, H), table=mo.angle_table(W, H).numpy()))

    def gd_call(b, o, ctx):
        slope, e1 = mo.goal_direction(b["k"], W, H, b["ax"], b["ay"], want_error=True)
        angle, e2 = mo.goal_direction(b["k"], W, H, b["ax"], b["ay"], mode="angle", table=b["table"], want_error=True)
        return dict(slope=slope, angle=angle, error=e1, error_angle=e2)

    def gd_ref(h):
        s, e = obs_ref.goal_direction(h["k"], W, H, h["ax"], h["ay"])
        a, _ = obs_ref.goal_direction(h["k"], W, H, h["ax"], h["ay"], mode="angle")
        return dict(slope=s, angle=a, error=e, error_angle=e)
    out.append(Case("goal_direction" + tag, "obs", ["mg_obs_goal_direction"], gd_make, gd_call, ref=gd_ref))
    return out


# ------------------------------------------------------------------------------------------------- view and render
def _view_cases(Nn, W, H):
    from twoarmy_amd import minigrid_view as mv
    tag = " %dx%d N=%d" % (W, H, Nn)
    keys = ("ty", "co", "st", "ax", "ay", "ad")

    def gen_ref(h):
        import minigrid_view_oracle as mvo
        enc = np.stack([h["ty"], h["co"], h["st"]], -1).reshape(Nn, H, W, 3).transpose(0, 2, 1, 3)
        img, vis = mvo.gen_obs_batch(enc, h["ax"], h["ay"], h["ad"], 7, False)
        return dict(image=img, mask=vis)

    def step_make(seed):
        r = rng(seed, 6)
        return up(dict(pick(world_np(seed, Nn, W, H), *keys), action=r.integers(0, 7, Nn).astype(I32),
                       step_count=r.integers(0, 50, Nn).astype(I32)))

    def step_call(b, o, ctx):
        res = mv.step(b["ty"], b["st"], W, H, b["action"], b["ax"], b["ay"], b["ad"], b["step_count"], 50)
        return dict(_named(("reward", "term", "trunc", "error"), res), **pick(b, "ax", "ay", "ad", "step_count"))
    return [Case("gen_obs" + tag, "view", ["mg_gen_obs"], lambda seed: up(pick(world_np(seed, Nn, W, H), *keys)),
                 lambda b, o, ctx: dict(zip(("image", "mask"), mv.gen_obs(b["ty"], b["co"], b["st"], W, H, b["ax"], b["ay"], b["ad"], 7))),
                 ref=gen_ref),
            Case("mg_step" + tag, "view", ["mg_step"], step_make, step_call, note="default-stream run only")]


RW, RH, RN, RTS, RV = 5, 4, 3, 8, 3   # the renderer: one 5 x 4 world size, the smallest tile size test_render_gpu draws


def _render_cases():
    from twoarmy_amd import minigrid_render as mr
    keys = ("ty", "co", "st", "ax", "ay", "ad")

    def make(seed):
        r = rng(seed, 7)
        return up(dict(pick(world_np(seed, RN, RW, RH), *keys), hl=(r.random((RN, RW * RH)) < 0.5).astype(U8),
                       vis=(r.random((RN, RV, RV)) < 0.6).astype(U8)))

    def agent(b):
        return b["ax"], b["ay"], b["ad"]

    def render_call(b, o, ctx):
        mr.render(b["ty"], b["co"], b["st"], RW, RH, *agent(b), RTS, highlight=b["hl"], out=o["frame"], error=o["error"])
        return dict(o)

    def render_ref_(h):
        img, err = render_ref.render_frames(h["ty"], h["co"], h["st"], RW, RH, h["ax"], h["ay"], h["ad"], RTS, highlight=h["hl"])
        return dict(frame=img, error=np.asarray(err).astype(I32))

    def pov_call(b, o, ctx):
        mr.render_pov(b["ty"], b["co"], b["st"], RW, RH, *agent(b), RV, RTS, vis_mask=b["vis"], out=o["frame"], error=o["error"])
        return dict(o)

    def atlas_call(b, o, ctx):
        M().call("mg_render_build_atlas", o["tiles"], RTS, M().ptr(o["tiles"]))
        return dict(o)
    err = lambda: torch.empty(RN, dtype=torch.int32, device=DEV)                              # noqa: E731
    return [
        Case("render", "render", ["mg_render"], make, render_call, ref=render_ref_,
             outs=lambda: dict(frame=torch.empty((RN, RH * RTS, RW * RTS, 3), dtype=torch.uint8, device=DEV), error=err())),
        Case("render_pov", "render", ["mg_render_pov"], make, pov_call, note="default-stream run only",
             outs=lambda: dict(frame=torch.empty((RN, RV * RTS, RV * RTS, 3), dtype=torch.uint8, device=DEV), error=err())),
        Case("highlight_mask", "render", ["mg_highlight_mask"], make,
             lambda b, o, ctx: dict(mask=mr.highlight_mask(b["vis"], RW, RH, *agent(b), RV)),
             ref=lambda h: dict(mask=np.stack([render_ref.highlight_mask(h["vis"][n], RW, RH, int(h["ax"][n]), int(h["ay"][n]),
                                                                         int(h["ad"][n]), RV) for n in range(RN)]))),
        Case("build_atlas (C ABI)", "render", ["mg_render_build_atlas"], lambda seed: {}, atlas_call,
             outs=lambda: dict(tiles=torch.empty(mr.atlas_bytes(RTS), dtype=torch.uint8, device=DEV)),
             note="default-stream run only; through the C ABI: TileAtlas synchronises after the launch (EXEMPT).  No inputs: part A "
                  "can see an unwritten output here, not a stale read"),
    ]


# ---------------------------------------------------------------------------------------------------------- engine
EN, ESEED = 130, 9981


def _engine(T_out):
    def setup(seed):
        from twoarmy_amd.engine import TwoarmyEngine
        eng = TwoarmyEngine(6, EN, 17, device=DEV, seed=ESEED)
        out = eng.alloc_outputs(T_out)
        for k, t in out.items():
            t.fill_(float("nan") if t.dtype.is_floating_point else 0xAB)
        torch.cuda.synchronize()
        return eng, out
    return setup


def _acts(Tn):
    return lambda seed: dict(actions=dev(rng(seed, 8).integers(0, 5, (Tn, EN) if Tn else (EN,)).astype(I32)))


def _oracle(Tn, actions):
    import twoarmy_oracle as orc
    return orc.rollout(6, EN, Tn, ESEED, actions=actions)


def _rollout_case(name, Tn):
    def call(b, o, ctx):
        eng, out = ctx
        eng.rollout(Tn, out, actions=b["actions"])
        return dict(out)
    return Case(name, "engine", ["tw_rollout"], _acts(Tn), call, setup=_engine(Tn), ref=lambda h: _oracle(Tn, h["actions"]),
                exempt_b="own test: test_engine_rollout_captured_and_replayed")


def _step_call(b, o, ctx):
    eng, out = ctx
    eng.step(b["actions"], out, autoreset=True, policy_idx=True)
    return dict(out)


def _reset_setup(seed):
    eng, out = _engine(None)(seed)
    eng.step(torch.ones(EN, dtype=torch.int32, device=DEV), out, autoreset=True, policy_idx=True)
    torch.cuda.synchronize()
    return eng, out


def _reset_call(b, o, ctx):
    ctx[0].reset(mask=b["mask"], obs=o["obs"])
    return dict(obs=o["obs"], view=ctx[0].gen_obs(7))


def _time_call(b, o, ctx):
    ctx[0].time_rollout(8, ctx[1], actions=b["actions"], iters=1)
    return dict(ctx[1])


def _decode_call(b, o, ctx):
    from twoarmy_amd.engine import TwoarmyEngine
    return dict(matrix=TwoarmyEngine.decode_matrix(b["codes"]))


def _decode_ref(h):
    from twoarmy_amd.engine import MATRIX_CODE_VALUES
    return dict(matrix=np.array(MATRIX_CODE_VALUES, F32)[h["codes"]])


ENGINE = [
    Case("decode_matrix", "engine", [], lambda seed: dict(codes=dev(rng(seed).integers(0, 4, (N, 289)).astype(U8))), _decode_call,
         ref=_decode_ref),            # no C function: the look-up table is a front-end constant (defect 2)
    _rollout_case("rollout pipelined T=8", 8), _rollout_case("rollout sequential T=7", 7),
    Case("step", "engine", ["tw_step"], _acts(None), _step_call, setup=_engine(None),
         ref=lambda h: {k: v[0] for k, v in _oracle(1, h["actions"][None]).items()},
         ref_in_b=False),             # the oracle of calls 2 and 3 needs the engine's step counter: B uses the eager sequence
    Case("reset + gen_obs", "engine", ["tw_reset", "tw_gen_obs"], lambda seed: dict(mask=dev((rng(seed).random(EN) < 0.5).astype(U8))),
         _reset_call, setup=_reset_setup, outs=lambda: dict(obs=torch.empty((EN, 17, 17, 3), dtype=torch.uint8, device=DEV)),
         note="default-stream run only"),
    Case("fill_actions", "engine", ["tw_fill_actions"], lambda seed: {}, lambda b, o, ctx: dict(actions=ctx[0].fill_actions(8)),
         setup=_engine(8), note="default-stream run only.  No inputs: part A can see an unwritten output here, not a stale read"),
    Case("time_rollout", "engine", ["tw_time_rollout"], _acts(8), _time_call, setup=_engine(8), blocks_host=True,
         exempt_b="returns a host float: it waits for its own events by design",
         note="default-stream run only; the call returns when its work is done, so the delay cannot outlast it"),
]
CASES += _obs_cases(3, 5, 9) + _obs_cases(N, 17, 17) + _view_cases(3, 5, 9) + _view_cases(N, 17, 17) + _render_cases() + ENGINE

# Calls that synchronise or size their outputs on the host by design: exempt from part B only.
EXEMPT = {
    "ppo_ops.her_relabel": "the record count is read back to size the outputs; its two launches are captured one by one",
    "tw_create": "allocates and initialises the engine", "tw_destroy": "frees the engine",
    "tw_alloc_outputs": "allocates the slab", "tw_free_outputs": "frees the slab",
    "tw_get_state_host": "copies the state to the host", "tw_set_state_host": "copies the state from the host",
    "tw_fallback_count": "reads a device counter back", "tw_time_rollout": "waits for its own events and returns a host float",
    "TileAtlas()": "synchronises so that frames may be rendered on any stream later; mg_render_build_atlas itself is captured",
    "EpisodeTracker.read / VisitTracker.read / PathTracker.read": "one device-to-host copy of the summary",
}
PART_B = [c for c in CASES if c.exempt_b is None]
FAMILIES = ("engine", "ppo", "replay", "scans", "bonuses", "navigation", "obs", "view", "render")

_baseline = {}


def baseline(case):
    """The default-stream run of the real input set, computed once and shared by part A and the controls."""
    if case.name not in _baseline:
        _baseline[case.name] = run_default(case, 1)
    return _baseline[case.name]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_eager_on_a_side_stream(case):
    want = baseline(case)
    got, still_running = run_side(case, 1)
    print("enqueue %-40s %.3f ms" % (case.name, ENQUEUE_MS[case.name]))
    if not case.blocks_host:
        assert still_running, "the delay ended before the host had enqueued %s (%.3f ms): the run proves nothing" % (
            case.name, ENQUEUE_MS[case.name])
    check_same(case, got, want, "side stream")
    if case.ref is not None:
        h = {k: host(v) for k, v in case.make(1).items()}
        check_against_ref(case, got, case.ref(h), "side stream")
    if case.also is not None:
        case.also("A", got, run_default(case, 0))
    assert hip_error() == 0


@pytest.mark.parametrize("case", [GAE, ADV_NORM, BONUS_EPISODE], ids=repr)
def test_control_call_on_the_default_stream_is_seen(case):
    """The protocol with the mistake it looks for made on purpose: the inputs are staged on the side stream behind the
    delay, the call goes to the default stream and reads the decoy (valid memory: a mis-ordering, not a fault)."""
    want = baseline(case)
    got, still_running = run_side(case, 1, call_on_default=True)
    assert still_running
    assert not all(same_bits(got[k], want[k]) for k in want), "a call on the wrong stream went unnoticed"
    assert hip_error() == 0


@pytest.mark.parametrize("case", PART_B, ids=repr)
def test_captured_and_replayed(case):
    eager, cpu = expected_sequence(case)
    got = run_captured(case)
    for i, g in enumerate(got, 1):
        check_same(case, g, eager[i], "replay %d" % i)
        if cpu and case.ref_in_b:
            check_against_ref(case, g, cpu[i], "replay %d" % i)
    if case.also is not None:
        case.also("B", *got)
    assert hip_error() == 0


KEYS = ("obs", "matrix", "pos", "reward", "terminated", "truncated")


@pytest.mark.parametrize("Tn", [8, 7])
def test_engine_rollout_captured_and_replayed(Tn):
    """One captured rollout launch (T = 8: the pipelined kernel with its flag-gated fallback, T = 7: sequential; slab
    outputs, actions in a static buffer): warm-up, replay, an eager launch in between, replay = the oracle's 4 * T steps.
    The engine's state and Philox step counter carry through the graph and through eager calls mixed with it."""
    acts = rng(0, 9).integers(0, 5, (4 * Tn, EN)).astype(I32)
    ref = _oracle(4 * Tn, acts)
    eng, out = _engine(Tn)(0)
    s = torch.cuda.Stream()

    def check(i):
        s.synchronize()
        for k in KEYS:
            assert np.array_equal(host(out[k]), ref[k][i * Tn:(i + 1) * Tn]), (Tn, i, k)
    with torch.cuda.stream(s):
        static = dev(acts[:Tn])
        eng.rollout(Tn, out, actions=static)                   # eager and not pinned yet: the buffers swap
        check(0)
        assert eng.last_launch()["pipelined"] == int(Tn >= 8)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.rollout(Tn, out, actions=static)
        assert eng.last_launch()["pipelined"] == int(Tn >= 8)
        static.copy_(dev(acts[Tn:2 * Tn]))
        g.replay()
        check(1)
        eng.rollout(Tn, out, actions=dev(acts[2 * Tn:3 * Tn]))  # an eager launch between two replays
        check(2)
        static.copy_(dev(acts[3 * Tn:]))
        g.replay()
        check(3)
    torch.cuda.synchronize()
    assert eng.fallback_count() == 0 and hip_error() == 0
    eng.close()


def test_captured_step_survives_eager_pipelined_rollouts_of_a_pinned_engine():
    """pin_state(), then a captured step() replayed after an eager pipelined rollout: the state has not moved."""
    acts = rng(0, 10).integers(0, 5, (10, EN)).astype(I32)
    ref = _oracle(10, acts)
    eng, out1 = _engine(None)(0)
    out8 = eng.alloc_outputs(8)
    eng.pin_state()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        static = dev(acts[0])
        eng.step(static, out1, autoreset=True, policy_idx=True)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.step(static, out1, autoreset=True, policy_idx=True)
        eng.rollout(8, out8, actions=dev(acts[1:9]))
        assert eng.last_launch()["pipelined"] == 1
        static.copy_(dev(acts[9]))
        g.replay()
        s.synchronize()
        for k in KEYS:
            assert np.array_equal(host(out8[k]), ref[k][1:9]), k
            assert np.array_equal(host(out1[k]), ref[k][9]), k
    torch.cuda.synchronize()
    assert eng.fallback_count() == 0 and hip_error() == 0
    eng.close()


def test_every_family_has_a_cpu_comparison():
    for f in FAMILIES:
        assert any(c.family == f and c.ref is not None for c in CASES), f
    assert {c.family for c in CASES} == set(FAMILIES)


def stream_functions():
    names = set()
    for fn in sorted(os.listdir(os.path.join(ROOT, "include"))):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", fn)).read(), flags=re.S)
        for name, params in re.findall(r"\b((?:tw|ppo|mg)_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
            if re.search(r"void\s*\*\s*stream\b", params):
                names.add(name)
    return names


def test_every_stream_function_has_a_case():
    want = stream_functions()
    print("%d prototypes take a stream" % len(want))
    assert len(want) >= 61 and "tw_rollout" in want and "mg_obs_onehot" in want and "ppo_gae_runs" in want
    part_a = {f for c in CASES for f in c.fns}
    part_b = {f for c in CASES for f in c.fns if c.exempt_b is None or c.exempt_b.startswith("own test")} | \
        {f for f in want if f in EXEMPT}
    assert want - part_a == set(), "no part-A case reaches %s" % sorted(want - part_a)
    assert want - part_b == set(), "neither a part-B case nor EXEMPT names %s" % sorted(want - part_b)
    assert part_a <= want, "a case names a function that takes no stream: %s" % sorted(part_a - want)
