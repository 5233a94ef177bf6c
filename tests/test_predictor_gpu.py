"""SURVEY 8 rows a15 and f4 ON THE GPU: the predictor path (MIOpen conv / BatchNorm / ConvTranspose, the 3 x 1024
LSTM on rocBLAS, 8-frame actor / critic) and the offline world-model training, against the numbers recorded from
the reference (tests/golden/predictor.npz, pretrain.npz) -- the same checks tests/test_predictor_cpu.py and
tests/test_pretrain_cpu.py run on the CPU.

Tolerances (stated here because fp32 GEMM / conv reduction order differs between MIOpen / rocBLAS and the CPU run
that produced the goldens): forward outputs rtol 2e-5 / atol 2e-6 (values of O(1)), per-update losses atol 1e-5
(north_star's loss tolerance)."""
import numpy as np
import pytest
import torch

from test_ppo_common import GOLDEN
from test_predictor_cpu import check_pred_states_and_heads
from test_pretrain_cpu import check_offline_world_model_training

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_pred_states_and_heads_match_reference_on_gpu():
    check_pred_states_and_heads(DEV, 2.0)


def test_predictor_sampler_and_update_on_gpu_match_cpu_torch():
    """ppo_predictor.select_action / update (PPO_Predictor.py:85-193) on the device: the 8-frame inputs are the golden
    ones; log-prob of the HIP sampler == log(probs[a]) of the reference's forward, and one update step's losses ==
    the same step evaluated with plain torch on the CPU (fp32, tolerance 1e-5)."""
    from twoarmy_amd import ppo_ops
    agent, x, p, goal = check_pred_states_and_heads(DEV, 2.0)
    g = dict(np.load(GOLDEN + "/predictor.npz"))
    probs = torch.tensor(g["probs"], device=DEV)
    u = torch.tensor([0.05, 0.5, 0.95], device=DEV)
    a, logp = ppo_ops.sample(probs, u)
    import ppo_oracle as po
    want_a, want_logp = po.sample(g["probs"], u.cpu().numpy())
    assert np.array_equal(a.cpu().numpy(), want_a)
    np.testing.assert_allclose(logp.cpu().numpy(), want_logp, rtol=1e-6, atol=1e-6)
    # one minibatch step on the device vs a literal torch evaluation of PPO_Predictor.py:136-176 on the CPU
    adv = torch.tensor([[0.3], [-0.2], [0.05]], device=DEV)
    tgt = torch.tensor([[0.1], [0.4], [-0.3]], device=DEV)
    old = logp.view(-1, 1) - 0.02
    import copy
    actor_cpu, critic_cpu = copy.deepcopy(agent.actor).cpu(), copy.deepcopy(agent.critic).cpu()
    agent.actor.train(); agent.critic.train()
    la, lv = agent.minibatch_step_x(x, p, goal, a, old, adv, tgt)
    actor_cpu.train(); critic_cpu.train()
    pc = actor_cpu(x.cpu(), p.cpu(), goal.cpu())
    dist = torch.distributions.Categorical(probs=pc)
    ratio = torch.exp(dist.log_prob(a.cpu().long()).view(-1, 1) - old.cpu())
    s1, s2 = ratio * adv.cpu(), torch.clamp(ratio, 0.9, 1.1) * adv.cpu()
    want_la = (-torch.min(s1, s2) - 0.01 * dist.entropy().view(-1, 1)).mean()
    want_lv = torch.nn.functional.smooth_l1_loss(critic_cpu(x.cpu(), p.cpu(), goal.cpu()), tgt.cpu())
    assert abs(float(la) - float(want_la)) < 1e-5 and abs(float(lv) - float(want_lv)) < 1e-5


def _world_model(seed0=31):
    from twoarmy_amd.soa.agent.encoder_LSTM_decoder import encoder_lstm_decoder
    from test_predictor_cpu import det_weights_v2
    torch.manual_seed(9981)
    m = encoder_lstm_decoder()
    for i, net in enumerate((m.encoder, m.decoder)):
        net.load_state_dict(det_weights_v2(net, seed0 + i))
    sd = {}
    for k, (name, prm) in enumerate(m.predictor.state_dict().items()):
        n = prm.numel()
        sd[name] = torch.tensor((0.03 * np.sin(0.37 * np.arange(n, dtype=np.float64) + 1.3 * k)).reshape(tuple(prm.shape)),
                                dtype=prm.dtype)
    m.predictor.load_state_dict(sd)
    return m


@pytest.mark.parametrize("stage", ["autoencoder", "predictor"])
def test_offline_losses_and_gradients_on_gpu_equal_cpu_at_identical_weights(stage):
    """One training step of each offline stage (encoder_LSTM_decoder.py:120-135 / :226-240) at IDENTICAL weights and
    minibatch: the loss on the device within 1e-5 of the CPU's; every parameter gradient within 1e-2 relative L2 of the
    CPU's (train mode: BatchNorm batch statistics, MIOpen conv / conv-transpose backward, the 3 x 1024 LSTM backward).
    The gradient tolerance is what stock MIOpen delivers, not a property of code in this repository: the CPU fp32
    gradients are within 3e-5 of an fp64 evaluation, MIOpen's reach 2.5e-3 on the encoder's first conv (three
    train-mode BatchNorm backward passes amplify their rounding); conv biases in front of a BatchNorm have an exactly
    zero gradient, hence the absolute floor."""
    g = dict(np.load(GOLDEN + "/pretrain.npz"))
    res = {}
    for dev in ("cpu", DEV):
        m = _world_model()
        nets = (m.encoder, m.decoder) if stage == "autoencoder" else (m.predictor,)
        for net in (m.encoder, m.decoder, m.predictor):
            net.to(dev)
            net.train()
        if stage == "autoencoder":
            loss = m._recon_loss(torch.tensor(g["buf_s"][:8, 4].reshape(-1, 1, 289), device=dev))
        else:
            m.encoder.eval(); m.decoder.eval()
            loss = m._predictor_loss(torch.tensor(g["buf_s"][:8], device=dev))
        loss.backward()
        res[dev] = (float(loss), [p.grad.detach().cpu().double() for net in nets for p in net.parameters()])
    assert abs(res["cpu"][0] - res[DEV][0]) < 1e-5
    rel = []
    for a, b in zip(res["cpu"][1], res[DEV][1]):
        if float(a.norm()) < 1e-4:          # analytically zero (conv bias in front of BatchNorm): only rounding noise
            assert float(b.norm()) < 5e-2
        else:
            rel.append(float((a - b).norm()) / float(a.norm()))
    print("relative L2 gradient differences cpu vs gpu:", ["%.1e" % r for r in rel])
    assert max(rel) <= 1e-2, rel


def test_offline_world_model_training_matches_reference_on_gpu(monkeypatch):
    """Whole two-stage training on the device vs the losses the reference logged (CPU run).  Adam(eps = 1e-9) turns
    every near-zero gradient element into a full +-lr step, so reduction-order differences between MIOpen and the
    CPU kernels compound from step to step: the first two steps of each stage (nothing compounded yet) must agree
    within 1e-5 (stage 2: 1e-4, it starts from stage 1's already drifted encoder), the 12-step trajectories within 5e-4
    for the auto-encoder (observed 1.4e-4) and 5e-3 for the 25 M-parameter LSTM (observed 2.6e-3); the per-step
    1e-5 claim is carried by test_offline_losses_and_gradients_on_gpu_equal_cpu_at_identical_weights."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # scoped: restored after this test
    check_offline_world_model_training(DEV, 5e-4, atol_first=1e-5, atol_pre=5e-3)


def test_lstm_gemm_inference_path_equals_the_miopen_rnn():
    """all_net.LSTM._forward_gemm (the frozen world model as explicit GEMMs + pointwise cell ops, used under eval +
    no_grad on the GPU) == the nn.LSTM module's own forward (MIOpen RNN) within 1e-5."""
    from twoarmy_amd.soa.agent.net.all_net import LSTM
    torch.manual_seed(3)
    m = LSTM().to(DEV).eval()
    z = torch.randn(37, 4, 64, 4, 4, device=DEV) * 0.5
    with torch.no_grad():
        fast, _ = m(z)
    with torch.enable_grad():                                   # grad mode selects the module path
        ref, _ = m(z)
    assert fast.shape == ref.shape == (37, 7, 64, 4, 4)
    assert torch.allclose(fast, ref.detach(), atol=1e-5, rtol=1e-5)


def test_lstm_cell_kernel_vs_torch():
    """ppo_lstm_cell (gate order i, f, g, o; c updated in place) == the torch expression of nn.LSTM's cell, incl. large
    pre-activations (saturated gates) and a batch that does not fill the last workgroup."""
    from twoarmy_amd import ppo_ops
    torch.manual_seed(8)
    for B, H, scale in ((3, 1024, 1.0), (2048, 1024, 4.0), (77, 64, 30.0), (1, 4, 1.0), (513, 4, 1.0)):
        gates = torch.randn(B, 4 * H, device=DEV) * scale
        c0 = torch.randn(B, H, device=DEV)
        i, f, g, o = gates.double().chunk(4, dim=1)
        c_want = torch.sigmoid(f) * c0.double() + torch.sigmoid(i) * torch.tanh(g)
        h_want = torch.sigmoid(o) * torch.tanh(c_want)
        c = c0.clone()
        h = ppo_ops.lstm_cell_(gates, c)
        assert float((c.double() - c_want).abs().max()) < 2e-6 * max(1.0, float(c_want.abs().max()))
        assert float((h.double() - h_want).abs().max()) < 2e-6
        assert torch.isfinite(h).all() and torch.isfinite(c).all()
        # the same pre-activations split into GEMM result + strided slice of the input projections + bias, and with
        # the GEMM result absent (first step)
        xin = torch.randn(B, 3, 4 * H, device=DEV) * scale
        bias = torch.randn(4 * H, device=DEV)
        ga = gates - xin[:, 1] - bias
        c2 = c0.clone()
        h2 = ppo_ops.lstm_cell_(ga, c2, xin[:, 1], bias)
        assert float((h2 - h).abs().max()) < 1e-5 * max(1.0, scale) and float((c2 - c).abs().max()) < 1e-5 * max(1.0, scale)
        c3 = c0.clone()
        h3 = ppo_ops.lstm_cell_(None, c3, xin[:, 2], bias)
        c4 = c0.clone()
        h4 = ppo_ops.lstm_cell_((xin[:, 2] + bias).contiguous(), c4)
        assert float((h3 - h4).abs().max()) < 2e-6 and float((c3 - c4).abs().max()) < 2e-6 * max(1.0, float(c4.abs().max()))
    # pre-activations at and far beyond saturation (exp(88) is the last finite fp32 power, exp(104) and exp(1e4) are not),
    # each magnitude in each gate with either sign, the other gates random: finite, and float64's value
    H, mags = 8, (88.0, 104.0, 1e4)
    rows = [(q, s * m) for q in range(4) for m in mags for s in (1.0, -1.0)]
    gates = torch.randn(len(rows) + len(mags), 4 * H, device=DEV)
    for r, (q, v) in enumerate(rows):
        gates[r, q * H:(q + 1) * H] = v
    for r, m in enumerate(mags, len(rows)):                  # f saturates high, i saturates low: the cell keeps its state
        gates[r, 0:H], gates[r, H:2 * H] = -m, m
    c0 = torch.randn(gates.shape[0], H, device=DEV)
    c0 = torch.where(c0 < 0, c0 - 0.1, c0 + 0.1)             # |c| >= 0.1: sigmoid(-88) = 6e-39 is far below half an ulp of it
    i, f, g, o = gates.double().chunk(4, dim=1)
    c_want = torch.sigmoid(f) * c0.double() + torch.sigmoid(i) * torch.tanh(g)
    h_want = torch.sigmoid(o) * torch.tanh(c_want)
    c = c0.clone()
    h = ppo_ops.lstm_cell_(gates, c)
    assert torch.isfinite(h).all() and torch.isfinite(c).all()
    assert float((c.double() - c_want).abs().max()) < 2e-6 * max(1.0, float(c_want.abs().max()))
    assert float((h.double() - h_want).abs().max()) < 2e-6
    assert torch.equal(c[len(rows):], c0[len(rows):])
    # the same rows with the saturating value split over GEMM result, input projection and bias (each term finite)
    c2 = c0.clone()
    h2 = ppo_ops.lstm_cell_((gates * 0.5).contiguous(), c2, (gates * 0.25).contiguous(), None)
    c3 = c0.clone()
    h3 = ppo_ops.lstm_cell_((gates * 0.75).contiguous(), c3)
    assert torch.equal(h2, h3) and torch.equal(c2, c3)       # 0.5 x + 0.25 x == 0.75 x exactly in binary floating point


def test_lstm_cell_rejections_launch_nothing():
    """H % 4, no pre-activations at all, pointers off 16-byte alignment by one float, a row pitch shorter than a row or
    no multiple of 4 floats, an empty batch: TW_E_ARG on the host, c and h untouched."""
    import ctypes as C
    from twoarmy_amd import _lib, _marshal
    lib = _lib.lib()
    B, H = 5, 8
    store = {k: torch.full((B * 4 * H + 8,), 0.5, device=DEV) for k in ("ga", "gb", "bias", "c", "h")}

    def call(B_=B, H_=H, ldb=4 * H, off=(), null=()):
        p = {k: (None if k in null else C.c_void_p(v.data_ptr() + (4 if k in off else 0))) for k, v in store.items()}
        rc = lib.ppo_lstm_cell(p["ga"], p["gb"], ldb, p["bias"], p["c"], p["h"], B_, H_, _marshal.stream(store["c"]))
        torch.cuda.synchronize()
        return rc

    bad = [dict(H_=6), dict(H_=0), dict(null=("ga", "gb")), dict(null=("c",)), dict(null=("h",)), dict(B_=0), dict(B_=-1),
           dict(ldb=4 * H - 4), dict(ldb=4 * H + 2)]
    bad += [dict(off=(k,)) for k in ("c", "h", "gb", "bias", "ga")]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert all(bool((v == 0.5).all()) for v in store.values()), kw
    assert call() == 0 and call(null=("gb",)) == 0 and call(null=("ga", "bias")) == 0 and call(ldb=4 * H + 4, B_=4) == 0
    assert not bool((store["h"][:B * H] == 0.5).all()) and bool((store["h"][B * H:] == 0.5).all())


def test_fused_encoder_path_equals_the_module_path():
    """ppo_predictor.pred_frames (encoder's first conv fused with the x4 upsampling, eval-mode BatchNorm folded into its
    weights; LSTM as GEMMs) == pred_states[0] through the literal modules, with BatchNorm statistics that are not the
    identity."""
    from test_predictor_cpu import det_weights_v2
    from twoarmy_amd.soa.agent.PPO_Predictor import ppo_predictor
    torch.manual_seed(5)
    agent = ppo_predictor()
    for i, net in enumerate((agent.encoder, agent.decoder)):
        net.load_state_dict(det_weights_v2(net, 41 + i))
    agent.to(DEV)
    s = torch.tensor([0.9, -0.9, -0.5, 0.3], device=DEV)[torch.randint(0, 4, (70, 4, 289), device=DEV)]
    agent.pred_chunk = 32                                       # also exercises the slicing
    fast = agent.pred_frames(s)
    with torch.no_grad():
        z_c, z_up = agent.encoder(s.reshape(-1, 1, 289))        # literal modules (need_upsampled=True)
        z_pred, _ = agent.predictor(z_c.view(-1, 4, 64, 4, 4))
        ref = agent.decoder(z_pred[:, 3:7])[0]
    assert z_up is not None and fast.shape == ref.shape == (70, 4, 289)
    assert torch.allclose(fast, ref, atol=2e-5, rtol=2e-5)


def test_predictor_update_on_window_records_matches_reference():
    """ppo_predictor.update (PPO_Predictor.py:123-193) on 9-frame window records -- a real episode stored and relabelled by
    the reference's own pre_store / pre_her_func, 48 records, minibatch 16, 2 epochs -- vs the per-minibatch losses the
    reference logged (tests/golden/predictor_update.npz), minibatch order replayed.  North-star bound: 1e-5 fp32."""
    g = dict(np.load(GOLDEN + "/predictor_update.npz"))
    agent, _, _, _ = check_pred_states_and_heads(DEV, 2.0)           # the seeded weights of the golden run
    from twoarmy_amd.soa.env_buffer import Buffer_gridworld
    dt = Buffer_gridworld.window_dtype(17)
    buf = np.zeros(g["buf_s"].shape[0], dtype=dt)
    for k in dt.names:
        buf[k] = g["buf_" + k]
    agent.batch_size, agent.K_epochs = 16, 2
    agent.update(buf, DEV, 0, permutations=g["perms"])
    la = np.array([v for _, v in agent.writer.scalars["loss/action_loss_update"]])
    lv = np.array([v for _, v in agent.writer.scalars["loss/value_loss_update"]])
    assert la.shape == g["action_loss"].shape == (6,)
    np.testing.assert_allclose(la, g["action_loss"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(lv, g["value_loss"], rtol=0, atol=1e-5)


def test_predictor_select_action_reference_signature(tmp_path):
    """select_action(5-deep numpy stacks) acts on frames 1..4 + their predictions (PPO_Predictor.py:85-111): the returned
    log-prob is the golden probability of the returned action; save_param writes the reference's checkpoint keys."""
    g = dict(np.load(GOLDEN + "/predictor.npz"))
    agent, _, _, _ = check_pred_states_and_heads(DEV, 2.0)
    seen = set()
    for i in range(3):
        sm = np.concatenate([g["in_s"][i][:1], g["in_s"][i]])           # frame 0 of the 5-stack is not looked at
        st = np.concatenate([g["in_p"][i][:1], g["in_p"][i]])
        for _ in range(4):
            a, logp = agent.select_action(sm, st, g["in_g"][i], DEV)
            assert 0 <= a < 5 and abs(logp - float(np.log(g["probs"][i][a]))) < 2e-5
            seen.add(a)
    assert len(seen) > 1
    agent.filepath, agent.name = str(tmp_path), "ppo_predictor_test"
    ck = torch.load(agent.save_param(3, 0.5), map_location="cpu", weights_only=True)
    assert set(ck) == {"model_actor", "model_critic", "model_encoder", "model_decoder", "model_predictor", "optimizer_actor",
                       "optimizer_critic", "epoch"} and ck["epoch"] == 3
    assert set(ck["model_predictor"]) == set(agent.predictor.state_dict())


def test_fused_decoder_path_equals_the_module_path():
    """Net_Decoder inference through ppo_decoder_frames (three transposed convs + pooling fused per frame, the 68x68
    image never formed) vs the nn.Sequential + AvgPool2d path, on latents the world model really produces and on random
    ones (negative pre-activations exercise both ReLUs), incl. a frame count that is not a multiple of the grid."""
    from twoarmy_amd.soa.agent.net.all_net import Net_Decoder
    from test_predictor_cpu import det_weights_v2
    torch.manual_seed(2)
    dec = Net_Decoder()
    dec.load_state_dict(det_weights_v2(dec, 14))
    dec.to(DEV).eval()
    for n, scale in ((3, 1.0), (700, 3.0), (1031, 0.2)):
        z = (torch.randn(n, 4, 64, 4, 4, device=DEV) * scale)
        with torch.no_grad():
            want, full = dec(z)
            got, none = dec(z, need_full=False)
        assert none is None and full is not None and got.shape == want.shape == (n, 4, 289)
        tol = 1e-5 * max(1.0, float(want.abs().max()))
        assert float((got - want).abs().max()) < tol, (n, float((got - want).abs().max()), tol)
    # the agent's inference path uses it
    agent, x, p, goal = check_pred_states_and_heads(DEV, 2.0)
    s = x[:, :4].contiguous()
    assert float((agent.pred_frames(s) - agent.pred_states(s)[0]).abs().max()) < 1e-5
