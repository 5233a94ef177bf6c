#!/usr/bin/env python3
"""Achieved HBM bandwidth of the PPO-side HIP kernels (csrc/ppo_kernels.hip) at BASELINE configs[2] sizes
(T = 128 steps x N = 4096 envs = 524 288 samples; minibatch 32 768).  One JSON line per kernel:
algorithmic bytes / HIP-event time, as a fraction of the 8 TB/s peak."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from twoarmy_amd import ppo_ops  # noqa: E402

dev = torch.device("cuda", 0)
T, N, B, A = 128, 4096, 32768, 5
g = torch.Generator(device="cpu").manual_seed(0)


def timed(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def report(name, nbytes, s, note=""):
    print(json.dumps({"kernel": name, "us": s * 1e6, "algorithmic_MB": nbytes / 1e6, "GBs": nbytes / s / 1e9,
                      "frac_of_8TBs": nbytes / s / 8e12, "note": note}), flush=True)


probs = torch.softmax(torch.randn(T * N, A, generator=g), 1).to(dev)
u = torch.rand(T * N, generator=g).to(dev)
report("ppo_sample (524288 x 5)", T * N * (A * 4 + 4 + 4 + 4), timed(lambda: ppo_ops.sample(probs, u)))
report("ppo_sample, Philox uniforms", T * N * (A * 4 + 4 + 4), timed(lambda: ppo_ops.sample(probs, None, seed=1, offset=0)))

r, v, nv = (torch.randn(T, N, generator=g).to(dev) for _ in range(3))
done = (torch.rand(T, N, generator=g) < 0.02).to(torch.uint8).to(dev)
report("ppo_gae lambda=0 (reference targets)", T * N * (3 * 4 + 3 * 4),
       timed(lambda: ppo_ops.gae(r, v, nv, None, gamma=0.99, lam=0.0, use_done_mask=False)))
report("ppo_gae lambda=0.95 + done mask", T * N * (3 * 4 + 1 + 3 * 4),
       timed(lambda: ppo_ops.gae(r, v, nv, done, gamma=0.99, lam=0.95, use_done_mask=True)))
# hindsight records: H = 2^21 in runs of 1..64 (what ppo_her_relabel emits), against the one-step call on [1][H] they use
# without her_gae.  Floor: 3 floats + 2 bytes read, 3 floats written per record; the scan reads its inputs twice (40 B).
H = 1 << 21
hr, hv, hnv = (torch.randn(H, generator=g).to(dev) for _ in range(3))
run_end = torch.zeros(H, dtype=torch.uint8)
run_end[torch.cumsum(torch.randint(1, 65, (H,), generator=g), 0).clamp_(max=H) - 1] = 1
run_end = run_end.to(dev)
rt = torch.arange(H, dtype=torch.int32, device=dev)
rn, rgoal = torch.zeros(H, dtype=torch.int32, device=dev), torch.zeros((H, 2), device=dev)
report("ppo_gae [1][H] lambda=0 (records today)", H * (3 * 4 + 3 * 4),
       timed(lambda: ppo_ops.gae(hr.view(1, H), hv.view(1, H), hnv.view(1, H), None, gamma=0.99, lam=0.0)))
report("ppo_gae_runs lambda=0.95 + done mask", H * (3 * 4 + 2 + 3 * 4),
       timed(lambda: ppo_ops.gae_runs(hr, hv, hnv, run_end, run_end, 0.99, 0.95, True)), "3 launches, inputs read twice")
report("ppo_run_ends", H * (4 + 4 + 8 + 1 + 1), timed(lambda: ppo_ops.run_ends(rt, rn, rgoal, run_end)))
adv = torch.randn(T * N, generator=g).to(dev)
report("ppo_adv_norm (2 passes)", T * N * (4 + 4 + 4), timed(lambda: ppo_ops.adv_norm_(adv)))

pb = torch.softmax(torch.randn(B, A, generator=g), 1).to(dev).requires_grad_(True)
val = torch.randn(B, 1, generator=g).to(dev).requires_grad_(True)
act = torch.randint(0, A, (B,), generator=g, dtype=torch.int32).to(dev)
olp, ad, tg = (torch.randn(B, 1, generator=g).to(dev) for _ in range(3))
report("ppo_loss_fwd_bwd (minibatch 32768)", B * (A * 4 + 4 + 4 + 4 + 4 + 4 + A * 4 + 4),
       timed(lambda: ppo_ops.ppo_losses(pb, val, act, olp, ad, tg, clip=0.1, ent_coef=0.01)), "launch-bound at this size")
loss_stats = torch.zeros(ppo_ops.UPDATE_STATS_WORDS, dtype=torch.float64, device=dev)
report("ppo_loss_fwd_bwd_stats (minibatch 32768)", B * (A * 4 + 4 + 4 + 4 + 4 + 4 + A * 4 + 4) + 2 * (B // 256) * 12 * 8,
       timed(lambda: ppo_ops.ppo_losses(pb, val, act, olp, ad, tg, clip=0.1, ent_coef=0.01, stats=loss_stats)),
       "the row above plus the update diagnostics; same two launches")

frames = torch.randn(T + 4, N, 292, generator=g).to(dev)[..., :289]
codes = torch.randint(0, 4, (T + 4, N, 304), generator=g, dtype=torch.uint8).to(dev)[..., :289]
pos = torch.randn(T + 4, N, 2, generator=g).to(dev)
k = torch.randint(3, T + 3, (B,), generator=g, dtype=torch.int32).to(dev)
n = torch.randint(0, N, (B,), generator=g, dtype=torch.int32).to(dev)
age = torch.randint(0, 50, (B,), generator=g, dtype=torch.int32).to(dev)
init_f, init_p = torch.randn(289, generator=g).to(dev), torch.randn(2, generator=g).to(dev)
report("ppo_gather_stack f32 frames (32768 x 4 x 289)", B * 4 * 289 * 8,
       timed(lambda: ppo_ops.gather_stack(frames, pos, k, n, age, init_f, init_p)))
report("ppo_gather_stack_u8 code frames", B * 4 * 289 * 5,
       timed(lambda: ppo_ops.gather_stack(codes, pos, k, n, age, init_f, init_p)))
term = (torch.rand(T, N, generator=g) < 0.01).to(torch.uint8).to(dev)
trunc = (torch.rand(T, N, generator=g) < 0.02).to(torch.uint8).to(dev)
age0 = torch.zeros(N, dtype=torch.int32, device=dev)
report("ppo_age_scan", T * N * (1 + 1 + 4), timed(lambda: ppo_ops.age_scan(term, trunc, age0)))
rw5 = torch.tensor([-0.01, -0.1, -0.9, 0.2, 0.9])[torch.randint(0, 5, (T, N), generator=g)].to(dev)
act_tn = torch.randint(0, A, (T, N), generator=g, dtype=torch.int32).to(dev)
carry_r, carry_l = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
ep_r, ep_l = ppo_ops.episode_scan(rw5, term, trunc, carry_r, carry_l)
report("ppo_episode_scan (per-step outputs)", T * N * (4 + 1 + 1 + 8 + 4),
       timed(lambda: ppo_ops.episode_scan(rw5, term, trunc, carry_r, carry_l, out=(ep_r, ep_l))), "latency-bound: one lane per env")
mv_flat = torch.randint(0, 32, (T * N,), generator=g, dtype=torch.uint8).to(dev)
report("ppo_prior_loss_fwd_bwd (524288 x 5)", T * N * (A * 4 + 1) * 2 + T * N * A * 4,
       timed(lambda: ppo_ops.prior_loss(probs, mv_flat, 0.1)), "two launches, probs and moves read twice; includes 5 allocations")
ep_score = torch.zeros(1, dtype=torch.float64, device=dev)
ep_out = (torch.empty(8, dtype=torch.float64, device=dev), torch.empty(A, dtype=torch.int64, device=dev),
          torch.empty(6, dtype=torch.int64, device=dev),
          torch.empty(ppo_ops.episode_summary_workspace(T, N), dtype=torch.float64, device=dev))
n_done = int(((term | trunc) != 0).sum())
report("ppo_episode_summary (partials + ordered final pass)", T * N * (4 + 1 + 1 + 4) + n_done * 12,
       timed(lambda: ppo_ops.episode_summary(ep_r, ep_l, term, trunc, rw5, act_tn, A, 0.99, 0.01, ep_score, *ep_out)),
       "two launches")
p2 = torch.randint(1, 16, (T, N, 2), generator=g).float().to(dev)
rw = torch.randn(T, N, generator=g).to(dev)
report("ppo_her_relabel (count + scan + emit, one host sync)", T * N * (8 + 1 + 1 + 4) * 2,
       timed(lambda: ppo_ops.her_relabel(p2, term, trunc, age0, rw, seed=1), iters=5), "includes the record-count sync")


def update_path_rows():
    """The kernels around the update's convolutions at 4096 samples of 4 frames (33 x 33 x 64 activations, 1.1 GB), the
    decoder at 4096 frames and the LSTM cell at 4096 x 256: raw C ABI calls on buffers made once."""
    from twoarmy_amd._marshal import call, ptr, query
    CL = torch.channels_last
    Bc, F, H = 4096, 4, 256
    act_bytes = Bc * 1089 * 64 * 4
    y = torch.randn(Bc, 64, 33, 33, generator=g).to(dev).contiguous(memory_format=CL)
    gy = torch.randn(Bc, 64, 33, 33, generator=g).to(dev).contiguous(memory_format=CL)
    gx = torch.empty_like(y)
    bias = torch.randn(64, generator=g).to(dev)
    report("ppo_bias_relu_nhwc (4096 x 33 x 33 x 64)", 2 * act_bytes,
           timed(lambda: call("ppo_bias_relu_nhwc", y, ptr(y, None, CL), ptr(bias), Bc * 1089, 64)))
    blocks = query("ppo_relu_bwd_bias_grad_nhwc_blocks", Bc * 1089, 64)
    part = torch.empty((blocks, 64), device=dev)
    report("ppo_relu_bwd_bias_grad_nhwc (4096 x 33 x 33 x 64)", 3 * act_bytes,
           timed(lambda: call("ppo_relu_bwd_bias_grad_nhwc", y, ptr(gy, None, CL), ptr(y, None, CL), ptr(gx, None, CL),
                              ptr(part), Bc * 1089, 64)))
    frames4 = torch.randn(Bc, F, 289, generator=g).to(dev)
    wf = ppo_ops.fold_conv1_weights(torch.randn(64, F, 4, 4, generator=g).to(dev) * 0.2)
    report("ppo_conv1_up4_bias_relu (4096 x 4 frames -> 33 x 33 x 64)", act_bytes + Bc * F * 289 * 4,
           timed(lambda: call("ppo_conv1_up4_bias_relu", y, ptr(frames4), Bc, F, ptr(wf), ptr(bias), ptr(y, None, CL))))
    groups = query("ppo_conv1_up4_bwd_groups", Bc)
    gw_part, gb_part = torch.empty((groups, 16, F, 64), device=dev), torch.empty((groups, 4, 64), device=dev)
    report("ppo_conv1_up4_bwd (4096 x 4 frames)", 2 * act_bytes + 4 * Bc * F * 289 * 4,
           timed(lambda: call("ppo_conv1_up4_bwd", y, ptr(frames4), Bc, F, ptr(gy, None, CL), ptr(y, None, CL), ptr(gw_part),
                              ptr(gb_part))))
    z = torch.randn(Bc, 64, 4, 4, generator=g).to(dev)
    w1, b1 = (torch.randn(64, 16, 2, 2, generator=g) * 0.2).to(dev), torch.randn(16, generator=g).to(dev)
    w2, b2 = (torch.randn(16, 16, 5, 5, generator=g) * 0.2).to(dev), torch.randn(16, generator=g).to(dev)
    kfold = ppo_ops.fold_decoder_tail((torch.randn(16, 1, 4, 4, generator=g) * 0.2).to(dev))
    dec_out = torch.empty((Bc, 289), device=dev)
    report("ppo_decoder_frames (4096 frames)", Bc * (1024 + 289) * 4,
           timed(lambda: call("ppo_decoder_frames", z, ptr(z), Bc, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(kfold), 0.0,
                              ptr(dec_out))), "compute-bound: activations stay in LDS")
    gates, xin = torch.randn(Bc, 4 * H, generator=g).to(dev), torch.randn(Bc, 2, 4 * H, generator=g).to(dev)
    lb, c = torch.randn(4 * H, generator=g).to(dev), torch.randn(Bc, H, generator=g).to(dev)
    report("ppo_lstm_cell (4096 x 256, gates + gates_b + bias)", Bc * H * 4 * (4 + 4 + 3) + 4 * H * 4,
           timed(lambda: ppo_ops.lstm_cell_(gates, c, gates_b=xin[:, 1], bias=lb)))
    report("ppo_lstm_cell (4096 x 256, gates alone)", Bc * H * 4 * (4 + 3), timed(lambda: ppo_ops.lstm_cell_(gates, c)))


update_path_rows()
if "--ppo" in sys.argv[1:]:            # the rows of csrc/ppo_kernels.hip alone: none of the sections below
    sys.exit(0)

# Shortest-path prior: the label launch over a whole rollout (one field per env, every acting state) and the set-valued
# imitation loss with its gradient over the same 524 288 rows; ppo_episode_scan above is the yardstick.
from twoarmy_amd import minigrid_nav as nav  # noqa: E402
nav_dist = torch.randint(0, 40, (N, 289), generator=g, dtype=torch.int16).to(dev).view(torch.uint16)
pos_b = torch.randint(1, 16, (T, N, 2), generator=g).float().to(dev)
age_tn = torch.randint(0, 50, (T, N), generator=g, dtype=torch.int32).to(dev)
init_yx = torch.tensor([15.0, 3.0], device=dev)
mv_out = torch.empty((T, N), dtype=torch.uint8, device=dev)
ad_out = torch.empty((T, N), dtype=torch.uint16, device=dev)
report("mg_nav_optimal_moves (4096 x 128, moves + acting_dist)", T * N * (8 + 4 + 1 + 2) + N * 578,
       timed(lambda: nav.optimal_moves(nav_dist, pos_b, 17, 17, age=age_tn, init_pos=init_yx, out=mv_out, dist_out=ad_out)),
       "one launch")
# The same labels for hindsight records under their own goals: the records of a REAL relabelled 4096 x 128 rollout (an
# untrained policy on v6), labelled on the engine's planes.  The flood work scales with the heads -- records whose (env,
# goal cell) differs from their predecessor's, plus the first of every 1024 -- not with the bytes; the row above is the
# yardstick.  A record, no threshold.  The head count below is the one at 16-byte aligned outputs (torch allocations: a
# workgroup's share then starts at a multiple of 1024) and for goals inside the world (relabelled goals are visited
# positions, so truncation is the kernel's cell rule).
from twoarmy_amd.engine import TwoarmyEngine  # noqa: E402
from twoarmy_amd.soa.agent.PPO import PPO  # noqa: E402
from twoarmy_amd.soa.ppo_vec import VecPPOTrainer  # noqa: E402
torch.manual_seed(0)
h_eng = TwoarmyEngine(6, N, 17, device=dev, seed=9981)
h_tr = VecPPOTrainer(PPO().to(dev).use_nhwc(), h_eng, rollout_steps=T, minibatch=B)
h_tr.collect()
her = h_tr.relabel()
R = int(her["t"].numel())
h_cell = her["goal"][:, 0].long() * 17 + her["goal"][:, 1].long()
h_head = torch.ones(R, dtype=torch.bool, device=dev)
h_head[1:] = (her["n"][1:] != her["n"][:-1]) | (h_cell[1:] != h_cell[:-1])
h_head[::1024] = True
n_heads = int(h_head.sum())
hm_out, hd_out = torch.empty(R, dtype=torch.uint8, device=dev), torch.empty(R, dtype=torch.uint16, device=dev)
h_pos, h_age = h_tr.pos[3:3 + T], h_tr.age[:-1]
h_s = timed(lambda: h_eng.goal_moves(her, h_pos, h_age, h_tr.init_pos, pass_types=nav.PASS_DEFAULT | nav.PASS_BALL,
                                     out=hm_out, dist_out=hd_out))
report("mg_nav_goal_moves (%d hindsight records of a 4096 x 128 rollout, %d heads)" % (R, n_heads),
       R * (4 + 4 + 8 + 8 + 4 + 1 + 2) + N * 289, h_s,
       "one launch; %d records, %d heads, %.1f floods per us" % (R, n_heads, n_heads / (h_s * 1e6)))
# Look-ahead labels of that rollout (mg_nav_ahead, steps 3) next to the move sets of the same elements, on REAL fields -- the
# engine's static field and its six-phase one -- and the rollout's own positions and ages: on a random field hardly any
# neighbour is one nearer and the frontier dies after one round.  Three windows each, the spread of the number.
r_field = h_tr._static_field(reuse=False)
r_field6 = torch.empty((N, nav.TWOARMY_PERIOD, 289), dtype=nav.DIST_DTYPE, device=dev)
h_eng.timed_field(agent=False, out=r_field6)
ah_out = torch.empty((T, N), dtype=torch.int64, device=dev)
rom_s = timed(lambda: nav.optimal_moves(r_field, h_pos, 17, 17, age=h_age, init_pos=h_tr.init_pos, out=mv_out, dist_out=ad_out))
report("mg_nav_optimal_moves (the rollout on its static field)", T * N * (8 + 4 + 1 + 2) + N * 578, rom_s, "one launch")
rtm_s = timed(lambda: nav.timed_moves(r_field6, h_pos, 17, 17, h_age, h_tr.init_pos, out=mv_out, dist_out=ad_out))
report("mg_nav_timed_moves (the rollout on its timed field, P = 6)", T * N * (8 + 4 + 1 + 2) + N * 6 * 578, rtm_s, "one launch")
ah_cells = None
for _ in range(3):
    a_s = timed(lambda: nav.ahead(r_field, h_pos, 17, 17, steps=3, age=h_age, init_pos=h_tr.init_pos, out=ah_out, dist_out=ad_out))
    if ah_cells is None:                                       # the mean size of a final frontier: the work is real
        ah_cells = float(nav.ahead_bits(ah_out).sum()) / float((ah_out != 0).sum().clamp(min=1))
    report("mg_nav_ahead (the rollout, steps 3, static)", T * N * (8 + 4 + 8 + 2) + N * 578, a_s,
           "one launch; %.2f x mg_nav_optimal_moves; %.2f cells per non-empty label" % (a_s / rom_s, ah_cells))
for _ in range(3):
    a_s = timed(lambda: nav.ahead(r_field6, h_pos, 17, 17, steps=3, age=h_age, init_pos=h_tr.init_pos, out=ah_out, dist_out=ad_out))
    report("mg_nav_ahead (the rollout, steps 3, P = 6)", T * N * (8 + 4 + 8 + 2) + N * 6 * 578, a_s,
           "one launch; %.2f x mg_nav_timed_moves" % (a_s / rtm_s))
# Path efficiency of that rollout (PathTracker.account: mg_nav_path_scan + mg_nav_path_summary) on the same two fields, next
# to the nearest existing thing on the rollout's own flags: ppo_episode_scan + ppo_episode_summary (EpisodeTracker.account).
h_after = h_tr.pos[4:4 + T]
h_ep = ppo_ops.episode_scan(h_tr.reward, h_tr.term, h_tr.trunc, carry_r, carry_l)
ep_s = timed(lambda: (ppo_ops.episode_scan(h_tr.reward, h_tr.term, h_tr.trunc, carry_r, carry_l, out=h_ep),
                      ppo_ops.episode_summary(*h_ep, h_tr.term, h_tr.trunc, h_tr.reward, h_tr.action, A, 0.99, 0.01, ep_score,
                                              *ep_out)))
report("ppo_episode_scan + ppo_episode_summary (the rollout)", T * N * (4 + 1 + 1 + 8 + 4) + T * N * (4 + 1 + 1 + 4), ep_s,
       "three launches")
for p_field, p_name in ((r_field, "static"), (r_field6, "P = 6")):
    p_tr = nav.PathTracker(N, dev, 17, 17, period=1 if p_field.dim() == 2 else nav.TWOARMY_PERIOD)
    p_s = timed(lambda: p_tr.account(p_field, h_pos, h_after, h_tr.term, h_tr.trunc, h_age, h_tr.init_pos))
    report("PathTracker.account (the rollout, %s): mg_nav_path_scan + mg_nav_path_summary" % p_name,
           T * N * (8 + 8 + 4 + 1 + 1 + 2 + 2 + 4 + 4) + T * N * (1 + 1) + p_field.numel() * 2, p_s,
           "three launches; %.2f x ppo_episode_scan + ppo_episode_summary" % (p_s / ep_s))
# The records' look-ahead labels (mg_nav_goal_ahead, steps 3): the same floods, a frontier walk per record and 8-byte labels.
ha_out = torch.empty(R, dtype=torch.int64, device=dev)
for _ in range(3):                                             # three windows: the spread of the number below
    ha_s = timed(lambda: h_eng.goal_ahead(her, h_pos, h_age, h_tr.init_pos, steps=3, pass_types=nav.PASS_DEFAULT | nav.PASS_BALL,
                                          out=ha_out, dist_out=hd_out))
    report("mg_nav_goal_ahead (the same %d records, %d heads, steps 3)" % (R, n_heads),
           R * (4 + 4 + 8 + 8 + 4 + 8 + 2) + N * 289, ha_s, "one launch; %.2f x mg_nav_goal_moves" % (ha_s / h_s))
# The same records labelled over (cell, phase): six phases per flood, the balls on their schedule.  The row above, taken
# in the same process on the same records, is the yardstick.
ht_s = timed(lambda: h_eng.timed_goal_moves(her, h_pos, h_age, h_tr.init_pos, out=hm_out, dist_out=hd_out))
report("mg_nav_timed_goal_moves (the same %d records, %d heads, P = 6)" % (R, n_heads),
       R * (4 + 4 + 8 + 8 + 4 + 1 + 2) + N * 289, ht_s,
       "one launch; %.1f floods per us, %.2f x mg_nav_goal_moves" % (n_heads / (ht_s * 1e6), ht_s / h_s))
# The records' look-ahead labels over (cell, phase) (mg_nav_timed_goal_ahead, steps 3): the floods of the row above, the frontier
# walk and 8-byte labels of mg_nav_goal_ahead.  Both yardsticks are taken in the same process on the same records.
for _ in range(3):                                             # three windows: the spread of the number below
    hta_s = timed(lambda: h_eng.timed_goal_ahead(her, h_pos, h_age, h_tr.init_pos, steps=3, out=ha_out, dist_out=hd_out))
    report("mg_nav_timed_goal_ahead (the same %d records, %d heads, P = 6, steps 3)" % (R, n_heads),
           R * (4 + 4 + 8 + 8 + 4 + 8 + 2) + N * 289, hta_s,
           "one launch; %.2f x mg_nav_timed_goal_moves, %.2f x mg_nav_goal_ahead" % (hta_s / ht_s, hta_s / ha_s))
# Shaping of the same records under their own goals: on the static map, and over (cell, phase).  The yardsticks of the
# timed launch are the two rows it is made of: mg_nav_goal_shape (its staging and stores) and mg_nav_timed_goal_moves (its
# floods), taken in the same process on the same records.
hs_out, hs_f = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
hs_mask = torch.empty(R, dtype=torch.uint8, device=dev)
hs_s = timed(lambda: h_eng.goal_shape(her, h_pos, h_after, h_age, h_tr.init_pos, pass_types=nav.PASS_DEFAULT | nav.PASS_BALL,
                                      scale=0.05, gamma=0.99, out=hs_out, shaping_out=hs_f, mask_out=hs_mask))
report("mg_nav_goal_shape (the same %d records, %d heads)" % (R, n_heads),
       R * (4 + 4 + 8 + 8 + 8 + 4 + 4 + 4 + 4 + 1) + N * 289, hs_s, "one launch; %.2f x mg_nav_goal_moves" % (hs_s / h_s))
for _ in range(3):                                             # three windows: the spread of the number below
    hts_s = timed(lambda: h_eng.timed_goal_shape(her, h_pos, h_after, h_age, h_tr.init_pos, scale=0.05, gamma=0.99,
                                                 out=hs_out, shaping_out=hs_f, mask_out=hs_mask))
    report("mg_nav_timed_goal_shape (the same %d records, %d heads, P = 6)" % (R, n_heads),
           R * (4 + 4 + 8 + 8 + 8 + 4 + 4 + 4 + 4 + 1) + N * 289, hts_s,
           "one launch; %.2f x mg_nav_timed_goal_moves, %.2f x mg_nav_goal_shape" % (hts_s / ht_s, hts_s / hs_s))
h_eng.close()
del h_tr, h_eng, her

# Visited cells (csrc/visitation.hip): the scan, the three dense histograms a VisitTracker.account() launches and an
# indexed one over 100 000 hindsight records, on positions as concentrated as a rollout's (every env walks away from one
# start cell and returns to it when its episode ends) and on uniformly spread ones; beside them the torch expression a
# user would otherwise write for the plain matrix.
W = H = 17
walk = torch.zeros(T, N, 2)
cur = torch.tensor([15.0, 1.0]).repeat(N, 1)
moves = torch.tensor([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
ended = ((term | trunc) != 0).cpu()
for t in range(T):
    cur = (cur + moves[torch.randint(0, 5, (N,), generator=g)]).clamp_(1.0, 15.0)
    walk[t] = cur
    cur = torch.where(ended[t].view(-1, 1), torch.tensor([15.0, 1.0]), cur)
done_tn = term | trunc
her_t = torch.randint(0, T, (100000,), generator=g, dtype=torch.int32).to(dev)
her_n = torch.randint(0, N, (100000,), generator=g, dtype=torch.int32).to(dev)
for label, pv in (("rollout-like walks", walk.to(dev)), ("uniform cells", p2)):
    v_carry = torch.zeros(ppo_ops.visit_carry_words(W, H, N), dtype=torch.int32, device=dev)
    fv, ec = ppo_ops.visit_scan(pv, term, trunc, v_carry, W, H)
    counts = torch.zeros(W * H + 1, dtype=torch.int64, device=dev)
    report("ppo_visit_scan (%s)" % label, T * N * (8 + 1 + 1 + 1 + 4),
           timed(lambda: ppo_ops.visit_scan(pv, term, trunc, v_carry, W, H, out=(fv, ec))), "latency-bound: one lane per env")
    report("ppo_visit_hist dense (%s)" % label, T * N * 8, timed(lambda: ppo_ops.visit_hist(pv, counts, W, H)))
    report("ppo_visit_hist dense, first-visit mask (%s)" % label, T * N * 1 + int(fv.sum()) * 8,
           timed(lambda: ppo_ops.visit_hist(pv, counts, W, H, mask=fv)))
    report("ppo_visit_hist dense, done mask (%s)" % label, T * N * 1 + n_done * 8,
           timed(lambda: ppo_ops.visit_hist(pv, counts, W, H, mask=done_tn)))
    report("ppo_visit_hist indexed, 100000 records (%s)" % label, 100000 * 16,
           timed(lambda: ppo_ops.visit_hist(pv, counts, W, H, t_idx=her_t, n_idx=her_n)))
    report("torch.bincount((y * 17 + x).long()) (%s)" % label, T * N * 8,
           timed(lambda: torch.bincount((pv[..., 0] * 17 + pv[..., 1]).long().view(-1), minlength=289)),
           "several torch kernels and a device-to-host sync inside bincount")
    ref = torch.bincount((pv[..., 0] * 17 + pv[..., 1]).long().view(-1), minlength=289)
    one = ppo_ops.visit_hist(pv, torch.zeros(W * H + 1, dtype=torch.int64, device=dev), W, H)
    assert torch.equal(one[:289], ref) and int(one[289]) == 0

# Exploration bonuses (csrc/exploration_bonus.hip): one BonusTracker.account() of a 4096 x 128 rollout per kind mask and
# scope, on the same two kinds of positions; ppo_episode_scan and ppo_visit_scan above are the yardsticks.
from twoarmy_amd.exploration import BonusTracker  # noqa: E402
act7 = torch.randint(0, 7, (T, N), generator=g, dtype=torch.int32).to(dev)
dir_tn = torch.randint(0, 4, (T, N), generator=g, dtype=torch.int32).to(dev)
shaped = torch.empty_like(rw5)
for label, pv in (("rollout-like walks", walk.to(dev)), ("uniform cells", p2)):
    for scope in ("env", "shared"):
        for kinds in (("state",), ("action",), ("state", "action")):
            bt = BonusTracker(N, dev, kinds, scope, 1.0, W, H, 7)
            moved = T * N * (8 + 4 + 4 + 4 * len(kinds)) + (T * N * 8 if "action" in kinds else 0)
            report("ppo_bonus_scan %s, %s scope (%s)" % ("+".join(kinds), scope, label), moved,
                   timed(lambda: bt.account(pv, act7, rw5, term, dir=dir_tn, out=shaped)),
                   "one wavefront per env" if scope == "env" else "row histograms + key scan + gather")
            del bt
