"""Entry point of the PPO baseline -- same flag names as the reference's soa/train_ppo.py:23-40, driving the
vectorised HIP engine instead of one Python env.

  python -m twoarmy_amd.soa.train_ppo --env MiniGrid-twoarmy-17x17-v6 --num_envs 4096 --updates 10
  python -m torch.distributed.run --nproc-per-node 8 ... train_ppo.py --num_envs 8192      (envs sharded per rank)

Reference-only flags that concerned the matplotlib window / absolute log paths are accepted and ignored;
--dump_frames DIR --dump_envs K writes the rendered frames of the first K envs once per update (off by default).
--visit_dir DIR writes the reference's heatmap MATRIX (heatmap.py:58-81; not the picture) once per update, counted on
the device, and --track_buffer_file DIR its track dump (heatmap.py:79) for the first --dump_envs envs.
--bonus {state,action,both} shapes the training reward with the reference's count-based exploration bonuses
(gym_minigrid/wrappers.py:34-102), counted on the device; off by default.  --bonus_scope episode clears an env's counts
at each of its episode ends, and --bonus_form first then pays only the first visit within an episode.
--goal_distance adds the shortest-path distance to the goal (static map) at the done steps and over all steps of every
rollout to the log line: one field and one lookup launch per rollout (minigrid_nav); off by default.
--prior_coef C [--prior_decay D] trains the actor with the shortest-path prior: C * D^update times the set-valued
imitation loss over the optimal moves of every acting state (one label launch per rollout, one loss launch pair per
minibatch); --expert_agreement only labels and reports.  Both append `expert agree` / `opt_mass` to the log line; off by default.
--prior_hindsight (with either) also labels the hindsight records, each under its own goal (one more launch per rollout),
trains on those labels too and appends `her agree`; off by default.
--prior_timed (with either) takes the rollout's labels from the time-expanded search instead: the row-8 balls follow their
period-6 schedule and "wait one step" is a label where the gap is closed (minigrid_nav.timed_field / timed_moves: the
same two launches per rollout); off by default.
--prior_hindsight_timed (with --prior_hindsight) labels the hindsight records by the time-expanded search too, each under
its own goal (minigrid_nav.timed_goal_moves in place of goal_moves: still one launch per rollout); off by default.
--shaping_scale S trains on the potential-shaped reward r + gamma * Phi(s') - Phi(s), Phi = -S * distance to the goal
(minigrid_nav.shape, one launch per rollout; the hindsight records each under their own goal, minigrid_nav.goal_shape,
unless --shaping_no_hindsight; --shaping_timed: the rollout's potential from the time-expanded field); appends
`shaping mean` / `unshaped` to the log line; off by default.
--shaping_hindsight_timed (with --shaping_scale, not with --shaping_no_hindsight) shapes the hindsight records by the
time-expanded search too, each under its own goal (minigrid_nav.timed_goal_shape in place of goal_shape: still one launch
per rollout), so that with --shaping_timed both halves of a critic batch use one potential; off by default.
--orient_prior_coef C [--orient_prior_decay D] [--orient_prior_steps K] (train_SoA.py, the self-orientation agent only) adds
C * D^update times the set-valued look-ahead prior to the NLL of every orientation minibatch: the mass the orientation head
puts on the displacements a shortest path reaches in K (default 3) steps (minigrid_nav.ahead, one launch per rollout);
--orient_agreement only labels and reports.  Both append `orient agree` to the log line.  --orient_prior_timed takes the
labels from the time-expanded field, --orient_prior_hindsight labels the hindsight records too, each under its own goal
(minigrid_nav.goal_ahead, one more launch; appends `her realised`), --orient_prior_hindsight_timed (with
--orient_prior_hindsight) labels them by the time-expanded search (minigrid_nav.timed_goal_ahead in its place, so that with
--orient_prior_timed both kinds of sample wait for the balls), --orient_prior_every_state adds every rollout step that is no
success sample as a prior-only row; all off by default.
--update_stats accumulates the update's diagnostics inside its loss kernel (ppo_ops.ppo_losses(stats=): no launch more
per minibatch, one host read per update) and appends `ent`, `kl`, `clipfrac`, `ev` (of the last epoch that ran) and
`epochs` to the log line; --target_kl X (implies it) skips the remaining epochs of an update once an epoch's `kl` exceeds X
(one two-element host read per epoch); both off by default.
--her_gae (plain PPO agent) keeps the hindsight records when --gae_lambda > 0: their advantages are GAE(lambda) scanned
along each relabelled run on the device (ppo_ops.run_ends + gae_runs, two calls per update) instead of the one-step
targets that --gae_lambda 0 uses; without it --gae_lambda > 0 trains on the rollout alone; off by default.
--her_select {late,near,rare} picks the hindsight goals of every episode by rule on the device (ppo_ops.her_select, one
launch per rollout, two more for near's field and lookup) instead of the reference's uniform draw: the latest first
visits, those nearest the real goal on the static map, or those in the cells visited least so far (rare counts the
visited cells of every rollout, after relabelling); appends `her_sel` to the log line; random, the default, is the draw.
--reward_norm [--reward_norm_clip C] [--reward_norm_no_hindsight] divides the training reward, as --bonus and
--shaping_scale left it, by the running standard deviation of its discounted return (VecPPOTrainer.enable_reward_norm: the
statistics advance once per rollout on the device, the targets get a scaled copy clamped to [-C, C], default 10, and the
hindsight records' rewards one by the same statistics unless --reward_norm_no_hindsight); everything logged stays raw;
appends `rstd` to the log line; every rank keeps its own statistics; not with the self-orientation agent; off by default.
"""
import argparse
import math
import os
import random
import time

import numpy as np
import torch


class _TargetKL(argparse.Action):
    """--target_kl X: the value, and --update_stats with it (the stop reads the update's KL estimate)."""

    def __call__(self, parser, namespace, values, option_string=None):
        namespace.target_kl = values
        namespace.update_stats = True


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--env", default="MiniGrid-twoarmy-17x17-v4")
    p.add_argument("--seed", type=int, default=9981)
    p.add_argument("--tile_size", type=int, default=17)
    p.add_argument("--batch_size", type=int, default=128, help="reference minibatch for its 2048-record buffer; "
                   "the vectorised loop uses --minibatch")
    p.add_argument("--her", default=True)
    p.add_argument("--gamma", type=float, default=0.99)
    p.add_argument("--lr", type=float, default=0.0001)
    p.add_argument("--weight_decay", type=float, default=0.0001)
    p.add_argument("--lr_gamma", type=float, default=0.8)
    p.add_argument("--lr_step_size", type=int, default=200)
    p.add_argument("--track_buffer_file", default=None, metavar="DIR",
                   help="write the after-step (y, x) positions of the first --dump_envs envs of every update to "
                        "DIR/track_<update>.npy, float64 [T, k, 2] (the reference's track dump, heatmap.py:79); off by default")
    p.add_argument("--num_episodes", type=int, default=1000000)
    p.add_argument("--max_steps", type=int, default=50)
    p.add_argument("--log_dir", default=None)
    p.add_argument("--cuda", default="cuda:0")
    p.add_argument("--server", default=True)
    # vectorised-engine options (no reference counterpart)
    p.add_argument("--num_envs", type=int, default=4096, help="total envs over all ranks")
    p.add_argument("--rollout_steps", type=int, default=128)
    p.add_argument("--minibatch", type=int, default=4096)
    p.add_argument("--updates", type=int, default=1)
    p.add_argument("--amp", default="fp32", choices=["fp32", "bf16"],
                   help="GEMM dtype of the actor-critic (bf16 = torch.autocast, no parity claim; fp32 = reference)")
    p.add_argument("--conv_layout", default="nhwc", choices=["nhwc", "nchw"],
                   help="nhwc: channels-last conv stacks + fused bias/ReLU epilogues (fast on MI355X); nchw: the literal "
                        "nn.Sequential path")
    p.add_argument("--graph_rollout", default="auto", choices=["auto", "on", "off"],
                   help="replay the rollout (actor in the loop) as one HIP graph; auto = on for <= 512 envs per rank "
                        "(plain PPO agent), where the ~25 launches per step are host-bound (1.7x at 256 envs)")
    p.add_argument("--frame_codes", action="store_true", help="store rollout frames as uint8 codes (4x smaller, exact)")
    p.add_argument("--miopen_benchmark", action="store_true",
                   help="torch.backends.cudnn.benchmark = True: MIOpen benchmarks its solvers once per conv shape (minutes at "
                        "start-up, cached on disk) instead of taking its heuristic pick: epoch 1.66 -> 1.56 s at 4096 envs")
    p.add_argument("--k_epochs", type=int, default=10)
    p.add_argument("--k_epochs_orientation", type=int, default=50, help="SoA: epochs of the orientation head per update")
    p.add_argument("--gae_lambda", type=float, default=0.0)
    p.add_argument("--normalize_adv", action="store_true")
    p.add_argument("--her_gae", action="store_true",
                   help="with --gae_lambda > 0: relabel as with --gae_lambda 0 and give the hindsight records GAE(lambda) "
                        "advantages, scanned along each relabelled run and cut at its end on the device; plain PPO agent "
                        "only; off by default (then --gae_lambda > 0 switches relabelling off)")
    p.add_argument("--her_select", default="random", choices=["random", "late", "near", "rare"],
                   help="which first-visited cells of an episode become hindsight goals: random = the reference's uniform "
                        "draw; late = the latest first visits (the longest prefixes); near = the smallest shortest-path "
                        "distance to the real goal on the static map; rare = the smallest lifetime visit count, as counted "
                        "before the rollout being relabelled; ties fall by a Philox word; appends `her_sel` to the log line")
    p.add_argument("--score", default="rollout", choices=["rollout", "episode"],
                   help="what drives the HER switch and the logged score: rollout = one EMA step per rollout with the "
                        "rollout's reward sum over its finished episodes; episode = the reference's fold, one step per "
                        "finished episode with that episode's return (train_ppo.py:140), kept on the device")
    p.add_argument("--predictor_file", default=None, help="checkpoint with model_encoder / model_decoder / "
                   "model_predictor (train_ppo_predictor.py:38,81-85); random-init world model when absent")
    p.add_argument("--dump_frames", default=None, metavar="DIR",
                   help="write the rendered RGB frames (the reference's get_full_render, drawn on the device) of the "
                        "first --dump_envs envs after the last rollout step of every update to DIR/update_<u>_frames.npy, "
                        "with the state they were drawn from in update_<u>_state.npz; off by default")
    p.add_argument("--dump_envs", type=int, default=4)
    p.add_argument("--visit_dir", default=None, metavar="DIR",
                   help="count the visited cells of every rollout on the device (the reference's heatmap matrix, "
                        "heatmap.py:58-81, hindsight records included while relabelling is on) and write "
                        "DIR/visits_<update>_rank<r>.npz with rollout, first_visit_map, terminal_map, cumulative [17, 17] "
                        "and other; adds the cells covered per episode and the share of room 2 to the log line; off by default")
    p.add_argument("--bonus", default="none", choices=["none", "state", "action", "both"],
                   help="count-based exploration bonus added to the TRAINING reward on the device: the reference's "
                        "StateBonus (1/sqrt N(cell)), ActionBonus (1/sqrt N(cell, dir, action)) or both "
                        "(gym_minigrid/wrappers.py:34-102); scores, episode returns and the HER switch stay extrinsic")
    p.add_argument("--bonus_scope", default="shared", choices=["env", "shared", "episode"],
                   help="env: one count table per env (N copies of the reference's wrapper); shared: one table for all envs "
                        "of a rank, a time step counted as simultaneous; episode: one table per env whose counts clear at "
                        "each of the env's episode ends.  With several ranks every rank keeps its own tables")
    p.add_argument("--bonus_form", default="sqrt", choices=["sqrt", "first"],
                   help="sqrt: scale / sqrt(count); first (with --bonus_scope episode only): scale at the first visit of a "
                        "key within an episode, nothing after it")
    p.add_argument("--bonus_scale", type=float, default=1.0,
                   help="factor on the bonus; 1.0 is the reference's value and dwarfs the task's rewards of -0.01 ... 0.9")
    p.add_argument("--bonus_dir", default=None, metavar="DIR",
                   help="with --bonus: write DIR/bonus_<update>_rank<r>.npz with the count maps (state [17, 17], action "
                        "[4, 7, 17, 17], summed over the rank's envs) once per update; off by default")
    p.add_argument("--goal_distance", action="store_true",
                   help="once per rollout: the shortest-path distance to the goal on the static map (balls and patrols "
                        "passable) at every step, one field and one lookup launch on the device; adds `goal_dist end "
                        "mean/min` over the finished episodes and `goal_dist mean` over all steps to the log line; off by default")
    p.add_argument("--path_stats", action="store_true",
                   help="once per rollout: rate every episode against the shortest paths of the static map (balls and "
                        "patrols passable), exactly and across rollout boundaries, on the device; appends `spl` (success "
                        "weighted by path length over the episodes that ended), `progress` (the share of the start distance "
                        "they made good) and `off_path` (the share of their steps off a shortest path) to the log line; off "
                        "by default")
    p.add_argument("--path_stats_timed", action="store_true",
                   help="with --path_stats: rate against the time-expanded field instead, in which the row-8 balls follow "
                        "their period-6 schedule: waiting for the gap is on the path, walking into a ball is not")
    p.add_argument("--prior_coef", type=float, default=0.0,
                   help="shortest-path prior: add C * (the mean of -log of the policy's mass on the optimal moves of the "
                        "static map) to the actor's loss of every minibatch; rewards, returns and the critic are untouched; "
                        "plain PPO agent only; 0 = off")
    p.add_argument("--prior_decay", type=float, default=1.0, help="with --prior_coef: the coefficient of update u is C * D^u")
    p.add_argument("--expert_agreement", action="store_true",
                   help="label every rollout with the optimal moves and append `expert agree` (share of the taken actions "
                        "that are optimal) and `opt_mass` (the acting policy's mean mass on the optimal moves) to the log "
                        "line, without training on them; implied by --prior_coef")
    p.add_argument("--prior_hindsight", action="store_true",
                   help="with --prior_coef / --expert_agreement: label the hindsight records too, each under its own goal "
                        "(one more launch per rollout), let them enter the prior term with those labels instead of none, "
                        "and append `her agree` (share of the labelled records whose taken action is an optimal move "
                        "towards the hindsight goal) to the log line")
    p.add_argument("--prior_timed", action="store_true",
                   help="with --prior_coef / --expert_agreement: label the rollout with the time-expanded expert, which "
                        "plans the row-8 balls by their period-6 schedule and waits for the gap instead of walking into "
                        "a ball; the hindsight labels stay those of the static map unless --prior_hindsight_timed is given")
    p.add_argument("--prior_hindsight_timed", action="store_true",
                   help="with --prior_hindsight: label the hindsight records with the time-expanded expert as well, each "
                        "under its own goal (a relabelled record is no longer taught to step into a row-8 ball); "
                        "independent of --prior_timed")
    p.add_argument("--shaping_scale", type=float, default=0.0, metavar="S",
                   help="potential-based reward shaping: train on r + gamma * Phi(s') - Phi(s) with Phi = -S * (the "
                        "shortest-path distance to the goal on the static map), one more launch per rollout; the logged "
                        "rewards, the score and the HER switch stay extrinsic; appends `shaping mean` (mean term over the "
                        "shaped steps) and `unshaped` (share of steps without a distance) to the log line; 0 = off")
    p.add_argument("--shaping_timed", action="store_true",
                   help="with --shaping_scale: take the rollout's potential from the time-expanded field, in which the "
                        "row-8 balls follow their period-6 schedule; the hindsight records stay on the static map unless "
                        "--shaping_hindsight_timed is given")
    p.add_argument("--shaping_hindsight_timed", action="store_true",
                   help="with --shaping_scale: shape the hindsight records by the time-expanded search as well, each "
                        "under its own goal (a relabelled record is no longer rewarded for stepping into a row-8 ball); "
                        "independent of --shaping_timed, not with --shaping_no_hindsight")
    p.add_argument("--shaping_no_hindsight", action="store_true",
                   help="with --shaping_scale: leave the hindsight records unshaped (by default each is shaped under its "
                        "own goal, one more launch per rollout, and `her shaping mean` / `her unshaped` are logged)")
    p.add_argument("--orient_prior_coef", type=float, default=0.0, metavar="C",
                   help="self-orientation agent: add C * (the mean of -log of the orientation head's mass on the "
                        "displacements a shortest path reaches in --orient_prior_steps steps) to the NLL of every "
                        "orientation minibatch; one label launch per rollout; 0 = off")
    p.add_argument("--orient_prior_decay", type=float, default=1.0, help="with --orient_prior_coef: the coefficient of update u is C * D^u")
    p.add_argument("--orient_prior_steps", type=int, default=3, metavar="K", help="steps of the look-ahead, 1..3 (the head predicts 3 ahead)")
    p.add_argument("--orient_prior_timed", action="store_true",
                   help="with --orient_prior_coef / --orient_agreement: labels from the time-expanded field (the row-8 "
                        "balls on their period-6 schedule, the age of a step being its clock)")
    p.add_argument("--orient_prior_hindsight", action="store_true",
                   help="with --orient_prior_coef / --orient_agreement: label the hindsight records too, each under its "
                        "own goal on the static map (one more launch per rollout), and append `her realised` (share of "
                        "the labelled hindsight samples whose realised displacement lies in the label)")
    p.add_argument("--orient_prior_hindsight_timed", action="store_true",
                   help="with --orient_prior_hindsight: label the hindsight records by the time-expanded search too, each "
                        "under its own goal (minigrid_nav.timed_goal_ahead in place of goal_ahead: still one launch)")
    p.add_argument("--orient_prior_every_state", action="store_true",
                   help="with --orient_prior_coef: every rollout step that is no success sample joins the orientation "
                        "minibatches as a prior-only row under the env's goal (no NLL)")
    p.add_argument("--orient_agreement", action="store_true",
                   help="self-orientation agent: label every rollout with the look-ahead and append `orient agree` (share of "
                        "the labelled steps whose drawn orientation sample lies in the label) to the log line, without "
                        "training on it; implied by --orient_prior_coef")
    p.add_argument("--update_stats", action="store_true",
                   help="accumulate the diagnostics of every update inside its loss kernel (one row per epoch, read once per "
                        "update): appends `ent` (policy entropy), `kl` (approximate KL between the acting and the updated "
                        "policy), `clipfrac` (share of samples outside the clip range), `ev` (explained variance of the "
                        "critic), all of the last epoch that ran, and `epochs` to the log line; off by default")
    p.add_argument("--target_kl", type=float, default=None, metavar="X", action=_TargetKL,
                   help="KL early stop: skip the remaining epochs of an update after an epoch whose `kl` exceeds X (one small "
                        "host read per epoch; summed over the ranks first); implies --update_stats; off by default")
    p.add_argument("--reward_norm", action="store_true",
                   help="divide the training reward (bonus and shaping included) by the running standard deviation of its "
                        "discounted return, kept on the device (gym's NormalizeReward; three launches per update): "
                        "--bonus_scale and --shaping_scale then are ratios to the task's own return spread; logged rewards, "
                        "the score and the HER switch stay raw; appends `rstd` (that standard deviation) to the log line; "
                        "every rank keeps its own statistics; off by default")
    p.add_argument("--reward_norm_clip", type=float, default=None, metavar="C",
                   help="with --reward_norm: clamp the scaled reward to [-C, C]; 0 or inf: no clamp; default 10")
    p.add_argument("--reward_norm_no_hindsight", action="store_true",
                   help="with --reward_norm: leave the hindsight records' rewards unscaled (by default they are scaled by "
                        "the same statistics, one launch per update)")
    return p


def relabel_wanted(her, gae_lambda, her_gae):
    """Whether this update relabels: the HER switch is on, and the records have targets -- the one-step ones at
    lambda = 0, GAE along their runs with --her_gae."""
    return bool(her) and (gae_lambda == 0.0 or bool(her_gae))


def update_fields(us):
    """Tail of the log line with --update_stats (VecPPOTrainer.update_stats())."""
    return " ent %.4f kl %.6f clipfrac %.4f ev %.4f epochs %d" % (us["entropy"], us["approx_kl"], us["clip_frac"],
                                                                 us["explained_variance"], us["epochs_run"])


def select_fields(rule, hs):
    """Tail of the log line with --her_select (VecPPOTrainer.her_select_stats())."""
    if hs is None:
        return " her_sel %s -" % rule
    key = "-" if hs["mean_key"] is None else "%.2f" % hs["mean_key"]
    return " her_sel %s picks %d prefix %.2f key %s unreachable %d" % (rule, hs["picks"], hs["mean_prefix"], key,
                                                                      hs["unreachable"])


def orient_fields(os_, hindsight=False):
    """Tail of the log line with --orient_prior_coef / --orient_agreement (VecSoATrainer.orientation_prior_stats());
    hindsight: with --orient_prior_hindsight."""
    def f(x):
        return "-" if x is None else "%.3f" % x
    tail = " orient agree %s" % f(os_["agree"])
    if hindsight:
        tail += " her realised %s" % f(os_["her_realised"])
    return tail


def prior_fields(ps, hindsight=False):
    """Tail of the log line with --prior_coef / --expert_agreement (VecPPOTrainer.prior_stats()); hindsight: with
    --prior_hindsight."""
    tail = " expert agree %.3f opt_mass %.3f" % (ps["agree"], ps["opt_mass"]) if ps["labelled"] else \
        " expert agree - opt_mass -"
    if hindsight:
        tail += " her agree %.3f" % ps["her_agree"] if ps["her_labelled"] else " her agree -"
    return tail


def shaping_fields(ss, hindsight=True):
    """Tail of the log line with --shaping_scale (VecPPOTrainer.shaping_stats()); hindsight: unless --shaping_no_hindsight."""
    def f(x):
        return "-" if x is None else "%.4f" % x
    tail = " shaping mean %s unshaped %s" % (f(ss["mean"]), f(ss["unshaped"]))
    if hindsight:
        tail += " her shaping mean %s her unshaped %s" % (f(ss["her_mean"]), f(ss["her_unshaped"]))
    return tail


def distance_fields(ds):
    """Tail of the log line with --goal_distance (VecPPOTrainer.distance_stats())."""
    def f(x, fmt):
        return "-" if x is None else fmt % x
    return " goal_dist end mean/min %s/%s goal_dist mean %s" % (f(ds["end_mean"], "%.2f"), f(ds["end_min"], "%d"),
                                                               f(ds["mean"], "%.2f"))


def path_fields(ps):
    """Tail of the log line with --path_stats (VecPPOTrainer.path_stats())."""
    def f(x):
        return "-" if x is None else "%.4f" % x
    return " spl %s progress %s off_path %s" % (f(ps["spl"]), f(ps["progress"]), f(ps["off_path_rate"]))


def dump_bonus(bs, path, update, rank):
    os.makedirs(path, exist_ok=True)
    maps = {k: bs[k] for k in ("state", "action") if k in bs}
    maps.update({"other_" + k: np.int64(v) for k, v in bs["other"].items()})
    np.savez(os.path.join(path, "bonus_%06d_rank%d.npz" % (update, rank)), **maps)


def dump_frames(engine, path, update, k, tile_size):
    """Frames of the engine's first k envs as uint8[k, 17*ts, 17*ts, 3] and the planes / records behind them."""
    os.makedirs(path, exist_ok=True)
    k = max(1, min(int(k), engine.num_envs))
    idx = torch.arange(k, dtype=torch.int32, device=engine.device)
    frames = engine.render(env_index=idx, tile_size=tile_size).cpu().numpy()
    ty, co, rec = engine.get_state()
    np.save(os.path.join(path, "update_%d_frames.npy" % update), frames)
    np.savez_compressed(os.path.join(path, "update_%d_state.npz" % update), type=ty[:k], colour=co[:k], records=rec[:k])


def episode_fields(es):
    """Tail of the log line: what the rollout's finished episodes looked like (VecPPOTrainer.episode_stats())."""
    def f(x):
        return "-" if x is None or x in (float("inf"), float("-inf")) else "%.4f" % x
    return " ep_return mean/min/max %s/%s/%s ep_len mean %s actions [%s] rewards [%s]" % (
        f(es["mean_return"]), f(es["min_return"]), f(es["max_return"]), f(es["mean_length"]),
        " ".join(str(c) for c in es["action_hist"]), " ".join(str(c) for c in es["reward_hist"]))


def visit_fields(vs):
    """Tail of the log line with --visit_dir: distinct cells per finished episode (VecPPOTrainer.visit_stats()) and the
    share of the rollout's records that lie in room 2 (y < 8, beyond the ball gap)."""
    def f(x, fmt):
        return "-" if x is None else fmt % x
    records = int(vs["rollout"].sum()) + vs["other"]
    room2 = float(vs["rollout"][:8].sum()) / records if records else None
    return " cells mean/min/max %s/%s/%s room2 %s" % (f(vs["cells_mean"], "%.2f"), f(vs["cells_min"], "%d"),
                                                     f(vs["cells_max"], "%d"), f(room2, "%.4f"))


def dump_visits(vs, path, update, rank):
    os.makedirs(path, exist_ok=True)
    np.savez(os.path.join(path, "visits_%06d_rank%d.npz" % (update, rank)), rollout=vs["rollout"],
             first_visit_map=vs["first_visit_map"], terminal_map=vs["terminal_map"], cumulative=vs["cumulative"],
             other=np.int64(vs["other"]))


def dump_track(trainer, path, update, k):
    """After-step (y, x) of the first k envs over the rollout, float64 [T, k, 2] (heatmap.py:79 saves buffer['p'][:, 4])."""
    os.makedirs(path, exist_ok=True)
    k = max(1, min(int(k), trainer.N))
    np.save(os.path.join(path, "track_%06d.npy" % update), trainer.pos[4:4 + trainer.T, :k].double().cpu().numpy())


def main(argv=None, predictor=False, soa=False):
    args = build_parser().parse_args(argv)
    if args.bonus_form == "first" and args.bonus_scope != "episode":
        raise SystemExit("--bonus_form first needs --bonus_scope episode")
    if args.prior_hindsight and not (args.prior_coef != 0.0 or args.expert_agreement):
        raise SystemExit("--prior_hindsight needs --prior_coef or --expert_agreement")
    if args.prior_hindsight_timed and not args.prior_hindsight:
        raise SystemExit("--prior_hindsight_timed needs --prior_hindsight")
    if args.prior_timed and not (args.prior_coef != 0.0 or args.expert_agreement):
        raise SystemExit("--prior_timed needs --prior_coef or --expert_agreement")
    if not (math.isfinite(args.shaping_scale) and args.shaping_scale >= 0.0):
        raise SystemExit("--shaping_scale must be a finite number >= 0")
    if (args.shaping_timed or args.shaping_no_hindsight) and args.shaping_scale == 0.0:
        raise SystemExit("--shaping_timed / --shaping_no_hindsight need --shaping_scale")
    if args.shaping_hindsight_timed and args.shaping_scale == 0.0:
        raise SystemExit("--shaping_hindsight_timed needs --shaping_scale")
    if args.shaping_hindsight_timed and args.shaping_no_hindsight:
        raise SystemExit("--shaping_hindsight_timed shapes the hindsight records: not with --shaping_no_hindsight")
    if args.path_stats_timed and not args.path_stats:
        raise SystemExit("--path_stats_timed needs --path_stats")
    if args.target_kl is not None and not (math.isfinite(args.target_kl) and args.target_kl >= 0.0):
        raise SystemExit("--target_kl must be a finite number >= 0")
    use_orient = args.orient_prior_coef != 0.0 or args.orient_agreement
    if not (math.isfinite(args.orient_prior_coef) and args.orient_prior_coef >= 0.0):
        raise SystemExit("--orient_prior_coef must be a finite number >= 0")
    if (use_orient or args.orient_prior_timed or args.orient_prior_hindsight or args.orient_prior_every_state) and not soa:
        raise SystemExit("--orient_prior_* / --orient_agreement: self-orientation agent only")
    if (args.orient_prior_timed or args.orient_prior_hindsight or args.orient_prior_every_state) and not use_orient:
        raise SystemExit("--orient_prior_timed / _hindsight / _every_state need --orient_prior_coef or --orient_agreement")
    if args.orient_prior_hindsight_timed and not args.orient_prior_hindsight:
        raise SystemExit("--orient_prior_hindsight_timed needs --orient_prior_hindsight")
    if not 1 <= args.orient_prior_steps <= 3:
        raise SystemExit("--orient_prior_steps must be 1, 2 or 3")
    if args.her_gae and (predictor or soa):
        raise SystemExit("--her_gae: plain PPO agent only")
    if (args.reward_norm_clip is not None or args.reward_norm_no_hindsight) and not args.reward_norm:
        raise SystemExit("--reward_norm_clip / --reward_norm_no_hindsight need --reward_norm")
    if args.reward_norm_clip is not None and not args.reward_norm_clip >= 0.0:
        raise SystemExit("--reward_norm_clip must be a number >= 0 (0 or inf: no clamp)")
    if args.reward_norm and soa:
        raise SystemExit("--reward_norm: not with the self-orientation agent")
    if args.reward_norm and not 0.0 <= args.gamma <= 1.0:
        raise SystemExit("--reward_norm needs --gamma in [0, 1]")
    from .. import dist as twdist
    from ..engine import TwoarmyEngine
    from .agent.PPO import PPO
    from .ppo_vec import VecPPOTrainer

    rank, world, local_rank = twdist.init_from_env()
    seed = None if args.seed == -1 else args.seed
    random.seed(seed); np.random.seed(seed); os.environ["PYTHONHASHSEED"] = str(seed)
    if seed is not None:
        torch.manual_seed(seed); torch.cuda.manual_seed_all(seed)
    device = torch.device("cuda", local_rank % max(1, torch.cuda.device_count())) if world > 1 else torch.device(args.cuda)
    torch.cuda.set_device(device)
    if args.miopen_benchmark:
        torch.backends.cudnn.benchmark = True

    if soa:
        from .agent.Self_orientation_agent import self_orinetation_agent
        from .soa_vec import VecSoATrainer
        agent = self_orinetation_agent(log_root=args.log_dir)
        agent.K_epochs_pre_agent_position = args.k_epochs_orientation
        if args.predictor_file:
            agent.load_world_model(torch.load(args.predictor_file, map_location="cpu", weights_only=True))
    elif predictor:
        from .agent.PPO_Predictor import ppo_predictor
        agent = ppo_predictor(log_root=args.log_dir)
        if args.predictor_file:
            agent.load_world_model(torch.load(args.predictor_file, map_location="cpu", weights_only=True))
    else:
        agent = PPO(log_root=args.log_dir)
    agent.name = "%s_%s_%sseed_" % ("soa" if soa else ("ppo_predictor" if predictor else "ppo"), args.env, seed)
    agent.gamma, agent.K_epochs = args.gamma, args.k_epochs
    agent.gae_lambda, agent.use_done_mask, agent.normalize_adv = args.gae_lambda, args.gae_lambda > 0, args.normalize_adv
    agent.sample_seed = (seed or 0) + 7919 * rank
    agent.amp_dtype = torch.bfloat16 if args.amp == "bf16" else None
    agent.to(device)
    if args.conv_layout == "nhwc":
        agent.use_nhwc()
    twdist.broadcast_parameters([agent.actor, agent.critic] +
                                ([agent.encoder, agent.decoder, agent.predictor] if (predictor or soa) else []) +
                                ([agent.agent_position_preditor] if soa else []))
    if world > 1:
        agent.grad_sync = twdist.GradBucket([list(agent.actor.parameters()), list(agent.critic.parameters())])
        if soa:                                  # the orientation head has its own optimiser step, hence its own bucket
            agent.grad_sync_orient = twdist.GradBucket(list(agent.agent_position_preditor.parameters()))

    lo, hi = twdist.shard_range(args.num_envs, rank, world)
    variant = 4 if args.env.endswith("v4") else 6
    engine = TwoarmyEngine(variant, hi - lo, 17, device=device, seed=seed or 0, env_id0=lo, max_steps=args.max_steps)
    Trainer = VecSoATrainer if soa else VecPPOTrainer
    trainer = Trainer(agent, engine, args.rollout_steps, args.minibatch, frame_codes=args.frame_codes)
    trainer.use_graph = (not predictor and not soa) and (args.graph_rollout == "on" or
                                                         (args.graph_rollout == "auto" and hi - lo <= 512))
    if args.bonus != "none":
        trainer.enable_bonus(("state", "action") if args.bonus == "both" else (args.bonus,), args.bonus_scope,
                             args.bonus_scale, args.bonus_form)
    use_prior = args.prior_coef != 0.0 or args.expert_agreement
    if use_prior:
        if predictor or soa:
            raise SystemExit("--prior_coef / --expert_agreement: plain PPO agent only")
        trainer.enable_prior(args.prior_coef, args.prior_decay, hindsight=args.prior_hindsight, timed=args.prior_timed,
                             hindsight_timed=args.prior_hindsight_timed)
    use_shaping = args.shaping_scale != 0.0
    if use_shaping:
        trainer.enable_shaping(args.shaping_scale, hindsight=not args.shaping_no_hindsight, timed=args.shaping_timed,
                               hindsight_timed=args.shaping_hindsight_timed)
    if use_orient:
        trainer.enable_orientation_prior(args.orient_prior_coef, args.orient_prior_decay, steps=args.orient_prior_steps,
                                         timed=args.orient_prior_timed, hindsight=args.orient_prior_hindsight,
                                         every_state=args.orient_prior_every_state,
                                         hindsight_timed=args.orient_prior_hindsight_timed)
    if args.update_stats:
        trainer.enable_update_stats(args.target_kl)
    if args.reward_norm:
        trainer.enable_reward_norm(10.0 if args.reward_norm_clip is None else args.reward_norm_clip,
                                   hindsight=not args.reward_norm_no_hindsight)
    trainer.her_gae = args.her_gae
    use_select = args.her_select != "random"
    if use_select:
        trainer.enable_her_select(args.her_select)
    her = str(args.her).lower() not in ("false", "0", "no")
    score = 0.0
    for u in range(args.updates):
        t0 = time.perf_counter()
        trainer.collect()
        if args.bonus != "none" or use_shaping:
            trainer.shape_rewards()
        her = trainer.her_switch(her, score)                  # train_ppo.py:128-131 of the reference
        relabel = relabel_wanted(her, agent.gae_lambda, args.her_gae)
        if relabel:
            trainer.relabel()
        if use_shaping:                                       # behind relabel(): the records copy the unshaped reward_train
            trainer.shape_potential(expect_her=relabel)
        trainer.account_episodes()
        if args.visit_dir or args.her_select == "rare":       # behind relabel(): rare reads the counts before this rollout
            trainer.account_visits(trainer.her)
        if args.goal_distance:
            trainer.account_distance()
        if args.path_stats:
            trainer.account_paths(timed=args.path_stats_timed)
        if use_prior:
            trainer.label_expert()
        if use_orient:                                        # behind relabel(): its records are labelled too
            trainer.label_ahead()
        es = None
        if args.score == "episode":
            es = trainer.episode_stats()
            score = es["score"]
        else:
            score = trainer.running_score(score)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n_her = 0 if trainer.her is None else int(trainer.her["t"].numel())
        ps = trainer.prior_stats() if use_prior else None       # the policy that acted, before the update changes it
        ss = trainer.shaping_stats() if use_shaping else None   # before update() drops the records
        ots = trainer.orientation_prior_stats() if use_orient else None   # before update() drops the records
        if use_prior or use_shaping or use_orient:
            torch.cuda.synchronize()
            t1 = time.perf_counter()                            # the statistics are not part of the update's time
        la, lv = trainer.update()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if args.dump_frames and rank == 0:                      # outside both timed spans; the update leaves the envs alone
            dump_frames(engine, args.dump_frames, u, args.dump_envs, args.tile_size)
        st = trainer.stats()
        es = trainer.episode_stats() if es is None else es
        tail = ""
        if args.visit_dir:                                      # every rank writes its own file: counts are additive
            vs = trainer.visit_stats()
            dump_visits(vs, args.visit_dir, u, rank)
            tail = visit_fields(vs)
        if args.bonus != "none":                                # behind every other field; every rank has its own counts
            bs = trainer.bonus_stats()
            if args.bonus_dir:
                dump_bonus(bs, args.bonus_dir, u, rank)
            tail += " bonus mean %.4f" % bs["mean"]
        if args.goal_distance:                                  # behind every other field
            tail += distance_fields(trainer.distance_stats())
        if use_prior:                                           # behind every other field
            tail += prior_fields(ps, args.prior_hindsight)
        if use_shaping:                                         # behind every other field
            tail += shaping_fields(ss, not args.shaping_no_hindsight)
        if use_orient:                                          # behind every other field
            tail += orient_fields(ots, args.orient_prior_hindsight)
        if args.path_stats:                                     # behind every other field
            tail += path_fields(trainer.path_stats())
        if args.reward_norm:                                    # the statistics the update just trained under
            tail += " rstd %.6f" % trainer.reward_norm_stats()["std"]
        if use_select:                                          # in front of the update's diagnostics only
            tail += select_fields(args.her_select, trainer.her_select_stats() if relabel else None)
        if args.update_stats:                                   # behind every other field
            us = trainer.update_stats()
            tail += update_fields(us)
            for tag, key in (("diag/entropy", "entropy"), ("diag/approx_kl", "approx_kl"), ("diag/clip_frac", "clip_frac"),
                             ("diag/explained_variance", "explained_variance"), ("diag/epochs_run", "epochs_run")):
                agent.writer.add_scalar(tag, us[key], u)
        if args.track_buffer_file and rank == 0:
            dump_track(trainer, args.track_buffer_file, u, args.dump_envs)
        trainer.carry_over()
        if rank == 0:
            print("update %d: rollout %.3fs (%.0f env-steps/s/rank) update %.3fs action_loss %.5f value_loss %.5f "
                  "episodes %d successes %d mean_r %.4f her_records %d score %.4f" % (u, t1 - t0, trainer.T * trainer.N / (t1 - t0), t2 - t1,
                                                            float(la), float(lv), st["episodes"], st["successes"],
                                                            st["mean_reward"], n_her, score) + episode_fields(es) + tail, flush=True)
    engine.close()
    return trainer


if __name__ == "__main__":
    main()
