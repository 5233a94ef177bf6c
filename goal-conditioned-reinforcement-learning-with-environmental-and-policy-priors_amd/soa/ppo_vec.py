"""Vectorised PPO rollout / update loop on device-resident rollout tensors (replaces the per-transition
loop of the reference's soa/train_ppo.py:99-160 and the numpy ring buffer for the N-env path).

Rollout storage is time-major and holds ONE 289-float frame per env-step (not the reference's 5-frame
stack per record, train_ppo.py:93-97): frames[k] for k = -3..T, pos[k], age[t] (steps since the env's
reset).  The 4-frame policy input of any (t, n) is assembled on the fly by ppo_gather_stack, which
repeats the reset frame at episode starts exactly like np.tile in Env_transact.reset.
"""
import collections
import math
import time

import torch

from .. import ppo_ops

HER_MAX_LEN = 64              # longest episode ppo_her_relabel handles (csrc/ppo_kernels.hip)

INIT_POS = (15.0, 3.0)        # agent (y, x) after reset (twoarmy_v6.py:10, env_buffer.py:320-322)
GOAL_YX = (2.0, 14.0)


def agree_on_steps(local_steps, device):
    """Optimiser steps per epoch every rank will take: the MAX over ranks of ceil(samples / minibatch) (relabelled-record
    counts differ per rank, and every rank must take part in the same number of gradient all-reduces)."""
    if not (torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1):
        return int(local_steps)
    on_cpu = torch.distributed.get_backend() != "nccl"
    m = torch.tensor([int(local_steps)], device="cpu" if on_cpu else device)
    torch.distributed.all_reduce(m, op=torch.distributed.ReduceOp.MAX)
    return int(m.item())


def padded_permutation(perm, n_steps, minibatch):
    """An epoch's index stream stretched to exactly n_steps minibatches: a rank with fewer samples than its peers
    revisits samples of this epoch (cyclically) so that it issues as many gradient all-reduces as every other rank."""
    if n_steps > -(-perm.numel() // minibatch):
        perm = perm[torch.arange(n_steps * minibatch, device=perm.device) % perm.numel()]
    return perm


def kl_stop(k3_sum, rows, target_kl):
    """The KL early stop of VecPPOTrainer.update: after an epoch whose accumulators (ppo_ops.UPDATE_STATS) are k3_sum and
    rows, skip the remaining epochs iff approx_kl = k3_sum / rows EXCEEDS target_kl (a value equal to it goes on).  No
    rows: nothing was measured, go on."""
    return rows > 0 and k3_sum / rows > target_kl


class VecPPOTrainer:
    def __init__(self, agent, engine, rollout_steps=128, minibatch=4096, value_chunk=16384, frame_codes=False):
        """frame_codes=True stores the rollout's frames as uint8 codes (TW_F_MATRIX_CODE; 304 B instead of 1168 B
        per env-step) and expands them to the same fp32 policy inputs when stacks are gathered: bit-identical
        training, 3.8x less frame memory (BASELINE config 5)."""
        self.agent, self.engine = agent, engine
        self.T, self.N = int(rollout_steps), engine.num_envs
        self.minibatch, self.value_chunk = int(minibatch), int(value_chunk)
        d = self.device = engine.device
        T, N = self.T, self.N
        self.frame_codes = bool(frame_codes)
        self.reuse_next_values = True             # V(s'_t) = V(s_{t+1}) inside an episode (_values_rollout)
        self.fixed_shapes = True                  # pad partial minibatches / value chunks to the full size (masked rows)
        # agents whose policy input holds frames PREDICTED by a frozen world model (ppo_predictor): those frames depend only
        # on the acting state's 4-frame stack, so the rollout's own evaluation is kept ([T][N][4][289], 2.4 GB at
        # 4096 x 128) and the target pass and every epoch reuse it instead of re-running the encoder -> LSTM -> decoder
        # (7x the flops of the policy itself) on the same states
        self.cache_predictions = hasattr(agent, "pred_states")
        self.pred_frames, self._pred_valid = None, False
        self.use_graph = False                    # collect(): replay the rollout as one HIP graph (see collect)
        self._graph, self._graph_warm = None, False
        self._graph_base = torch.zeros(1, dtype=torch.int64, device=d)
        self.time_phases = False                  # update(): wall time of target computation vs epochs (one extra sync)
        self.value_rows = 0                       # critic forward rows issued by the last compute_targets (incl. padding)
        self.last_update_timing = None
        if self.frame_codes:
            self.frames_buf = torch.zeros((T + 4, N, 304), dtype=torch.uint8, device=d)
        else:
            self.frames_buf = torch.zeros((T + 4, N, 292), dtype=torch.float32, device=d)
        self.frames = self.frames_buf[..., :289]
        self.pos = torch.zeros((T + 4, N, 2), dtype=torch.float32, device=d)
        self.action = torch.zeros((T, N), dtype=torch.int32, device=d)
        self.logp = torch.zeros((T, N), dtype=torch.float32, device=d)
        self.reward = torch.zeros((T, N), dtype=torch.float32, device=d)
        self.term = torch.zeros((T, N), dtype=torch.uint8, device=d)
        self.trunc = torch.zeros((T, N), dtype=torch.uint8, device=d)
        self.age = torch.zeros((T + 1, N), dtype=torch.int32, device=d)
        self.goal1 = torch.tensor([GOAL_YX], device=d)
        self.goal = self.goal1.expand(N, 2).contiguous()
        self.n_all = torch.arange(N, dtype=torch.int32, device=d)
        # frame index of the newest frame of the acting state at step t (row t), for ppo_gather_stack
        self.k_rows = (torch.arange(T + 1, dtype=torch.int32, device=d) + 3).view(-1, 1).expand(T + 1, N).contiguous()
        self._zero_age = torch.zeros(N, dtype=torch.int32, device=d)
        self.init_pos = torch.tensor(INIT_POS, device=d)
        # the reset frame is a constant of the task: take it from a scratch engine step-free reset
        self.init_frame = self._reset_frame()
        self.frames[:4] = self._encode(self.init_frame) if self.frame_codes else self.init_frame
        self.pos[:4] = self.init_pos
        agent.to(d)
        self.her = None                       # relabelled index records of the current rollout (relabel())
        self.her_out_of_pattern = 0           # records of the last update whose V(s') could not be taken from a neighbour
        self.her_gae = False                  # GAE(lambda) along the relabelled runs instead of their one-step targets
        self.her_targets = None               # her_gae: {"value", "next_value", "run_end"} of the last compute_targets()
        # hindsight relabelling looks back over every rollout an episode ending now may have started in:
        # ceil((max_steps - 1) / T) earlier ones; each entry is (pos, term, trunc, reward, age0) of one rollout
        self.max_steps = int(getattr(engine, "max_steps", 50))
        self._hist = collections.deque(maxlen=max(1, -(-(self.max_steps - 1) // self.T)))
        self.her_seed = int(getattr(engine, "seed", 9981))
        self.her_select_rule = None           # "late" | "near" | "rare": enable_her_select(); None: the reference's draw
        self._her_select_stats = None         # int64[6] of the last relabel() that selected (ppo_her_select's stats)
        self.episodes = None                  # EpisodeTracker, made by the first account_episodes()
        self.visits = None                    # VisitTracker, made by the first account_visits()
        self.nav_field = self.goal_dist = None  # made by the first account_distance()
        self._nav_field_at = -1               # env_steps when nav_field was last computed: one field per rollout
        self.timed_field = None               # uint16[N, 6, 289], made by the first _timed_field(): one for every feature
        self._timed_field_at = -1             # env_steps when timed_field was last computed
        self.paths = None                     # PathTracker, made by the first account_paths()
        self.prior = None                     # shortest-path prior: {"coef", "decay", "updates"}, made by enable_prior()
        self.expert_moves = self.expert_dist = self.act_probs = None   # made by enable_prior() / label_expert()
        self.her_moves = self.her_dist = None # labels of the hindsight records (enable_prior(hindsight=True)) ...
        self._her_moves_of = None             # ... and the records (the dict relabel() made) they belong to
        self.bonus = None                     # BonusTracker, made by enable_bonus()
        self.reward_train = self.reward       # what targets and hindsight records use: the shaped reward when a bonus is on
        self.shaping = None                   # potential-based shaping: {"scale", "hindsight", "timed", "hindsight_timed"}, made by enable_shaping()
        self._relabel_at = -1                 # env_steps when relabel() last ran: shape_potential() comes after it
        self.dir = None                       # agent direction after each step [T, N], kept only for the action bonus
        self.update_diag = None               # update diagnostics: {"stats", "target_kl", "epochs_run"}, made by enable_update_stats()
        self.reward_norm = None               # RewardNormalizer, made by enable_reward_norm()
        self.env_steps = 0
        self.episodes_done = 0
        self.return_sum = 0.0

    @staticmethod
    def _encode(frame):
        """float matrix -> codes (0 free/goal 0.9, 1 wall -0.9, 2 ball -0.5, 3 agent 0.3)."""
        c = torch.zeros_like(frame, dtype=torch.uint8)
        c[frame == -0.9] = 1
        c[frame == -0.5] = 2
        c[frame == 0.3] = 3
        return c

    def _reset_frame(self):
        ty, _, rec = self.engine.get_state()
        m = torch.where(torch.tensor(ty[0] == 2), -0.9, torch.where(torch.tensor(ty[0] == 6), -0.5, 0.9)).float()
        m[15 * 17 + 3] = 0.3
        # valid only for freshly reset envs; the engine was just created / reset by the caller
        return m.to(self.device)

    # ------------------------------------------------------------------ rollout
    def _collect_steps(self, uniforms=None, offset_dev=None):
        """The T steps of a rollout: stack gather -> actor -> sample -> engine step -> age.  No host synchronisation
        and no host-dependent control flow, so the same body runs eagerly or under HIP-graph capture."""
        T, N = self.T, self.N
        step_out = [{"obs": None, "matrix": self.frames[t + 4], "pos": self.pos[t + 4], "reward": self.reward[t],
                     "terminated": self.term[t], "truncated": self.trunc[t]} for t in range(T)]
        if self.cache_predictions and self.pred_frames is None:
            self.pred_frames = torch.empty((T, N, 4, 289), dtype=torch.float32, device=self.device)
        self._pred_valid = False
        for t in range(T):
            s4, p4 = ppo_ops.gather_stack(self.frames, self.pos, self.k_rows[t], self.n_all, self.age[t], self.init_frame,
                                          self.init_pos)
            if self.cache_predictions:
                x = self.agent.policy_input(s4)
                self.pred_frames[t] = x[:, 4:]
                a, logp = self.agent.act_batch(s4, p4, self.goal, None if uniforms is None else uniforms[t], x=x)
            elif self.act_probs is not None:          # enable_prior(): the acting distribution is kept for prior_stats()
                a, logp = self.agent.act_batch(s4, p4, self.goal, None if uniforms is None else uniforms[t],
                                               offset_dev=offset_dev, offset_add=t * N, probs_out=self.act_probs[t])
            elif offset_dev is None:
                a, logp = self.agent.act_batch(s4, p4, self.goal, None if uniforms is None else uniforms[t])
            else:
                a, logp = self.agent.act_batch(s4, p4, self.goal, None, offset_dev=offset_dev, offset_add=t * N)
            self.action[t], self.logp[t] = a, logp
            self.engine.step(a, step_out[t], autoreset=True, policy_idx=True)
            if self.dir is not None:
                self.dir[t].copy_(self._dir_now)
            torch.where((self.term[t] | self.trunc[t]) != 0, self._zero_age, self.age[t] + 1, out=self.age[t + 1])
        self._pred_valid = self.cache_predictions

    def _policy_x(self, t_idx, n_idx, after):
        """(network input, positions) of samples (t, n): 4-frame stacks run through agent.policy_input, with the world
        model's predicted frames taken from the rollout's cache for acting states."""
        s, p = self._stacks(t_idx, n_idx, after=after)
        if self._pred_valid and not after:
            return torch.cat([s, self.pred_frames[t_idx.long(), n_idx.long()]], dim=1), p
        return self.agent.policy_input(s), p

    @torch.no_grad()
    def collect(self, uniforms=None):
        """One rollout.  With `use_graph` (small per-GPU batches, where ~25 launches per step make the host the
        bottleneck: 0.5-0.7 ms per step at 256 envs whatever the GPU does) the whole T-step rollout is captured ONCE
        as a HIP graph and replayed: the first rollout runs eagerly (MIOpen searches its kernels then), the second is
        captured, every later one is a single graph launch.  The sampler's stream position is read from device memory
        at replay time, so graph and eager rollouts draw the very same actions."""
        T, N = self.T, self.N
        if not (self.use_graph and uniforms is None and not self.cache_predictions):
            self._collect_steps(uniforms)
        elif not self._graph_warm:
            self._collect_steps(None)
            self._graph_warm = True
        else:
            if self._graph is None:
                from .agent.net.all_net import clear_fold_cache
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                clear_fold_cache(self.agent.trainable_nets())         # nothing folded eagerly may be read by the graph ...
                with torch.cuda.graph(g):
                    self._collect_steps(None, offset_dev=self._graph_base)
                clear_fold_cache(self.agent.trainable_nets())         # ... and nothing folded under capture by eager code
                self._graph = g
            self._graph_base.fill_(self.agent.sample_count)
            self._graph.replay()
            self.agent.sample_count += T * N
        self.env_steps += T * N

    def carry_over(self):
        """Make the last 4 frames the history of the next rollout (and keep what hindsight relabelling needs of
        this one: episodes that end in the next rollout start here)."""
        T = self.T
        self._hist.append((self.pos[4:4 + T].clone(), self.term.clone(), self.trunc.clone(), self.reward_train.clone(),
                           self.age[0].clone()))
        self.frames_buf[:4] = self.frames_buf[T:T + 4].clone()
        self.pos[:4] = self.pos[T:T + 4].clone()
        self.age[0] = self.age[T]

    # ------------------------------------------------------------------ update
    def _stacks(self, t_idx, n_idx, after):
        """4-frame stacks of samples (t, n): before the step (s[:,0:4]) or after it (s[:,1:5])."""
        k = t_idx + (4 if after else 3)
        age = self.age[:-1].reshape(-1)[t_idx.long() * self.N + n_idx.long()] + (1 if after else 0)
        return ppo_ops.gather_stack(self.frames, self.pos, k.int(), n_idx.int(), age.int(), self.init_frame,
                                    self.init_pos)

    # ------------------------------------------------------------------ hindsight relabelling
    @torch.no_grad()
    def relabel(self, choices=None, max_goals=4):
        """Buffer_gridworld.her_func (env_buffer.py:101-143) for every episode that lies inside this rollout:
        relabelled transitions are index records (t, n, goal', reward', done') produced on the device
        (ppo_her_relabel); update() then trains on the rollout plus these records, like the reference trains on
        its ring buffer with the appended copies.

        Episodes that began in an earlier rollout are relabelled over a window of rollouts long enough to hold any
        episode that ends now (carry_over keeps positions, rewards and done flags of ceil((max_steps-1)/T) earlier
        rollouts); only the records that lie in the current rollout are returned -- the earlier part of such a prefix
        belongs to samples whose frames are gone.

        Agents trained on 9-frame window records (ppo_predictor, self_orinetation_agent: `her_window_delay` = 4) get
        pre_her_func / pre_f_her_func (env_buffer.py:145-280) instead: the goal candidates are the states after steps
        4, 5, ... of the episode (`skip`), see ppo_her_relabel_window in include/twoarmy_ppo.h."""
        T, N = self.T, self.N
        skip = int(getattr(self.agent, "her_window_delay", 0))
        if self.shaping is not None and self._shaped_at == self.env_steps:
            raise RuntimeError("enable_shaping(): call relabel() before shape_potential(), the records copy reward_train")
        self._relabel_at = self.env_steps
        if self.max_steps > HER_MAX_LEN:
            raise ValueError("hindsight relabelling handles episodes of up to %d steps (max_steps = %d)"
                             % (HER_MAX_LEN, self.max_steps))
        start = self.env_steps // N - T                       # global step index of this rollout's first step
        select = self.her_select_rule if choices is None else None
        if not self._hist or choices is not None:
            pos, age0 = self.pos[4:4 + T], self.age[0].contiguous()
            if select is not None:
                choices = self._select_goals(pos, self.term, self.trunc, age0, start, max_goals, skip)
            self.her = ppo_ops.her_relabel(pos, self.term, self.trunc, age0,
                                           self.reward_train, choices, seed=self.her_seed, env_id0=self.engine.env_id0,
                                           step0=start, max_goals=max_goals, skip=skip)
            return self.her
        hist = list(self._hist)
        back = T * len(hist)
        pos = torch.cat([x[0] for x in hist] + [self.pos[4:4 + T]])
        term, trunc = torch.cat([x[1] for x in hist] + [self.term]), torch.cat([x[2] for x in hist] + [self.trunc])
        if select is not None:                                # over the same window, so the picks see whole episodes
            choices = self._select_goals(pos, term, trunc, hist[0][4], start - back, max_goals, skip)
        h = ppo_ops.her_relabel(pos, term, trunc, hist[0][4],
                                torch.cat([x[3] for x in hist] + [self.reward_train]), choices,
                                seed=self.her_seed, env_id0=self.engine.env_id0, step0=start - back, max_goals=max_goals,
                                skip=skip)
        keep = h["t"] >= back
        self.her = dict(t=(h["t"][keep] - back).contiguous(), n=h["n"][keep].contiguous(), goal=h["goal"][keep].contiguous(),
                        reward=h["reward"][keep].contiguous(), done=h["done"][keep].contiguous())
        self.her["counts"] = torch.bincount(self.her["n"].long(), minlength=N).int()
        return self.her

    def enable_her_select(self, rule):
        """Pick the hindsight goals of relabel() by rule instead of the reference's uniform draw (ppo_ops.her_select):
        "late": the latest first visits of an episode, i.e. the longest prefixes; "near": the first visits nearest the
        real goal by the shortest-path field of the static map (TwoarmyEngine.distance_field as account_distance() takes
        it, one lookup over the achieved positions; unreachable cells last); "rare": the first visits in the cells the
        VisitTracker has counted least over its lifetime (`cumulative`; the tracker is made here if there is none, and
        something has to feed it: account_visits() once per rollout).  relabel() comes before account_visits(), so "rare"
        reads the counts as they stand BEFORE the rollout being relabelled is accounted.  Ties fall by a Philox word of
        her_seed.  None: the reference's draw again.  relabel(choices=...) is never overridden.  "near" takes ONE field,
        the map as it stands when relabel() runs (the wall drops at this rollout's end, like account_distance()), for
        every episode of the window: an episode that ended in an earlier rollout, or before a wall dropped, is ranked
        against the present map, not the one it was played on."""
        if rule not in (None, "late", "near", "rare"):
            raise ValueError("enable_her_select(): rule is one of 'late', 'near', 'rare' or None, got %r" % (rule,))
        self.her_select_rule = rule
        self._her_select_stats = None
        if rule == "rare" and self.visits is None:
            from ..visitation import VisitTracker
            self.visits = VisitTracker(self.N, self.device, 17, 17)

    def _select_goals(self, pos, term, trunc, age0, step0, max_goals, skip):
        """`choices` of her_relabel for the arrays relabel() is about to pass it, by the enabled rule; the stats of this
        selection replace the last ones.  Two launches more at most (field and lookup of "near"), no host
        synchronisation."""
        rule, key16, table = self.her_select_rule, None, None
        if rule == "near":
            from .. import minigrid_nav as nav
            key16 = nav.lookup(self._static_field(reuse=True), pos, 17, 17)
        elif rule == "rare":
            table = self.visits.cumulative
        choices, self._her_select_stats = ppo_ops.her_select(
            pos, term, trunc, age0, {"late": "late", "near": "key16", "rare": "table"}[rule], key16=key16, table=table,
            seed=self.her_seed, env_id0=self.engine.env_id0, step0=step0, max_goals=max_goals, skip=skip)
        return choices

    def her_select_stats(self):
        """What the last relabel() selected under the enabled rule: {"episodes", "candidates", "picks", "mean_prefix":
        records per pick, "mean_key": the mean key of the picks that have one ("near": the distance, unreachable picks
        left out; "rare": the visit count; "late": None), "unreachable": picks whose cell the field does not reach};
        None where nothing was selected.  Counted over the arrays relabel() ran on: with earlier rollouts in the window,
        their episodes are in it again.  One device-to-host copy."""
        if self.her_select_rule is None or self._her_select_stats is None:
            return None
        episodes, cand, picks, records, keys, unreachable = self._her_select_stats.cpu().tolist()
        if picks == 0:
            return None
        keyed = picks - unreachable
        mean_key = None if self.her_select_rule == "late" or keyed == 0 else keys / keyed
        return {"episodes": episodes, "candidates": cand, "picks": picks, "mean_prefix": records / picks,
                "mean_key": mean_key, "unreachable": unreachable}

    def sample_goal(self, t_idx, n_idx, goal2, done):
        """Hook: per-sample goal record carried through targets / update (default: the 2-d goal itself)."""
        return goal2

    def goal_input(self, goal, after):
        """Hook: what the networks get as goal before / after the step, from a sample_goal() record."""
        return goal

    def _values_one(self, t_idx, n_idx, goal, after):
        """critic(s, g) (after=False) or critic(s', g) (after=True) of samples (t, n) with per-sample goals, in chunks."""
        total = t_idx.numel()
        v = torch.empty(total, device=self.device)
        self.agent.critic.eval()
        C = self.value_chunk
        if self.fixed_shapes and total < C:
            C = max(256, 1 << (total - 1).bit_length())          # small sets: next power of two (a handful of shapes in all)
        for i in range(0, total, C):
            sl = torch.arange(i, min(total, i + C), device=self.device)
            n_real = sl.numel()
            if self.fixed_shapes and n_real < C:
                sl = torch.cat([sl, sl[torch.arange(C - n_real, device=self.device) % n_real]])   # pad: one conv batch size
            x, p = self._policy_x(t_idx[sl], n_idx[sl], after)
            self.value_rows += int(sl.numel())
            out = self.agent.critic_value(x, p, self.goal_input(goal[sl], after)).view(-1)
            v[i:i + n_real] = out[:n_real]
        return v

    def _values(self, t_idx, n_idx, goal):
        """critic(s, g) and critic(s', g) of samples (t, n) with per-sample goals."""
        return self._values_one(t_idx, n_idx, goal, False), self._values_one(t_idx, n_idx, goal, True)

    def _values_rollout(self, goal, done):
        """V(s_t) and V(s'_t) of every rollout sample with ONE critic pass over the rollout instead of two: unless the
        episode ends at t, the state after step t IS the acting state of step t + 1 (same frames, same positions, same
        goal input), so V(s'_t) = V(s_{t+1}); only done steps and the last row need their own evaluation
        (the reference evaluates s[:,1:5] and s[:,0:4] separately because its records are independent, PPO.py:112-114)."""
        T, N = self.T, self.N
        idx = torch.arange(T * N, device=self.device)
        t_idx, n_idx = idx // N, idx % N
        v = self._values_one(t_idx, n_idx, goal, False)
        nv = torch.empty_like(v)
        nv.view(T, N)[:-1] = v.view(T, N)[1:]
        need = torch.nonzero((done.view(-1) != 0) | (t_idx == T - 1)).view(-1)
        nv[need] = self._values_one(t_idx[need], n_idx[need], goal[need], True)
        return v, nv

    def _her_next_values(self, h, hgoal, hv):
        """V(s') of relabelled records from V(s) of the record behind them.  Valid only while the records come as runs
        of consecutive steps of one env under one goal, each run ending with its done record (ppo_her_relabel's emission
        order, also after relabel()'s `keep` filter): checked on the device (one sync per update, next to the ones the
        record count already costs); records that break the pattern -- external `choices`, a changed kernel -- get
        their own evaluation of the after-state instead of a neighbour's value."""
        t, n, done = h["t"].long(), h["n"].long(), h["done"] != 0
        g = h["goal"]
        ok_next = torch.zeros_like(done)
        ok_next[:-1] = (n[1:] == n[:-1]) & (t[1:] == t[:-1] + 1) & (g[1:] == g[:-1]).all(-1)
        need = torch.nonzero(done | ~ok_next).view(-1)          # run ends, plus anything out of pattern (incl. the last row)
        hnv = self._next_values_from_neighbours(h, hgoal, hv, need)
        self.her_out_of_pattern = int((~done & ~ok_next).sum())
        return hnv

    def _next_values_from_neighbours(self, h, hgoal, hv, need):
        """V(s') of every record: V(s) of the record behind it, except at the indices `need`, whose after-states are
        evaluated."""
        hnv = torch.full_like(hv, float("nan"))                  # a row nobody fills would poison the loss visibly
        hnv[:-1] = hv[1:]
        hnv[need] = self._values_one(h["t"][need], h["n"][need], hgoal[need], True)
        return hnv

    def _her_targets_one_step(self, h, hgoal):
        """The default: the reference's one-step target with the relabelled goal and reward (PPO.py:112-114)."""
        assert self.agent.gae_lambda == 0.0 and not self.agent.use_done_mask, "HER records use the TD(0) targets"
        if self.reuse_next_values:
            # a relabelled prefix is a run of consecutive steps of one episode under ONE goal that ends with its
            # done record (ppo_her_relabel's emission order), so V(s'_j) of a record that is not done is V(s) of the
            # record behind it; only the prefix ends are evaluated on their after-states
            hv = self._values_one(h["t"], h["n"], hgoal, False)
            hnv = self._her_next_values(h, hgoal, hv)
        else:
            hv, hnv = self._values(h["t"], h["n"], hgoal)
        H = hv.numel()
        hadv, htarget, _ = ppo_ops.gae(h["reward"].view(1, H), hv.view(1, H), hnv.view(1, H), None,
                                       gamma=self.agent.gamma, lam=0.0, use_done_mask=False)
        return hadv.view(-1), htarget.view(-1)

    def _her_targets_gae(self, h, hgoal):
        """her_gae: GAE(lambda) over the relabelled records, scanned along each run and cut at its end (ppo_run_ends +
        ppo_gae_runs) -> (adv, critic target).  A record that breaks the run pattern is a run of its own: its after-state
        is evaluated and its advantage is its one-step delta.  The done mask follows the agent as for the rollout rows;
        without it a run's last record keeps its bootstrap like every done record of the reference (PPO.py:113)."""
        ag = self.agent
        hv = self._values_one(h["t"], h["n"], hgoal, False)
        broken = torch.zeros(1, dtype=torch.int32, device=self.device)
        run_end = ppo_ops.run_ends(h["t"], h["n"], h["goal"], h["done"], broken)
        hnv = self._next_values_from_neighbours(h, hgoal, hv, torch.nonzero(run_end).view(-1))
        self.her_out_of_pattern = int(broken)
        self.her_targets = dict(value=hv, next_value=hnv, run_end=run_end)
        hadv, htarget, hret = ppo_ops.gae_runs(h["reward"], hv, hnv, h["done"], run_end, ag.gamma, ag.gae_lambda,
                                               ag.use_done_mask)
        return hadv, htarget if ag.gae_lambda == 0.0 else hret

    @torch.no_grad()
    def compute_targets(self):
        T, N = self.T, self.N
        total = T * N
        self.value_rows = 0
        idx = torch.arange(total, device=self.device)
        done = (self.term | self.trunc).contiguous()
        goal = self.sample_goal(idx // N, idx % N, self.goal1.expand(total, 2), done.view(-1))
        v, nv = self._values_rollout(goal, done) if self.reuse_next_values else self._values(idx // N, idx % N, goal)
        reward = self.reward_train if self.reward_norm is None else self.normalize_rewards()
        adv, target, ret = ppo_ops.gae(reward, v.view(T, N), nv.view(T, N), done, gamma=self.agent.gamma,
                                       lam=self.agent.gae_lambda, use_done_mask=self.agent.use_done_mask)
        critic_target = target if self.agent.gae_lambda == 0.0 else ret
        adv, critic_target = adv.view(-1), critic_target.view(-1)
        if self.her is not None and self.her["t"].numel():
            h = self.her                                          # relabelled records, with their own goals and rewards
            if self.reward_norm is not None and self._reward_norm_hindsight:
                h = dict(h, reward=self.reward_norm.apply(h["reward"]))      # a scaled copy: self.her stays raw
            hgoal = self.sample_goal(h["t"], h["n"], h["goal"], h["done"])
            if self.her_gae:
                hadv, htarget = self._her_targets_gae(h, hgoal)
            else:
                hadv, htarget = self._her_targets_one_step(h, hgoal)
            adv = torch.cat([adv, hadv])
            critic_target = torch.cat([critic_target, htarget])
        if self.agent.normalize_adv:
            if self.agent.grad_sync is not None and torch.distributed.is_initialized() and \
                    torch.distributed.get_world_size() > 1:
                from .. import dist as twdist
                twdist.global_adv_norm_(adv)                      # statistics over every rank's samples
            else:
                ppo_ops.adv_norm_(adv)
        return adv, critic_target

    def update(self, permutations=None):
        ag = self.agent
        T, N = self.T, self.N
        prior_coef = 0.0 if self.prior is None else self.prior_coef()
        if prior_coef != 0.0 and self._moves_at != self.env_steps:
            raise RuntimeError("enable_prior(): call label_expert() after collect() and before update()")
        her_prior = prior_coef != 0.0 and self.prior["hindsight"] and self.her is not None and self.her["t"].numel() > 0
        if her_prior and self._her_moves_of is not self.her:
            raise RuntimeError("enable_prior(hindsight=True): call label_expert() after relabel() and before update()")
        t_begin = time.perf_counter() if self.time_phases else 0.0
        adv, target = self.compute_targets()
        if self.time_phases:
            torch.cuda.synchronize(self.device)
            t_targets = time.perf_counter()
        total = adv.numel()                                           # rollout samples + relabelled records
        base = torch.arange(T * N, device=self.device)
        smp_t, smp_n = (base // N).int(), (base % N).int()
        smp_goal = self.sample_goal(smp_t, smp_n, self.goal1.expand(T * N, 2), (self.term | self.trunc).view(-1))
        if total > T * N:
            h = self.her
            smp_goal = torch.cat([smp_goal, self.sample_goal(h["t"], h["n"], h["goal"], h["done"])])
            smp_t = torch.cat([smp_t, h["t"]])
            smp_n = torch.cat([smp_n, h["n"]])
        flat = smp_t.long() * N + smp_n.long()                        # action / old log-prob are those of (t, n)
        act, logp = self.action.view(-1)[flat], self.logp.view(-1)[flat]
        smp_moves = None
        if prior_coef != 0.0:
            from .. import minigrid_nav as nav
            # hindsight records get mask 0 (their goal is not the field's source) unless they were labelled under
            # their own goals: enable_prior(hindsight=True)
            smp_moves = torch.zeros(total, dtype=torch.uint8, device=self.device)
            smp_moves[:T * N] = nav.to_policy_mask(self.expert_moves, self.act_probs.shape[-1]).view(-1)
            if her_prior:
                smp_moves[T * N:] = nav.to_policy_mask(self.her_moves, self.act_probs.shape[-1])
        ag.actor.train(); ag.critic.train()
        la = lv = None
        local_steps = n_steps = -(-total // self.minibatch)
        synced = ag.grad_sync is not None and torch.distributed.is_initialized()
        if synced:
            n_steps = agree_on_steps(n_steps, self.device)
        diag = self.update_diag
        if diag is not None:                                          # one row per epoch, cleared with one fill
            if diag["stats"].shape[0] != ag.K_epochs:
                diag["stats"] = torch.zeros((ag.K_epochs, ppo_ops.UPDATE_STATS_WORDS), dtype=torch.float64, device=self.device)
            else:
                diag["stats"].zero_()
            diag["epochs_run"] = 0
        for ep in range(ag.K_epochs):
            if diag is not None:
                ag.stats_row = diag["stats"][ep]
            perm = (torch.randperm(total) if permutations is None else torch.as_tensor(permutations[ep])).to(self.device)
            if synced:
                perm = padded_permutation(perm, n_steps, self.minibatch)
            done_steps = 0
            for i in range(0, perm.numel(), self.minibatch):
                idx = perm[i:i + self.minibatch]
                n_valid = None
                if self.fixed_shapes and idx.numel() < self.minibatch <= perm.numel():
                    # the epoch's last, partial minibatch: padded to the full shape with masked rows (same loss and
                    # gradients; a new batch size would cost a MIOpen kernel search -- seconds -- every update)
                    n_valid = idx.numel()
                    idx = torch.cat([idx, idx[torch.arange(self.minibatch - n_valid, device=self.device) % n_valid]])
                with torch.no_grad():
                    x0, p0 = self._policy_x(smp_t[idx], smp_n[idx], False)
                if smp_moves is None:
                    la, lv = ag.minibatch_step_x(x0, p0, self.goal_input(smp_goal[idx], False), act[idx],
                                                 logp[idx].view(-1, 1), adv[idx].view(-1, 1), target[idx].view(-1, 1), n_valid)
                else:
                    la, lv = ag.minibatch_step_x(x0, p0, self.goal_input(smp_goal[idx], False), act[idx],
                                                 logp[idx].view(-1, 1), adv[idx].view(-1, 1), target[idx].view(-1, 1), n_valid,
                                                 prior=(smp_moves[idx], prior_coef))
                done_steps += 1
            assert done_steps == n_steps or not synced, (done_steps, n_steps)
            if diag is not None:
                diag["epochs_run"] = ep + 1
                if diag["target_kl"] is not None:                     # the one two-element host read per epoch
                    k3, rows = diag["stats"][ep, [ppo_ops.UPDATE_STATS["k3_sum"], ppo_ops.UPDATE_STATS["rows"]]].tolist()
                    if synced:                                        # every rank stops at the same epoch
                        from .. import dist as twdist
                        k3, rows = twdist.sum_over_ranks([k3, rows], self.device)
                    if kl_stop(k3, rows, diag["target_kl"]):
                        break
        if diag is not None:
            ag.stats_row = None
        if ag.use_lr_decay:
            ag.scheduler_actor.step(); ag.scheduler_critic.step()
        if self.time_phases:
            torch.cuda.synchronize(self.device)
            t_end = time.perf_counter()
            self.last_update_timing = {"targets_s": t_targets - t_begin, "epochs_s": t_end - t_targets,
                                       "epoch_s": (t_end - t_targets) / max(1, ag.K_epochs), "samples": int(total)}
        self.her = None
        if self.prior is not None:
            self.prior["updates"] += 1
        return la, lv

    def her_switch(self, her, score):
        """The reference's hysteresis (train_ppo.py:128-131): relabelling off above 0.1, on again below 0."""
        return False if score > 0.1 else (True if score < 0.0 else her)

    def running_score(self, score):
        """EMA of episode returns (train_ppo.py:140: score <- 0.99 score + 0.01 ep_reward per finished episode),
        applied once per rollout with the mean return of the E episodes that ended in it."""
        done = (self.term | self.trunc) != 0
        E = int(done.sum())
        if E == 0:
            return score
        mean_ret = float(self.reward.sum()) / E
        k = 0.99 ** E
        return score * k + mean_ret * (1.0 - k)

    def account_episodes(self):
        """Account the rollout just collected (call after collect(), before carry_over()): per-episode returns and
        lengths carried across rollout boundaries, the summary of the episodes that ended in it, and the reference's
        running score folded over them one by one (train_ppo.py:140).  Two launches, no host synchronisation."""
        if self.episodes is None:
            from ..episode_stats import EpisodeTracker
            self.episodes = EpisodeTracker(self.N, self.device, n_actions=5)
        self.episodes.account(self.reward, self.term, self.trunc, self.action)

    def episode_stats(self):
        """EpisodeTracker.read() of the last accounted rollout plus mean_neg_logp = -mean log pi(a|s) of its actions."""
        if self.episodes is None:
            raise RuntimeError("episode_stats() before account_episodes()")
        out = self.episodes.read()
        out["mean_neg_logp"] = float(-self.logp.mean())
        return out

    # ------------------------------------------------------------------ exploration bonuses
    def enable_bonus(self, kinds=("state",), scope="shared", scale=1.0, form="sqrt"):
        """Shape the training reward with the reference's count-based bonuses (gym_minigrid/wrappers.py:34-102):
        shape_rewards() then fills `reward_train`, which compute_targets(), relabel() and carry_over() use, while
        `reward` -- and with it account_episodes(), running_score(), stats() and the HER switch -- stays extrinsic.
        The action bonus keys on the env's action (policy index 4 is env action 6) and on the agent's direction after
        the step, copied out of the engine's records once per step.  scope "episode": the counts of an env clear at each
        of its episode ends (`term | trunc`); form "first" (that scope only) pays the first visit of an episode alone."""
        from ..exploration import BonusTracker
        self.bonus = BonusTracker(self.N, self.device, kinds, scope, scale, 17, 17, 7, form)
        self.reward_train = torch.zeros_like(self.reward)
        if "action" in self.bonus.kinds:
            self.dir = torch.zeros((self.T, self.N), dtype=torch.int32, device=self.device)
            self._dir_now = self.engine.dir_view()
            self._graph = None
        return self.bonus

    def env_actions(self):
        """The rollout's actions as the env saw them (Env_transact.env_action: policy index 4 -> actions.done = 6)."""
        return torch.where(self.action == 4, 6, self.action).to(torch.int32)

    def shape_rewards(self):
        """reward_train <- reward + bonuses of the rollout just collected (call after collect(), before relabel());
        terminated steps are counted but keep their reward, as under the reference's Env_transact.step.  One
        ppo_bonus_scan call, no host synchronisation.  Without enable_bonus(): reward_train is reward, nothing runs."""
        if self.bonus is not None and self.bonus.scope == "episode":
            self.bonus.account(self.pos[4:4 + self.T], self.env_actions(), self.reward, dir=self.dir, out=self.reward_train,
                               keep=self.term, terminated=self.term, truncated=self.trunc)
        elif self.bonus is not None:
            self.bonus.account(self.pos[4:4 + self.T], self.env_actions(), self.reward, self.term, dir=self.dir,
                               out=self.reward_train)
        elif self.shaping is not None:        # enable_shaping() without a bonus: the potential is added to a copy
            self.reward_train.copy_(self.reward)
        return self.reward_train

    def bonus_stats(self):
        """BonusTracker.read() plus the mean bonus per kind over the last shaped rollout and their sum, "mean"."""
        if self.bonus is None:
            raise RuntimeError("bonus_stats() before enable_bonus()")
        out = self.bonus.read()
        out["mean_by_kind"] = {k: float(b.mean()) for k, b in self.bonus.bonus.items()}
        out["mean"] = sum(out["mean_by_kind"].values())
        return out

    def account_visits(self, her=None):
        """Count the cells of the rollout just collected (call after collect(), before carry_over(), outside the
        rollout's graph capture): the reference's heatmap matrix over the after-step positions (heatmap.py:58-81), with
        the hindsight records `her` (relabel()'s result) counted like its appended copies, and the distinct cells each
        episode covered, carried across rollout boundaries.  No host synchronisation."""
        if self.visits is None:
            from ..visitation import VisitTracker
            self.visits = VisitTracker(self.N, self.device, 17, 17)
        self.visits.account(self.pos[4:4 + self.T], self.term, self.trunc, her)

    def visit_stats(self):
        """VisitTracker.read() of the last accounted rollout."""
        if self.visits is None:
            raise RuntimeError("visit_stats() before account_visits()")
        return self.visits.read()

    # ------------------------------------------------------------------ distance to the goal
    def account_distance(self):
        """Distance to the goal at every step of the rollout just collected (call after collect(), before
        carry_over()): ONE field of the static map per env -- balls and patrols passable, the wall drops as they stand
        at the rollout's end -- and one lookup over the after-step positions; `goal_dist` uint16[T, N] afterwards
        (65535 where a wall has dropped onto the cell since).  Under in-kernel auto-reset the terminal state is gone
        but the terminal position is in the stream.  Two launches, no host synchronisation."""
        from .. import minigrid_nav as nav
        if self.goal_dist is None:
            self.goal_dist = torch.empty((self.T, self.N), dtype=nav.DIST_DTYPE, device=self.device)
        self._static_field(reuse=False)
        nav.lookup(self.nav_field, self.pos[4:4 + self.T], 17, 17, out=self.goal_dist)
        return self.goal_dist

    def _static_field(self, reuse):
        """`nav_field` <- the field of the static map (balls and patrols passable, the wall drops as they stand now);
        reuse: keep the one already computed for this rollout."""
        from .. import minigrid_nav as nav
        if self.nav_field is None:
            self.nav_field = torch.empty((self.N, 289), dtype=nav.DIST_DTYPE, device=self.device)
        if not (reuse and self._nav_field_at == self.env_steps):
            self.engine.distance_field(pass_types=nav.PASS_DEFAULT | nav.PASS_BALL, agent=False, out=self.nav_field)
            self._nav_field_at = self.env_steps
        return self.nav_field

    def _timed_field(self, reuse):
        """`timed_field` <- TwoarmyEngine.timed_field's six phases per env (the row-8 balls on their schedule, the engine's
        planes as they stand), one buffer and one launch per rollout for every feature that reads it; reuse: keep the one
        already computed for this rollout -- a pure function of the planes and the cached schedule, neither of which
        changes between collect() and carry_over()."""
        from .. import minigrid_nav as nav
        if self.timed_field is None:
            self.timed_field = torch.empty((self.N, nav.TWOARMY_PERIOD, 289), dtype=nav.DIST_DTYPE, device=self.device)
        if not (reuse and self._timed_field_at == self.env_steps):
            self.engine.timed_field(agent=False, out=self.timed_field)
            self._timed_field_at = self.env_steps
        return self.timed_field

    def distance_stats(self):
        """{"end_mean", "end_min": over the done steps of the last accounted rollout, "mean": over all its steps,
        "cut_off": steps whose cell is unreachable in the field (left out of the three)}; None where nothing counts.
        One device-to-host copy."""
        if self.goal_dist is None:
            raise RuntimeError("distance_stats() before account_distance()")
        from .. import minigrid_nav as nav
        d = nav.as_int(self.goal_dist).long()
        ok = d != nav.UNREACHABLE
        end = ok & ((self.term | self.trunc) != 0)
        v = torch.stack([end.sum(), (d * end).sum(), torch.where(end, d, nav.UNREACHABLE).min(), ok.sum(), (d * ok).sum(),
                         (~ok).sum()]).cpu().tolist()
        return {"end_mean": v[1] / v[0] if v[0] else None, "end_min": v[2] if v[0] else None,
                "mean": v[4] / v[3] if v[3] else None, "cut_off": v[5]}

    # ------------------------------------------------------------------ path efficiency per episode
    def account_paths(self, timed=False):
        """Rate the episodes of the rollout just collected against the shortest paths (call after collect(), before
        carry_over(), outside the rollout's graph capture; include/minigrid_nav.h, "Path efficiency"): the static-map field
        exactly as account_distance() / label_expert() take it (reused if one of them already ran for this rollout), or with
        timed=True TwoarmyEngine.timed_field's (the row-8 balls on their schedule, the age of a step being its clock),
        then PathTracker.account() over the positions before and after each step, episode starts at the reset position.
        The field is the map as it stands when the rollout ends; an episode that spans a rollout boundary keeps the start
        distance it got from the earlier rollout's field.  A field launch and the tracker's two calls, no host
        synchronisation."""
        from .. import minigrid_nav as nav
        T, timed = self.T, bool(timed)
        if self.paths is None:
            self.paths = nav.PathTracker(self.N, self.device, 17, 17, period=nav.TWOARMY_PERIOD if timed else 1)
        if timed != (self.paths.period > 1):
            raise RuntimeError("account_paths(timed=%s) after account_paths(timed=%s): one tracker, one field" % (timed, not timed))
        field = self._timed_field(reuse=True) if timed else self._static_field(reuse=True)
        self.paths.account(field, self.pos[3:3 + T], self.pos[4:4 + T], self.term, self.trunc, self.age[:-1], self.init_pos)

    def path_stats(self):
        """PathTracker.read() of the last accounted rollout."""
        if self.paths is None:
            raise RuntimeError("path_stats() before account_paths()")
        return self.paths.read()

    # ------------------------------------------------------------------ shortest-path prior
    def enable_prior(self, coef, decay=1.0, hindsight=False, timed=False, hindsight_timed=False):
        """Train the actor with the shortest-path prior: update() adds coef * decay^(updates done) times the set-valued
        imitation term (ppo_ops.prior_loss) over the optimal-move sets label_expert() makes to the actor's loss of every
        minibatch.  Rewards, returns, targets, advantages, the critic, the running score and the HER switch are
        untouched (this is no reward shaping).  coef = 0: label and report only, no loss launch.  From here on the
        rollout also keeps its acting distributions (T x N x 5 floats) for prior_stats().  hindsight=True: the
        hindsight records of relabel() are labelled too, each under its own goal (one mg_nav_goal_moves launch in
        label_expert()), and enter the term with those labels instead of an empty mask.  timed=True: the rollout's own
        labels come from the time-expanded search (TwoarmyEngine.timed_field, mg_nav_timed_moves): the row-8 balls follow
        their schedule and "wait one step" (the stay bit, policy index 4) is a label where the gap is closed; this
        switch leaves the hindsight labels those of the static map.  hindsight_timed=True (needs hindsight=True,
        independent of timed): the hindsight records are labelled by the time-expanded search under their own goals
        instead (one mg_nav_timed_goal_moves launch in place of the mg_nav_goal_moves one), the age of a step being its
        clock."""
        import inspect
        if hindsight_timed and not hindsight:
            raise ValueError("enable_prior(hindsight_timed=True) needs hindsight=True")
        if "probs_out" not in inspect.signature(self.agent.act_batch).parameters or self.cache_predictions:
            raise ValueError("the shortest-path prior needs the plain PPO agent's act_batch")
        self.prior = {"coef": float(coef), "decay": float(decay), "updates": 0, "hindsight": bool(hindsight),
                      "timed": bool(timed), "hindsight_timed": bool(hindsight_timed)}
        self.her_moves = self.her_dist = self._her_moves_of = None
        self.act_probs = torch.zeros((self.T, self.N, 5), dtype=torch.float32, device=self.device)
        self._moves_at = -1
        self._graph = None                    # a captured rollout does not write act_probs
        return self.prior

    def prior_coef(self):
        """The coefficient of the next update(): coef * decay^(updates done)."""
        return self.prior["coef"] * self.prior["decay"] ** self.prior["updates"]

    def label_expert(self):
        """Optimal-move sets of every acting state of the rollout just collected (call after collect(), before
        carry_over()): the static-map field exactly as account_distance() takes it (reused if that already ran for this
        rollout) and ONE mg_nav_optimal_moves launch over the positions before each step, episode starts at the reset
        position; `expert_moves` uint8[T, N] (bits: left, right, up, down, stay) and `expert_dist` uint16[T, N]
        afterwards.  With enable_prior(hindsight=True) and records from relabel() (call it first): ONE
        mg_nav_goal_moves launch more labels every hindsight record under its own goal, on the engine's planes as they
        stand and the same static map; `her_moves` uint8[R] and `her_dist` uint16[R] afterwards.  No host
        synchronisation.  With enable_prior(timed=True) the field is TwoarmyEngine.timed_field's (six phases per env, the
        engine's planes as they stand) and the labels are mg_nav_timed_moves', the age of a step being its clock.  With
        enable_prior(hindsight_timed=True) the launch over the hindsight records is mg_nav_timed_goal_moves instead
        (TwoarmyEngine.timed_goal_moves): the same records, positions, ages and reset position, the balls on their
        schedule."""
        from .. import minigrid_nav as nav
        T, N = self.T, self.N
        timed = self.prior is not None and self.prior["timed"]
        if self.expert_moves is None:
            self.expert_moves = torch.empty((T, N), dtype=torch.uint8, device=self.device)
            self.expert_dist = torch.empty((T, N), dtype=nav.DIST_DTYPE, device=self.device)
        if timed:                             # the same two launches: a field of six phases, labels by the age as clock
            nav.timed_moves(self._timed_field(reuse=True), self.pos[3:3 + T], 17, 17, self.age[:-1], self.init_pos,
                            out=self.expert_moves, dist_out=self.expert_dist)
        else:
            self._static_field(reuse=True)
            nav.optimal_moves(self.nav_field, self.pos[3:3 + T], 17, 17, age=self.age[:-1], init_pos=self.init_pos,
                              out=self.expert_moves, dist_out=self.expert_dist)
        self._moves_at = self.env_steps
        self.her_moves = self.her_dist = self._her_moves_of = None
        if self.prior is not None and self.prior["hindsight"] and self.her is not None and self.her["t"].numel():
            if self.prior["hindsight_timed"]:
                self.her_moves, self.her_dist = self.engine.timed_goal_moves(
                    self.her, self.pos[3:3 + T], self.age[:-1], self.init_pos)
            else:
                self.her_moves, self.her_dist = self.engine.goal_moves(
                    self.her, self.pos[3:3 + T], self.age[:-1], self.init_pos, pass_types=nav.PASS_DEFAULT | nav.PASS_BALL)
            self._her_moves_of = self.her                     # these labels belong to these records
        return self.expert_moves

    def prior_stats(self):
        """How the policy that ACTED in the last labelled rollout stands to the expert: {"agree": share of the labelled
        steps whose taken action is an optimal move, "opt_mass": mean probability it put on the optimal moves,
        "labelled": steps with a non-empty move set, "coef": the coefficient of the next update(), "her_labelled":
        hindsight records with a non-empty move set under their own goal, "her_agree": the share of those whose TAKEN
        action is an optimal move towards that goal -- how direct the relabelled trajectories are; no opt_mass for them:
        the acting distribution was conditioned on the other goal}; None where nothing is labelled (the two her_ fields:
        without labelled records).  One device-to-host copy."""
        if self.prior is None or self.expert_moves is None:
            raise RuntimeError("prior_stats() before enable_prior() and label_expert()")
        from .. import minigrid_nav as nav
        A = self.act_probs.shape[-1]
        mask = nav.to_policy_mask(self.expert_moves, A).to(torch.int32)
        lab = mask != 0
        hit = ((mask >> self.action) & 1) != 0
        bits = ((mask.unsqueeze(-1) >> torch.arange(A, device=self.device, dtype=torch.int32)) & 1).double()
        p = self.act_probs.double()
        mass = (p * bits).sum(-1) / p.sum(-1)
        sums = [lab.sum().double(), (hit & lab).sum().double(), torch.where(lab, mass, 0.0).sum()]
        her = self.her_moves is not None and self._her_moves_of is self.her
        if her:
            h = self.her
            hmask = nav.to_policy_mask(self.her_moves, A).to(torch.int32)
            hact = self.action.view(-1)[h["t"].long() * self.N + h["n"].long()]
            sums += [(hmask != 0).sum().double(), (((hmask >> hact) & 1) != 0).sum().double()]
        v = torch.stack(sums).cpu().tolist()
        n, hn = int(v[0]), int(v[3]) if her else 0
        return {"agree": v[1] / n if n else None, "opt_mass": v[2] / n if n else None, "labelled": n,
                "coef": self.prior_coef(), "her_labelled": hn if her else None, "her_agree": v[4] / hn if hn else None}

    # ------------------------------------------------------------------ potential-based reward shaping
    def enable_shaping(self, scale, hindsight=True, timed=False, hindsight_timed=False):
        """Shape the training reward with the distance to the goal as a potential (include/minigrid_nav.h, "Reward
        shaping"): shape_potential() then adds F = gamma * Phi(s') - Phi(s), Phi = -scale * distance, to `reward_train`,
        which compute_targets() and carry_over() use, while `reward` -- and with it account_episodes(), running_score(),
        stats() and the HER switch -- stays extrinsic.  gamma is the agent's, and the terminal rule (Phi(s') = 0 at a done
        step) follows agent.use_done_mask.  hindsight=True: the records of relabel() are shaped too, each under its own
        goal (one mg_nav_goal_shape launch over her["reward"]).  timed=True: the rollout's potential comes from the
        time-expanded field (TwoarmyEngine.timed_field, the age of a step being its clock); this switch leaves the records
        on the static map.  hindsight_timed=True (needs hindsight=True, independent of timed, as in enable_prior): the
        records are shaped by the time-expanded search under their own goals instead (one mg_nav_timed_goal_shape launch
        in place of the mg_nav_goal_shape one) -- with timed=True both halves of a critic batch then use one potential
        around the balls.  Call order in a rollout: collect() -> shape_rewards() -> relabel() -> shape_potential() ->
        label_expert() / compute_targets() -> carry_over()."""
        scale = float(scale)
        if not math.isfinite(scale) or scale <= 0.0:
            raise ValueError("enable_shaping(): scale must be a positive finite number, got %r" % scale)
        if not isinstance(hindsight, bool) or not isinstance(timed, bool) or not isinstance(hindsight_timed, bool):
            raise ValueError("enable_shaping(): hindsight, timed and hindsight_timed are booleans")
        if hindsight_timed and not hindsight:
            raise ValueError("enable_shaping(hindsight_timed=True) needs hindsight=True")
        self.shaping = {"scale": scale, "hindsight": hindsight, "timed": timed, "hindsight_timed": hindsight_timed}
        if self.reward_train is self.reward:
            self.reward_train = torch.zeros_like(self.reward)
        self.shape_f = torch.zeros((self.T, self.N), dtype=torch.float32, device=self.device)
        self.shape_mask = torch.zeros((self.T, self.N), dtype=torch.uint8, device=self.device)
        self.her_shape_f = self.her_shape_mask = self._her_shape_of = None
        self._shaped_at = -1
        return self.shaping

    @torch.no_grad()
    def shape_potential(self, expect_her=False):
        """reward_train += F of the rollout just collected, in place, under the env's goal: the static-map field of
        account_distance() / label_expert() (reused if one of them already ran for this rollout), or with
        enable_shaping(timed=True) TwoarmyEngine.timed_field's, and ONE mg_nav_shape launch over the positions before and
        after each step; `shape_f` float32[T, N] and `shape_mask` uint8[T, N] afterwards.  With hindsight shaping and
        records from relabel(): ONE mg_nav_goal_shape launch more shapes her["reward"] in place, each record under its
        own goal on the static map -- relabel() copied reward_train into the records BEFORE the env goal's term was
        added, so no record carries another goal's term; `her_shape_f` and `her_shape_mask` afterwards.  With
        enable_shaping(hindsight_timed=True) that launch is mg_nav_timed_goal_shape instead
        (TwoarmyEngine.timed_goal_shape): the same records, positions, ages, reset position, terminal flag and in-place
        her["reward"], the balls on their schedule.  Call after
        shape_rewards() and relabel(), once per rollout; expect_her=True (the caller relabels this rollout) makes a call
        before relabel() an error.  No host synchronisation."""
        from .. import minigrid_nav as nav
        if self.shaping is None:
            raise RuntimeError("shape_potential() before enable_shaping()")
        if self._shaped_at == self.env_steps:
            raise RuntimeError("shape_potential() ran already for this rollout: the potential would be added twice")
        if expect_her and self.shaping["hindsight"] and self._relabel_at != self.env_steps:
            raise RuntimeError("enable_shaping(hindsight=True): call relabel() before shape_potential()")
        T = self.T
        sh = self.shaping
        before, after = self.pos[3:3 + T], self.pos[4:4 + T]
        zero_terminal = bool(self.agent.use_done_mask)
        done = (self.term | self.trunc).contiguous() if zero_terminal else None
        field = self._timed_field(reuse=True) if sh["timed"] else self._static_field(reuse=True)
        nav.shape(field, before, after, 17, 17, reward=self.reward_train, age=self.age[:-1], init_pos=self.init_pos,
                  done=done, scale=sh["scale"], gamma=self.agent.gamma, zero_terminal=zero_terminal, out=self.reward_train,
                  shaping_out=self.shape_f, mask_out=self.shape_mask)
        self._shaped_at = self.env_steps
        self.her_shape_f = self.her_shape_mask = self._her_shape_of = None
        if sh["hindsight"] and self.her is not None and self.her["t"].numel():
            if sh["hindsight_timed"]:
                _, self.her_shape_f, self.her_shape_mask = self.engine.timed_goal_shape(
                    self.her, before, after, self.age[:-1], self.init_pos, scale=sh["scale"], gamma=self.agent.gamma,
                    zero_terminal=zero_terminal, out=self.her["reward"])
            else:
                _, self.her_shape_f, self.her_shape_mask = self.engine.goal_shape(
                    self.her, before, after, self.age[:-1], self.init_pos, pass_types=nav.PASS_DEFAULT | nav.PASS_BALL,
                    scale=sh["scale"], gamma=self.agent.gamma, zero_terminal=zero_terminal, out=self.her["reward"])
            self._her_shape_of = self.her                     # these terms belong to these records
        return self.reward_train

    def shaping_stats(self):
        """{"mean": mean F over the shaped steps of the last shaped rollout, "unshaped": the share of its steps left
        unshaped, "her_mean", "her_unshaped": the same two over the hindsight records (None without shaped records)};
        None where nothing counts.  One device-to-host copy."""
        if self.shaping is None or self._shaped_at < 0:
            raise RuntimeError("shaping_stats() before enable_shaping() and shape_potential()")
        m = self.shape_mask != 0
        sums = [m.sum().double(), torch.where(m, self.shape_f, 0.0).double().sum()]
        her = self.her_shape_f is not None and self._her_shape_of is self.her
        if her:
            hm = self.her_shape_mask != 0
            sums += [hm.sum().double(), torch.where(hm, self.her_shape_f, 0.0).double().sum()]
        v = torch.stack(sums).cpu().tolist()
        total, n = self.T * self.N, int(v[0])
        hn, htotal = (int(v[2]), int(self.her_shape_f.numel())) if her else (0, 0)
        return {"mean": v[1] / n if n else None, "unshaped": 1.0 - n / total,
                "her_mean": v[3] / hn if hn else None, "her_unshaped": 1.0 - hn / htotal if htotal else None}

    # ------------------------------------------------------------------ reward normalisation
    def enable_reward_norm(self, clip=10.0, hindsight=True):
        """Divide the training reward by the running standard deviation of its discounted return (RewardNormalizer;
        include/twoarmy_ppo.h, "Reward normalisation"), gamma being the agent's as it stands now.  compute_targets() then
        advances the statistics once per rollout from `reward_train` as the bonus and shaping stages left it, and hands
        ppo_ops.gae a SCALED COPY, `reward_scaled`, clamped to [-clip, clip] (clip <= 0 or inf: no clamp).
        hindsight=True: the records' rewards, the 0.9 of a record's last step included, enter their targets through a
        scaled copy as well, by the same statistics.  Nothing else changes: `reward`, `reward_train`, the history window
        of relabel(), her["reward"], account_episodes(), running_score() and stats() keep raw values, so no reward is
        scaled twice and relabel() never copies a scaled one.  With several ranks every rank keeps its own statistics."""
        from ..exploration import RewardNormalizer
        if not isinstance(hindsight, bool):
            raise ValueError("enable_reward_norm(): hindsight is a boolean")
        try:
            self.reward_norm = RewardNormalizer(self.N, self.agent.gamma, clip, self.device)
        except ValueError as ex:
            raise ValueError("enable_reward_norm(): %s" % ex) from None
        self._reward_norm_hindsight = hindsight
        self._reward_norm_at = -1             # env_steps when the statistics last advanced: once per rollout
        self.reward_scaled = torch.zeros_like(self.reward)
        return self.reward_norm

    @torch.no_grad()
    def normalize_rewards(self):
        """`reward_scaled` <- reward_train of the rollout just collected, scaled and clamped; the first call after a
        collect() counts that rollout's returns first.  Call after shape_rewards() / shape_potential() (compute_targets()
        does).  Three launches, no host synchronisation."""
        if self.reward_norm is None:
            raise RuntimeError("normalize_rewards() before enable_reward_norm()")
        if self._reward_norm_at != self.env_steps:
            self.reward_norm.update(self.reward_train, self.term, self.trunc)
            self._reward_norm_at = self.env_steps
        return self.reward_norm.apply(self.reward_train, out=self.reward_scaled)

    def reward_norm_stats(self):
        """RewardNormalizer.read(): {"count", "mean", "var", "std", "scale"} of the returns seen so far.  One
        device-to-host copy."""
        if self.reward_norm is None:
            raise RuntimeError("reward_norm_stats() before enable_reward_norm()")
        return self.reward_norm.read()

    # ------------------------------------------------------------------ update diagnostics
    def enable_update_stats(self, target_kl=None):
        """Keep the diagnostics of every update() on the device: one float64[16] row per epoch (float64[K_epochs, 16],
        cleared with one fill at the start of update()), which the loss launch of every minibatch of that epoch adds to
        (agent.stats_row -> ppo_ops.ppo_losses(stats=), ppo_loss_fwd_bwd_stats in include/twoarmy_ppo.h): entropy, the
        approximate KL between the acting and the updated policy, the share of clipped samples, how much of the targets'
        variance the critic explains.  Losses, gradients and parameters are the same bits as without it.
        target_kl: after an epoch whose approx_kl exceeds it, the remaining epochs of that update are skipped (kl_stop);
        their rows stay zero and the LR schedulers step once per update as before.  This costs ONE two-element host read
        per epoch (a synchronisation; without target_kl update() adds none).  With a process group of several ranks k3_sum
        and rows are summed over the ranks first (dist.sum_over_ranks, one more small all-reduce per epoch), so every rank
        stops at the same epoch and takes part in the same gradient all-reduces."""
        if target_kl is not None and not (math.isfinite(float(target_kl)) and float(target_kl) >= 0.0):
            raise ValueError("enable_update_stats(): target_kl must be a finite number >= 0 or None, got %r" % (target_kl,))
        self.update_diag = {"stats": torch.zeros((self.agent.K_epochs, ppo_ops.UPDATE_STATS_WORDS), dtype=torch.float64,
                                                 device=self.device),
                            "target_kl": None if target_kl is None else float(target_kl), "epochs_run": 0}
        return self.update_diag

    def update_stats(self):
        """ppo_ops.update_stats_read() of the last update(): {"per_epoch": its dict of arrays over the K_epochs rows (rows
        of skipped epochs are zero, their means NaN), "epochs_run", and the values of the last epoch that ran under the
        plain key names (rows, calls, entropy, approx_kl, approx_kl_k1, clip_frac, ratio_dev_max, explained_variance,
        saturated_frac, top_mass)}.  One device-to-host copy."""
        if self.update_diag is None or self.update_diag["epochs_run"] == 0:
            raise RuntimeError("update_stats() before enable_update_stats() and update()")
        per = ppo_ops.update_stats_read(self.update_diag["stats"])
        n = self.update_diag["epochs_run"]
        out = {k: float(v[n - 1]) for k, v in per.items()}
        out.update(per_epoch=per, epochs_run=n)
        return out

    def stats(self):
        done = (self.term | self.trunc) != 0
        out = {"env_steps": self.env_steps, "episodes": int(done.sum()), "successes": int(self.term.sum()),
               "mean_reward": float(self.reward.mean())}
        if self.update_diag is not None and self.update_diag["epochs_run"]:
            out.update({k: v for k, v in self.update_stats().items() if k != "per_epoch"})
        return out
