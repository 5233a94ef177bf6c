"""Vectorised trainer of the self-orientation agent (reference soa/train_SoA.py:123-272 +
Self_orientation_agent.py:166-294) on the time-major rollout of VecPPOTrainer.

The reference keeps 9-frame window records (3 history frames, the acting state at index 3, 5 future frames) so that
`update_orientation` can read the position three states ahead (p[:,6] - p[:,3]) and `update_policy` the
orientation sample of the next step (f[:,1]).  Here both are index arithmetic on the rollout: f is stored per step,
the next step's f is f[t+1] (or f[t] again when the episode ends at t, which is what the reference's four terminal
window shifts produce), and the 3-step displacement is pos[min(t+3, end+1)] - pos[t] inside the episode.
The orientation head trains, like the reference (train_SoA.py:206-224, 243-262), only on trajectories that reach
their goal: episodes that terminated, plus the hindsight records of the others.

Success replay (train_SoA.py:200-205, 243-262): the reference keeps the window records of the last 99 episodes that
reached the goal in a FIFO that survives its buffer resets, and trains the orientation head on that FIFO at every
update.  Here the FIFO holds materialised orientation samples (4-frame stacks, positions, goal, displacement) of
goal-reaching episodes of EARLIER rollouts; an update trains on every goal-reaching episode of the current rollout
plus the newest (99 - that number, if positive) episodes of the FIFO -- exactly the reference's "last 99 successes"
whenever the current rollout holds at most 99 of them (its scale), and never fewer samples than the rollout offers.

Orientation prior (enable_orientation_prior, off by default): the head is asked where the agent stands three steps ahead, and
the distance fields know where a shortest path leads in three steps (include/minigrid_nav.h, "Look-ahead").  label_ahead()
labels every acting state of the rollout (and, on request, every hindsight record under its own goal) with that set of
displacements, and update_orientation adds the set-valued term minigrid_nav.ahead_loss to the NLL of every minibatch."""
import collections
import math

import torch

from .. import ppo_ops
from .ppo_vec import VecPPOTrainer


class VecSoATrainer(VecPPOTrainer):
    def __init__(self, agent, engine, rollout_steps=128, minibatch=4096, value_chunk=16384, frame_codes=False,
                 orient_minibatch=None):
        super().__init__(agent, engine, rollout_steps, minibatch, value_chunk, frame_codes)
        T, N = self.T, self.N
        self.future = torch.zeros((T + 1, N, 2), dtype=torch.float32, device=self.device)     # f of the acting state t
        self.pending_future = None                       # f already drawn for the first state of the next rollout
        self.orient_minibatch = int(orient_minibatch or minibatch)
        self.replay_episodes = 99                        # len(fp_terminate_buffer) > 99 -> pop(0), train_SoA.py:204-205
        self._replay = collections.deque()               # oldest first; one dict of sample tensors per episode
        self.orient_prior = None                         # look-ahead prior of the head, made by enable_orientation_prior()

    # ------------------------------------------------------------------ rollout
    @torch.no_grad()
    def collect(self, uniforms=None):
        """uniforms: f32[T+1, N, 3] or None (row T feeds the orientation draw of the state after the last step)."""
        T, N = self.T, self.N
        ag = self.agent
        self._pred_valid = False                         # this rollout loop does not fill the prediction cache
        for t in range(T + 1):
            k = torch.full((N,), t + 3, dtype=torch.int32, device=self.device)
            s4, p4 = ppo_ops.gather_stack(self.frames, self.pos, k, self.n_all, self.age[t], self.init_frame, self.init_pos)
            u = None if uniforms is None else uniforms[t]
            if t == T:                                   # only the orientation draw: it belongs to the next rollout's step 0
                _, _, self.future[T] = ag.act_batch_soa(s4, p4, self.goal, u, orient_only=True)
                break
            forced = self.pending_future if t == 0 else None
            a, logp, f = ag.act_batch_soa(s4, p4, self.goal, u, future=forced)
            self.action[t], self.logp[t], self.future[t] = a, logp, f
            out = {"obs": None, "matrix": self.frames[t + 4], "pos": self.pos[t + 4], "reward": self.reward[t],
                   "terminated": self.term[t], "truncated": self.trunc[t]}
            self.engine.step(a, out, autoreset=True, policy_idx=True)
            if self.dir is not None:
                self.dir[t].copy_(self._dir_now)
            done = (self.term[t] | self.trunc[t]) != 0
            self.age[t + 1] = torch.where(done, torch.zeros_like(self.age[t]), self.age[t] + 1)
        self.pending_future = self.future[T].clone()
        self.env_steps += T * N

    # ------------------------------------------------------------------ goals seen by the networks
    def sample_goal(self, t_idx, n_idx, goal2, done):
        """[goal(2), f of the acting state(2), f of the next state(2)]; the next state's f repeats the current one
        when the (possibly relabelled) episode ends at this step."""
        t, n = t_idx.long(), n_idx.long()
        f_cur = self.future[t, n]
        f_next = torch.where((done != 0).view(-1, 1), f_cur, self.future[t + 1, n])
        return torch.cat([goal2, f_cur, f_next], dim=1)

    def goal_input(self, goal, after):
        return torch.cat([goal[:, 0:2], goal[:, 4:6] if after else goal[:, 2:4]], dim=1)

    # ------------------------------------------------------------------ orientation head
    @torch.no_grad()
    def _episode_ends(self):
        """(end long[T, N]: the step at which the episode of (t, n) ends, >= T when it does not end in this rollout;
        success bool[T, N]: it ends by reaching the goal).  No host synchronisation."""
        T, N = self.T, self.N
        dev = self.device
        done = ((self.term | self.trunc) != 0)
        tt = torch.arange(T, device=dev).view(T, 1).expand(T, N)
        big = torch.full((T, N), T + 8, device=dev, dtype=torch.long)
        end = torch.flip(torch.cummin(torch.flip(torch.where(done, tt, big), [0]), 0).values, [0])   # end step of the episode
        ended = end < T
        success = ended & (self.term.long().gather(0, end.clamp(max=T - 1)) != 0)
        return end, success

    @torch.no_grad()
    def orientation_samples(self):
        """(t, n, goal2, displacement) of the samples the orientation head trains on."""
        T, N = self.T, self.N
        dev = self.device
        end, success = self._episode_ends()
        t_idx, n_idx = torch.nonzero(success, as_tuple=True)
        u = end[t_idx, n_idx]
        goal2 = self.goal1.expand(t_idx.numel(), 2)
        self._n_success_samples = int(t_idx.numel())
        self._success_key = u * N + n_idx                                            # episode id: (end step, env)
        if self.her is not None and self.her["t"].numel():
            h = self.her
            hs = torch.nonzero(h["done"]).view(-1)                                   # last record of every relabelled prefix
            j = torch.searchsorted(hs, torch.arange(h["t"].numel(), device=dev))
            hu = h["t"].long()[hs[j]]
            # hindsight records of episodes that did NOT reach the real goal (train_SoA.py:217-219)
            keep = ~success[h["t"].long(), h["n"].long()]
            if self.orient_prior is not None:
                self._her_sample_rec = torch.nonzero(keep).view(-1)                  # the record behind every hindsight sample
            t_idx = torch.cat([t_idx, h["t"].long()[keep]])
            n_idx = torch.cat([n_idx, h["n"].long()[keep]])
            u = torch.cat([u, hu[keep]])
            goal2 = torch.cat([goal2, h["goal"][keep]])
        # state index s (before step s) of env n sits in self.pos[s + 3]; the first state of an episode is the reset state
        start = self.age[:-1].long()[t_idx, n_idx] == 0
        p_now = torch.where(start.view(-1, 1), self.init_pos.view(1, 2), self.pos[t_idx + 3, n_idx])
        p_fut = self.pos[torch.minimum(t_idx + 3, u + 1) + 3, n_idx]
        return t_idx.int(), n_idx.int(), goal2, p_fut - p_now

    # ------------------------------------------------------------------ success replay (train_SoA.py:200-205)
    @torch.no_grad()
    def replay_samples(self, n_current_episodes):
        """Materialised samples of the newest (replay_episodes - n_current_episodes) remembered episodes, or None."""
        k = max(0, self.replay_episodes - int(n_current_episodes))
        eps = list(self._replay)[-k:] if k else []
        if not eps:
            return None
        keys = ("s0", "p0", "goal2", "disp") + (("ahead",) if self.orient_prior is not None else ())
        return {key: torch.cat([e[key] for e in eps]) for key in keys}

    @torch.no_grad()
    def remember_successes(self, t_idx, n_idx, goal2, disp, ahead=None):
        """Push the goal-reaching episodes of this rollout (the first _n_success_samples samples) into the FIFO in
        completion order (end step, then env); only the newest `replay_episodes` are kept.  ahead (with the orientation
        prior): the look-ahead label of every sample, remembered with it."""
        ns = self._n_success_samples
        if ns == 0:
            return
        keys, inv = torch.unique(self._success_key, return_inverse=True)              # ascending = completion order
        first = max(0, keys.numel() - self.replay_episodes)
        sel = torch.nonzero(inv >= first).view(-1)
        s0, p0 = self._stacks(t_idx[:ns][sel], n_idx[:ns][sel], after=False)
        ep = (inv[sel] - first).cpu()
        order = torch.argsort(ep, stable=True)
        counts = torch.bincount(ep, minlength=keys.numel() - first).tolist()
        sel_o = order.to(self.device)
        s0, p0, g2, dp = s0[sel_o], p0[sel_o], goal2[:ns][sel][sel_o], disp[:ns][sel][sel_o]
        la = None if ahead is None else ahead[:ns][sel][sel_o]
        off = 0
        for c in counts:
            self._replay.append(dict(s0=s0[off:off + c].clone(), p0=p0[off:off + c].clone(),
                                     goal2=g2[off:off + c].clone(), disp=dp[off:off + c].clone()))
            if la is not None:
                self._replay[-1]["ahead"] = la[off:off + c].clone()
            off += c
        while len(self._replay) > self.replay_episodes:
            self._replay.popleft()

    # ------------------------------------------------------------------ look-ahead prior of the orientation head
    def enable_orientation_prior(self, coef, decay=1.0, steps=3, timed=False, hindsight=False, every_state=False,
                                 hindsight_timed=False):
        """Train the orientation head with the look-ahead prior: update_orientation adds coef * decay^(updates done) times
        minigrid_nav.ahead_loss -- minus the log of the mass the head's two 7-way distributions put on the displacements a
        shortest path reaches in `steps` steps -- to the NLL of every minibatch, over the labels label_ahead() makes.  The
        actor, the critic, rewards and targets are untouched.  coef = 0: label and report only.  timed=True: the rollout's
        labels come from the time-expanded field (TwoarmyEngine.timed_field, the age of a step being its clock).
        hindsight=True: the hindsight records of relabel() are labelled too, each under its own goal on the static map (one
        mg_nav_goal_ahead launch in label_ahead()); without it a hindsight sample has no label and no prior term.
        hindsight_timed=True (needs hindsight=True): that one launch is mg_nav_timed_goal_ahead instead -- the records are
        labelled over (cell, phase) with the schedule of timed=True's field, so that they wait for the balls as the rollout's
        labels do.
        every_state=True (with coef > 0): every rollout step that is no success sample joins the sample set as a prior-only
        row under the env's goal; it carries no NLL, and the NLL mean stays over the NLL rows.  From here on the success
        FIFO remembers the label of every sample."""
        coef, decay, steps = float(coef), float(decay), int(steps)
        if not (math.isfinite(coef) and coef >= 0.0):
            raise ValueError("enable_orientation_prior(): coef must be a finite number >= 0, got %r" % coef)
        if not 1 <= steps <= 3:
            raise ValueError("enable_orientation_prior(): steps must be 1, 2 or 3, got %r" % steps)
        if hindsight_timed and not hindsight:
            raise ValueError("enable_orientation_prior(): hindsight_timed=True needs hindsight=True")
        self.orient_prior = {"coef": coef, "decay": decay, "updates": 0, "steps": steps, "timed": bool(timed),
                             "hindsight": bool(hindsight), "every_state": bool(every_state) and coef > 0.0,
                             "hindsight_timed": bool(hindsight_timed)}
        self.expert_ahead = self.ahead_dist = None
        self.her_ahead = self.her_ahead_dist = self._her_ahead_of = None
        self._her_sample_rec = None
        self._ahead_at = -1
        for e in self._replay:                           # episodes remembered before the prior: no label
            e.setdefault("ahead", torch.zeros(e["disp"].shape[0], dtype=torch.int64, device=self.device))
        return self.orient_prior

    def orientation_prior_coef(self):
        """The coefficient of the next update_orientation(): coef * decay^(updates done)."""
        return self.orient_prior["coef"] * self.orient_prior["decay"] ** self.orient_prior["updates"]

    @torch.no_grad()
    def label_ahead(self):
        """Look-ahead labels of every acting state of the rollout just collected (call after collect() and, when
        relabelling, after relabel(); before carry_over()): the static-map field of account_distance() (reused if it ran
        for this rollout), or with timed=True TwoarmyEngine.timed_field's, and ONE mg_nav_ahead launch over the positions
        before each step, episode starts at the reset position; `expert_ahead` int64[T, N] and `ahead_dist` uint16[T, N]
        afterwards.  With hindsight=True and records from relabel(): ONE mg_nav_goal_ahead launch more, on the engine's
        planes as they stand and the same static map -- with hindsight_timed=True ONE mg_nav_timed_goal_ahead launch in its
        place, over (cell, phase) with the age of a record's step as its clock; `her_ahead` int64[R] and `her_ahead_dist`
        uint16[R] afterwards.  No host synchronisation."""
        from .. import minigrid_nav as nav
        op = self.orient_prior
        if op is None:
            raise RuntimeError("label_ahead() before enable_orientation_prior()")
        T, N = self.T, self.N
        if self.expert_ahead is None:
            self.expert_ahead = torch.empty((T, N), dtype=nav.AHEAD_DTYPE, device=self.device)
            self.ahead_dist = torch.empty((T, N), dtype=nav.DIST_DTYPE, device=self.device)
        if op["timed"]:
            field = self._timed_field(reuse=True)
        else:
            field = self._static_field(reuse=True)
        nav.ahead(field, self.pos[3:3 + T], 17, 17, steps=op["steps"], age=self.age[:-1], init_pos=self.init_pos,
                  out=self.expert_ahead, dist_out=self.ahead_dist)
        self._ahead_at = self.env_steps
        self.her_ahead = self.her_ahead_dist = self._her_ahead_of = None
        if op["hindsight"] and self.her is not None and self.her["t"].numel():
            if op["hindsight_timed"]:
                self.her_ahead, self.her_ahead_dist = self.engine.timed_goal_ahead(
                    self.her, self.pos[3:3 + T], self.age[:-1], self.init_pos, steps=op["steps"])
            else:
                self.her_ahead, self.her_ahead_dist = self.engine.goal_ahead(
                    self.her, self.pos[3:3 + T], self.age[:-1], self.init_pos, steps=op["steps"],
                    pass_types=nav.PASS_DEFAULT | nav.PASS_BALL)
            self._her_ahead_of = self.her                     # these labels belong to these records
        return self.expert_ahead

    @torch.no_grad()
    def orientation_prior_stats(self):
        """{"labelled": rollout steps with a non-empty label, "agree": the share of those whose drawn orientation sample
        future[t] lies in the label, "her_labelled": hindsight samples (records of episodes that did not reach the real
        goal) with a non-empty label under their own goal, "her_realised": the share of those whose realised displacement
        lies in the label, "coef": the coefficient of the next update}; None where nothing is labelled (the two her_
        fields: without labelled records).  One device-to-host copy."""
        if self.orient_prior is None or self.expert_ahead is None:
            raise RuntimeError("orientation_prior_stats() before enable_orientation_prior() and label_ahead()")
        T, N = self.T, self.N
        lab = self.expert_ahead
        cls = (self.future[:T] + 3).long().clamp(0, 6)
        hit = ((lab >> (cls[..., 0] * 7 + cls[..., 1])) & 1) != 0
        on = lab != 0
        sums = [on.sum(), (hit & on).sum()]
        her = self.her_ahead is not None and self._her_ahead_of is self.her
        if her:
            h = self.her
            t, n = h["t"].long(), h["n"].long()
            end, success = self._episode_ends()
            R = t.numel()                                     # the last record of a record's relabelled prefix: the next done one
            at = torch.where(h["done"] != 0, torch.arange(R, device=self.device), torch.full_like(t, R - 1))
            hu = t[torch.flip(torch.cummin(torch.flip(at, [0]), 0).values, [0])]
            start = self.age[:-1].long()[t, n] == 0
            p_now = torch.where(start.view(-1, 1), self.init_pos.view(1, 2), self.pos[t + 3, n])
            p_fut = self.pos[torch.minimum(t + 3, hu + 1).clamp(max=T) + 3, n]
            hc = (p_fut - p_now + 3).long().clamp(0, 6)
            hon = (self.her_ahead != 0) & ~success[t, n]
            hhit = ((self.her_ahead >> (hc[:, 0] * 7 + hc[:, 1])) & 1) != 0
            sums += [hon.sum(), (hhit & hon).sum()]
        v = torch.stack(sums).cpu().tolist()
        n_lab, hn = int(v[0]), int(v[2]) if her else 0
        return {"labelled": n_lab, "agree": v[1] / n_lab if n_lab else None, "her_labelled": hn if her else None,
                "her_realised": v[3] / hn if hn else None, "coef": self.orientation_prior_coef()}

    @torch.no_grad()
    def _prior_rows(self, t_idx, n_idx, goal2, disp):
        """The sample set of update_orientation with the prior on: (t, n, goal2, displacement, label int64, nll bool or
        None).  A rollout sample gets expert_ahead[t, n], a hindsight sample her_ahead of its record (0 without labelled
        records); with every_state the rollout steps that are no success sample follow as prior-only rows (nll False)."""
        if self._ahead_at != self.env_steps:
            raise RuntimeError("enable_orientation_prior(): call label_ahead() for this rollout before update()")
        ns = self._n_success_samples
        lab = torch.zeros(t_idx.numel(), dtype=torch.int64, device=self.device)
        lab[:ns] = self.expert_ahead[t_idx[:ns].long(), n_idx[:ns].long()]
        if t_idx.numel() > ns and self.her_ahead is not None and self._her_ahead_of is self.her:
            lab[ns:] = self.her_ahead[self._her_sample_rec]
        if not self.orient_prior["every_state"]:
            return t_idx, n_idx, goal2, disp, lab, None
        _, success = self._episode_ends()
        et, en = torch.nonzero(~success, as_tuple=True)
        ne = et.numel()
        nll = torch.cat([torch.ones(t_idx.numel(), dtype=torch.bool, device=self.device),
                         torch.zeros(ne, dtype=torch.bool, device=self.device)])
        self._n_prior_only = int(ne)
        return (torch.cat([t_idx, et.int()]), torch.cat([n_idx, en.int()]), torch.cat([goal2, self.goal1.expand(ne, 2)]),
                torch.cat([disp, torch.zeros((ne, 2), dtype=disp.dtype, device=self.device)]),
                torch.cat([lab, self.expert_ahead[et, en]]), nll)

    def update_orientation(self, permutations=None):
        ag = self.agent
        t_idx, n_idx, goal2, disp = self.orientation_samples()
        prior = self.orient_prior is not None
        lab = nll_rows = None
        coef = 0.0
        if prior:
            t_idx, n_idx, goal2, disp, lab, nll_rows = self._prior_rows(t_idx, n_idx, goal2, disp)
            coef = self.orientation_prior_coef()
        n_rollout = t_idx.numel()
        n_cur_eps = int(torch.unique(self._success_key).numel()) if self._n_success_samples else 0
        rep = self.replay_samples(n_cur_eps)
        n_rep = 0 if rep is None else int(rep["disp"].shape[0])
        total = n_rollout + n_rep                            # sample ids: [0, n_rollout) rollout, then the replay
        local_steps = n_steps = -(-total // self.orient_minibatch)
        synced = ag.grad_sync_orient is not None and torch.distributed.is_initialized()
        if synced:
            # EVERY rank joins this collective, also one without a single orientation sample (no success, no
            # hindsight record): it then takes part in each gradient all-reduce with zero gradients
            from .ppo_vec import agree_on_steps
            n_steps = agree_on_steps(n_steps, self.device)
        if n_steps == 0:
            return None
        ag.agent_position_preditor.train()
        loss = None
        for ep in range(ag.K_epochs_pre_agent_position):
            if total == 0:
                for _ in range(n_steps):
                    ag.orientation_idle_step()
                continue
            perm = (torch.randperm(total) if permutations is None else torch.as_tensor(permutations[ep])).to(self.device)
            if synced and n_steps > -(-perm.numel() // self.orient_minibatch):
                perm = perm[torch.arange(n_steps * self.orient_minibatch, device=self.device) % perm.numel()]
            done_steps = 0
            for i in range(0, perm.numel(), self.orient_minibatch):
                idx = perm[i:i + self.orient_minibatch]
                cur = idx[idx < n_rollout]
                s0, p0 = self._stacks(t_idx[cur], n_idx[cur], after=False)
                g2, dp = goal2[cur], disp[cur]
                la = lab[cur] if prior else None
                nr = nll_rows[cur] if nll_rows is not None else None
                if n_rep:
                    old = idx[idx >= n_rollout] - n_rollout
                    s0, p0 = torch.cat([s0, rep["s0"][old]]), torch.cat([p0, rep["p0"][old]])
                    g2, dp = torch.cat([g2, rep["goal2"][old]]), torch.cat([dp, rep["disp"][old]])
                    if prior:
                        la = torch.cat([la, rep["ahead"][old]])
                    if nr is not None:
                        nr = torch.cat([nr, torch.ones(old.numel(), dtype=torch.bool, device=self.device)])
                n_valid = None
                if self.fixed_shapes and idx.numel() < self.orient_minibatch:
                    # partial minibatch: padded to the full shape (or, for a sample set smaller than one minibatch, to
                    # the next power of two) with masked rows behind the real ones -- the sample count changes every
                    # update and every new conv batch size costs a MIOpen kernel search
                    full = self.orient_minibatch if perm.numel() >= self.orient_minibatch else \
                        max(64, 1 << (idx.numel() - 1).bit_length())
                    if full > idx.numel():
                        n_valid = idx.numel()
                        pad = torch.arange(full - n_valid, device=self.device) % n_valid
                        s0, p0 = torch.cat([s0, s0[pad]]), torch.cat([p0, p0[pad]])
                        g2, dp = torch.cat([g2, g2[pad]]), torch.cat([dp, dp[pad]])
                        if prior:                            # padding rows carry no label and no NLL
                            la = torch.cat([la, torch.zeros(full - n_valid, dtype=torch.int64, device=self.device)])
                        if nr is not None:
                            nr = torch.cat([nr, torch.zeros(full - n_valid, dtype=torch.bool, device=self.device)])
                with torch.no_grad():
                    x8 = ag.policy_input(s0)
                if prior:
                    loss = ag.orientation_step(x8, p0, g2, dp, n_valid, ahead=la, prior_coef=coef, nll_rows=nr)
                else:
                    loss = ag.orientation_step(x8, p0, g2, dp, n_valid)
                done_steps += 1
            assert done_steps == n_steps or not synced, (done_steps, n_steps)
        if ag.use_lr_decay:
            ag.scheduler_agent_position_preditor.step()
        self.remember_successes(t_idx, n_idx, goal2, disp, lab)
        if prior:
            self.orient_prior["updates"] += 1
        return loss

    def update(self, permutations=None, orient_permutations=None):
        """update_policy, then update_orientation (train_SoA.py:264-265); the hindsight records serve both."""
        her = self.her
        la, lv = super().update(permutations)
        self.her = her
        lo = self.update_orientation(orient_permutations)
        self.her = None
        self.last_orientation_loss = lo
        return la, lv
