"""Count-based exploration bonuses on the device: the reference's StateBonus / ActionBonus wrappers
(gym_minigrid/wrappers.py:69-102 and :34-66, `reward += 1 / math.sqrt(count)`) for N envs at once.  One ppo_bonus_scan
call per rollout (include/twoarmy_ppo.h) and no host synchronisation until read().

scope "env": one count table per env, N independent copies of the reference's wrapper.  scope "shared": one table for
all envs of this process, a time step counted as simultaneous (every env standing on a key in one row gets the bonus of
the count that includes the whole row).  With several ranks every rank keeps its own tables.

scope "episode": the env scope with counts that clear at each episode end (ppo_bonus_scan_episode), the per-episode
counts of RIDE / NovelD / AGAC; form "sqrt" pays scale / sqrt(count), form "first" pays scale at the first visit of a key
within the episode and nothing after it.

RewardNormalizer, below BonusTracker: the answer to what scale such a bonus should have -- the training reward divided by
the running standard deviation of its discounted return."""
import numpy as np
import torch

from . import ppo_ops

KINDS = ("state", "action")
SCOPES = tuple(ppo_ops.BONUS_SCOPES) + ("episode",)


class BonusTracker:
    def __init__(self, num_envs, device, kinds=("state",), scope="env", scale=1.0, width=17, height=17, n_actions=7,
                 form="sqrt"):
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        assert kinds and all(k in KINDS for k in kinds), "kinds: a non-empty subset of %s" % (KINDS,)
        assert scope in SCOPES
        if form not in ppo_ops.BONUS_FORMS:
            raise ValueError("form: one of %s, got %r" % (tuple(ppo_ops.BONUS_FORMS), form))
        if form != "sqrt" and scope != "episode":
            raise ValueError('form=%r needs scope="episode": a lifetime count has one first visit ever' % (form,))
        self.N, self.device = int(num_envs), torch.device(device)
        self.kinds = tuple(k for k in KINDS if k in kinds)
        self.scope, self.scale, self.form = scope, float(scale), form
        self.width, self.height, self.n_actions = int(width), int(height), int(n_actions)
        self.cells = self.width * self.height
        words = (ppo_ops.bonus_episode_words,) if scope == "episode" else (ppo_ops.bonus_table_words, scope)
        self.tables = {k: torch.zeros(words[0](k, *words[1:], width, height, n_actions, self.N), dtype=torch.int32,
                                      device=self.device) for k in self.kinds}
        self.mask = sum(ppo_ops.BONUS_KINDS[k] for k in self.kinds)
        self.workspace = None                                                # sized by the first account()
        self.bonus = {}                                                      # kind -> f32[T,N] of the last account()

    def reset_counts(self):
        for t in self.tables.values():
            t.zero_()

    def account(self, pos, action, reward, terminated=None, dir=None, dir_ptr=None, out=None, keep=None, truncated=None):
        """Shape one rollout: pos [T,N,2] (y, x) after each step, action / reward [T,N], terminated u8[T,N] (its steps
        are counted but keep their reward: Env_transact.step sets it to 0.9 above the wrappers) -- or one step: [N,2],
        [N].  dir: the agent's direction after each step, [T,N] / [N], or dir_ptr (see ppo_ops.bonus_scan).  Returns the
        shaped reward (`out`, which may be `reward`, or a new tensor); self.bonus holds the bonuses per kind.
        scope "episode": terminated and truncated u8[T,N] are the episode ends and both are required; the steps that keep
        their reward are keep u8[T,N] (None: none).  In the other scopes keep, where given, stands for terminated."""
        episodic = self.scope == "episode"
        if episodic and (terminated is None or truncated is None):
            raise ValueError('scope="episode" cuts the counts at the episode ends: pass terminated= and truncated=')
        if not episodic:
            keep = terminated if keep is None else keep
        one = pos.dim() == 2
        if one:
            pos, action, reward = pos.view(1, -1, 2), action.view(1, -1), reward.view(1, -1)
            keep, terminated, truncated = (None if t is None else t.view(1, -1) for t in (keep, terminated, truncated))
            dir = None if dir is None else dir.view(1, -1)
            out = None if out is None else out.view(1, -1)
        T, N = reward.shape
        assert N == self.N, "tracker made for %d envs, got %d" % (self.N, N)
        for k in self.kinds:
            if k not in self.bonus or self.bonus[k].shape[0] != T:
                self.bonus[k] = torch.empty((T, N), dtype=torch.float32, device=self.device)
        if self.scope == "shared":
            need = ppo_ops.bonus_workspace_bytes(self.mask, self.scope, T, self.width, self.height, self.n_actions) // 4
            if self.workspace is None or self.workspace.numel() < need:
                self.workspace = torch.empty(need, dtype=torch.int32, device=self.device)
        out = torch.empty_like(reward) if out is None else out
        common = dict(state_table=self.tables.get("state"), action_table=self.tables.get("action"), scale=self.scale,
                      width=self.width, height=self.height, n_actions=self.n_actions, keep=keep, dir=dir, dir_ptr=dir_ptr,
                      bonus_state=self.bonus.get("state"), bonus_action=self.bonus.get("action"), reward_out=out)
        if episodic:
            ppo_ops.bonus_scan_episode(pos, action, reward, terminated, truncated, form=self.form, **common)
        else:
            ppo_ops.bonus_scan(pos, action, reward, scope=self.scope, workspace=self.workspace, **common)
        return out[0] if one else out

    def counts(self, kind):
        """The table of one kind as a device tensor [N, K] (env scope, int32 holding uint32) or [K] int64 (shared); in
        the episode scope the running episodes' counts, int64[N, K], decoded from the stamped words (a new tensor)."""
        t = self.tables[kind]
        if self.scope == "episode":
            return ppo_ops.bonus_episode_counts(t, self.N)
        return t.view(self.N, -1) if self.scope == "env" else t.view(torch.int64)

    def read(self, per_env=False):
        """Count maps as numpy int64, summed over envs in env scope (on the device): "state" [height, width], "action"
        [4, n_actions, height, width], and the counts of invalid steps in "other" = {kind: int}; per_env=True (env and
        episode scope) keeps the envs apart instead: a leading [N] on every map, "other" = {kind: int64[N]}.  In the
        episode scope the counts are those of the running episodes.  One device-to-host copy."""
        by_env = self.scope in ("env", "episode")
        per_env = per_env and by_env
        parts = []
        for k in self.kinds:
            c = self.counts(k)
            if by_env:
                c = c.to(torch.int64) & 0xFFFFFFFF                            # the words are uint32
                c = c if per_env else c.sum(0)
            parts.append(c.reshape(-1))
        host = torch.cat(parts).cpu().numpy()
        out, other, at = {}, {}, 0
        lead = self.N if per_env else 1
        for k in self.kinds:
            K = self.cells + 1 if k == "state" else self.cells * 4 * self.n_actions + 1
            tab = host[at:at + lead * K].reshape(lead, K)
            at += lead * K
            if k == "state":
                maps = tab[:, :-1].reshape(lead, self.height, self.width)
            else:
                maps = tab[:, :-1].reshape(lead, self.height, self.width, 4, self.n_actions).transpose(0, 3, 4, 1, 2)
            out[k] = np.ascontiguousarray(maps if per_env else maps[0])
            other[k] = tab[:, -1].copy() if per_env else int(tab[0, -1])
        out["other"] = other
        return out


class RewardNormalizer:
    """Rewards divided by the running standard deviation of the discounted return (gym's NormalizeReward, the baselines'
    VecNormalize) for N envs on the device: update() advances the moments by one rollout (ppo_ops.reward_norm_update),
    apply() scales any reward array by the scale that stands when the launch runs and clamps it to [-clip, clip]
    (ppo_ops.reward_norm_apply; clip <= 0 or inf: no clamp).  It owns the envs' running returns `ret_carry` f64[N], `stats`
    f64[4] = (count, mean, M2, scale) and the workspace; no host synchronisation until read().  With several ranks every
    rank keeps its own statistics."""

    def __init__(self, num_envs, gamma, clip=10.0, device="cuda"):
        gamma, clip = float(gamma), float(clip)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("gamma must lie in [0, 1], got %r" % (gamma,))
        if clip != clip:
            raise ValueError("clip must be a number (<= 0 or inf: no clamp), got %r" % (clip,))
        self.N, self.gamma, self.clip, self.device = int(num_envs), gamma, clip, torch.device(device)
        self.ret_carry = torch.zeros(self.N, dtype=torch.float64, device=self.device)
        self.stats = torch.zeros(4, dtype=torch.float64, device=self.device)
        self.workspace = torch.empty(ppo_ops.reward_norm_workspace(self.N), dtype=torch.float64, device=self.device)

    def update(self, reward, terminated, truncated):
        """Count the returns of one rollout: reward f32[T,N], terminated / truncated u8[T,N].  Returns stats."""
        assert reward.shape[1:] == (self.N,), "normalizer made for %d envs, got %s" % (self.N, tuple(reward.shape))
        return ppo_ops.reward_norm_update(reward, terminated, truncated, self.gamma, self.ret_carry, self.stats, self.workspace)

    def apply(self, reward, out=None):
        """reward (f32, any shape) scaled and clamped -> out (reward itself: in place; None: a new tensor)."""
        return ppo_ops.reward_norm_apply(reward, self.stats, self.clip, out)

    def read(self):
        return ppo_ops.reward_norm_read(self.stats)

    def reset(self):
        """Forget everything: nothing seen, every env at an episode's start."""
        self.stats.zero_()
        self.ret_carry.zero_()

    def state_dict(self):
        return {"ret_carry": self.ret_carry.clone(), "stats": self.stats.clone(), "gamma": self.gamma, "clip": self.clip}

    def load_state_dict(self, state):
        """Continue from a state_dict(): the tensors are copied into this normalizer's own, in place (a captured launch
        keeps reading them); gamma and clip are taken over."""
        assert tuple(state["ret_carry"].shape) == (self.N,) and tuple(state["stats"].shape) == (4,)
        self.ret_carry.copy_(state["ret_carry"])
        self.stats.copy_(state["stats"])
        self.gamma, self.clip = float(state["gamma"]), float(state["clip"])
