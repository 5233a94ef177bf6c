"""Count-based exploration bonuses on the device: the reference's StateBonus / ActionBonus wrappers
(gym_minigrid/wrappers.py:69-102 and :34-66, `reward += 1 / math.sqrt(count)`) for N envs at once.  One ppo_bonus_scan
call per rollout (include/twoarmy_ppo.h) and no host synchronisation until read().

scope "env": one count table per env, N independent copies of the reference's wrapper.  scope "shared": one table for
all envs of this process, a time step counted as simultaneous (every env standing on a key in one row gets the bonus of
the count that includes the whole row).  With several ranks every rank keeps its own tables.

scope "episode": the env scope with counts that clear at each episode end (ppo_bonus_scan_episode), the per-episode
counts of RIDE / NovelD / AGAC; form "sqrt" pays scale / sqrt(count), form "first" pays scale at the first visit of a key
within the episode and nothing after it."""
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
