"""gym.vector-style front end of the HIP engine: N Twoarmy envs stepped by one kernel launch.

  env = TwoarmyVecEnv("MiniGrid-twoarmy-17x17-v6", num_envs=4096)
  obs = env.reset()                                  # uint8 [N, V, V, 3] device tensor
  obs, reward, terminated, truncated, info = env.step(actions)      # actions: int tensor [N]

Semantics follow gym.vector with in-kernel auto-reset: for envs that finished, `obs` is the first
observation of the next episode and info["final_observation"] holds the terminal one (as a dense
tensor + info["_final_observation"] mask, no host sync).  `policy_actions=True` (default) takes the
policy's 5 indices (4 -> done) like Env_transact.env_action (reference soa/env_buffer.py:364-376).
Extra per-step tensors the reference computes in Python are fused into the same launch:
`env.state_matrix` [N,289] (matrix_env) and `env.agent_yx` [N,2] (data_env).
`env.render(env_index=None)` draws the RGB frames of the reference's get_full_render on the device (tile_size and
highlight are constructor arguments).
`record_episode_statistics=True` adds info["episode"] = {"r": float64 [N], "l": int32 [N]} and the mask
info["_episode"] like gym.vector's RecordEpisodeStatistics, accounted on the device (episode_stats.EpisodeTracker).
`record_visitation=True` adds info["visitation"] = {"cells": int32 [N], "first_visit": bool [N]} -- the distinct cells the
running episode has stood on and whether this step's cell is new to it -- with the mask info["_visitation"] = done (where
it is set, "cells" is the finished episode's coverage), and `env.visit_tracker` (visitation.VisitTracker) with the maps.
`state_bonus=True` / `action_bonus=True` make step() return the reward shaped by the reference's StateBonus / ActionBonus
wrappers (gym_minigrid/wrappers.py:34-102; `bonus_scope` "env" = one wrapper per env, "shared" = one count table for all
envs; `bonus_scale` 1.0 = the reference), counted on the device by `env.bonus_tracker` (exploration.BonusTracker);
info["reward_extrinsic"] keeps the env's own reward.  Episode statistics stay extrinsic.
"""
import torch

from .engine import TwoarmyEngine

_IDS = {"MiniGrid-twoarmy-17x17-v4": 4, "MiniGrid-twoarmy-17x17-v6": 6, "v4": 4, "v6": 6, 4: 4, 6: 6}


class TwoarmyVecEnv:
    def __init__(self, env_id="MiniGrid-twoarmy-17x17-v6", num_envs=4096, agent_view_size=17, device=None,
                 seed=9981, env_id0=0, policy_actions=True, autoreset=True, record_episode_statistics=False,
                 tile_size=17, highlight=False, record_visitation=False, state_bonus=False, action_bonus=False,
                 bonus_scope="env", bonus_scale=1.0):
        self.variant = _IDS[env_id]
        self.num_envs = int(num_envs)
        self.view_size = agent_view_size
        self.tile_size, self.highlight = int(tile_size), bool(highlight)
        self.policy_actions, self.autoreset = policy_actions, autoreset
        self.engine = TwoarmyEngine(self.variant, num_envs, agent_view_size, device=device, seed=seed, env_id0=env_id0)
        self.device = self.engine.device
        self._out = self.engine.alloc_outputs()
        self._init_obs = torch.empty((self.num_envs, agent_view_size, agent_view_size, 3), dtype=torch.uint8,
                                     device=self.device)
        self.engine.reset(obs=self._init_obs)                      # the reset observation is a constant of the task
        self.goal_yx = torch.tensor([2.0, 14.0], device=self.device).expand(self.num_envs, 2)
        self.single_observation_shape = (agent_view_size, agent_view_size, 3)
        self.single_action_n = 5 if policy_actions else 7
        self.episode_tracker = None
        if record_episode_statistics:
            from .episode_stats import EpisodeTracker
            self.episode_tracker = EpisodeTracker(self.num_envs, self.device, n_actions=self.single_action_n)
        self.visit_tracker = None
        if record_visitation:
            from .visitation import VisitTracker
            self.visit_tracker = VisitTracker(self.num_envs, self.device, 17, 17)

        self.bonus_tracker = None
        if state_bonus or action_bonus:
            from .exploration import BonusTracker
            kinds = (("state",) if state_bonus else ()) + (("action",) if action_bonus else ())
            self.bonus_tracker = BonusTracker(self.num_envs, self.device, kinds, bonus_scope, bonus_scale, 17, 17, 7)
            self._shaped = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)

    def reset(self):
        self.engine.reset(obs=self._out["obs"])
        if self.episode_tracker is not None:
            self.episode_tracker.reset()
        if self.visit_tracker is not None:
            self.visit_tracker.reset()
        return self._out["obs"]

    def step(self, actions):
        a = actions.to(device=self.device, dtype=torch.int32).contiguous()
        o = self._out
        self.engine.step(a, o, autoreset=self.autoreset, policy_idx=self.policy_actions)
        done = (o["terminated"] | o["truncated"]).bool()
        info = {}
        obs = o["obs"]
        if self.autoreset:
            info["final_observation"] = obs
            info["_final_observation"] = done
            obs = torch.where(done.view(-1, 1, 1, 1), self._init_obs, obs)
        if self.episode_tracker is not None:
            # gym.vector's RecordEpisodeStatistics: return / length of the episodes ending at this step (dense tensors,
            # valid where the mask is set; overwritten by the next step, like final_observation)
            tr = self.episode_tracker
            tr.account(o["reward"], o["terminated"], o["truncated"], a)
            info["episode"] = {"r": tr.ep_return[0], "l": tr.ep_length[0]}
            info["_episode"] = done
        if self.visit_tracker is not None:
            vt = self.visit_tracker
            vt.account(o["pos"], o["terminated"], o["truncated"])
            info["visitation"] = {"cells": vt.ep_cells[0], "first_visit": vt.first_visit[0].bool()}
            info["_visitation"] = done
        reward = o["reward"]
        if self.bonus_tracker is not None:
            # the wrappers see the env's action (policy index 4 is actions.done = 6) and the direction in the records
            env_a = torch.where(a == 4, 6, a).to(torch.int32) if self.policy_actions else a
            reward = self.bonus_tracker.account(o["pos"], env_a, o["reward"], dir_ptr=self.engine.dir_ptr(),
                                                out=self._shaped)
            info["reward_extrinsic"] = o["reward"]
        return obs, reward, o["terminated"].bool(), o["truncated"].bool(), info

    @property
    def state_matrix(self):
        return self._out["matrix"]

    @property
    def agent_yx(self):
        return self._out["pos"]

    def render(self, env_index=None, out=None):
        """uint8[n, 17*tile_size, 17*tile_size, 3] device tensor: the reference's get_full_render image of every env,
        or of the envs listed in env_index (int tensor / sequence), drawn on the device from the current state."""
        if env_index is not None:
            env_index = torch.as_tensor(env_index).to(device=self.device, dtype=torch.int32).contiguous().view(-1)
            if env_index.numel() == 0:
                return torch.empty((0, 17 * self.tile_size, 17 * self.tile_size, 3), dtype=torch.uint8, device=self.device)
        return self.engine.render(env_index=env_index, tile_size=self.tile_size, highlight=self.highlight, out=out)

    def close(self):
        self.engine.close()
