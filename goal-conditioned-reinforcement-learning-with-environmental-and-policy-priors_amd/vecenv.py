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
highlight are constructor arguments), `env.render_pov(env_index=None)` those of get_pov_render (the agent's view).
`record_episode_statistics=True` adds info["episode"] = {"r": float64 [N], "l": int32 [N]} and the mask
info["_episode"] like gym.vector's RecordEpisodeStatistics, accounted on the device (episode_stats.EpisodeTracker).
`record_visitation=True` adds info["visitation"] = {"cells": int32 [N], "first_visit": bool [N]} -- the distinct cells the
running episode has stood on and whether this step's cell is new to it -- with the mask info["_visitation"] = done (where
it is set, "cells" is the finished episode's coverage), and `env.visit_tracker` (visitation.VisitTracker) with the maps.
`state_bonus=True` / `action_bonus=True` make step() return the reward shaped by the reference's StateBonus / ActionBonus
wrappers (gym_minigrid/wrappers.py:34-102; `bonus_scope` "env" = one wrapper per env, "shared" = one count table for all
envs; `bonus_scale` 1.0 = the reference), counted on the device by `env.bonus_tracker` (exploration.BonusTracker);
info["reward_extrinsic"] keeps the env's own reward.  Episode statistics stay extrinsic.
`observation=` selects what reset() / step() return first and what info["final_observation"] holds (minigrid_obs, the
reference's observation wrappers, gym_minigrid/wrappers.py): "image" (default) the egocentric view uint8[N, V, V, 3];
"onehot" its one-hot uint8[N, V, V, 21]; "flat" float32[N, V*V*3 + 96*28], the image and the one-hot mission string;
"full" the whole grid with the agent stamped in, uint8[N, 17, 17, 3]; "symbolic" int32[N, 17, 17, 3] = (x, y, idx);
"rgb" the pixels of render(), uint8[N, 17*tile_size, 17*tile_size, 3] (RGBImgObsWrapper); "rgb_partial" the pixels of
render_pov(), uint8[N, V*tile_size, V*tile_size, 3] (RGBImgPartialObsWrapper).
`goal_direction="slope" | "angle"` adds info["goal_direction"] float64[N] (DirectionObsWrapper) for the state `obs`
shows, and info["final_goal_direction"] under auto-reset.  "onehot" and "flat" are passes over the engine's image;
"full", "symbolic", "rgb", "rgb_partial" and the goal direction read the engine's state after the step, so with autoreset=True the env steps
without the in-kernel reset, emits the final observation, resets the finished envs (engine.reset(mask=done)) and emits
again; everything else the env returns is what the default env returns.
`goal_distance=True` adds info["goal_distance"] int32[N], the moves on a shortest path from the agent to the goal through
the cells it may enter now (balls and patrols block; 65535 = cut off), and info["expert_action"] int32[N], the first move
of such a path as an ENV action (0 left, 1 right, 2 up, 3 down, 6 stay, -1 none): one more launch per step
(minigrid_nav, agent values only, no field).  Both describe the state the env returns: under auto-reset those of a done
env belong to the new episode, as the direction of a done step does for the action bonus.  The two tensors are the env's
own and are overwritten by the next step, like final_observation.  `goal_distance="timed"` fills the same two fields
from the time-expanded search instead (TwoarmyEngine.timed_field: the row-8 balls follow their schedule, the distance
counts moves AND waits, and expert_action 6 away from the goal means "wait one step"): one launch per step as well.
"""
import torch

from .engine import TwoarmyEngine

_IDS = {"MiniGrid-twoarmy-17x17-v4": 4, "MiniGrid-twoarmy-17x17-v6": 6, "v4": 4, "v6": 6, 4: 4, 6: 6}


class TwoarmyVecEnv:
    def __init__(self, env_id="MiniGrid-twoarmy-17x17-v6", num_envs=4096, agent_view_size=17, device=None,
                 seed=9981, env_id0=0, policy_actions=True, autoreset=True, record_episode_statistics=False,
                 tile_size=17, highlight=False, record_visitation=False, state_bonus=False, action_bonus=False,
                 bonus_scope="env", bonus_scale=1.0, observation="image", goal_direction=None, goal_distance=False):
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
        V = agent_view_size
        if observation not in ("image", "onehot", "full", "symbolic", "flat", "rgb", "rgb_partial"):
            raise ValueError("observation must be image, onehot, full, symbolic, flat, rgb or rgb_partial, not %r"
                             % (observation,))
        if goal_direction not in (None, "slope", "angle"):
            raise ValueError("goal_direction must be None, slope or angle, not %r" % (goal_direction,))
        self.observation, self.goal_direction = observation, goal_direction
        # the kinds read from the engine's state (not from its image) take the reset out of the step kernel
        self._state_obs = observation in ("full", "symbolic", "rgb", "rgb_partial") or goal_direction is not None
        self._goal_index = self._angle_table = self._state_src = None
        if observation != "image" or goal_direction is not None:
            from . import minigrid_obs
            self._mo = minigrid_obs
            N, d = self.num_envs, self.device
            if observation == "onehot":
                self.single_observation_shape = (V, V, minigrid_obs.ONEHOT_BITS)
                self._obs_buf = [torch.empty((N, V, V, minigrid_obs.ONEHOT_BITS), dtype=torch.uint8, device=d) for _ in range(2)]
                self._init_kind = minigrid_obs.onehot(self._init_obs)
            elif observation == "flat":
                self._tail = torch.from_numpy(minigrid_obs.mission_tail("get to the green goal square")).to(d)
                self.single_observation_shape = (V * V * 3 + self._tail.numel(),)
                self._obs_buf = [torch.empty((N,) + self.single_observation_shape, dtype=torch.float32, device=d) for _ in range(2)]
                self._init_kind = minigrid_obs.flat_obs(self._init_obs, self._tail)
            elif observation in ("full", "symbolic"):
                self.single_observation_shape = (17, 17, 3)
                dt = torch.uint8 if observation == "full" else torch.int32
                self._obs_buf = [torch.empty((N, 17, 17, 3), dtype=dt, device=d) for _ in range(2)]
            elif observation in ("rgb", "rgb_partial"):
                side = (17 if observation == "rgb" else V) * self.tile_size
                self.single_observation_shape = (side, side, 3)
                self._obs_buf = [torch.empty((N, side, side, 3), dtype=torch.uint8, device=d) for _ in range(2)]
            if goal_direction is not None:
                self._dir_buf = [torch.empty(N, dtype=torch.float64, device=d) for _ in range(2)]
                if goal_direction == "angle":
                    self._angle_table = minigrid_obs.angle_table(17, 17, d)
        assert goal_distance in (True, False, "timed"), "goal_distance: True, False or \"timed\""
        self.goal_distance = goal_distance
        if self.goal_distance:                            # distance, action, error: overwritten by the next step
            self._nav_buf = tuple(torch.empty(self.num_envs, dtype=torch.int32, device=self.device) for _ in range(3))
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
        if self.goal_direction is not None and self._goal_index is None:
            self._goal_index = self._mo.goal_index(self._state()[0], 17, 17)                   # once: goal_position is cached
        return self._emit(self._out["obs"], 0)

    # ------------------------------------------------------------------ observation kinds (minigrid_obs)
    def _emit(self, image, slot):
        """The chosen observation of the engine's image / current state, into buffer `slot` (0 = returned, 1 = final)."""
        kind = self.observation
        if kind == "image":
            return image
        mo, out = self._mo, self._obs_buf[slot]
        if kind == "onehot":
            return mo.onehot(image, out=out)
        if kind == "flat":
            return mo.flat_obs(image, self._tail, out=out)
        if kind == "rgb":
            return self.render(out=out)
        if kind == "rgb_partial":
            return self.render_pov(out=out)
        ty, co, agent = self._state()
        if kind == "full":
            return mo.full_obs(ty, co, None, 17, 17, *agent, out=out)
        return mo.symbolic_obs(ty, 17, 17, out=out)

    def _state(self):
        """(type plane, colour plane, agent views) of the engine: views that hold while the engine writes its state in place, as step() and
        reset() do (a pipelined rollout would swap the buffers; this env launches none)."""
        if self._state_src is None:
            self._state_src = self.engine.plane_views() + (self.engine.agent_views(),)
        return self._state_src

    def _emit_direction(self, slot):
        if self._goal_index is None:                     # once, as DirectionObsWrapper caches goal_position
            self._goal_index = self._mo.goal_index(self._state()[0], 17, 17)
        return self._mo.goal_direction(self._goal_index, 17, 17, *self._state()[2][:2], mode=self.goal_direction,
                                       table=self._angle_table, out=self._dir_buf[slot])

    def step(self, actions):
        a = actions.to(device=self.device, dtype=torch.int32).contiguous()
        o = self._out
        self.engine.step(a, o, autoreset=self.autoreset and not self._state_obs, policy_idx=self.policy_actions)
        done = (o["terminated"] | o["truncated"]).bool()
        info = {}
        obs = o["obs"]
        if self._state_obs:
            # the state after the step is the observation's source: final observation, reset of the finished envs, again
            if self.autoreset:
                info["final_observation"] = self._emit(obs, 1)
                info["_final_observation"] = done
                if self.goal_direction is not None:
                    info["final_goal_direction"] = self._emit_direction(1)
                self.engine.reset(mask=o["terminated"] | o["truncated"])
                obs = torch.where(done.view(-1, 1, 1, 1), self._init_obs, obs)
            obs = self._emit(obs, 0)
            if self.goal_direction is not None:
                info["goal_direction"] = self._emit_direction(0)
        elif self.observation != "image":
            obs = self._emit(obs, 1 if self.autoreset else 0)
            if self.autoreset:
                info["final_observation"] = obs
                info["_final_observation"] = done
                obs = torch.where(done.view((-1,) + (1,) * (obs.dim() - 1)), self._init_kind, obs)
        elif self.autoreset:
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
        if self.goal_distance:
            d, act, err = self._nav_buf
            field = self.engine.timed_field if self.goal_distance == "timed" else self.engine.distance_field
            field(want_field=False, agent_out=(d, act), error_out=err)
            info["goal_distance"], info["expert_action"] = d, act
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

    def render_pov(self, env_index=None, out=None):
        """uint8[n, V*tile_size, V*tile_size, 3] device tensor: the reference's get_pov_render image (the agent's view,
        V = agent_view_size) of every env, or of the envs listed in env_index, drawn on the device from the current state."""
        if env_index is not None:
            env_index = torch.as_tensor(env_index).to(device=self.device, dtype=torch.int32).contiguous().view(-1)
            if env_index.numel() == 0:
                side = self.view_size * self.tile_size
                return torch.empty((0, side, side, 3), dtype=torch.uint8, device=self.device)
        return self.engine.render_pov(env_index=env_index, tile_size=self.tile_size, out=out)

    def close(self):
        self.engine.close()
