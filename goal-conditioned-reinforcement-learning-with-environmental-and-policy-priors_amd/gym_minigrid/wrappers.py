"""The one wrapper of the reference's gym_minigrid/wrappers.py that lies on the path:
ViewSizeWrapper (wrappers.py:428-460), the only place a 7x7 egocentric view exists.  The reference re-slices the
grid with gen_obs_grid(agent_view_size) after every reset / step; here that is one tw_gen_obs launch at the requested
view size on the wrapped env's device state.  StateBonus and ActionBonus (wrappers.py:69-102, 34-66), the reference's
count-based exploration bonuses, count on the device (exploration.BonusTracker, one ppo_bonus_scan launch per step);
thousands of envs take them through TwoarmyVecEnv(state_bonus=..., action_bonus=...) or train_ppo --bonus.  (The other
wrappers -- one-hot / RGB / flat / symbolic / direction observations -- are out of scope; a vector env takes its view
size as a constructor argument instead, see TwoarmyEngine / TwoarmyVecEnv.)"""
import numpy as np
import torch

from .minigrid import _Space


class ViewSizeWrapper:
    def __init__(self, env, agent_view_size=7):
        assert agent_view_size % 2 == 1
        assert agent_view_size >= 3
        self.env = env
        self.unwrapped = getattr(env, "unwrapped", env)
        self.agent_view_size = agent_view_size
        self.observation_space = dict(getattr(env, "observation_space", {}))
        self.observation_space["image"] = _Space(shape=(agent_view_size, agent_view_size, 3))

    def __getattr__(self, name):                       # everything else is the wrapped env's (gym.Wrapper behaviour)
        return getattr(self.env, name)

    def observation(self, obs):
        grid, vis_mask = self.unwrapped.gen_obs_grid(self.agent_view_size)
        return {**obs, "image": grid.encode(vis_mask)}

    def reset(self, **kwargs):
        out = self.env.reset(**kwargs)
        if kwargs.get("return_info"):
            return self.observation(out[0]), out[1]
        return self.observation(out)

    def step(self, action):
        obs, reward, terminated, truncated, info = self.env.step(action)
        return self.observation(obs), reward, terminated, truncated, info


class _Bonus:
    """`reward += 1 / math.sqrt(count)` with the count kept in a device table; `counts` is the reference's dict."""
    kind = None

    def __init__(self, env):
        from ..exploration import BonusTracker
        self.env = env
        self.unwrapped = getattr(env, "unwrapped", env)
        u = self.unwrapped
        self._device = u._eng.device
        self._tracker = BonusTracker(1, self._device, (self.kind,), "env", 1.0, u.width, u.height, len(u.actions))

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, **kwargs):
        return self.env.reset(**kwargs)

    def step(self, action):
        obs, reward, terminated, truncated, info = self.env.step(action)
        u, d = self.unwrapped, self._device
        pos = torch.tensor([[float(u.agent_pos[1]), float(u.agent_pos[0])]], dtype=torch.float32, device=d)
        shaped = self._tracker.account(pos, torch.tensor([int(action)], dtype=torch.int32, device=d),
                                       torch.tensor([reward], dtype=torch.float32, device=d),
                                       dir=torch.tensor([int(u.agent_dir)], dtype=torch.int32, device=d))
        return obs, float(shaped[0]), terminated, truncated, info

    @property
    def counts(self):
        maps = self._tracker.read()[self.kind]
        if self.kind == "state":
            return {(int(x), int(y)): int(maps[y, x]) for y, x in zip(*np.nonzero(maps))}
        return {((int(x), int(y)), int(d), int(a)): int(maps[d, a, y, x]) for d, a, y, x in zip(*np.nonzero(maps))}


class StateBonus(_Bonus):
    """wrappers.py:69-102: a bonus of 1 / sqrt(visits of agent_pos), counted over the wrapper's whole life."""
    kind = "state"


class ActionBonus(_Bonus):
    """wrappers.py:34-66: a bonus of 1 / sqrt(visits of (agent_pos, agent_dir, action))."""
    kind = "action"
