"""The wrappers of the reference's gym_minigrid/wrappers.py, computing on the device.

ViewSizeWrapper (wrappers.py:428-460), the only place a 7x7 egocentric view exists: the reference re-slices the grid
with gen_obs_grid(agent_view_size) after every reset / step; here that is one tw_gen_obs launch at the requested view
size on the wrapped env's device state.  StateBonus and ActionBonus (:69-102, :34-66), the count-based exploration
bonuses, count on the device (exploration.BonusTracker, one ppo_bonus_scan launch per step).  The observation wrappers
ImgObsWrapper (:105-114), OneHotPartialObsWrapper (:117-154), FullyObsWrapper (:220-246), FlatObsWrapper (:367-425),
DirectionObsWrapper (:463-494) and SymbolicObsWrapper (:497-526) go through minigrid_obs (csrc/minigrid_obs.hip) on the
facade's engine state and return what the reference classes return, quirks included: SymbolicObsWrapper's reshape of the
flat cell list (the transposed world), DirectionObsWrapper's goal_position = (k // height, k % width), its reset() without
kwargs that returns the observation without goal_direction, and its goal_position cached for the wrapper's life.
ReseedWrapper (:13-31) is host code.  Thousands of envs take all of these through TwoarmyVecEnv(agent_view_size=...,
state_bonus=..., action_bonus=..., observation=..., goal_direction=...) or train_ppo --bonus.  The pixel wrappers
RGBImgObsWrapper (:157-186) and RGBImgPartialObsWrapper (:189-217) return the device renderer's frames
(csrc/minigrid_render.hip); as in the reference their tile_size sizes only the declared space, the picture is drawn by
the env's get_full_render / get_pov_render with the env's own tile_size.  Out of scope: DictObservationSpaceWrapper."""
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


class ReseedWrapper:
    """wrappers.py:13-31: reset() always passes the next seed of a fixed list (the engine's worlds do not depend on it)."""

    def __init__(self, env, seeds=[0], seed_idx=0):
        self.seeds = list(seeds)
        self.seed_idx = seed_idx
        self.env = env
        self.unwrapped = getattr(env, "unwrapped", env)

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, **kwargs):
        seed = self.seeds[self.seed_idx]
        self.seed_idx = (self.seed_idx + 1) % len(self.seeds)
        return self.env.reset(seed=seed, **kwargs)

    def step(self, action):
        return self.env.step(action)


class _ObservationWrapper:
    """gym.ObservationWrapper: reset() and step() return observation(obs) in place of obs."""

    def __init__(self, env):
        self.env = env
        self.unwrapped = getattr(env, "unwrapped", env)
        self._eng = self.unwrapped._eng
        self._device = self._eng.device
        self.observation_space = dict(getattr(env, "observation_space", {}))

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, **kwargs):
        out = self.env.reset(**kwargs)
        if isinstance(out, tuple):
            return self.observation(out[0]), out[1]
        return self.observation(out)

    def step(self, action):
        out = self.env.step(action)
        return (self.observation(out[0]),) + tuple(out[1:])

    def _image_on_device(self, obs):
        return torch.from_numpy(np.ascontiguousarray(obs["image"], np.uint8)).to(self._device).unsqueeze(0)


class ImgObsWrapper(_ObservationWrapper):
    """wrappers.py:105-114: the image alone, no direction / mission."""

    def __init__(self, env):
        super().__init__(env)
        self.observation_space = env.observation_space["image"]

    def observation(self, obs):
        return obs["image"]


class OneHotPartialObsWrapper(_ObservationWrapper):
    """wrappers.py:117-154: obs["image"] as uint8[V, V, 21] (mg_obs_onehot); an index of 21 or more is an IndexError."""

    def __init__(self, env, tile_size=8):
        super().__init__(env)
        self.tile_size = tile_size
        shape = env.observation_space["image"].shape
        self.observation_space["image"] = _Space(shape=(shape[0], shape[1], 21))

    def observation(self, obs):
        from .. import minigrid_obs
        out, err = minigrid_obs.onehot(self._image_on_device(obs), want_error=True)
        if int(err[0]):
            raise IndexError("one-hot index out of bounds for axis 2 with size 21")
        return {**obs, "image": out[0].cpu().numpy()}


class RGBImgObsWrapper(_ObservationWrapper):
    """wrappers.py:157-186: obs["image"] = get_full_render().  The wrapper keeps tile_size and highlight = True for
    itself; gym.Wrapper forwards get_full_render to the env, which draws with its own tile_size and highlight, so the
    declared shape (width * tile_size, height * tile_size, 3) is the image's only when the two tile sizes agree."""

    def __init__(self, env, tile_size=8):
        super().__init__(env)
        self.highlight = True
        self.tile_size = tile_size
        self.observation_space["image"] = _Space(shape=(self.env.width * tile_size, self.env.height * tile_size, 3))

    def observation(self, obs):
        return {**obs, "image": self.get_full_render()}


class RGBImgPartialObsWrapper(_ObservationWrapper):
    """wrappers.py:189-217: obs["image"] = get_pov_render(), drawn by the env with its own tile_size (see above);
    sets unwrapped.agent_pov, so the env's render() shows the agent's view from then on."""

    def __init__(self, env, tile_size=8):
        super().__init__(env)
        self.unwrapped.agent_pov = True
        self.tile_size = tile_size
        shape = env.observation_space["image"].shape
        self.observation_space["image"] = _Space(shape=(shape[0] * tile_size, shape[1] * tile_size, 3))

    def observation(self, obs):
        return {**obs, "image": self.get_pov_render()}


class FullyObsWrapper(_ObservationWrapper):
    """wrappers.py:220-246: the whole grid, the agent's cell (10, 0, agent_dir) (mg_obs_full on the engine's state)."""

    def __init__(self, env):
        super().__init__(env)
        self.observation_space["image"] = _Space(shape=(self.unwrapped.width, self.unwrapped.height, 3))

    def observation(self, obs):
        from .. import minigrid_obs
        u = self.unwrapped
        ty, co = self._eng.plane_views()
        out = minigrid_obs.full_obs(ty, co, None, u.width, u.height, *self._eng.agent_views())
        return {**obs, "image": out[0].cpu().numpy()}


class SymbolicObsWrapper(_ObservationWrapper):
    """wrappers.py:497-526: int64[W, H, 3] = (x, y, idx), idx -1 where the cell is empty (mg_obs_symbolic)."""

    def __init__(self, env):
        super().__init__(env)
        self.observation_space["image"] = _Space(shape=(self.unwrapped.width, self.unwrapped.height, 3))

    def observation(self, obs):
        from .. import minigrid_obs
        u = self.unwrapped
        out = minigrid_obs.symbolic_obs(self._eng.plane_views()[0], u.width, u.height)
        obs["image"] = out[0].cpu().numpy().astype(np.int64)
        return obs


class FlatObsWrapper(_ObservationWrapper):
    """wrappers.py:367-425: float32[V*V*3 + maxStrLen*28], the image and the one-hot mission string (mg_obs_flat)."""

    def __init__(self, env, maxStrLen=96):
        super().__init__(env)
        self.maxStrLen = maxStrLen
        self.numCharCodes = 28
        n = int(np.prod(env.observation_space["image"].shape))
        self.observation_space = _Space(shape=(n + self.numCharCodes * maxStrLen,))
        self.cachedStr = None

    def observation(self, obs):
        from .. import minigrid_obs
        mission = obs["mission"]
        if mission != self.cachedStr:
            self.cachedArray = minigrid_obs.mission_tail(mission, self.maxStrLen).reshape(self.maxStrLen, self.numCharCodes)
            self.cachedStr = mission.lower()
            self._tail = torch.from_numpy(self.cachedArray.reshape(-1)).to(self._device)
        return minigrid_obs.flat_obs(self._image_on_device(obs), self._tail)[0].cpu().numpy()


class DirectionObsWrapper(_ObservationWrapper):
    """wrappers.py:463-494: obs["goal_direction"] = the slope to the goal, or its arctan (type="angle")
    (mg_obs_goal_index at the first reset, mg_obs_goal_direction per step)."""

    def __init__(self, env, type="slope"):
        super().__init__(env)
        self.goal_position = None
        self.type = type
        self._goal_index = self._table = None

    def reset(self):                                   # the reference's override: no kwargs, observation() not applied
        obs = self.env.reset()
        if not self.goal_position:
            from .. import minigrid_obs
            u = self.unwrapped
            self._goal_index = minigrid_obs.goal_index(self._eng.plane_views()[0], u.width, u.height)
            k = int(self._goal_index[0])
            self.goal_position = [] if k < 0 else (int(k / u.height), k % u.width)
        return obs

    def observation(self, obs):
        from .. import minigrid_obs
        u = self.unwrapped
        if self.goal_position is None:
            raise TypeError("'NoneType' object is not subscriptable")          # observation() before the first reset()
        if not self.goal_position:
            raise IndexError("list index out of range")                        # a world without a goal
        mode = "angle" if self.type == "angle" else "slope"
        if mode == "angle" and self._table is None:
            self._table = minigrid_obs.angle_table(u.width, u.height, self._device)
        out = minigrid_obs.goal_direction(self._goal_index, u.width, u.height, *self._eng.agent_views()[:2], mode=mode,
                                          table=self._table)
        obs["goal_direction"] = out.cpu().numpy()[0]
        return obs
