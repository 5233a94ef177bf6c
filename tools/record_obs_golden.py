#!/usr/bin/env python3
"""Record tests/golden/obs_wrappers.npz from the reference's own observation wrappers (build container only).

TEST INFRASTRUCTURE ONLY, like tools/record_bonus_golden.py: imports the reference through oracle/ref_harness.py, drives
Twoarmy v6 / v4 over scripted actions with the engine's Philox draws patched in, hands every observation to the
reference's OneHotPartialObsWrapper, FullyObsWrapper, SymbolicObsWrapper, FlatObsWrapper and DirectionObsWrapper
(slope and angle) and stores what they RETURN.  No reference text is written.  Runs only where the reference exists.

  python tools/record_obs_golden.py            # -> tests/golden/obs_wrappers.npz

The stand-in gym's Wrapper does not forward observation_space and the reference's envs carry no `new_step_api`; the tool
sets both before the wrappers' constructors run.  All wrappers sit on ONE env per script; the two DirectionObsWrappers
are stacked so that one reset() (theirs: it takes no kwargs and returns the observation without goal_direction) resets
the env once.  An episode end is followed by reset(), op -1; every script also starts with one.

Contents, per script <name> (n_ops ops; S = the ops that are steps)
  ops_<name>       int32[n_ops]            env actions, -1 = reset
  meta_<name>      int32[2]                (variant, env_id)
  term_<name>, trunc_<name>   uint8[S]    the flags of each step
  agent_<name>     int32[n_ops][3]         agent_pos and agent_dir (x, y, dir) after every op
  grid_<name>      uint8[n_ops][17][17][3] the world itself, Grid.encode(), after every op: the wrappers' input
  full_<name>      uint8[n_ops][17][17][3] FullyObsWrapper, after every op (a reset returns an observation too)
  symbolic_<name>  int16[n_ops][17][17][3] SymbolicObsWrapper (returned as int64; stored narrower, the values are small)
  slope_<name>, angle_<name>   float64[S]  DirectionObsWrapper's goal_direction of each step
  sel_<name>       int32[K]                the steps (every 8th and every episode end) whose image-derived kinds are kept
  image_<name>     uint8[K][17][17][3]     obs["image"] of those steps
  onehot_<name>    uint8[K][17][17][21]    OneHotPartialObsWrapper
  flatimg_<name>   uint8[K][867]           FlatObsWrapper's first 867 values (float32 whole numbers, stored as bytes)
flat_tail          float32[2688]           FlatObsWrapper's values behind the image: the same in every observation
goal_position      int32[2]                DirectionObsWrapper.goal_position
Synthetic worlds syn<i> (W != H, doors in every state, every object kind), several agents each
  syn<i>_grid      uint8[W][H][3]          Grid.encode()
  syn<i>_agent     int32[A][3]             (x, y, dir)
  syn<i>_full      uint8[A][W][H][3];  syn<i>_symbolic int16[W][H][3];  syn<i>_onehot uint8[W][H][21]
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import ref_harness as rh  # noqa: E402
from record_bonus_golden import SCRIPTS as V6_SCRIPTS  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
R = gg.OP_RESET
PATH = [1] * 7 + [2] * 7
# v4: into room 2 and left along the patrol's row (the spawn), wait out the time limit, then the goal run
V4_SCRIPT = ("v4_patrol", 40, PATH + [2, 2, 2] + [0] * 6 + [2, 2, 1, 1] + [6] * 30 + PATH + [2] * 7 + [1] * 4 + [6, 6] + [1, 2] * 4)


def wrap(cls, env, *args, **kw):
    w = cls.__new__(cls)
    w.observation_space = env.observation_space
    w.__init__(env, *args, **kw)
    w.new_step_api = True
    return w


def run(variant, env_id, actions, wr):
    slots = gg.PhiloxSlots(gg.SEED, env_id)
    out = dict(ops=[], agent=[], grid=[], term=[], trunc=[], full=[], symbolic=[], slope=[], angle=[], sel=[], image=[],
               onehot=[], flatimg=[])
    tails, balls = [], 0
    with rh.patched_choice(rh.SlotRecorder(slots)):
        env = rh.make_env("v%d" % variant)
        base = env.unwrapped
        env.new_step_api = base.new_step_api = True
        onehot, full, symb, flat = (wrap(c, env) for c in (wr.OneHotPartialObsWrapper, wr.FullyObsWrapper,
                                                            wr.SymbolicObsWrapper, wr.FlatObsWrapper))
        dslope = wrap(wr.DirectionObsWrapper, env, type="slope")
        dangle = wrap(wr.DirectionObsWrapper, dslope, type="angle")

        def state_kinds(obs, op):
            out["ops"].append(op)
            out["agent"].append([int(base.agent_pos[0]), int(base.agent_pos[1]), int(base.agent_dir)])
            out["grid"].append(base.grid.encode().astype(np.uint8))
            out["full"].append(full.observation(dict(obs))["image"].copy())
            s = symb.observation(dict(obs))["image"]
            assert s.dtype == np.int64 and np.array_equal(s, s.astype(np.int16))
            out["symbolic"].append(s.astype(np.int16))

        obs = dangle.reset()
        assert "goal_direction" not in obs
        state_kinds(obs, R)
        step = 0
        for t, a in enumerate(actions):
            slots.begin_step(t)
            obs, _, term, trunc, _ = env.step(a)
            out["term"].append(bool(term))
            out["trunc"].append(bool(trunc))
            state_kinds(obs, a)
            with np.errstate(divide="ignore", invalid="ignore"):
                out["slope"].append(np.float64(dslope.observation(dict(obs))["goal_direction"]))
                out["angle"].append(np.float64(dangle.observation(dict(obs))["goal_direction"]))
            balls = max(balls, int((base.grid.encode()[:, :, 0] == 6).sum()))
            if step % 8 == 0 or term or trunc:
                out["sel"].append(step)
                out["image"].append(obs["image"].copy())
                out["onehot"].append(onehot.observation(dict(obs))["image"].copy())
                f = flat.observation(dict(obs))
                assert f.dtype == np.float32 and f.shape == (867 + 2688,)
                assert np.array_equal(f[:867], f[:867].astype(np.uint8))
                out["flatimg"].append(f[:867].astype(np.uint8))
                tails.append(f[867:].copy())
            step += 1
            if (term or trunc) and t + 1 < len(actions):
                state_kinds(dangle.reset(), R)
    assert dslope.goal_position == dangle.goal_position
    return out, tails, balls, dslope.goal_position


def synthetic(wr):
    import gym_minigrid.minigrid as mg
    env = rh.make_env("v6")
    base = env.unwrapped
    env.new_step_api = base.new_step_api = True
    onehot, full, symb = (wrap(c, env) for c in (wr.OneHotPartialObsWrapper, wr.FullyObsWrapper, wr.SymbolicObsWrapper))
    colors = list(mg.COLOR_TO_IDX.keys())
    z = {}
    for i, (W, H, seed) in enumerate([(5, 9, 1), (9, 4, 2)]):
        rs = np.random.RandomState(seed)
        makers = [lambda c: mg.Wall(), lambda c: mg.Door(c, is_open=True), lambda c: mg.Door(c), lambda c: mg.Door(c, is_locked=True),
                  lambda c: mg.Key(c), lambda c: mg.Box(c), lambda c: mg.Ball(c), lambda c: mg.Lava(), lambda c: mg.Goal(),
                  lambda c: mg.Floor(c)]
        grid = mg.Grid(W, H)
        cells = [(x, y) for y in range(H) for x in range(W)]
        rs.shuffle(cells)
        for k, (x, y) in enumerate(cells[:2 * len(makers) + 4]):       # every kind twice, a few more; the rest stays empty
            grid.set(x, y, makers[k % len(makers)](colors[rs.randint(len(colors))]))
        base.grid, base.width, base.height = grid, W, H
        agents = [(0, 0, 0), (W - 1, H - 1, 3), cells[0] + (1,), cells[-1] + (2,), (W - 1, 0, 1), (0, H - 1, 2)]
        fulls = []
        for x, y, d in agents:
            base.agent_pos, base.agent_dir = (x, y), d
            fulls.append(full.observation({})["image"].copy())
        s = symb.observation({})["image"]
        assert s.dtype == np.int64 and s.shape == (W, H, 3)
        enc = grid.encode().astype(np.uint8)
        onehot.observation_space.spaces["image"] = types.SimpleNamespace(shape=(W, H, 21))
        z["syn%d_grid" % i] = enc
        z["syn%d_agent" % i] = np.array(agents, np.int32)
        z["syn%d_full" % i] = np.stack(fulls).astype(np.uint8)
        z["syn%d_symbolic" % i] = s.astype(np.int16)
        z["syn%d_onehot" % i] = onehot.observation({"image": enc})["image"].copy()
        print("synthetic %dx%d: %d objects, kinds %s, door states %s" % (
            W, H, int((enc[:, :, 0] != 1).sum()), sorted(set(enc[:, :, 0].reshape(-1).tolist())),
            sorted(set(enc[enc[:, :, 0] == 4][:, 2].tolist()))), flush=True)
    z["n_synthetic"] = np.int32(2)
    return z


def main():
    rh.setup()
    import gym_minigrid.wrappers as wr
    z, tail = {}, None
    scripts = [(6,) + s for s in V6_SCRIPTS] + [(4,) + V4_SCRIPT]
    for variant, name, env_id, actions in scripts:
        out, tails, balls, goal = run(variant, env_id, actions, wr)
        tail = tails[0] if tail is None else tail
        assert all(np.array_equal(t, tail) for t in tails)
        assert variant == 6 or balls > 3, "the v4 script must reach the spawn (patrol balls)"
        z["ops_" + name] = np.array(out["ops"], np.int32)
        z["meta_" + name] = np.array([variant, env_id], np.int32)
        for k, dt in (("agent", np.int32), ("grid", np.uint8), ("term", np.uint8), ("trunc", np.uint8), ("full", np.uint8),
                      ("symbolic", np.int16), ("slope", np.float64), ("angle", np.float64), ("sel", np.int32),
                      ("image", np.uint8), ("onehot", np.uint8), ("flatimg", np.uint8)):
            z["%s_%s" % (k, name)] = np.array(out[k], dt)
        z["goal_position"] = np.array(goal, np.int32)
        sl = z["slope_" + name]
        print("script %s (v%d): %d steps, %d episodes, %d sampled, balls <= %d, slopes: %d inf, %d nan, %d -0.0" % (
            name, variant, len(actions), int(sum(out["term"]) + sum(out["trunc"])), len(out["sel"]), balls,
            int(np.isinf(sl).sum()), int(np.isnan(sl).sum()), int(((sl == 0) & np.signbit(sl)).sum())), flush=True)
    z["flat_tail"] = tail.astype(np.float32)
    z["script_names"] = np.array([s[1] for s in scripts])
    z.update(synthetic(wr))
    path = os.path.join(GOLD, "obs_wrappers.npz")
    np.savez_compressed(path, **z)
    print("-> %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
