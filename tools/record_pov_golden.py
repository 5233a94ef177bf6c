#!/usr/bin/env python3
"""Record tests/golden/pov.npz from the reference's own get_pov_render and pixel wrappers (build container only).

TEST INFRASTRUCTURE ONLY, like tools/record_render_golden.py: imports the reference through oracle/ref_harness.py,
drives MiniGridEnv.get_pov_render, RGBImgObsWrapper and RGBImgPartialObsWrapper and stores what they RETURN.  No
reference text is written.  Runs only where the reference exists.

  python tools/record_pov_golden.py            # -> tests/golden/pov.npz

Contents
  Occlusion worlds: all 30 worlds of tests/golden/occlusion.npz (none had to be dropped for the file's size), each
  with see_through_walls=False, in all four agent directions, at (V, tile size) = (3, 8), (7, 8), (3, 1), (3, 3)
    n_worlds; w_grid_<c> uint8[W][H][3] (Grid.encode()); w_meta_<c> int32[4] = (W, H, agent x, agent y) -- worlds 0-3
    have the agent moved into a corner, so that the view leaves the world on two sides in every direction somewhere;
    w_carry_<c> uint8[3] = encode() of the carried object, type 0 = nothing (worlds 4-9: key, ball, box in two colours)
    w_pov_<c>_<V>_<ts> uint8[4][V*ts][V*ts][3]   get_pov_render() per agent direction
    w_vis_<c>_<V>      uint8[4][V][V]            gen_obs_grid's mask behind those frames, indexed [i][j]
  Twoarmy scripts K4_goal and K5_ball_onto_agent of tools/record_render_golden.py at agent_view_size=7, tile_size=8
  (see_through_walls=True: every cell highlighted)
    s_pov_<name> uint8[1 + n_ops][56][56][3]     get_pov_render() after the constructor's reset and after every op,
                                                 stored as frame[0], frame[t] ^ frame[t-1] (tests/pov_ref.py undoes it)
    s_ops_<name>, s_meta_<name> = (variant, env_id, agent_view_size, tile_size), s_agents_<name> int32[1 + n_ops][3],
    s_done_<name> uint8[n_ops][2] = (terminated, truncated) of every op that is a step (0, 0 for a reset)
  The same two scripts as a vector env with auto-reset lives them: the ops up to the first step that ends the episode,
  reset() at once (the scripts above take a few more steps on the finished episode first, which moves state that
  outlives reset()), then the script's ops behind its reset
    a_ops_<name> int32[m]; a_pov_<name> uint8[1 + m][56][56][3] and a_full_<name> uint8[1 + m][289][289][3]
    (get_full_render() at tile_size 17): the frame after that reset(), then after every op; XOR deltas as above
  Pixel wrappers on one v6 env built with tile_size=17, agent_view_size=7; both wrappers with their default tile_size=8
    wr_ops int32[3]; wr_full uint8[4][...], wr_partial uint8[4][...]: obs["image"] of RGBImgObsWrapper /
    RGBImgPartialObsWrapper after the reset and after each op, through the wrappers' own observation() -- the stand-in
    gym.Wrapper forwards get_full_render / get_pov_render to the env as gym's does; wr_full_space, wr_partial_space
    int32[3] = observation_space["image"].shape; wr_agent_pov uint8[2] = unwrapped.agent_pov before / after
    RGBImgPartialObsWrapper's constructor; wr_env = (tile_size, agent_view_size, highlight) of the env
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden as gg  # noqa: E402
import ref_harness as rh  # noqa: E402
from record_obs_golden import wrap  # noqa: E402
from record_render_golden import SCRIPTS  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
R = gg.OP_RESET
VIEWS = ((3, 8), (7, 8), (3, 1), (3, 3))
POV_SCRIPTS = ("K4_goal", "K5_ball_onto_agent")
WRAPPER_OPS = [1, 1, 2]


def record_worlds(mg, out):
    z = np.load(os.path.join(GOLD, "occlusion.npz"))
    env = rh.make_env("v6").unwrapped
    n = int(z["n_cases"])
    carried = {4: mg.Key("red"), 5: mg.Key("blue"), 6: mg.Ball("green"), 7: mg.Ball("yellow"), 8: mg.Box("purple"),
               9: mg.Box("grey")}
    two_sides = set()
    for c in range(n):
        enc, meta = z["c%03d_grid" % c], z["c%03d_meta" % c]
        W, H, ax, ay = (int(v) for v in meta[:4])
        if c < 4:
            ax, ay = ((0, 0), (W - 1, H - 1), (W - 1, 0), (0, H - 1))[c]
        grid, _ = mg.Grid.decode(enc)
        carry = carried.get(c)
        out["w_grid_%02d" % c] = enc
        out["w_meta_%02d" % c] = np.array([W, H, ax, ay], np.int32)
        out["w_carry_%02d" % c] = np.array(carry.encode() if carry else (0, 0, 0), np.uint8)
        for V, ts in VIEWS:
            frames, masks = [], []
            for d in range(4):
                env.grid, env.width, env.height = grid, W, H
                env.agent_pos, env.agent_dir, env.agent_view_size = (ax, ay), d, V
                env.carrying, env.see_through_walls, env.tile_size = carry, False, ts
                _, vis = env.gen_obs_grid()
                img = np.asarray(env.get_pov_render())
                assert img.dtype == np.uint8 and img.shape == (V * ts, V * ts, 3)
                frames.append(img.copy())
                masks.append(np.asarray(vis, np.uint8))
                tx, ty, bx, by = env.get_view_exts()
                if (tx < 0 or bx > W) and (ty < 0 or by > H) and V == 7:
                    two_sides.add(d)
            out["w_pov_%02d_%d_%d" % (c, V, ts)] = np.stack(frames)
            out["w_vis_%02d_%d" % (c, V)] = np.stack(masks)
    assert two_sides == {0, 1, 2, 3}, two_sides
    out["n_worlds"] = np.int32(n)


def record_script(name, variant, ops, env_id, view, ts):
    slots = gg.PhiloxSlots(gg.SEED, env_id)
    frames, agents, done, t = [], [], [], 0
    with rh.patched_choice(rh.SlotRecorder(slots)):
        env = rh.make_env(variant, agent_view_size=view, tile_size=ts)
        assert env.unwrapped.see_through_walls

        def state():
            frames.append(np.asarray(env.get_pov_render(), np.uint8).copy())
            agents.append([int(env.agent_pos[0]), int(env.agent_pos[1]), int(env.agent_dir)])
        state()
        for op in ops:
            if op == R:
                env.reset()
                done.append((0, 0))
            else:
                slots.begin_step(t)
                t += 1
                _, _, term, trunc, _ = env.step(op)
                done.append((int(bool(term)), int(bool(trunc))))
            state()
    frames = np.stack(frames)
    frames[1:] ^= frames[:-1].copy()
    return dict(pov=frames, ops=np.array(ops, np.int32), agents=np.array(agents, np.int32), done=np.array(done, np.uint8),
                meta=np.array([4 if variant == "v4" else 6, env_id, view, ts], np.int32))


def record_autoreset(name, variant, ops, env_id, view, ts):
    slots = gg.PhiloxSlots(gg.SEED, env_id)
    pov, full = [], []
    with rh.patched_choice(rh.SlotRecorder(slots)):
        env = rh.make_env(variant, agent_view_size=view, tile_size=ts)
        base = env.unwrapped

        def state():
            pov.append(np.asarray(env.get_pov_render(), np.uint8).copy())
            base.tile_size = 17
            full.append(np.asarray(env.get_full_render(), np.uint8).copy())
            base.tile_size = ts
        t = 0
        for op in ops:
            assert op != R
            slots.begin_step(t)
            t += 1
            _, _, term, trunc, _ = env.step(op)
            if term or trunc:
                break
        env.reset()
        state()
        tail = ops[ops.index(R) + 1:]
        for op in tail:
            slots.begin_step(t)
            t += 1
            env.step(op)
            state()
    pov, full = np.stack(pov), np.stack(full)
    pov[1:] ^= pov[:-1].copy()
    full[1:] ^= full[:-1].copy()
    return dict(ops=np.array(tail, np.int32), pov=pov, full=full)


def record_wrappers(wr, out):
    slots = gg.PhiloxSlots(gg.SEED, 0)
    with rh.patched_choice(rh.SlotRecorder(slots)):
        env = rh.make_env("v6", tile_size=17, agent_view_size=7)
        base = env.unwrapped
        env.new_step_api = base.new_step_api = True
        full = wrap(wr.RGBImgObsWrapper, env)
        before = bool(base.agent_pov)
        partial = wrap(wr.RGBImgPartialObsWrapper, env)
        out["wr_agent_pov"] = np.array([before, bool(base.agent_pov)], np.uint8)
        out["wr_env"] = np.array([base.tile_size, base.agent_view_size, int(base.highlight)], np.int32)
        assert full.tile_size == partial.tile_size == 8
        out["wr_full_space"] = np.array(full.observation_space.spaces["image"].shape, np.int32)
        out["wr_partial_space"] = np.array(partial.observation_space.spaces["image"].shape, np.int32)
        obs = env.reset()
        fulls = [full.observation(dict(obs))["image"].copy()]
        parts = [partial.observation(dict(obs))["image"].copy()]
        for t, op in enumerate(WRAPPER_OPS):
            slots.begin_step(t)
            obs = env.step(op)[0]
            fulls.append(full.observation(dict(obs))["image"].copy())
            parts.append(partial.observation(dict(obs))["image"].copy())
    out["wr_ops"] = np.array(WRAPPER_OPS, np.int32)
    out["wr_full"] = np.stack(fulls).astype(np.uint8)
    out["wr_partial"] = np.stack(parts).astype(np.uint8)
    print("wrappers: declared %s / %s, returned %s / %s" % (tuple(out["wr_full_space"]), tuple(out["wr_partial_space"]),
                                                          out["wr_full"].shape[1:], out["wr_partial"].shape[1:]), flush=True)


def main():
    rh.setup()
    import gym_minigrid.minigrid as mg
    import gym_minigrid.wrappers as wr
    out = {}
    record_worlds(mg, out)
    names = []
    for (name, variant, ops, eid, nat, hl, view) in SCRIPTS:
        if name in POV_SCRIPTS:
            r = record_script(name, variant, ops, eid, 7, 8)
            for k, v in r.items():
                out["s_%s_%s" % (k, name)] = v
            for k, v in record_autoreset(name, variant, list(ops), eid, 7, 8).items():
                out["a_%s_%s" % (k, name)] = v
            names.append(name)
            print("script %s: %d frames, done flags %s" % (name, len(r["pov"]), r["done"].sum(axis=0).tolist()), flush=True)
    out["script_names"] = np.array(names)
    record_wrappers(wr, out)
    path = os.path.join(GOLD, "pov.npz")
    np.savez_compressed(path, **out)
    print("-> %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
