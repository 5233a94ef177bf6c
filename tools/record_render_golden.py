#!/usr/bin/env python3
"""Record tests/golden/render.npz from the reference's own renderer (build container only).

TEST INFRASTRUCTURE ONLY, like oracle/gen_golden.py: imports the reference through oracle/ref_harness.py, drives
Grid.render_tile / MiniGridEnv.get_full_render and stores what they RETURN (uint8 arrays, key tables, the action
scripts and the logged draws).  No reference text is written.  Runs only where the reference exists.

  python tools/record_render_golden.py            # -> tests/golden/render.npz, prints the reference's ms / frame

Contents
  tiles_<ts>      uint8[K][ts][ts][3]   Grid.render_tile(...) cast to uint8 the way Grid.render's assignment casts it
  tilekeys_<ts>   int32[K][5]           (type, colour, state, agent_dir or -1, highlight) of each tile
  frames_<name>   uint8[1 + n_ops][289][289][3]   get_full_render() after the constructor's reset and after every op
                  of the script (tile_size 17), stored as frame[0], frame[t] ^ frame[t-1] (consecutive frames differ
                  in a few tiles, so the file stays small); tests/render_ref.py:load_frames undoes it
  grids_<name>    uint8[1 + n_ops][17][17][3]  env.grid.encode() behind each frame; agents_<name> int32[1 + n_ops][3] =
                  (agent x, agent y, agent_dir)
  ops_<name>, draws_<name> (natural-stream scripts: the draw log of oracle/gen_golden.py), meta_<name> =
                  (variant, env_id, natural, highlight, agent_view_size)
  mask_grid_<c>, mask_meta_<c> = (W, H, ax, ay) of the 30 worlds of occlusion.npz; mask_vis_<c>_<V> uint8[4][V][V]
                  (gen_obs_grid's mask per agent direction, indexed [i][j]) and mask_out_<c>_<V> uint8[4][W][H]
                  (env.agent_coordinate per direction, indexed [i][j]), V in 3, 7, 17
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import ref_harness as rh  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
R = gg.OP_RESET
PATH = [1] * 7 + [2] * 7
SCRIPTS = [          # (name, variant, ops, env_id, natural seed, highlight, agent_view_size): SURVEY.md section 4
    ("K1_wall_drop", "v6", [1, 6, 6], 0, None, False, 17),
    ("K2_blocked_room2", "v6", [1, 1, 1] + [2] * 12, 1, None, False, 17),
    ("K3_risk_trunc", "v6", [1] * 4 + [2] * 6 + [6] * 20, 2, None, False, 17),
    ("K4_goal", "v6", PATH + [6, 6] + [2] * 6 + [1] * 4 + [6, 2, 1, R, 1, 2], 3, None, False, 17),
    ("K5_ball_onto_agent", "v6", PATH + [6] * 5 + [6, 6, 2, 2, R, 2], 4, None, False, 17),
    ("K6_timeout", "v6", [0] * 50 + [0, 1, R, 1], 5, None, False, 17),
    ("K8_natural_seed9981", "v4", PATH + [2, 2, 2] + [6] * 30, 38, 9981, False, 17),
    ("K4_goal_hl7", "v6", PATH + [6, 6] + [2] * 6 + [1] * 4 + [6, 2, 1, R, 1, 2], 3, None, True, 7),
    ("K5_ball_onto_agent_hl7", "v6", PATH + [6] * 5 + [6, 6, 2, 2, R, 2], 4, None, True, 7),
]


def tile_objects(mg, twoarmy_only):
    """(type, colour, state) of every object the device renderer draws."""
    T = mg.OBJECT_TO_IDX
    if twoarmy_only:
        return [(1, 0, 0), (T["wall"], 5, 0), (T["ball"], 4, 0), (T["goal"], 1, 0)]
    objs = [(0, 0, 0), (1, 0, 0)]
    for name in ("wall", "floor", "key", "ball", "box", "goal"):
        objs += [(T[name], c, 0) for c in range(6)]
    objs += [(T["door"], c, s) for c in range(6) for s in range(3)]
    return objs


def record_tiles(mg, ts, twoarmy_only):
    mg.Grid.tile_cache.clear()
    keys, tiles = [], []
    for (t, c, s) in tile_objects(mg, twoarmy_only):
        obj = mg.WorldObj.decode(t, c, s)
        for agent in (-1, 0, 1, 2, 3):
            for hl in (0, 1):
                img = mg.Grid.render_tile(obj, agent_dir=None if agent < 0 else agent, highlight=bool(hl), tile_size=ts)
                out = np.zeros((ts, ts, 3), np.uint8)
                out[:, :, :] = img                     # the cast Grid.render's `img[...] = tile_img` performs
                keys.append((t, c, s, agent, hl))
                tiles.append(out)
    return np.array(keys, np.int32), np.stack(tiles)


def record_script(name, variant, ops, env_id, natural, highlight, view):
    slots = gg.PhiloxSlots(gg.SEED, env_id)
    nat_log = []
    if natural is None:
        rec = rh.SlotRecorder(slots)
    else:
        np.random.seed(natural)
        real_choice = np.random.choice

        def nat(lo, n):
            v = int(real_choice(range(lo, lo + n), 1).item()) if n > 1 else lo
            slot = slots.slot_of(lo, n)
            slots.calls.append((lo, n))
            nat_log.append((slots.t, slot, lo, n, v))
            return v
        rec = rh.SlotRecorder(nat)
    frames, grids, agents, t, secs = [], [], [], 0, []

    def state():
        grids.append(env.grid.encode().astype(np.uint8))
        agents.append([int(env.agent_pos[0]), int(env.agent_pos[1]), int(env.agent_dir)])
    with rh.patched_choice(rec):
        env = rh.make_env(variant, highlight=highlight, agent_view_size=view)
        frames.append(np.asarray(env.get_full_render(), np.uint8).copy())
        state()
        for op in ops:
            if op == R:
                env.reset()
            else:
                slots.begin_step(t)
                t += 1
                env.step(op)
            t0 = time.perf_counter()
            img = env.get_full_render()
            secs.append(time.perf_counter() - t0)
            frames.append(np.asarray(img, np.uint8).copy())
            state()
    log = nat_log if natural is not None else slots.log
    frames = np.stack(frames)
    frames[1:] ^= frames[:-1].copy()
    return dict(frames=frames, grids=np.stack(grids), agents=np.array(agents, np.int32), ops=np.array(ops, np.int32), draws=np.array(log, np.int64).reshape(-1, 5),
                meta=np.array([4 if variant == "v4" else 6, env_id, int(natural is not None), int(highlight), view],
                              np.int32)), secs


def record_masks(mg, out):
    z = np.load(os.path.join(GOLD, "occlusion.npz"))
    env = rh.make_env("v6", highlight=True, tile_size=1).unwrapped
    n = int(z["n_cases"])
    for c in range(n):
        enc, meta = z["c%03d_grid" % c], z["c%03d_meta" % c]
        W, H, ax, ay = (int(v) for v in meta[:4])
        grid, _ = mg.Grid.decode(enc)
        out["mask_grid_%02d" % c] = enc
        out["mask_meta_%02d" % c] = np.array([W, H, ax, ay], np.int32)
        for V in (3, 7, 17):
            vis_d, out_d = [], []
            for d in range(4):
                env.grid, env.width, env.height = grid, W, H
                env.agent_pos, env.agent_dir, env.agent_view_size = (ax, ay), d, V
                env.carrying, env.see_through_walls = None, False
                _, vis = env.gen_obs_grid()
                env.get_full_render()
                vis_d.append(np.asarray(vis, np.uint8))
                out_d.append(np.asarray(env.agent_coordinate, np.uint8))
            out["mask_vis_%02d_%d" % (c, V)] = np.stack(vis_d)
            out["mask_out_%02d_%d" % (c, V)] = np.stack(out_d)
    out["n_mask_worlds"] = np.int32(n)


def main():
    rh.setup()
    import gym_minigrid.minigrid as mg
    out = {}
    for ts, sub in ((8, True), (17, False), (32, False)):
        t0 = time.perf_counter()
        out["tilekeys_%d" % ts], out["tiles_%d" % ts] = record_tiles(mg, ts, sub)
        print("tiles ts=%d: %d tiles in %.1f s" % (ts, len(out["tiles_%d" % ts]), time.perf_counter() - t0), flush=True)
    warm = []
    names = []
    for (name, variant, ops, eid, nat, hl, view) in SCRIPTS:
        r, secs = record_script(name, variant, ops, eid, nat, hl, view)
        for k, v in r.items():
            out["%s_%s" % (k, name)] = v
        names.append(name)
        warm += secs[5:]
        print("script %s: %d frames" % (name, len(secs)), flush=True)
    out["script_names"] = np.array(names)
    out["ref_ms_per_frame_warm"] = np.float64(1e3 * float(np.median(warm)))
    print("reference get_full_render(): median %.1f ms / 289x289 frame with its tile cache warm (one CPU core)"
          % out["ref_ms_per_frame_warm"], flush=True)
    record_masks(mg, out)
    path = os.path.join(GOLD, "render.npz")
    np.savez_compressed(path, **out)
    print("-> %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
