#!/usr/bin/env python3
"""Record tests/golden/bonus.npz from the reference's own StateBonus / ActionBonus wrappers (build container only).

TEST INFRASTRUCTURE ONLY, like tools/record_render_golden.py: imports the reference through oracle/ref_harness.py,
drives Twoarmy_v6 bare and wrapped in StateBonus, ActionBonus and ActionBonus(StateBonus(.)) over scripted actions and
stores what they RETURN.  No reference text is written.  Runs only where the reference exists.

  python tools/record_bonus_golden.py            # -> tests/golden/bonus.npz

The reference's wrappers read `env.new_step_api`, which its envs do not carry; the tool sets it on the instance before
wrapping.  An episode end (terminated | truncated) is followed by reset(), recorded as op -1; the wrappers' counts
outlive it.

Contents, per script <name> (S = its steps, i.e. the ops that are not -1)
  ops_<name>      int32[n_ops]     env actions, -1 = reset
  meta_<name>     int32[2]         (variant, env_id)
  action_<name>   int32[S]         the action of each step
  xy_<name>       int32[S][2]      agent_pos (x, y) after the step;  dir_<name> int32[S] agent_dir after the step
  term_<name>, trunc_<name> uint8[S];  reward_<name> float64[S] the bare env's reward
  shaped_<name>   float64[3][S]    the reward returned by StateBonus, ActionBonus, ActionBonus(StateBonus(.))
  state_counts_<name>   int64[n][3]  (x, y, count): StateBonus.counts at the end
  action_counts_<name>  int64[n][5]  (x, y, dir, action, count): ActionBonus.counts at the end
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402
import ref_harness as rh  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
R = gg.OP_RESET
PATH = [1] * 7 + [2] * 7
GOAL = PATH + [6, 6] + [2] * 6 + [1] * 4 + [6, 2, 1]
SCRIPTS = [          # (name, env_id, actions); resets are inserted where an episode ends
    ("still", 0, [0] * 60 + [6] * 30 + [0, 1, 0, 1] * 10),             # repeated keys over several episodes, action 6
    ("blocked_goal", 1, [1, 1, 1] + [2] * 12 + [3] * 40 + GOAL + [1, 2] + GOAL + [0, 3] * 8),   # K2, timeout, K4 twice
    ("walk", 2, [int(a) for a in np.random.RandomState(7).choice([0, 1, 2, 3, 6], 200, p=[.2, .25, .3, .15, .1])]),
]
STACKS = ("bare", "state", "action", "both")


def run(stack, env_id, actions, wrappers):
    slots = gg.PhiloxSlots(gg.SEED, env_id)
    rec = rh.SlotRecorder(slots)
    out = dict(ops=[], action=[], xy=[], dir=[], term=[], trunc=[], reward=[])
    with rh.patched_choice(rec):
        env = rh.make_env("v6")
        base = env.unwrapped
        env.new_step_api = True
        sb = ab = None
        if stack in ("state", "both"):
            env = sb = wrappers.StateBonus(env)
            env.new_step_api = True
        if stack in ("action", "both"):
            env = ab = wrappers.ActionBonus(env)
        for t, a in enumerate(actions):
            slots.begin_step(t)
            _, reward, term, trunc, _ = env.step(a)
            out["ops"].append(a)
            out["action"].append(a)
            out["xy"].append([int(base.agent_pos[0]), int(base.agent_pos[1])])
            out["dir"].append(int(base.agent_dir))
            out["term"].append(bool(term))
            out["trunc"].append(bool(trunc))
            out["reward"].append(float(reward))
            if term or trunc:
                env.reset()
                out["ops"].append(R)
    counts_s = None if sb is None else np.array(sorted((x, y, c) for (x, y), c in sb.counts.items()), np.int64)
    counts_a = None if ab is None else np.array(sorted((x, y, d, a, c) for ((x, y), d, a), c in ab.counts.items()), np.int64)
    return out, counts_s, counts_a


def main():
    rh.setup()
    import gym_minigrid.wrappers as wrappers
    z = {}
    for name, env_id, actions in SCRIPTS:
        assert len(actions) <= 200
        runs = {s: run(s, env_id, actions, wrappers) for s in STACKS}
        bare = runs["bare"][0]
        for s in STACKS[1:]:                                           # the four envs walked the same trajectory
            for k in ("ops", "xy", "dir", "term", "trunc"):
                assert runs[s][0][k] == bare[k], (name, s, k)
        z["ops_" + name] = np.array(bare["ops"], np.int32)
        z["meta_" + name] = np.array([6, env_id], np.int32)
        z["action_" + name] = np.array(bare["action"], np.int32)
        z["xy_" + name] = np.array(bare["xy"], np.int32)
        z["dir_" + name] = np.array(bare["dir"], np.int32)
        z["term_" + name] = np.array(bare["term"], np.uint8)
        z["trunc_" + name] = np.array(bare["trunc"], np.uint8)
        z["reward_" + name] = np.array(bare["reward"], np.float64)
        z["shaped_" + name] = np.array([runs[s][0]["reward"] for s in STACKS[1:]], np.float64)
        z["state_counts_" + name] = runs["state"][1]
        z["action_counts_" + name] = runs["action"][2]
        assert np.array_equal(runs["both"][1], runs["state"][1]) and np.array_equal(runs["both"][2], runs["action"][2])
        print("script %s: %d steps, %d episodes (%d goals), %d cells, %d (cell, dir, action) keys" % (
            name, len(actions), int(sum(bare["term"]) + sum(bare["trunc"])), int(sum(bare["term"])),
            len(runs["state"][1]), len(runs["action"][2])), flush=True)
    z["script_names"] = np.array([s[0] for s in SCRIPTS])
    path = os.path.join(GOLD, "bonus.npz")
    np.savez_compressed(path, **z)
    print("-> %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
