#!/usr/bin/env python3
"""ppo_bonus_scan_episode against ppo_bonus_scan's env scope (csrc/exploration_bonus.hip) at T = 128 steps x N = 4096
envs, on positions as concentrated as a rollout's: every env walks away from one start cell and returns to it when its
episode of 50 steps ends (2 or 3 ends per env and call).  The neighbour of ppo_kernels_bench.py for DESIGN.md 6: one JSON
line per kernel and window, HIP-event time over 20 calls, three windows each, taken alternately."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from twoarmy_amd.exploration import BonusTracker  # noqa: E402

dev = torch.device("cuda", 0)
T, N, W, H = 128, 4096, 17, 17
g = torch.Generator(device="cpu").manual_seed(0)


def timed(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


age0 = torch.randint(0, 50, (N,), generator=g)
ended = ((age0.view(1, N) + torch.arange(1, T + 1).view(T, 1)) % 50) == 0
walk = torch.zeros(T, N, 2)
cur = torch.tensor([15.0, 1.0]).repeat(N, 1)
moves = torch.tensor([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
for t in range(T):
    cur = (cur + moves[torch.randint(0, 5, (N,), generator=g)]).clamp_(1.0, 15.0)
    walk[t] = cur
    cur = torch.where(ended[t].view(-1, 1), torch.tensor([15.0, 1.0]), cur)
pos = walk.to(dev)
trunc = ended.to(torch.uint8).to(dev)
term = torch.zeros_like(trunc)
act = torch.randint(0, 7, (T, N), generator=g, dtype=torch.int32).to(dev)
dirs = torch.randint(0, 4, (T, N), generator=g, dtype=torch.int32).to(dev)
reward = torch.full((T, N), -0.01, device=dev)
shaped = torch.empty_like(reward)

for kinds in (("state",), ("state", "action")):
    life = BonusTracker(N, dev, kinds, "env", 1.0, W, H, 7)
    runs = {"ppo_bonus_scan env scope": lambda: life.account(pos, act, reward, term, dir=dirs, out=shaped)}
    for form in ("sqrt", "first"):
        ep = BonusTracker(N, dev, kinds, "episode", 1.0, W, H, 7, form)
        runs["ppo_bonus_scan_episode form=%s" % form] = (
            lambda ep=ep: ep.account(pos, act, reward, dir=dirs, out=shaped, keep=term, terminated=term, truncated=trunc))
    # what the kernels are asked to move: pos, reward in and out, a bonus per kind, action and dir for the action keys,
    # and the two flags for the episodic scan; the gathers and stores in the tables come on top
    moved = T * N * (8 + 4 + 4 + 4 * len(kinds)) + (T * N * 8 if "action" in kinds else 0)
    for window in range(3):
        for name, fn in runs.items():
            nbytes = moved + (2 * T * N if "episode" in name else 0)
            s = timed(fn)
            print(json.dumps({"kernel": "%s %s" % (name, "+".join(kinds)), "window": window, "us": s * 1e6,
                              "algorithmic_MB": nbytes / 1e6, "GBs": nbytes / s / 1e9,
                              "episode_ends": int(ended.sum())}), flush=True)
