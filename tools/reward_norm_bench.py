#!/usr/bin/env python3
"""Cost of the reward normalisation kernels (csrc/reward_norm.hip) at T = 128 steps x N = 4096 envs, in one process with
their yardsticks: ppo_episode_scan, the same kind of per-env walk, for ppo_reward_norm_update, and a device fill of
2 x 2 MiB (what ppo_reward_norm_apply must at least move: 2 MiB read, 2 MiB written) for ppo_reward_norm_apply.  The
callers alternate, three rounds each, so that a drift of the machine shows in the spread.  One JSON line per round and
kernel, then a summary line with the medians."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from twoarmy_amd import ppo_ops  # noqa: E402

dev = torch.device("cuda", 0)
T, N = 128, 4096
g = torch.Generator(device="cpu").manual_seed(0)


def timed(fn, iters=200):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                      # microseconds per call


rw5 = torch.tensor([-0.01, -0.1, -0.9, 0.2, 0.9])[torch.randint(0, 5, (T, N), generator=g)].to(dev)
term = (torch.rand(T, N, generator=g) < 0.01).to(torch.uint8).to(dev)
trunc = (torch.rand(T, N, generator=g) < 0.02).to(torch.uint8).to(dev)
carry_r, carry_l = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
ep_r, ep_l = ppo_ops.episode_scan(rw5, term, trunc, carry_r, carry_l)
ret_carry, stats = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)
ws = torch.empty(ppo_ops.reward_norm_workspace(N), dtype=torch.float64, device=dev)
out = torch.empty_like(rw5)
fill = torch.empty(2 * T * N, dtype=torch.float32, device=dev)     # 2 x 2 MiB

callers = {
    "ppo_episode_scan (per-step outputs)": lambda: ppo_ops.episode_scan(rw5, term, trunc, carry_r, carry_l, out=(ep_r, ep_l)),
    "ppo_episode_scan (carries only)": lambda: ppo_ops.episode_scan(rw5, term, trunc, carry_r, carry_l, want_steps=False),
    "ppo_reward_norm_update (scan + fold)": lambda: ppo_ops.reward_norm_update(rw5, term, trunc, 0.99, ret_carry, stats, ws),
    "ppo_reward_norm_apply": lambda: ppo_ops.reward_norm_apply(rw5, stats, 10.0, out),
    "ppo_reward_norm_apply in place": lambda: ppo_ops.reward_norm_apply(out, stats, 0.0, out),
    "fill 2 x 2 MiB": lambda: fill.fill_(1.0),
}
rounds = {k: [] for k in callers}
for r in range(3):
    for name, fn in callers.items():
        us = timed(fn)
        rounds[name].append(us)
        print(json.dumps({"round": r, "kernel": name, "us": round(us, 3)}), flush=True)
med = {k: statistics.median(v) for k, v in rounds.items()}
print(json.dumps({"T": T, "N": N, "median_us": {k: round(v, 3) for k, v in med.items()},
                  "update_over_episode_scan": round(med["ppo_reward_norm_update (scan + fold)"] /
                                                    med["ppo_episode_scan (per-step outputs)"], 3),
                  "apply_over_fill": round(med["ppo_reward_norm_apply"] / med["fill 2 x 2 MiB"], 3),
                  "apply_GBs": round(2 * T * N * 4 / med["ppo_reward_norm_apply"] / 1e3, 1),
                  "stats": ppo_ops.reward_norm_read(stats)}), flush=True)
