"""Episode accounting on the device: per-episode return and length carried across rollouts, a summary of the
episodes each rollout finished, and the reference's running score (soa/train_ppo.py:124,136-141) folded over them
one by one.  Two kernel launches per rollout (ppo_episode_scan, ppo_episode_summary; include/twoarmy_ppo.h) and no
host synchronisation until read()."""
import torch

from . import ppo_ops

REWARD_BUCKETS = (-0.01, -0.1, -0.9, 0.2, 0.9, "other")       # reward_hist columns
SUMMARY_FIELDS = ("episodes", "successes", "truncated", "return_sum", "min_return", "max_return", "length_sum",
                  "max_length")


class EpisodeTracker:
    def __init__(self, num_envs, device, n_actions=5, keep=0.99, gain=0.01):
        self.N, self.device = int(num_envs), torch.device(device)
        self.n_actions, self.keep, self.gain = int(n_actions), float(keep), float(gain)
        d = self.device
        self.carry_return = torch.zeros(self.N, dtype=torch.float64, device=d)
        self.carry_length = torch.zeros(self.N, dtype=torch.int32, device=d)
        self.score = torch.zeros(1, dtype=torch.float64, device=d)          # running score, on the device
        self.summary = torch.zeros(8, dtype=torch.float64, device=d)
        self.action_hist = torch.zeros(self.n_actions, dtype=torch.int64, device=d)
        self.reward_hist = torch.zeros(6, dtype=torch.int64, device=d)
        self.summary[4], self.summary[5] = float("inf"), float("-inf")      # nothing accounted yet: no finished episode
        self.ep_return = self.ep_length = self._workspace = None            # sized by the first account()

    def reset(self):
        """Forget the running episodes (envs were reset); the score and the last summary stay."""
        self.carry_return.zero_()
        self.carry_length.zero_()

    def account(self, reward, terminated, truncated, action=None):
        """Account one rollout [T,N] (or one step [N]).  Afterwards ep_return / ep_length [T,N] hold, at every done
        step, the return and length of the episode that ends there, and summary / histograms / score are updated."""
        if reward.dim() == 1:
            reward, terminated, truncated = reward.view(1, -1), terminated.view(1, -1), truncated.view(1, -1)
            action = None if action is None else action.view(1, -1)
        T, N = reward.shape
        assert N == self.N, "tracker made for %d envs, got %d" % (self.N, N)
        if self.ep_return is None or self.ep_return.shape[0] != T:
            self.ep_return = torch.empty((T, N), dtype=torch.float64, device=self.device)
            self.ep_length = torch.empty((T, N), dtype=torch.int32, device=self.device)
            self._workspace = torch.empty(ppo_ops.episode_summary_workspace(T, N), dtype=torch.float64, device=self.device)
        ppo_ops.episode_scan(reward, terminated, truncated, self.carry_return, self.carry_length,
                             out=(self.ep_return, self.ep_length))
        ppo_ops.episode_summary(self.ep_return, self.ep_length, terminated, truncated, reward, action, self.n_actions,
                                self.keep, self.gain, self.score, self.summary, self.action_hist, self.reward_hist,
                                self._workspace)

    def read(self):
        """The last account()'s summary and the score as Python numbers (one device-to-host copy: the one sync)."""
        host = torch.cat([self.summary, self.score, self.action_hist.double(), self.reward_hist.double()]).cpu().tolist()
        out = dict(zip(SUMMARY_FIELDS, host[:8]))
        for k in ("episodes", "successes", "truncated", "length_sum", "max_length"):
            out[k] = int(out[k])
        E = out["episodes"]
        out["mean_return"] = out["return_sum"] / E if E else None
        out["mean_length"] = out["length_sum"] / E if E else None
        out["success_rate"] = out["successes"] / E if E else None
        out["score"] = host[8]
        out["action_hist"] = [int(x) for x in host[9:9 + self.n_actions]]
        out["reward_hist"] = [int(x) for x in host[9 + self.n_actions:]]
        return out
