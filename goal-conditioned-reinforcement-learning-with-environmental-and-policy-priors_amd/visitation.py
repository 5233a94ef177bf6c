"""Visited cells on the device: the visit-count matrix the reference builds for its heatmap after every PPO.update
(soa/agent/PPO.py:161 -> soa/img_proccess/heatmap.py:58-81, `values_matrix[y, x] += 1` over the buffer's after-step
positions, hindsight copies included) and how many distinct cells each episode covered.  One ppo_visit_scan and three or
four ppo_visit_hist launches per rollout (include/twoarmy_ppo.h) and no host synchronisation until read().  The seaborn
pictures are not drawn."""
import torch

from . import ppo_ops

MAPS = ("rollout", "first_visit_map", "terminal_map", "cumulative")


class VisitTracker:
    def __init__(self, num_envs, device, width=17, height=17):
        self.N, self.device = int(num_envs), torch.device(device)
        self.width, self.height = int(width), int(height)
        self.cells = self.width * self.height
        d = self.device
        self.carry = torch.zeros(ppo_ops.visit_carry_words(self.width, self.height, self.N), dtype=torch.int32, device=d)
        # one buffer, one copy in read(): the four maps [cells + 1] each (last entry: positions outside the grid), then
        # {episodes, sum, min, max} of the cells covered by the episodes the last account() finished
        self._buf = torch.zeros(4 * (self.cells + 1) + 4, dtype=torch.int64, device=d)
        maps = self._buf[:4 * (self.cells + 1)].view(4, self.cells + 1)
        self.rollout, self.first_visit_map, self.terminal_map, self.cumulative = maps[0], maps[1], maps[2], maps[3]
        self._stats = self._buf[4 * (self.cells + 1):]
        self.first_visit = self.ep_cells = None                             # sized by the first account()

    def reset(self):
        """Forget the running episodes (envs were reset); the maps stay."""
        self.carry.zero_()

    def account(self, pos, terminated, truncated, her=None):
        """Account one rollout: pos [T,N,2] (y, x) after each step, terminated / truncated [T,N] (or one step: [N,2],
        [N]); her: the hindsight records of VecPPOTrainer.relabel() (their "t", "n" index this rollout), counted into
        `rollout` like the reference's appended copies.  Afterwards first_visit / ep_cells [T,N] hold the scan's
        outputs, rollout / first_visit_map / terminal_map this rollout's counts and cumulative the sum of all rollouts."""
        if pos.dim() == 2:
            pos, terminated, truncated = pos.view(1, -1, 2), terminated.view(1, -1), truncated.view(1, -1)
        T, N = terminated.shape
        assert N == self.N, "tracker made for %d envs, got %d" % (self.N, N)
        if self.first_visit is None or self.first_visit.shape[0] != T:
            self.first_visit = torch.empty((T, N), dtype=torch.uint8, device=self.device)
            self.ep_cells = torch.empty((T, N), dtype=torch.int32, device=self.device)
        w, h = self.width, self.height
        ppo_ops.visit_scan(pos, terminated, truncated, self.carry, w, h, out=(self.first_visit, self.ep_cells))
        done = terminated | truncated
        self._buf[:3 * (self.cells + 1)].zero_()
        ppo_ops.visit_hist(pos, self.rollout, w, h)
        if her is not None:
            ppo_ops.visit_hist(pos, self.rollout, w, h, t_idx=her["t"], n_idx=her["n"])
        ppo_ops.visit_hist(pos, self.first_visit_map, w, h, mask=self.first_visit)
        ppo_ops.visit_hist(pos, self.terminal_map, w, h, mask=done)
        self.cumulative += self.rollout
        ended = done != 0
        cells = self.ep_cells.long()
        self._stats[0] = ended.sum()
        self._stats[1] = (cells * ended).sum()
        self._stats[2] = torch.where(ended, cells, self.cells + 1).min()
        self._stats[3] = torch.where(ended, cells, -1).max()

    def read(self):
        """The maps as [height, width] int64 numpy arrays, `other` (records of `rollout` outside the grid) and the cells
        covered by the episodes that finished in the last account() (one device-to-host copy: the one sync)."""
        host = self._buf.cpu().numpy()
        maps = host[:4 * (self.cells + 1)].reshape(4, self.cells + 1)
        out = {name: maps[i, :self.cells].reshape(self.height, self.width).copy() for i, name in enumerate(MAPS)}
        out["other"] = int(maps[0, self.cells])                              # of `rollout`: rollout.sum() + other = records
        out["other_by_map"] = {name: int(maps[i, self.cells]) for i, name in enumerate(MAPS)}
        E, total, lo, hi = (int(x) for x in host[4 * (self.cells + 1):])
        out["episodes"] = E
        out["cells_mean"] = total / E if E else None
        out["cells_min"] = lo if E else None
        out["cells_max"] = hi if E else None
        return out
