"""Plain numpy / dict statement of the exploration bonuses (include/twoarmy_ppo.h, ppo_bonus_scan): the reference's
StateBonus / ActionBonus wrappers (gym_minigrid/wrappers.py:34-102) for N envs, both scopes, keep mask, `other` slot.
Test infrastructure only; nothing here runs on a GPU."""
import math

import numpy as np


def cell_of(y, x, width, height):
    """visit_cell: valid iff 0 <= y < height and 0 <= x < width as float32 comparisons; None = outside."""
    y, x = np.float32(y), np.float32(x)
    if y >= 0 and y < np.float32(height) and x >= 0 and x < np.float32(width):     # NaN / inf fail
        return int(y) * width + int(x)
    return None


def key_of(kind, y, x, d, a, width, height, n_actions):
    """Table index of a step; the last slot K - 1 takes everything invalid."""
    c = cell_of(y, x, width, height)
    if kind == "state":
        return width * height if c is None else c
    if c is None or not (0 <= d < 4) or not (0 <= a < n_actions):
        return width * height * 4 * n_actions
    return (c * 4 + int(d)) * n_actions + int(a)


def table_size(kind, width, height, n_actions):
    return width * height + 1 if kind == "state" else width * height * 4 * n_actions + 1


def bonus_value(c, scale):
    return float(scale) * (1.0 / math.sqrt(float(c)))


class BonusRef:
    """tables[kind]: env scope [N][K] python ints, shared scope [K]; scan() advances them and returns the outputs."""

    def __init__(self, N, kinds=("state",), scope="env", scale=1.0, width=17, height=17, n_actions=7):
        self.N, self.kinds, self.scope, self.scale = N, tuple(k for k in ("state", "action") if k in kinds), scope, scale
        self.width, self.height, self.n_actions = width, height, n_actions
        self.tables = {k: np.zeros((N if scope == "env" else 1, table_size(k, width, height, n_actions)), np.int64)
                       for k in self.kinds}

    def keys(self, kind, pos, action, dirs):
        T, N = pos.shape[:2]
        out = np.empty((T, N), np.int64)
        for t in range(T):
            for n in range(N):
                out[t, n] = key_of(kind, pos[t, n, 0], pos[t, n, 1], dirs[t, n], action[t, n], self.width, self.height,
                                   self.n_actions)
        return out

    def scan(self, pos, action, reward, keep=None, dirs=None):
        """pos [T,N,2] float32, action [T,N], reward [T,N] float32, keep [T,N] | None, dirs [T,N] | [N] | None.
        Returns {"state": f32[T,N], "action": f32[T,N], "reward": f32[T,N], "count_state", "count_action": i64[T,N]}."""
        T, N = pos.shape[:2]
        action = np.zeros((T, N), np.int64) if action is None else np.asarray(action)
        dirs = np.zeros((T, N), np.int64) if dirs is None else np.broadcast_to(np.asarray(dirs), (T, N))
        b = {k: np.zeros((T, N), np.float64) for k in ("state", "action")}
        out = {}
        for kind in self.kinds:
            keys = self.keys(kind, pos, action, dirs)
            cnt = np.zeros((T, N), np.int64)
            tab = self.tables[kind]
            for t in range(T):
                if self.scope == "shared":                    # the row is simultaneous: count it all, then read
                    for n in range(N):
                        tab[0, keys[t, n]] += 1
                    for n in range(N):
                        cnt[t, n] = tab[0, keys[t, n]]
                else:
                    for n in range(N):
                        tab[n, keys[t, n]] += 1
                        cnt[t, n] = tab[n, keys[t, n]]
            for t in range(T):
                for n in range(N):
                    b[kind][t, n] = bonus_value(cnt[t, n], self.scale)
            out[kind] = b[kind].astype(np.float32)
            out["count_" + kind] = cnt
        r = np.asarray(reward, np.float32)
        shaped = ((r.astype(np.float64) + b["state"]) + b["action"]).astype(np.float32)
        out["reward"] = shaped if keep is None else np.where(np.asarray(keep) != 0, r, shaped)
        return out


def shared_by_definition(keys, carry):
    """c(t, n) = carry[key] + #{(t', n') : t' <= t, key(t', n') = key}, written as the double loop it is."""
    T, N = keys.shape
    out = np.zeros((T, N), np.int64)
    for t in range(T):
        for n in range(N):
            c = carry.get(int(keys[t, n]), 0)
            for t2 in range(t + 1):
                for n2 in range(N):
                    c += int(keys[t2, n2] == keys[t, n])
            out[t, n] = c
    return out
