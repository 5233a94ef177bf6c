"""Plain Python statement of the episodic count bonuses (include/twoarmy_ppo.h, ppo_bonus_scan_episode): a dict of counts
per env and kind that is emptied at every episode end, float64 with math.sqrt.  Independent of bonus_ref.py except for
the key rule.  The table layout of the header (stamped words, a generation per env) is restated next to it so that a
device table can be read and preset.  Test infrastructure only; nothing here runs on a GPU."""
import math

import numpy as np

from bonus_ref import key_of

KINDS = ("state", "action")
COUNT_BITS = 24
COUNT_MAX = (1 << COUNT_BITS) - 1                     # a count stays here once it gets here
GENERATIONS = 1 << (32 - COUNT_BITS)                  # 0 follows 255, and that step clears for real


def n_keys(kind, width=17, height=17, n_actions=7):
    return width * height + 1 if kind == "state" else width * height * 4 * n_actions + 1


def words(kind, N, width=17, height=17, n_actions=7):
    return N * (n_keys(kind, width, height, n_actions) + 1)


def value(c, scale, form):
    if form == "first":
        return float(scale) if c == 1 else 0.0
    return float(scale) * (1.0 / math.sqrt(float(c)))


class EpisodeBonusRef:
    """counts[kind][n]: {key: count} of env n's running episode; gen[kind][n]: episode ends seen so far mod 256, which
    is what the device keeps as its generation word.  scan() advances both and returns the outputs."""

    def __init__(self, N, kinds=("state",), scale=1.0, form="sqrt", width=17, height=17, n_actions=7):
        self.N, self.kinds, self.scale, self.form = N, tuple(k for k in KINDS if k in kinds), scale, form
        self.width, self.height, self.n_actions = width, height, n_actions
        self.counts = {k: [dict() for _ in range(N)] for k in self.kinds}
        self.gen = {k: [0] * N for k in self.kinds}

    def scan(self, pos, action, reward, terminated, truncated, keep=None, dirs=None):
        """pos [T,N,2] float32, action [T,N] | None, reward [T,N] float32, terminated / truncated [T,N], keep [T,N] | None,
        dirs [T,N] | [N] | None -> {"state", "action", "reward": f32[T,N], "count_state", "count_action": i64[T,N]}."""
        T, N = pos.shape[:2]
        action = np.zeros((T, N), np.int64) if action is None else np.asarray(action)
        dirs = np.zeros((T, N), np.int64) if dirs is None else np.broadcast_to(np.asarray(dirs), (T, N))
        b = {k: np.zeros((T, N), np.float64) for k in KINDS}
        cnt = {k: np.zeros((T, N), np.int64) for k in self.kinds}
        for n in range(N):
            for t in range(T):
                for kind in self.kinds:
                    key = key_of(kind, pos[t, n, 0], pos[t, n, 1], dirs[t, n], action[t, n], self.width, self.height,
                                 self.n_actions)
                    seen = self.counts[kind][n]
                    seen[key] = min(seen.get(key, 0) + 1, COUNT_MAX)
                    cnt[kind][t, n] = seen[key]
                    b[kind][t, n] = value(seen[key], self.scale, self.form)
                if terminated[t, n] or truncated[t, n]:             # the done step was counted and paid; now the clear
                    for kind in self.kinds:
                        self.counts[kind][n].clear()
                        self.gen[kind][n] = (self.gen[kind][n] + 1) % GENERATIONS
        out = {k: b[k].astype(np.float32) for k in self.kinds}
        out.update({"count_" + k: cnt[k] for k in self.kinds})
        r = np.asarray(reward, np.float32)
        shaped = ((r.astype(np.float64) + b["state"]) + b["action"]).astype(np.float32)
        out["reward"] = shaped if keep is None else np.where(np.asarray(keep) != 0, r, shaped)
        return out

    def table(self, kind):
        """The running episodes' counts as int64[N, K]."""
        out = np.zeros((self.N, n_keys(kind, self.width, self.height, self.n_actions)), np.int64)
        for n, seen in enumerate(self.counts[kind]):
            for key, c in seen.items():
                out[n, key] = c
        return out

    def preset(self, kind, counts, gen):
        """Start from the counts int64[N, K] and the generations [N] of a table made by encode()."""
        self.counts[kind] = [{int(k): int(row[k]) for k in np.flatnonzero(row)} for row in counts]
        self.gen[kind] = [int(g) for g in gen]


def decode(table, N):
    """The words of a device table (any integer dtype holding the 32-bit words) -> (counts int64[N, K], gen int64[N],
    stamps int64[N, K]) by the header's rule: a word counts while its stamp is its env's generation."""
    w = np.asarray(table).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    K = w.size // N - 1
    assert w.size == N * (K + 1)
    word, gen = w[:N * K].reshape(N, K), w[N * K:]
    stamp = word >> COUNT_BITS
    return np.where(stamp == gen[:, None], word & COUNT_MAX, 0), gen, stamp


def encode(counts, gen, stale=None):
    """int32 words of a table whose running counts are counts[N, K] under the generations gen[N].  stale: (stamp[N, K],
    count[N, K]) of words left over from earlier episodes, put wherever counts is 0 and the stamp is not the env's own."""
    counts, gen = np.asarray(counts, np.int64), np.asarray(gen, np.int64)
    word = np.where(counts > 0, gen[:, None] << COUNT_BITS | counts, 0)
    if stale is not None:
        stamp, old = (np.asarray(a, np.int64) for a in stale)
        word = np.where((counts == 0) & (stamp != gen[:, None]), stamp << COUNT_BITS | old, word)
    return np.concatenate([word.reshape(-1), gen]).astype(np.uint32).view(np.int32)
