"""Numpy restatement of the two episode-accounting contracts of include/twoarmy_ppo.h (ppo_episode_scan,
ppo_episode_summary): plain loops, float64, one operation per step in the stated order.  Test-side only."""
import numpy as np

REWARD_VALUES = (-0.01, -0.1, -0.9, 0.2, 0.9)


def episode_scan(reward, terminated, truncated, carry_return, carry_length):
    """reward float32 [T,N]; terminated / truncated [T,N]; carries [N].  Returns (ep_return f64 [T,N], ep_length i32
    [T,N], new carry_return, new carry_length).  Envs do not interact, so the loop over envs is written as an
    elementwise numpy operation: every env still sees one float64 addition per step, in step order."""
    reward = np.asarray(reward, dtype=np.float32)
    T, N = reward.shape
    done = (np.asarray(terminated) != 0) | (np.asarray(truncated) != 0)
    acc = np.array(carry_return, dtype=np.float64)
    length = np.array(carry_length, dtype=np.int32)
    ep_return = np.empty((T, N), np.float64)
    ep_length = np.empty((T, N), np.int32)
    for t in range(T):
        acc = acc + reward[t].astype(np.float64)
        length = length + np.int32(1)
        ep_return[t] = acc
        ep_length[t] = length
        acc = np.where(done[t], 0.0, acc)
        length = np.where(done[t], np.int32(0), length).astype(np.int32)
    return ep_return, ep_length, acc, length


def episode_summary(ep_return, ep_length, terminated, truncated, reward, action=None, n_actions=5, keep=0.99, gain=0.01,
                    score=0.0):
    """Sequential statement of ppo_episode_summary: done steps visited in row-major (t, then n) order."""
    terminated, truncated = np.asarray(terminated) != 0, np.asarray(truncated) != 0
    reward = np.asarray(reward, dtype=np.float32)
    out = dict(episodes=0, successes=0, truncated=0, return_sum=0.0, min_return=np.inf, max_return=-np.inf, length_sum=0,
               max_length=0, abs_return_sum=0.0)
    score = float(score)
    ts, ns = np.nonzero(terminated | truncated)                       # row-major order
    for t, n in zip(ts.tolist(), ns.tolist()):
        R, L = float(ep_return[t, n]), int(ep_length[t, n])
        score = score * keep + R * gain
        out["episodes"] += 1
        if terminated[t, n]:
            out["successes"] += 1
        else:
            out["truncated"] += 1
        out["return_sum"] += R
        out["abs_return_sum"] += abs(R)
        out["min_return"] = min(out["min_return"], R)
        out["max_return"] = max(out["max_return"], R)
        out["length_sum"] += L
        out["max_length"] = max(out["max_length"], L)
    out["score"] = score
    hist = [int((reward == np.float32(v)).sum()) for v in REWARD_VALUES]
    out["reward_hist"] = hist + [int(reward.size - sum(hist))]
    if action is None:
        out["action_hist"] = [0] * n_actions
    else:
        action = np.asarray(action)
        out["action_hist"] = [int((action == a).sum()) for a in range(n_actions)]
    return out


def golden_columns():
    """The 16 random traces of tests/golden/twoarmy_traces.npz (rand_v6_0..5, rand_v4_0..9) without their reset rows:
    {variant: list of (reward float64 [L], term [L], trunc [L])}, the rewards as the reference recorded them."""
    from golden_util import load_traces
    traces, _ = load_traces()
    cols = {6: [], 4: []}
    for tr in traces:
        name = str(tr["name"])
        if not name.startswith("rand_v"):
            continue
        keep = tr["op"] != -1                                          # reset rows carry no step
        r = tr["reward"][keep].astype(np.float64)
        assert not np.isnan(r).any()
        cols[int(name[6])].append((r, tr["term"][keep].astype(np.uint8), tr["trunc"][keep].astype(np.uint8)))
    return cols


def reference_loop(reward, term, trunc, keep=0.99, gain=0.01, score=0.0):
    """The reference's bookkeeping, literally (soa/train_ppo.py:124,136-141), on one env's recorded Python-float
    rewards: returns (list of (step index, ep_reward, ep_len) per finished episode, running_score)."""
    episodes, ep_reward, ep_len, running_score = [], 0.0, 0, float(score)
    for t in range(len(reward)):
        ep_reward += float(reward[t])
        ep_len += 1
        if term[t] or trunc[t]:
            running_score = running_score * keep + ep_reward * gain
            episodes.append((t, ep_reward, ep_len))
            ep_reward, ep_len = 0.0, 0
    return episodes, running_score


def stacked(cols):
    """Columns of one variant (equal lengths) as [T][N] arrays: float32 rewards (what the kernels get), uint8 flags."""
    r = np.stack([c[0] for c in cols], 1).astype(np.float32)
    return r, np.stack([c[1] for c in cols], 1), np.stack([c[2] for c in cols], 1)
