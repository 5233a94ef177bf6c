"""Numpy restatement of the two visit-counting contracts of include/twoarmy_ppo.h (ppo_visit_scan, ppo_visit_hist) in
plain loops, and the two statements of the reference they are checked against, literally: the heatmap loop
(soa/img_proccess/heatmap.py:58-63) and the goal-candidate set of her_func (soa/env_buffer.py:138).  Test-side only."""
import numpy as np


def cell_of(y, x, width, height):
    """Row-major cell of (y, x), or width * height ("other") when the position is outside the grid.  The comparisons are
    float32 ones: NaN and +-inf fail them, -0.0 passes as 0."""
    y, x = np.float32(y), np.float32(x)
    if y >= 0 and y < np.float32(height) and x >= 0 and x < np.float32(width):
        return int(y) * width + int(x)
    return width * height


def visit_scan(pos, terminated, truncated, width, height, seen=None):
    """pos [T,N,2]; terminated / truncated [T,N]; seen: list of N sets of cells (None: all empty).  Returns (first_visit
    u8 [T,N], ep_cells i32 [T,N], the N sets after the last step)."""
    pos = np.asarray(pos, np.float32)
    T, N = pos.shape[:2]
    seen = [set() for _ in range(N)] if seen is None else [set(s) for s in seen]
    first = np.zeros((T, N), np.uint8)
    cells = np.zeros((T, N), np.int32)
    for n in range(N):
        s = seen[n]
        for t in range(T):
            c = cell_of(pos[t, n, 0], pos[t, n, 1], width, height)
            if c < width * height:
                if c not in s:
                    first[t, n] = 1
                s.add(c)
            cells[t, n] = len(s)
            if terminated[t, n] or truncated[t, n]:
                s.clear()
    return first, cells, seen


def visit_hist(pos, width, height, mask=None, t_idx=None, n_idx=None, counts=None):
    """counts int64 [width*height + 1] (a copy of `counts`, or zeros) plus one per record: dense over (t, n) with a
    non-zero mask, or over the listed (t_idx[b], n_idx[b]); records outside [0,T) x [0,N) count as other."""
    pos = np.asarray(pos, np.float32)
    T, N = pos.shape[:2]
    out = np.zeros(width * height + 1, np.int64) if counts is None else np.array(counts, np.int64)
    if t_idx is None:
        for t in range(T):
            for n in range(N):
                if mask is None or mask[t, n] != 0:
                    out[cell_of(pos[t, n, 0], pos[t, n, 1], width, height)] += 1
    else:
        for t, n in zip(np.asarray(t_idx).tolist(), np.asarray(n_idx).tolist()):
            inside = 0 <= t < T and 0 <= n < N
            out[cell_of(pos[t, n, 0], pos[t, n, 1], width, height) if inside else width * height] += 1
    return out


def sets_to_carry(seen, width, height):
    """The kernel's carry layout: bit c & 31 of word [c >> 5][n], word-major over envs, flattened."""
    words = (width * height + 31) // 32
    carry = np.zeros((words, len(seen)), np.uint32)
    for n, s in enumerate(seen):
        for c in s:
            carry[c >> 5, n] |= np.uint32(1) << np.uint32(c & 31)
    return carry.reshape(-1)


def carry_to_sets(carry, n_envs, width, height):
    words = (width * height + 31) // 32
    carry = np.asarray(carry).view(np.uint32).reshape(words, n_envs)
    return [{c for c in range(width * height) if (int(carry[c >> 5, n]) >> (c & 31)) & 1} for n in range(n_envs)]


# ------------------------------------------------------------------ the reference, literally
def reference_heatmap(p):
    """heatmap.py:58-63 on buffer['p'][:, 4]: a 17x17 matrix, values_matrix[int(y), int(x)] += 1 per record."""
    values_matrix = np.zeros((17, 17))
    for i in range(len(p)):
        values_matrix[int(p[i][0]), int(p[i][1])] += 1
    return values_matrix


def reference_goal_candidates(episode_p):
    """env_buffer.py:138: the first index of every distinct achieved (y, x) of one episode, and how many there are."""
    uniq, index = np.unique(np.asarray(episode_p), axis=0, return_index=True)
    return sorted(index.tolist()), len(uniq)


def golden_columns():
    """The 16 random traces of tests/golden/twoarmy_traces.npz without their reset rows:
    {variant: list of (pos float32 [L,2] (y, x) after each step, term u8 [L], trunc u8 [L])}."""
    from golden_util import load_traces
    traces, _ = load_traces()
    cols = {6: [], 4: []}
    for tr in traces:
        name = str(tr["name"])
        if not name.startswith("rand_v"):
            continue
        keep = tr["op"] != -1                                          # reset rows carry no step
        cols[int(name[6])].append((tr["pos"][keep][:, 0:2].astype(np.float32), tr["term"][keep].astype(np.uint8),
                                   tr["trunc"][keep].astype(np.uint8)))
    return cols


def stacked(cols):
    """Columns of one variant (equal lengths) as time-major arrays: pos [T,N,2], term / trunc [T,N]."""
    return (np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1), np.stack([c[2] for c in cols], 1))


def her_buffers():
    """The reference's recorded buffers with their hindsight copies: [(name, p float32 [rows, 2])] for the 7 cases of
    tests/golden/her.npz, before and after her_func; p = buffer['p'][:, 4], the position after the transition."""
    import os
    from golden_util import GOLDEN
    z = np.load(os.path.join(GOLDEN, "her.npz"))
    out = []
    for c in range(7):
        for when in ("before", "after"):
            name = "c%d_%s_p" % (c, when)
            out.append((name, z[name][:, 4].astype(np.float32)))
    return out
