"""float64 statement of ppo_gae_runs and a numpy restatement of ppo_run_ends (include/twoarmy_ppo.h), shared by
test_gae_runs_cpu.py, test_gae_runs_gpu.py and the two cases of test_streams_gpu.py, with the record generator and the
rounding bound of the scan they use.  A plain module like update_stats_ref.py; it mirrors _gae64 of
test_ppo_kernels_edges_gpu.py, along a flat record array cut at the run ends instead of along the columns of a tile."""
import numpy as np

EPS32 = 2.0 ** -23
CHUNK, BLOCK = 64, 2048                          # records per shuffle scan / per workgroup (GR_BLOCK)


def run_ends(t, n, goal, done):
    """(run_end uint8[H], broken): run_end_j = 0 iff record j is not done and record j + 1 is the next step of the same
    env under the same goal (float compares: NaN never links, -0.0 == +0.0); broken = records that are not done and
    still end a run."""
    t, n, goal, done = np.asarray(t, np.int64), np.asarray(n), np.asarray(goal), np.asarray(done)
    H = len(t)
    link = np.zeros(H, bool)
    link[:-1] = (done[:-1] == 0) & (n[1:] == n[:-1]) & (t[1:] == t[:-1] + 1) & (goal[1:, 0] == goal[:-1, 0]) & \
        (goal[1:, 1] == goal[:-1, 1])
    return (~link).astype(np.uint8), int(((done == 0) & ~link).sum())


def gae_runs64(r, v, nv, done, run_end, gamma, lam, use_mask):
    """The formula in float64 on the float32 inputs, parameters as the kernel sees them: fp32(gamma) and
    c = fp32(fp32(gamma) * fp32(lambda)) * cut, c = 0 at a run end and at the last record.  Where c = 0, A_j = delta_j
    exactly (nothing behind enters).  Returns adv, target, ret, the magnitude sum
    S_j = sum over k >= j of the same run of prod(c) * (|r_k| + |gamma nv_k| + |v_k|), and L_j = the number of records
    k >= j that enter A_j (1 where c_j = 0)."""
    g32 = np.float32(gamma)
    c32 = float(np.float32(g32 * np.float32(lam)))
    H = len(r)
    cut = (1.0 - (np.asarray(done) != 0)) if use_mask else np.ones(H)
    r, v, nv = (np.asarray(x, np.float32).astype(np.float64) for x in (r, v, nv))
    tgt = r + float(g32) * nv * cut
    delta = tgt - v
    mag = np.abs(r) + np.abs(float(g32) * nv) + np.abs(v)
    c = c32 * cut
    c[np.asarray(run_end) != 0] = 0.0
    c[H - 1] = 0.0
    adv, S, L = np.zeros(H), np.zeros(H), np.ones(H, np.int64)
    nxt, snx, lnx = 0.0, 0.0, 0
    cl, dl, ml = c.tolist(), delta.tolist(), mag.tolist()
    for j in range(H - 1, -1, -1):
        if cl[j] != 0.0:
            nxt, snx, lnx = dl[j] + cl[j] * nxt, ml[j] + cl[j] * snx, lnx + 1
        else:
            nxt, snx, lnx = dl[j], ml[j], 1
        adv[j], S[j], L[j] = nxt, snx, lnx
    return adv, tgt, adv + v, S, L


def one_step32(r, v, nv, done, gamma, use_mask):
    """The one-step formula in float32 with the reference's rounding order (PPO.py:113-114): target, delta."""
    r, v, nv = (np.asarray(x, np.float32) for x in (r, v, nv))
    cut = (1 - (np.asarray(done) != 0)).astype(np.float32) if use_mask else np.ones(len(r), np.float32)
    t32 = r + (np.float32(gamma) * nv) * cut
    return t32, t32 - v


def inputs(H, seed):
    rs = np.random.RandomState(seed)
    r, v, nv = (rs.randn(H).astype(np.float32) for _ in range(3))
    return r, v, nv


def pattern(kind, H, seed=0):
    """run_end uint8[H] of a run pattern: "singletons"; "runs64" / "runs64+1": runs of exactly 64 from index 0 / 1;
    "her": random lengths 1..64; "one1000": one run of 1000 amid random short ones (H >= 3000); "whole": one run."""
    e = np.zeros(H, np.uint8)
    if kind == "singletons":
        e[:] = 1
    elif kind in ("runs64", "runs64+1"):
        first = 0 if kind == "runs64" else 1
        e[first + 63::64] = 1
        if first:
            e[0] = 1
    elif kind in ("her", "one1000"):
        rs = np.random.RandomState(1000 + seed)
        ends = np.cumsum(rs.randint(1, 65, H)) - 1
        e[ends[ends < H]] = 1
        if kind == "one1000":
            assert H >= 3000
            a = 2048 - 300                                     # starts in one 2048-record workgroup, ends in the next
            e[a - 1] = 1
            e[a:a + 1000] = 0
            e[a + 999] = 1
    else:
        assert kind == "whole"
    e[H - 1] = 1
    return e


def dones(run_end, seed, mid_run=0.02):
    """Done flags in the shape of hindsight records: every run end is done, plus a few done records inside runs (which
    the done mask cuts at and reference mode scans through)."""
    rs = np.random.RandomState(2000 + seed)
    return (run_end | (rs.rand(len(run_end)) < mid_run)).astype(np.uint8)


def _records(H, seed):
    """Records in ppo_her_relabel's shape: runs of 1..64 consecutive steps of one env under one goal, each ending done."""
    rs = np.random.RandomState(seed)
    end = pattern("her", H, seed)
    run = np.concatenate([[0], np.cumsum(end)[:-1]]).astype(np.int64)          # run index of every record
    start = np.concatenate([[0], np.nonzero(end)[0] + 1])[run]
    t = (rs.randint(0, 50, run.max() + 1)[run] + np.arange(H) - start).astype(np.int32)
    n = rs.randint(0, 64, run.max() + 1)[run].astype(np.int32)
    goal = rs.randint(0, 17, (run.max() + 1, 2))[run].astype(np.float32)
    done = end.copy()
    done[H - 1] = rs.randint(0, 2)                                 # the array may stop in mid-run
    return t, n, goal, done


def _levels(H):
    levels, n = 1, H
    while n > BLOCK:
        n, levels = -(-n // BLOCK), levels + 1
    return levels


def _k(L, H):
    """k of |adv - adv64| <= k * EPS32 * S_j, counted in roundings of 2^-24 = EPS32 / 2 (each relative to a partial
    magnitude <= S_j) along the longest path of one term delta_k, k >= j, into A_j; L_j terms enter A_j.

    Every term: 3 roundings of delta (gamma * nv, + r, - v).  Its coefficient is a product of k - j <= L_j - 1 factors c,
    joined pairwise by the shuffle scan, the folds and the carries: at most L_j - 2 multiplications (any order of
    evaluation, a serial one too, rounds a product of m factors m - 1 times).

    L_j <= 64: the terms lie in the chunk of j and the next one.  The partial sum a term sits in is rounded by the <= 6
    fmas of the shuffle scan of its own chunk, by the fma that takes the value into the chunk (gr_eval), and, if it comes
    from the next chunk, by the fma of gr_eval in the chunk of j: <= 8.  The run ends inside that next chunk, so its
    composite has c = 0, and whatever lies between the two chunks -- a wavefront's fold, a workgroup's composite, the
    levels above -- hands (0, d) on through the c == 0 branches without arithmetic.  3 + 62 + 8 = 73, one more for the
    second-order terms of (1 + 2^-24)^73: k = 74 / 2 = 37, whatever H and wherever the run lies.

    Longer runs: the sum a term sits in is rounded, per level of the tree it visits, by <= 6 shuffle fmas + 8 chunk folds
    + 4 wavefront folds on the way up and <= 3 wavefronts + 8 chunks + 1 on the way down: 31.  A run inside one
    workgroup visits level 0 only; a run that crosses a workgroup carry visits at most every level H has.  So
    2 k = 3 + (L_j - 1) + 31 * levels visited + 1.  The run length enters because the coefficient of the farthest term is
    a product of L_j - 1 factors; a run that crosses w carries has L_j <= 2048 (w + 1)."""
    j = np.arange(len(L))
    crosses = (j // BLOCK) != ((j + L - 1) // BLOCK)
    visited = np.where(crosses, _levels(H), 1)
    return np.where(L <= CHUNK, 37.0, (L + 3 + 31 * visited) / 2.0)
