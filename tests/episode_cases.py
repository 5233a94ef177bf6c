"""What tests/test_episode_edges_cpu.py and tests/test_episode_kernels_edges_gpu.py share: the grid rule of
ppo_episode_summary as include/twoarmy_ppo.h states it, the inputs of every case, the references of the score fold
(float64 sequential, exact rational, long double) and the bounds the device results are held to.  The bounds are derived
here from the number formats and the documented tree and checked on the CPU; no device output enters them.
Test-side only."""
import fractions
import functools

import numpy as np

import episode_ref as ER

U = 2.0 ** -53                                  # unit roundoff of float64, round to nearest
# The header's grid rule (include/twoarmy_ppo.h, ppo_episode_summary): elements a workgroup is sized for, the cap on
# workgroups, threads per workgroup, lanes of the final pass.  BATCH: a thread reads its run 8 elements at a time
# ("Episode accounting"), so a run longer than 8 is the first that loops.
BLOCK_ELEMS, MAX_BLOCKS, THREADS, LANES, BATCH = 2048, 256, 256, 64, 8
TREE_COMBINES = 6 + 3 + 4 + 6                   # lane levels, wavefronts, partials of one lane, lane levels
SWEEP_M = (1, 255, 256, 257, 2047, 2048, 2049, 131072, 131073, 524288, 524289)
PATH_SWEEP_M = SWEEP_M[4:]
CAP_SHAPES = {524288: (128, 4096), 524289: (3, 174763)}
ACTION_COUNTS = (2, 3, 4, 5, 7)
KEEP_GAIN = ((0.0, 1.0), (1.0, 1.0), (1.0, 0.0), (0.99, 0.01))
SCORE0 = 0.3125
INT32_MIN = -2 ** 31
EXACT_EPISODES = 2000                           # up to here the reference of the fold is the exact rational one


def ceil_div(a, b):
    return -(-a // b)


def grid(M):
    """The grid of ppo_episode_summary for M = T * N elements, by the header's rule."""
    nblocks = min(ceil_div(M, BLOCK_ELEMS), MAX_BLOCKS)
    per_block = ceil_div(M, nblocks)
    return dict(nblocks=nblocks, per_block=per_block, per_thread=ceil_div(per_block, THREADS),
                per_lane=ceil_div(nblocks, LANES))


def block_share(M, b):
    """[lo, hi) of workgroup b."""
    g = grid(M)
    return min(b * g["per_block"], M), min((b + 1) * g["per_block"], M)


def thread_run(M, b, i):
    """[lo, hi) of thread i of workgroup b; lo >= hi: the run is empty."""
    g = grid(M)
    lo, hi = block_share(M, b)
    return lo + i * g["per_thread"], min(lo + (i + 1) * g["per_thread"], hi)


def boundaries(M):
    """Indices a done step is placed on: the first and last element of the whole range, of every workgroup's share, and
    of the runs of the first, second, last threads of a wavefront and of the last thread that has a run, in the first,
    second and last workgroup."""
    g = grid(M)
    idx = {0, M - 1}
    for b in range(g["nblocks"]):
        lo, hi = block_share(M, b)
        assert lo < hi
        idx |= {lo, hi - 1}
    for b in sorted({0, 1, g["nblocks"] - 1} & set(range(g["nblocks"]))):
        lo, hi = block_share(M, b)
        last = ceil_div(hi - lo, g["per_thread"]) - 1
        for i in sorted({0, 1, 63, 64, 127, 128, 255, last} & set(range(last + 1))):
            tlo, thi = thread_run(M, b, i)
            assert tlo < thi
            idx |= {tlo, thi - 1}
    return np.array(sorted(idx), np.int64)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def summary_case(M, every=False):
    """Flat synthetic inputs of ppo_episode_summary for M elements in row-major order: done steps at a low random
    density plus boundaries(M) (every=True: all of them), a quiet NaN return and an INT32_MIN length wherever no episode
    ends, rewards of the five task values and one other, actions in [-1, 8]."""
    rng = np.random.default_rng(77 + M + (1 << 20) * every)
    done = rng.random(M) < min(0.05, 1200.0 / M)
    done[boundaries(M)] = True
    if every:
        done[:] = True
    term = done & (rng.random(M) < 0.6)
    trunc = done & (~term | (rng.random(M) < 0.2))
    ep_return = np.full(M, np.nan)
    ep_return[done] = rng.uniform(-2.5, 2.5, int(done.sum()))
    ep_length = np.full(M, INT32_MIN, np.int32)
    ep_length[done] = rng.integers(1, 51, int(done.sum()))
    reward = rng.choice(np.array(ER.REWARD_VALUES + (0.5,), np.float32), M)
    action = rng.integers(-1, 9, M).astype(np.int32)
    return _freeze(dict(M=M, done=done, term=term.astype(np.uint8), trunc=trunc.astype(np.uint8), ep_return=ep_return,
                        ep_length=ep_length, reward=reward, action=action, returns=ep_return[done]))


ORDER_EPISODES = 36
ORDER_SHAPES = {2049: (3, 683), 131073: (43691, 3)}
ORDER_KEEP, ORDER_GAIN = 0.5, 1.0


@functools.lru_cache(maxsize=None)
def order_case(M):
    """Inputs that tell one order of the fold from another, for keep = 0.5, gain = 1: E = 36 episodes, the i-th with the
    return r_i * 2^(E-1-i), 1 <= |r_i| < 2, so that every episode contributes about r_i to the score (the returns span
    eleven orders of magnitude) and exchanging any two of them moves the score by about |r_i - 2 r_j| >> the bound.
    They lie at both ends of thread runs, wavefronts, workgroup shares, the final pass's lanes and the whole range, the
    rest at random.  The shape is ORDER_SHAPES[M]: a column-major walk visits them in another order."""
    T, N = ORDER_SHAPES[M]
    assert T * N == M
    g = grid(M)
    pb, pt, E = g["per_block"], g["per_thread"], ORDER_EPISODES
    rng = np.random.default_rng(5 + M)
    must = {0, 1, pt - 1, pt, 64 * pt - 1, 64 * pt, pb - 1, pb, pb + 1, M - 1}
    if g["nblocks"] > 2:
        must |= {2 * pb - 1, 2 * pb, (g["nblocks"] - 2) * pb, (g["nblocks"] - 1) * pb - 1, (g["nblocks"] - 1) * pb}
    idx = set(must)
    while len(idx) < E:
        idx.add(int(rng.integers(0, M)))
    idx = np.array(sorted(idx), np.int64)
    assert len(idx) == E and idx[-1] == M - 1
    done = np.zeros(M, bool)
    done[idx] = True
    r = rng.uniform(1.0, 2.0, E) * rng.choice([-1.0, 1.0], E)
    ep_return = np.full(M, np.nan)
    ep_return[idx] = r * 2.0 ** (E - 1 - np.arange(E))
    ep_length = np.full(M, INT32_MIN, np.int32)
    ep_length[idx] = rng.integers(1, 51, E)
    term = done & (rng.random(M) < 0.5)
    reward = rng.choice(np.array(ER.REWARD_VALUES, np.float32), M)
    return _freeze(dict(M=M, T=T, N=N, done=done, idx=idx, term=term.astype(np.uint8), trunc=(done & ~term).astype(np.uint8),
                        ep_return=ep_return, ep_length=ep_length, reward=reward, action=None, returns=ep_return[idx]))


def column_major(c):
    """The done steps' returns of an order case as a column-major (n, then t) walk meets them."""
    t, n = np.divmod(c["idx"], c["N"])
    return c["ep_return"][c["idx"][np.lexsort((t, n))]]


def swapped_shares(c, b):
    """The same with the shares of workgroups b and b + 1 exchanged (each share in its own order)."""
    blk = c["idx"] // grid(c["M"])["per_block"]
    assert (blk == b).any() and (blk == b + 1).any()
    key = np.where(blk == b, b + 1, np.where(blk == b + 1, b, blk))
    return c["ep_return"][c["idx"][np.argsort(key, kind="stable")]]


@functools.lru_cache(maxsize=None)
def rollout(T, N, seed):
    """A rollout for ppo_episode_scan: float32 rewards (the task's values and others), both flags, non-zero carries."""
    rng = np.random.default_rng(seed)
    r = rng.choice(np.array(ER.REWARD_VALUES + (0.5, -1.75), np.float32), size=(T, N))
    term = (rng.random((T, N)) < 0.15).astype(np.uint8)
    trunc = (rng.random((T, N)) < 0.1).astype(np.uint8)
    action = rng.integers(0, 5, (T, N)).astype(np.int32)
    c0 = rng.normal(size=N) * 3
    l0 = rng.integers(1, 30, N).astype(np.int32)
    return _freeze(dict(reward=r, term=term, trunc=trunc, action=action, carry_return=c0, carry_length=l0))


TRACKER_N, TRACKER_CUTS = 130, (128, 1, 128, 1)           # the last call in the 1-D single-step form


@functools.lru_cache(maxsize=None)
def tracker_case():
    """The rollout EpisodeTracker.account() is fed in TRACKER_CUTS, and the scan's restatement over the whole of it."""
    c = dict(rollout(sum(TRACKER_CUTS), TRACKER_N, 4242))
    c["ep_return"], c["ep_length"], c["end_return"], c["end_length"] = ER.episode_scan(
        c["reward"], c["term"], c["trunc"], np.zeros(TRACKER_N), np.zeros(TRACKER_N, np.int32))
    return _freeze(c)


def tracker_returns():
    """The finished episodes' returns of each account() call, in the call's row-major order."""
    c, out, t = tracker_case(), [], 0
    for k in TRACKER_CUTS:
        done = (c["term"][t:t + k] | c["trunc"][t:t + k]) != 0
        out.append(c["ep_return"][t:t + k][done])
        t += k
    return out


# ---------------------------------------------------------------------------------------------- the fold and its bounds
def fold_seq(returns, keep, gain, score0):
    """The header's statement, one float64 multiply-multiply-add per episode (Python floats: no fused operation)."""
    s = float(score0)
    for R in np.asarray(returns, np.float64).tolist():
        s = s * keep + R * gain
    return s


def sum_seq(returns):
    s = 0.0
    for R in np.asarray(returns, np.float64).tolist():
        s += R
    return s


def fold_exact(returns, keep, gain, score0):
    """The fold of the float64 inputs in exact rational arithmetic."""
    F = fractions.Fraction
    s, k, g = F(float(score0)), F(float(keep)), F(float(gain))
    for R in np.asarray(returns, np.float64).tolist():
        s = s * k + F(R) * g
    return s


def longdouble_ok():
    return np.finfo(np.longdouble).nmant >= 63


def fold_longdouble(returns, keep, gain, score0):
    L = np.longdouble
    s, k, g = L(score0), L(keep), L(gain)
    for R in np.asarray(returns, np.float64):
        s = s * k + L(R) * g
    return s


def fold_reference(returns, keep, gain, score0):
    """(the higher-precision value of the fold, its kind): exact up to EXACT_EPISODES episodes, long double above (its own
    error is at most 2 E 2^-64 scale, a 2^-11 part of fold_bound); None where the platform's long double is too short."""
    if len(returns) <= EXACT_EPISODES:
        return fold_exact(returns, keep, gain, score0), "exact"
    if not longdouble_ok():
        return None, "long double has fewer than 63 mantissa bits"
    return fold_longdouble(returns, keep, gain, score0), "longdouble"


def sum_reference(returns):
    if len(returns) <= EXACT_EPISODES:
        return sum((fractions.Fraction(R) for R in np.asarray(returns, np.float64).tolist()), fractions.Fraction(0)), "exact"
    if not longdouble_ok():
        return None, "long double has fewer than 63 mantissa bits"
    return np.sum(np.asarray(returns, np.float64).astype(np.longdouble)), "longdouble"      # pairwise in long double


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): a product of k factors (1 + d), |d| <= u, is 1 + t with |t| <= gamma_k."""
    assert k * U < 0.5
    return k * U / (1.0 - k * U)


def fold_bound(E, keep, gain, score0, returns):
    """|device score - float64 sequential score| <= fold_bound, for 0 <= keep <= 1 and E finite returns.

    Exactly, score = score0 keep^E + sum_i gain R_i keep^(E-1-i).  Any evaluation in float64 gives the same expression
    with every term multiplied by a product of factors (1 + d), |d| <= u = 2^-53, one per rounded operation the term
    passes through; with |keep| <= 1 every term is at most |score0| or gain |R_i| in magnitude, so the error is at most
    gamma(K) * (|score0| + gain sum|R_i|) with K the largest number of factors a term collects.

    Sequential (tests/episode_ref.py): R_i * gain (1), its addition (1), and a multiplication by keep and an addition
    for each of the E-1-i later episodes; score0 the same from the first episode on: K_seq = 2 E.

    Device, the documented tree (include/twoarmy_ppo.h).  A partial result is the map score -> score a + b.
      thread: b = b keep + R gain per done step of its run: as above, 2 factors per episode from its own on.
      combine (v then w): b_v a_w + b_w, a_v a_w: a term of b_v takes 2 factors (1 where the compiler fuses) and the
        factors inside the computed a_w, a product of keep over w's n_w episodes: at most n_w (each multiplication of the
        product, in a thread or in a combine, rounds once, and there are fewer of them than episodes); a term of b_w takes
        1 factor.
      The w's that meet a term on its way to the root are disjoint sets of later episodes, as are the later episodes
      of its own thread: together they give at most 2 (E - 1) factors.  The path itself has at most 6 lane levels, 3
      wavefront combines, 4 partials of one lane and 6 lane levels = 19 combines: 2 * 19 factors.  The term's own
      R gain and addition give 2, the final score0 a + b gives 1 (score0 takes the E - 1 roundings inside a, the
      multiplication and the addition: fewer).
      K_tree = 2 (E - 1) + 2 * 19 + 2 + 1 = 2 E + 39.
    The difference of the two evaluations is at most the sum of their errors."""
    assert 0.0 <= keep <= 1.0 and len(returns) == E
    scale = abs(float(score0)) + abs(float(gain)) * float(np.abs(np.asarray(returns, np.float64)).sum())
    return (gamma(2 * E + 2 * TREE_COMBINES + 1) + gamma(2 * E)) * scale


def sum_bound(E, returns):
    """|device return_sum - float64 sequential sum| <= sum_bound: in either evaluation a term passes through at most
    E - 1 rounded additions (adding to an exact 0 rounds nothing), whatever the tree."""
    return 2 * gamma(max(E - 1, 1)) * float(np.abs(np.asarray(returns, np.float64)).sum())


def fold_sets():
    """Every (name, returns in row-major order, keep, gain, score0) the GPU file folds."""
    for M in SWEEP_M:
        yield "sweep %d" % M, summary_case(M)["returns"], 0.99, 0.01, SCORE0
    yield "every step done", summary_case(4097, True)["returns"], 0.99, 0.01, SCORE0
    for M in ORDER_SHAPES:
        yield "order %d" % M, order_case(M)["returns"], ORDER_KEEP, ORDER_GAIN, SCORE0
    for keep, gain in KEEP_GAIN:
        yield "keep %g gain %g" % (keep, gain), summary_case(2049)["returns"], keep, gain, SCORE0
    score = 0.0                                  # the tracker's score runs on from call to call
    for k, returns in enumerate(tracker_returns()):
        yield "tracker call %d" % k, returns, 0.99, 0.01, score
        score = fold_seq(returns, 0.99, 0.01, score)
