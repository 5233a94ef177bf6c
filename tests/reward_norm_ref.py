"""Numpy float64 restatement of the reward normalisation of include/twoarmy_ppo.h ("Reward normalisation";
ppo_reward_norm_update, ppo_reward_norm_apply): the scan with its Welford update, Chan's merge and its tree over the env
index, stats[3], and apply in float32 -- and the cases the GPU tests run.  Every formula is written one operation per
statement, as the header states it: numpy's float64 *, +, - , / and sqrt round once each, which is what the kernels are
held to bit for bit.  A plain module like episode_ref.py."""
import numpy as np

F64, F32, U8 = np.float64, np.float32, np.uint8
TASK_REWARDS = np.array([-0.01, -0.1, -0.9, 0.2, 0.9], F32)          # the engine's five values
EPS = F64(1e-8)


def scan(reward, terminated, truncated, gamma, ret_carry):
    """The scan over one rollout, all envs at once (elementwise float64) -> (ret_carry', k[N], mean[N], M2[N])."""
    T, N = reward.shape
    gamma = F64(gamma)
    G = np.array(ret_carry, F64)
    k, mean, m2 = np.zeros(N, F64), np.zeros(N, F64), np.zeros(N, F64)
    with np.errstate(all="ignore"):
        for t in range(T):
            p = gamma * G
            G = p + reward[t].astype(F64)
            k = k + F64(1.0)
            d = G - mean
            q = d / k
            mean = mean + q
            e = G - mean
            f = d * e
            m2 = m2 + f
            G = np.where((terminated[t] | truncated[t]) != 0, F64(0.0), G)
    return G, k, mean, m2


def merge(a, b):
    """Chan's rule on two (n, mean, M2) triples of float64 scalars, a = the left operand."""
    na, ma, sa = a
    nb, mb, sb = b
    if nb == 0.0:
        return a
    if na == 0.0:
        return b
    n = na + nb
    d = mb - ma
    dn = d * nb
    shift = dn / n
    mean = ma + shift
    dd = d * d
    dda = dd * na
    ddab = dda * nb
    between = ddab / n
    within = sa + sb
    return (n, mean, within + between)


EMPTY = (F64(0.0), F64(0.0), F64(0.0))


def tree(triples):
    """The balanced tree over the index: padded with empty triples to the next power of two, level l merges element
    2^l * 2j (left) with element 2^l * (2j + 1) (right)."""
    level = list(triples)
    P = 1
    while P < len(level):
        P *= 2
    level += [EMPTY] * (P - len(level))
    while len(level) > 1:
        level = [merge(level[2 * j], level[2 * j + 1]) for j in range(len(level) // 2)]
    return level[0]


def scale_of(n, m2):
    if n == 0.0:
        return F64(1.0)
    var = m2 / n
    v = var + EPS
    return F64(1.0) / np.sqrt(v)


def levels(k, mean, m2, count):
    """`count` levels of the same tree, level-wise over float64 arrays: the operations of merge() in its order, on every
    pair of a level at once, np.where choosing the other operand where one is empty.  -> the shorter (k, mean, m2), padded
    with empty elements to a multiple of 2^count first.  tree() stays the statement; this is asserted equal to it bit for
    bit (tests/test_reward_norm_cpu.py) and exists for the sizes at which tree()'s Python loop takes half a second."""
    k, mean, m2 = (np.array(x, F64) for x in (k, mean, m2))
    pad = -k.size % (1 << count)
    k, mean, m2 = (np.concatenate([x, np.zeros(pad, F64)]) for x in (k, mean, m2))
    with np.errstate(all="ignore"):                                  # 0 / 0 where both operands are empty: not chosen
        for _ in range(count):
            na, ma, sa, nb, mb, sb = k[0::2], mean[0::2], m2[0::2], k[1::2], mean[1::2], m2[1::2]
            n = na + nb
            d = mb - ma
            dn = d * nb
            shift = dn / n
            mu = ma + shift
            dd = d * d
            dda = dd * na
            ddab = dda * nb
            between = ddab / n
            within = sa + sb
            s = within + between
            k = np.where(nb == 0.0, na, np.where(na == 0.0, nb, n))
            mean = np.where(nb == 0.0, ma, np.where(na == 0.0, mb, mu))
            m2 = np.where(nb == 0.0, sa, np.where(na == 0.0, sb, s))
    return k, mean, m2


def tree_levelwise(k, mean, m2):
    """tree() of the triples (k[i], mean[i], m2[i]) through levels()."""
    count = 0
    while (1 << count) < len(k):
        count += 1
    k, mean, m2 = levels(k, mean, m2, count)
    return (k[0], mean[0], m2[0]) if len(k) else EMPTY


def update(reward, terminated, truncated, gamma, ret_carry, stats, levelwise=False):
    """ppo_reward_norm_update -> (ret_carry', stats') as new float64 arrays; T == 0 changes nothing.  levelwise: the tree
    through tree_levelwise() instead of tree(), for the large sizes."""
    ret_carry, stats = np.array(ret_carry, F64), np.array(stats, F64)
    if reward.shape[0] == 0:
        return ret_carry, stats
    G, k, mean, m2 = scan(reward, terminated, truncated, gamma, ret_carry)
    rollout = tree_levelwise(k, mean, m2) if levelwise else tree([(k[i], mean[i], m2[i]) for i in range(k.size)])
    n, mu, s = merge((stats[0], stats[1], stats[2]), rollout)
    return G, np.array([n, mu, s, scale_of(n, s)], F64)


def apply(reward, stats, clip):
    """ppo_reward_norm_apply -> float32 array of reward's shape."""
    s = F32(1.0) if stats[0] == 0.0 else F32(stats[3])
    x = np.asarray(reward, F32) * s
    clip = F32(clip)
    if clip > 0 and np.isfinite(clip):
        x = np.fmin(np.fmax(x, -clip), clip)
    return x.astype(F32)


def returns(reward, terminated, truncated, gamma, ret_carry):
    """The explicitly built return sequence [T, N] (no moments): what np.mean / np.var are taken over."""
    T, N = reward.shape
    out = np.zeros((T, N), F64)
    G = np.array(ret_carry, F64)
    for t in range(T):
        G = F64(gamma) * G + reward[t].astype(F64)
        out[t] = G
        G = np.where((terminated[t] | truncated[t]) != 0, 0.0, G)
    return out


# ------------------------------------------------------------------------------------------------------------ cases
SHAPES = [(1, 1), (3, 1), (5, 63), (5, 64), (5, 65), (4, 257), (7, 1000)]
GAMMAS = (0.0, 0.99, 1.0)
DONES = ("first", "last", "every", "none", "mixed")


def rewards(rng, T, N):
    """The five task values, and bonus-like floats (1 / sqrt(count), a shaping term) on about a third of the steps."""
    r = rng.choice(TASK_REWARDS, (T, N)).astype(F32)
    bonus = (1.0 / np.sqrt(rng.integers(1, 50, (T, N)))).astype(F32) + F32(0.05) * rng.standard_normal((T, N)).astype(F32)
    return np.where(rng.random((T, N)) < 0.35, r + bonus, r).astype(F32)


def flags(rng, T, N, dones):
    """(terminated, truncated): done at t = 0, at t = T - 1, at every step, at none, or at random with both flags set on
    some steps."""
    term, trunc = np.zeros((T, N), U8), np.zeros((T, N), U8)
    if dones == "first":
        term[0], trunc[0, ::2] = 1, 1
    elif dones == "last":
        trunc[T - 1], term[T - 1, ::3] = 1, 1
    elif dones == "every":
        term[:], trunc[::2] = 1, 1
    elif dones == "mixed":
        term = (rng.random((T, N)) < 0.2).astype(U8)
        trunc = (rng.random((T, N)) < 0.2).astype(U8)
    return term, trunc


def case(T, N, dones, seed=0):
    """Three consecutive rollouts of one shape -> a list of (reward, terminated, truncated)."""
    rng = np.random.default_rng(1000 * seed + 31 * T + N + 7 * DONES.index(dones))
    return [(rewards(rng, T, N),) + flags(rng, T, N, dones) for _ in range(3)]


def start_state(N, zero, seed=0):
    """(ret_carry, stats) a chain starts from: nothing seen, or a state three rollouts of mixed flags leave behind."""
    carry, stats = np.zeros(N, F64), np.zeros(4, F64)
    if not zero:
        for r, te, tr in case(6, N, "mixed", seed + 5):
            carry, stats = update(r, te, tr, 0.97, carry, stats)
    return carry, stats


# ------------------------------------------------------------------------------------- the fold's and the scan's edges
# N at which ppo_reward_norm_fold_kernel (one workgroup of 16 wavefronts, 64 elements per wavefront and pass, a pass's
# chunks taken 16 apart) changes its path, each named for the edge it sits on.  Run with FOLD_T rows: the scan is not the
# subject.  case() seeds from T and N, so these draw their own data without touching that of SHAPES.
FOLD_T = 2
FOLD_EDGES = [
    (1023, "16 chunks, one per wavefront, the last partial"),
    (1024, "16 full chunks: the last size with one chunk per wavefront"),
    (1025, "wavefront 0's second chunk holds one element, 63 lanes empty again"),
    (1088, "17 full chunks"),
    (2049, "wavefront 0's third chunk, one element"),
    (4095, "64 chunks, four per wavefront, the last partial; pass 1 is one partial chunk"),
    (4096, "the production size: pass 1 is one full chunk"),
    (4097, "first three-pass size: pass 1's second chunk is the one element at index 4096, pass 2 at stride 64^2"),
    (4160, "65 full chunks"),
    (65536, "64 chunks per wavefront in pass 0, 16 chunks in pass 1"),
    (65537, "17 chunks in pass 1: wavefront 0's second chunk of pass 1"),
    (262144, "64^3: three full passes"),
    (262145, "first four-pass size, stride 64^3"),
]
FOLD_SMALL = 4160                                  # up to here every start and flag pattern; beyond, one chain each

# T around the scan's batches of 8 rows (RN_ROWS of csrc/reward_norm.hip) at one lane and at a second block of one lane.
SCAN_T = (8, 9, 15, 16, 17, 24, 25)
SCAN_N = (1, 65)
SCAN_KINDS = ("edge", "mixed", "none")             # flags of scan_case(); "edge" runs at gamma 0.99, the others at 1.0
BATCH = 8


def edge_flags(T, N):
    """Done steps where the batches meet: the last row of a batch (7, 15) on even envs, the first row of the next (8, 16)
    on odd envs, where T has them; by (env // 2 + row) % 3 terminated alone, both flags, truncated alone."""
    term, trunc = np.zeros((T, N), U8), np.zeros((T, N), U8)
    for row in range(BATCH - 1, T, BATCH):
        for t, parity in ((row, 0), (row + 1, 1)):
            if t < T:
                n = np.arange(parity, N, 2)
                kind = (n // 2 + t) % 3
                term[t, n], trunc[t, n] = kind <= 1, kind >= 1
    return term, trunc


def scan_case(T, N, kind):
    """Three consecutive rollouts for the scan's batch edges -> a list of (reward, terminated, truncated); its own seeds."""
    rng = np.random.default_rng([77, T, N, SCAN_KINDS.index(kind)])
    return [(rewards(rng, T, N),) + (edge_flags(T, N) if kind == "edge" else flags(rng, T, N, kind)) for _ in range(3)]


# One NaN, one +inf and one -inf reward in a rollout of mixed flags, then a clean rollout.
NF_T, NF_N = 9, 130
NF_NAN, NF_PINF, NF_NINF = (3, 5), (8, 70), (5, 129)       # (row, env): first batch; first row of the second; a done step


def nonfinite_case():
    """Two rollouts -> [(reward, terminated, truncated)] * 2.  First: env 5 gets a NaN at row 3 and no done step behind it,
    env 70 +inf at the last row, which is no done step, env 129 -inf on a terminated step.  Second: clean; env 5 is done at
    row 4 (its NaN return is cleared), env 70 never is (its infinite return stays)."""
    rng = np.random.default_rng([78, NF_T, NF_N])
    rolls = [[rewards(rng, NF_T, NF_N)] + list(flags(rng, NF_T, NF_N, "mixed")) for _ in range(2)]
    (r, te, tr), (r2, te2, tr2) = rolls
    r[NF_NAN], r[NF_PINF], r[NF_NINF] = np.nan, np.inf, -np.inf
    te[NF_NAN[0]:, NF_NAN[1]] = tr[NF_NAN[0]:, NF_NAN[1]] = 0
    te[NF_PINF], tr[NF_PINF] = 0, 0
    te[NF_NINF], tr[NF_NINF] = 1, 0
    te2[4, NF_NAN[1]], tr2[4:, NF_NAN[1]], te2[5:, NF_NAN[1]] = 1, 0, 0
    te2[:, NF_PINF[1]] = tr2[:, NF_PINF[1]] = 0
    return [tuple(x) for x in rolls]


def special_rewards(n, nan=True):
    """rewards() of n elements with +-0, +-inf, denormals, the smallest normal and (nan) NaNs written over some of them."""
    r = rewards(np.random.default_rng([79, n]), 1, n).reshape(-1)
    vals = [0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-45, 1.1754944e-38, -3e-39] + ([np.nan, -np.nan] if nan else [])
    at = np.random.default_rng([80, n]).permutation(n)[:4 * len(vals)]
    r[at] = np.tile(np.array(vals, F32), 4)
    r[-1] = F32(np.nan) if nan else F32(-0.0)                        # the last element: the row store's tail
    return r
