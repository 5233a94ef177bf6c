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


def update(reward, terminated, truncated, gamma, ret_carry, stats):
    """ppo_reward_norm_update -> (ret_carry', stats') as new float64 arrays; T == 0 changes nothing."""
    ret_carry, stats = np.array(ret_carry, F64), np.array(stats, F64)
    if reward.shape[0] == 0:
        return ret_carry, stats
    G, k, mean, m2 = scan(reward, terminated, truncated, gamma, ret_carry)
    rollout = tree([(k[i], mean[i], m2[i]) for i in range(k.size)])
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
