"""Inputs and float64 references for the replay-side PPO kernels (tests/test_replay_edges_cpu.py,
tests/test_replay_kernels_edges_gpu.py): a synthetic rollout generator whose episodes sit on every length class the
hindsight kernel treats differently, and Net_Decoder evaluated in float64 with its rounding-error bound.

TEST INFRASTRUCTURE ONLY.  Nothing here touches the device or the HIP library."""
import numpy as np
import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------ synthetic rollouts (HER)
# 1, 2: shorter than any window delay; 4, 5: around skip = 4; 6: ordinary; 63, 64: one lane free / all 64 lanes live;
# 65, 70, 130: longer than HER_MAX_LEN (dropped), 130 longer than two 64-step chunks of the kernel's c0 loop.
LENGTHS = (1, 2, 4, 5, 6, 63, 64, 65, 70, 130)
TASK_REWARDS = np.array([-0.01, -0.1, -0.9, 0.2, 0.9], np.float32)     # ppo_episode_summary's reward_hist buckets
SWEEP_SEED, SWEEP_T, SWEEP_N = 7, 333, 37


def positions(rs, shape, mode):
    """Finite (y, x) from a 7 x 7 alphabet, so that an episode revisits cells.  "int": -1 .. 5.  "frac": the same
    times 0.5 with every zero randomly +0.0 or -0.0 (np.unique and the kernel's == both take them as one value)."""
    p = rs.randint(-1, 6, size=tuple(shape) + (2,)).astype(np.float32)
    if mode == "frac":
        p *= np.float32(0.5)
        neg = (p == 0) & (rs.rand(*p.shape) < 0.5)
        p[neg] = np.float32(-0.0)
    else:
        assert mode == "int"
    assert np.isfinite(p).all()
    return p


def synthetic_rollout(seed, T, N, mode):
    """Episodes laid end to end per env, lengths drawn uniformly from LENGTHS, the first episode start 0 .. 2 steps
    into the rollout, every end terminated, truncated or both, age0 != 0 for about 30 % of the envs.
    Returns dict(pos [T,N,2] f32, terminated, truncated [T,N] u8, age0 [N] i32, reward [T,N] f32,
    episodes = [(n, s0, t1)] of the episodes laid whole inside the rollout)."""
    rs = np.random.RandomState(seed)
    term = np.zeros((T, N), np.uint8)
    trunc = np.zeros((T, N), np.uint8)
    episodes = []
    for n in range(N):
        s0 = int(rs.randint(0, 3))
        if s0:
            term[s0 - 1, n] = 1                                   # whatever ran before the first laid episode ends here
        while True:
            L = int(LENGTHS[rs.randint(len(LENGTHS))])
            t1 = s0 + L - 1
            if t1 >= T:
                break                                             # the last episode is still running at the end
            kind = rs.randint(3)
            term[t1, n] = kind != 1
            trunc[t1, n] = kind != 0
            episodes.append((n, s0, t1))
            s0 = t1 + 1
    age0 = np.where(rs.rand(N) < 0.3, rs.randint(1, 40, N), 0).astype(np.int32)
    reward = TASK_REWARDS[rs.randint(0, 5, size=(T, N))]
    return dict(pos=positions(rs, (T, N), mode), terminated=term, truncated=trunc, age0=age0, reward=reward,
                episodes=episodes)


def relabelled_episodes(roll):
    """The laid episodes the oracle can see from their first step: those of an env with age0 != 0 and no done before
    the first laid start run on from before the rollout (their first episode merges with it)."""
    done = (roll["terminated"] | roll["truncated"]) != 0
    out = []
    for n, s0, t1 in roll["episodes"]:
        if roll["age0"][n] != 0 and not done[:s0, n].any():
            continue
        out.append((n, s0, t1))
    return out


def length_histogram(roll):
    h = {L: 0 for L in LENGTHS}
    for _, s0, t1 in relabelled_episodes(roll):
        h[t1 - s0 + 1] += 1
    return h


def straddling_64(roll):
    """64-step episodes that cross a 64-step chunk boundary of the kernel's c0 loop (start not chunk-aligned)."""
    return [(n, s0, t1) for n, s0, t1 in relabelled_episodes(roll) if t1 - s0 + 1 == 64 and s0 % 64 != 0]


def sweep_choices(seed, T, N):
    """Explicit picks with out-of-range (negative, >= U) and repeated entries."""
    return np.random.RandomState(seed + 1000).randint(-2, 20, size=(T, N, 4)).astype(np.int32)


def single_env(T, episodes, pos=None, age0=0, seed=0, mode="int"):
    """Hand-built rollout of one env: `episodes` = [(s0, t1)] sets a done at every t1 (and at s0 - 1 where s0 > 0 and
    no other episode ends there, so the episode starts at s0)."""
    rs = np.random.RandomState(seed)
    term = np.zeros((T, 1), np.uint8)
    for s0, t1 in episodes:
        term[t1, 0] = 1
        if s0 > 0:
            term[s0 - 1, 0] = 1
    p = positions(rs, (T, 1), mode) if pos is None else np.ascontiguousarray(pos, np.float32).reshape(T, 1, 2)
    return dict(pos=p, terminated=term, truncated=np.zeros((T, 1), np.uint8), age0=np.array([age0], np.int32),
                reward=TASK_REWARDS[rs.randint(0, 5, size=(T, 1))])


def same_bits(a, b):
    """Equality of dtype, shape and bit pattern (-0.0 != +0.0, unlike np.array_equal)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ Net_Decoder in float64
DEC_U = 2.0 ** -24               # unit roundoff of fp32
DEC_DEPTH = 280                  # see decoder_bound


def decoder_weights(seed):
    """Weights in ConvTranspose2d layout [C_in][C_out][kH][kW], uniform in +-1/sqrt(fan) like nn.ConvTranspose2d's
    default, float32 values (what the kernel is handed)."""
    g = torch.Generator().manual_seed(seed)

    def u(shape, fan):
        return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) / fan ** 0.5).float()
    return dict(w1=u((64, 16, 2, 2), 64), b1=u((16,), 64), w2=u((16, 16, 5, 5), 64), b2=u((16,), 64),
                w3=u((16, 1, 4, 4), 64), b3=u((1,), 64))


def decoder_latents(seed, n, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n, 64, 4, 4), generator=g, dtype=torch.float64) * scale).float()


def decoder_f64(z, w, relu=True):
    """Net_Decoder (all_net.py:100-137) literally, in float64 on the CPU, from the UNFOLDED weights:
    conv_transpose2d x 3 with ReLU between the layers, then avg_pool2d(4).  z [n,64,4,4] -> [n,289]."""
    d = {k: v.detach().cpu().double() for k, v in w.items()}
    act = F.relu if relu else (lambda x: x)
    a = act(F.conv_transpose2d(z.detach().cpu().double(), d["w1"], d["b1"], stride=2))
    a = act(F.conv_transpose2d(a, d["w2"], d["b2"], stride=4))
    a = F.conv_transpose2d(a, d["w3"], d["b3"], stride=2)
    return F.avg_pool2d(a, 4).reshape(z.shape[0], 289)


def decoder_bound(z, w):
    """Elementwise bound on |fp32 kernel - float64| to first order in u = 2^-24.

    The kernel evaluates three FMA dot products per output, of depth 64 (layer 1: 64 input channels, one source pixel),
    64 (layer 2: at most 4 overlapping source pixels x 16 channels) and 144 (folded tail: 9 taps x 16 channels), each
    started from its bias.  A depth-n FMA chain errs by at most n * u * sum|a_i||b_i| (+ u for the bias it starts from);
    ReLU is 1-Lipschitz and the later layers' |weights| carry an earlier layer's error forward, so with A_k = layer k of
    the same network evaluated on |z|, |w|, |b| without ReLU the error after layer 3 is at most
    (65 + 65 + 145) u A3 = 275 u A3, rounded up to DEC_DEPTH = 280 for the separate fp32 add of b3.  The host's fp32
    folding of w3 into kfold (up to 15 adds and a scale per tap) is not itemised: it is a worst case on top of a worst
    case, and the measured error sits far below the bound (the tests print the ratio)."""
    a3 = decoder_f64(z.abs(), {k: v.abs() for k, v in w.items()}, relu=False)
    return DEC_DEPTH * DEC_U * a3


def perturb_w3_tap(w, c, r, s, rel=1e-3):
    out = {k: v.clone() for k, v in w.items()}
    out["w3"][c, 0, r, s] *= 1.0 + rel
    return out
