"""The update diagnostics of ppo_loss_fwd_bwd_stats (include/twoarmy_ppo.h) stated in float64 numpy on float32 inputs: the
torch formulation of `_losses64` in test_ppo_kernels_edges_gpu.py (Categorical(probs = p) with the float32 clamp eps,
ratio = exp(logp - old)) extended by the thirteen accumulators, and an input generator in the style of that file's
`_loss_inputs` whose margins make the three counts a matter of the reference alone, and the float32 rounding bounds of the accumulators
(test_update_stats_gpu.py and the case of test_streams_gpu.py).  A plain module like ppo_util.py."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23: the clamp of the kernel's (float32) Categorical
CLIP, ENT = 0.1, 0.01
NAMES = ("rows", "entropy_sum", "logr_sum", "k3_sum", "clipped", "ratio_dev_max", "t_sum", "t_sq_sum", "e_sum", "e_sq_sum",
         "saturated", "top_mass_sum", "calls")
WORDS = 16                                        # 13..15 are reserved
RATIO_MARGIN, CLAMP_MARGIN, TIE_MARGIN = 1e-5, 1e-9, 1e-6


def rows64(p, a, old, value, target, clip=CLIP):
    """The per-row quantities in float64: q, l, H, logp, lr, ratio, k3, clipped, dev = |ratio - 1|, t, e, saturated, top."""
    p = np.asarray(p, np.float64)
    n = np.arange(p.shape[0])
    q = p / p.sum(1, keepdims=True)
    l = np.log(np.clip(q, EPS32, 1 - EPS32))
    lr = l[n, a] - np.asarray(old, np.float64)
    ratio = np.exp(lr)
    qa = q[n, a]
    return dict(q=q, l=l, H=-(q * l).sum(1), logp=l[n, a], lr=lr, ratio=ratio, k3=(ratio - 1.0) - lr,
                clipped=(ratio < 1 - clip) | (ratio > 1 + clip), dev=np.abs(ratio - 1.0), t=np.asarray(target, np.float64),
                e=np.asarray(target, np.float64) - np.asarray(value, np.float64), saturated=(qa < EPS32) | (qa > 1 - EPS32),
                top=q.max(1))


def accumulate(stats, p, a, old, value, target, clip=CLIP, n_valid=None):
    """stats float64[16] after one call on the rows b < n_valid -> (new stats, the per-row dict of those rows)."""
    v = slice(0, len(a) if n_valid is None else n_valid)
    R = rows64(p[v], a[v], old[v], value[v], target[v], clip)
    out = np.array(stats, np.float64, copy=True)
    out[0] += len(R["H"])
    out[1] += R["H"].sum()
    out[2] += R["lr"].sum()
    out[3] += R["k3"].sum()
    out[4] += R["clipped"].sum()
    out[5] = max(out[5], R["dev"].max())
    out[6] += R["t"].sum()
    out[7] += (R["t"] ** 2).sum()
    out[8] += R["e"].sum()
    out[9] += (R["e"] ** 2).sum()
    out[10] += R["saturated"].sum()
    out[11] += R["top"].sum()
    out[12] += 1
    return out, R


def read(stats):
    """What ppo_ops.update_stats_read derives from one row of accumulators, restated."""
    s = dict(zip(NAMES, np.asarray(stats, np.float64)[:13]))
    n = s["rows"]
    var = lambda s1, s2: s2 / n - (s1 / n) ** 2                                                   # noqa: E731
    with np.errstate(all="ignore"):                                             # 0 / 0 is the NaN the front end promises
        return _read(s, n, var)


def _read(s, n, var):
    return dict(rows=n, calls=s["calls"], entropy=s["entropy_sum"] / n, approx_kl=s["k3_sum"] / n,
                approx_kl_k1=-s["logr_sum"] / n, clip_frac=s["clipped"] / n, ratio_dev_max=s["ratio_dev_max"],
                explained_variance=1.0 - var(s["e_sum"], s["e_sq_sum"]) / var(s["t_sum"], s["t_sq_sum"]),
                saturated_frac=s["saturated"] / n, top_mass=s["top_mass_sum"] / n)


def inputs(B, seed, A=5, clip=CLIP):
    """(p, a, old, adv, value, target), float32 / int32: row sums anywhere in [0.3, 3]; a block of rows with q[a] = 0 and a
    block with q[a] = 1; ratios planted 1e-4 inside and 1e-4 outside both clip bounds; adv = 0 ties.  A random row that
    comes too close to a decision is moved away from it (its ratio to 1, its largest entry up by half), and the three
    margins are then asserted: with them the float32 kernel takes every decision as float64 does."""
    rs = np.random.RandomState(seed)
    p = rs.gamma(0.8, size=(B, A))
    p *= (rs.uniform(0.3, 3.0, B) / p.sum(1))[:, None]
    a = rs.randint(0, A, B)
    k = max(1, B // 16)
    p[:k, :] = np.where(np.arange(A)[None] == a[:k, None], 0.0, p[:k])          # q = 0 at the taken action
    one = np.arange(k, min(2 * k, B))                                           # (row, action) pairs: an index array, no slice
    p[one] = 0.0
    p[one, a[one]] = rs.uniform(0.3, 3.0, len(one))                             # q = 1 at the taken action
    srt = np.sort(p / p.sum(1, keepdims=True), 1)
    tie = srt[:, -1] - srt[:, -2] <= 4 * TIE_MARGIN
    p[tie, np.argmax(p[tie], 1)] *= 1.5
    p = p.astype(np.float32)
    q64 = p.astype(np.float64) / p.astype(np.float64).sum(1, keepdims=True)
    logp = np.log(np.clip(q64[np.arange(B), a], EPS32, 1 - EPS32))
    r = np.exp(rs.randn(B) * 0.15)
    r[np.minimum(np.abs(r - (1 - clip)), np.abs(r - (1 + clip))) <= 4 * RATIO_MARGIN] = 1.0
    sel = rs.randint(0, 5, B)
    r = np.where(sel == 1, 1 + clip - 1e-4, np.where(sel == 2, 1 + clip + 1e-4, np.where(
        sel == 3, 1 - clip + 1e-4, np.where(sel == 4, 1 - clip - 1e-4, r))))
    old = (logp - np.log(r)).astype(np.float32)
    adv = rs.randn(B).astype(np.float32)
    adv[rs.rand(B) < 0.1] = 0.0                                                 # adv = 0: s1 == s2 ties
    value = (rs.randn(B) * 2).astype(np.float32)
    target = rs.randn(B).astype(np.float32)
    a = a.astype(np.int32)
    # the margins, on what the kernel gets
    R = rows64(p, a, old, value, target, clip)
    assert (np.minimum(np.abs(R["ratio"] - (1 - clip)), np.abs(R["ratio"] - (1 + clip))) > RATIO_MARGIN).all()
    qa = R["q"][np.arange(B), a]
    planted = (qa == 0.0) | (qa == 1.0)
    assert (planted | (np.minimum(np.abs(qa - EPS32), np.abs(qa - (1 - EPS32))) > CLAMP_MARGIN)).all()
    assert planted[:2 * k].all() and R["saturated"][:2 * k].all()
    srt = np.sort(R["q"], 1)
    assert (srt[:, -1] - srt[:, -2] > TIE_MARGIN).all()
    return p, a, old, adv, value, target


def _bounds(x, R, n_valid):
    """Absolute bounds of the 16 entries after ONE call from zero, from the float64 rows R: the per-row float32 bounds
    that test_losses_vs_float64_autograd derives, summed over the rows, plus 2^-40 of the summed magnitudes for the
    double accumulation (a 64-lane tree, four wavefronts, a fold over the workgroups: far fewer than 2^12 roundings of
    2^-53 each).  Counts, calls and the reserved entries: 0."""
    old = x[2][:n_valid].astype(np.float64)
    acc = 2.0 ** -40
    # logp and ratio: q (A + 1 roundings), logf, expf of a difference of magnitude <= |logp| + |old|
    rel = 8 * EPS32 * (1 + np.abs(R["logp"]) + np.abs(old))
    b = np.zeros(WORDS)
    b[1] = (8 * EPS32 * (np.abs(R["l"]) + 2).sum(1)).sum() + acc * np.abs(R["H"]).sum()
    b[2] = rel.sum() + acc * np.abs(R["lr"]).sum()                 # lr: the absolute error of a logarithm of the ratio
    b[3] = (rel * (R["ratio"] + 1)).sum() + acc * (np.abs(R["ratio"] - 1) + np.abs(R["lr"])).sum()
    j = int(np.argmax(R["dev"]))
    b[5] = rel[j] * R["ratio"][j]                                  # the reference's maximising row
    b[6] = acc * np.abs(R["t"]).sum()                              # float32 -> double and its square are exact
    b[7] = acc * (R["t"] ** 2).sum()
    b[8] = (2.0 ** -24 * np.abs(R["e"])).sum() + acc * np.abs(R["e"]).sum()       # e: one float32 subtraction
    b[9] = (2.0 ** -23 * R["e"] ** 2).sum() + acc * (R["e"] ** 2).sum()
    b[11] = (6 * EPS32 * R["top"]).sum() + acc * R["top"].sum()    # max q: A + 1 roundings of one quotient
    return b
