"""PPO math kernels (csrc/ppo_kernels.hip) against plain float64 statements of their formulas, at the production
shapes and launch paths (block caps, grid strides, both GAE instantiations, every sampler width) and at the edges where
such kernels go wrong: zero probabilities, non-finite advantages, constant inputs, padding spanning workgroups.

No comparison here goes through oracle/ppo_oracle.py (which restates the kernels' own float32 arithmetic).  Every
tolerance is a float32 rounding bound derived next to it; a wrong carry, mask, block-cap remainder or chain-rule factor
is an O(1) error and far outside all of them."""
import numpy as np
import pytest
import torch

from ppo_util import DEV, accepted, dev as _dev, lib_module as _libmod, ops as _ops, ptr as _P, rejected

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)          # 2^-23
U_MAX = 1.0 - 2.0 ** -24                          # largest uniform of the Philox path: (2^24 - 1) * 2^-24
CANARY = -55.5                                    # what the outputs of a rejected call are filled with


def _marshal():
    from twoarmy_amd import _marshal
    return _marshal


# ------------------------------------------------------------------------------------------------------------ sampler
SAMPLE_A = (2, 3, 4, 5, 7)


def _inv_cdf64(q, u):
    """float64 inverse CDF of the rows q at u: min{k : cumsum(q)[k] > u}, else the last k with q > 0."""
    cum = np.cumsum(q, 1)
    a = (cum <= u[:, None]).sum(1)
    last = q.shape[1] - 1 - np.argmax((q > 0)[:, ::-1], 1)
    return np.minimum(a, last)


def _probs(rs, B, A):
    """Random rows, unnormalised (sums 0.3 .. 3), a quarter of them with exact zeros."""
    p = rs.gamma(0.7, size=(B, A))
    p *= (rs.uniform(0.3, 3.0, B) / p.sum(1))[:, None]
    z = rs.rand(B, A) < 0.25
    z[np.arange(B), rs.randint(0, A, B)] = False                  # at least one nonzero entry per row
    p[z] = 0.0
    return p.astype(np.float32)


@pytest.mark.parametrize("A", SAMPLE_A)
def test_sample_grid_uniforms_equal_float64_inverse_cdf(A):
    M = 1 << 20
    rs = np.random.RandomState(100 + A)
    p = _probs(rs, M, A)
    u = ((np.arange(M) + 0.5) / M).astype(np.float32)           # exact in fp32 (21 significant bits)
    a, logp = _ops().sample(_dev(p), _dev(u))
    a, logp = a.cpu().numpy().astype(np.int64), logp.cpu().numpy().astype(np.float64)
    q = p.astype(np.float64) / p.astype(np.float64).sum(1, keepdims=True)
    # fp32 sum of A terms, A divisions and A sequential adds: |cumsum32 - cumsum64| <= (2A + 1) * 2^-24 <= (A + 1) * eps
    band = (A + 1) * EPS32
    lo, hi = _inv_cdf64(q, u.astype(np.float64) - band), _inv_cdf64(q, u.astype(np.float64) + band)
    qa = q[np.arange(M), a]
    assert np.all((a >= lo) & (a <= hi)), "action outside the float64 inverse CDF (+- %d ulp band)" % (A + 1)
    assert np.all(qa > 0), "sampled an action of probability 0"
    exact = lo == hi
    assert exact.mean() > 0.99 and np.array_equal(a[exact], _inv_cdf64(q, u.astype(np.float64))[exact])
    # log q_a: q32 has relative error <= (A + 1) * 2^-24 (<= 4.8e-7) and logf <= 1 ulp of |log| <= 16 (<= 9.6e-7)
    ref = np.log(np.clip(qa, EPS32, 1.0 - EPS32))
    np.testing.assert_allclose(logp, ref, rtol=0, atol=2e-6)


@pytest.mark.parametrize("A", SAMPLE_A)
def test_sample_never_draws_a_zero_probability_action(A):
    """Rows with zeros at the start, the middle and the end; u = 0, every fp32 cumsum boundary and its neighbours,
    and 1 - 2^-24 (the rounded cumsum can end below it: the fallback must be the last action with q > 0)."""
    rows = []
    for z in ([0], [A // 2], [A - 1], [A - 2, A - 1], [0, A - 1], list(range(A - 1))):
        if len(set(z)) == A:                                     # (A = 2) a row needs one nonzero entry
            continue
        for scale in (1.0, 0.37, 2.9):
            r = np.random.RandomState(len(rows)).uniform(0.05, 1.0, A)
            r[z] = 0.0
            rows.append(r * scale / r.sum())
    rows.append(np.r_[[0.37, 0.82, 0.10], np.zeros(A - 3)] if A >= 5 else np.r_[np.zeros(A - 1), 1.0])
    P, U = [], []
    for r in np.asarray(rows, np.float32):
        cum = np.cumsum(r / r.sum(dtype=np.float32), dtype=np.float32)
        us = np.concatenate([[0.0, U_MAX], cum, np.nextafter(cum, np.float32(0)), np.nextafter(cum, np.float32(1))])
        us = np.unique(us[(us >= 0) & (us < 1)].astype(np.float32))
        P.append(np.repeat(r[None], len(us), 0)); U.append(us)
    p, u = np.concatenate(P), np.concatenate(U)
    a, logp = _ops().sample(_dev(p), _dev(u))
    a = a.cpu().numpy()
    assert np.all(p[np.arange(len(p)), a] > 0), "sampled an action of probability 0: rows %s" % np.nonzero(
        p[np.arange(len(p)), a] == 0)[0][:8].tolist()
    assert np.all(logp.cpu().numpy() > np.log(EPS32) + 1e-3)      # logp of a p > 0 entry of these rows is > log(eps)
    # the concrete case: [0.37, 0.82, 0.10, 0, 0] at u = 1 - 2^-24 is action 2
    if A >= 5:
        p1 = np.r_[[0.37, 0.82, 0.10], np.zeros(A - 3)].astype(np.float32)[None]
        a1, _ = _ops().sample(_dev(p1), _dev(np.array([U_MAX], np.float32)))
        assert int(a1[0]) == 2


def test_sample_philox_frequencies_match_q_seven_way():
    n = 2_000_000
    q = np.array([0.02, 0.3, 0.05, 0.18, 0.001, 0.249, 0.2])
    p = torch.tensor(q * 1.7, dtype=torch.float32, device=DEV).expand(n, 7).contiguous()   # unnormalised
    a, logp = _ops().sample(p, None, seed=20260, offset=12345)
    freq = torch.bincount(a.long(), minlength=7).cpu().numpy() / n
    # binomial sd sqrt(q(1-q)/n); the 2^-24 grid of u and fp32 q shift the mean by < 1e-6, far below 5 sd (>= 1e-4)
    sd = np.sqrt(q * (1 - q) / n)
    assert np.all(np.abs(freq - q) < 5 * sd), (freq, q)
    np.testing.assert_allclose(logp.cpu().numpy(), np.log(q)[a.cpu().numpy()], rtol=0, atol=2e-6)


@pytest.mark.parametrize("A", SAMPLE_A)
def test_sample_offset_dev_equals_plain_offset(A):
    rs = np.random.RandomState(A)
    p = _dev(_probs(rs, 70000, A))
    for a_off, b_off in ((0, 0), (5, 70000), (123456789, 2 ** 33 + 7)):
        dev_off = torch.tensor([b_off], dtype=torch.int64, device=DEV)
        a1, l1 = _ops().sample(p, None, seed=9981, offset=a_off, offset_dev=dev_off)
        a2, l2 = _ops().sample(p, None, seed=9981, offset=a_off + b_off)
        assert torch.equal(a1, a2) and torch.equal(l1, l2)


@pytest.mark.parametrize("A", [1, 6, 8, 9])
def test_sample_unsupported_width_raises(A):
    p = torch.full((4, A), 1.0 / A, device=DEV)
    with pytest.raises(_libmod().TwoarmyLibraryError):
        _ops().sample(p, None)


# ------------------------------------------------------------------------------------------------------------ GAE
def _gae64(r, v, nv, done, gamma, lam, use_mask):
    """float64 statement of the formula on the fp32 inputs; parameters as the kernel sees them (fp32 gamma, and
    c = fp32(gamma * lambda) * cut).  Where c = 0 A_t = delta_t exactly (the segment ends: nothing later enters).
    Returns adv, target, ret and the magnitude sum S_t = sum_{j>=t} prod(c) * (|r_j| + |gamma nv_j| + |v_j|)."""
    g32 = np.float32(gamma)
    c32 = np.float32(g32 * np.float32(lam))
    cut = (1.0 - done.astype(np.float64)) if use_mask else np.ones(r.shape)
    r, v, nv = (x.astype(np.float64) for x in (r, v, nv))
    tgt = r + float(g32) * nv * cut
    delta = tgt - v
    mag = np.abs(r) + np.abs(float(g32) * nv) + np.abs(v)
    c = float(c32) * cut
    T = r.shape[0]
    adv, S = np.zeros_like(r), np.zeros_like(r)
    nxt, snx = np.zeros(r.shape[1]), np.zeros(r.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            nxt = np.where(c[t] != 0, delta[t] + c[t] * nxt, delta[t])
            snx = np.where(c[t] != 0, mag[t] + c[t] * snx, mag[t])
            adv[t], S[t] = nxt, snx
    return adv, tgt, adv + v, S


def _gae_inputs(T, N, seed):
    rs = np.random.RandomState(seed)
    r, v, nv = (rs.randn(T, N).astype(np.float32) for _ in range(3))
    d = (rs.rand(T, N) < 0.05).astype(np.uint8)
    for t in (63, 64, T - 1):                                   # chunk edges and the last step
        if t < T:
            d[t, ::3] = 1
    d[:, 1::17] = 1                                              # columns done at every step
    return r, v, nv, d


GAE_SHAPES = [(1, 16384), (1, 524288 + 37), (128, 16384), (130, 16400),
              (128, 4096), (1, 2048), (200, 77), (64, 64), (65, 1)]
GAE_PARAMS = [(0.99, 0.0), (0.99, 0.95), (1.0, 1.0)]


@pytest.mark.parametrize("T,N", GAE_SHAPES)
def test_gae_vs_float64_formula(T, N):
    r, v, nv, d = _gae_inputs(T, N, T * 7 + N)
    tr, tv, tnv, td = (_dev(x) for x in (r, v, nv, d))
    nchunks = (T + 63) // 64
    for gamma, lam in GAE_PARAMS:
        for mask in (False, True):
            adv, tgt, ret = _ops().gae(tr, tv, tnv, td if mask else None, gamma=gamma, lam=lam, use_done_mask=mask)
            adv, tgt, ret = (x.cpu().numpy() for x in (adv, tgt, ret))
            cut = (1 - d).astype(np.float32) if mask else np.ones_like(r)
            t32 = r + (np.float32(gamma) * nv) * cut                # the reference's fp32 rounding order (PPO.py:113)
            assert np.array_equal(tgt, t32)
            if lam == 0.0:                                           # PPO.py:113-114: bit-exact on both launch paths
                assert np.array_equal(adv, t32 - v) and np.array_equal(ret, (t32 - v) + v)
                continue
            a64, _, r64, S = _gae64(r, v, nv, d, gamma, lam, mask)
            # in units of 2^-24 of the partial magnitudes (<= S_t): delta 3 roundings, 6 shuffle-level fmas, 6 c
            # products in a term's coefficient and the carry fma: 16; each chunk crossed: its 6 c products + 1 fma
            # (<= 8) -> k = (16 + 8 * chunks) / 2 in units of eps
            k = 8 + 4 * nchunks
            bound = k * EPS32 * S
            err = np.abs(adv - a64)
            assert np.all(err <= bound), "adv: worst %.3g x bound at %s (gamma %g lambda %g mask %d)" % (
                (err / bound).max(), np.unravel_index(np.argmax(err / bound), err.shape), gamma, lam, mask)
            # ret = fl(adv + v): the adv bound plus one rounding of |ret| <= S_t + |v|
            assert np.all(np.abs(ret - r64) <= bound + EPS32 * (S + np.abs(v)))


def test_gae_long_horizon_gamma_lambda_one():
    """T = 2048 (32 chunks of carries) with gamma = lambda = 1: nothing decays, every chunk's carry reaches t = 0."""
    T, N = 2048, 64
    r, v, nv, d = _gae_inputs(T, N, 2048)
    for mask in (False, True):
        adv, _, ret = _ops().gae(*(_dev(x) for x in (r, v, nv)), _dev(d) if mask else None, gamma=1.0, lam=1.0,
                                 use_done_mask=mask)
        a64, _, r64, S = _gae64(r, v, nv, d, 1.0, 1.0, mask)
        bound = (8 + 4 * 32) * EPS32 * S                           # k as in test_gae_vs_float64_formula, 32 chunks
        assert np.all(np.abs(adv.cpu().numpy() - a64) <= bound)
        assert np.all(np.abs(ret.cpu().numpy() - r64) <= bound + EPS32 * (S + np.abs(v)))


@pytest.mark.parametrize("N", [4096, 16384])                    # ppo_gae_kernel<16> and <64>
@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_gae_nonfinite_delta_stays_isolated(N, bad):
    """A non-finite delta at (t, n) (reward inf / NaN): at lambda = 0 (VecPPOTrainer's default, T = 128) every other
    element is bit-exact; at lambda > 0 with the done mask every element a done separates from it matches float64."""
    T = 128
    r, v, nv, _ = _gae_inputs(T, N, 77)
    d = np.zeros((T, N), np.uint8)
    spots = [(100, 5), (64, 6), (63, 7), (127, 8), (0, 9), (70, N - 1)]
    for t, n in spots:
        r[t, n] = bad
    d[90, 5] = 1; d[40, 6] = 1; d[63, 7] = 1; d[10, 8] = 1; d[69, N - 1] = 1; d[20, N - 1] = 1
    tr, tv, tnv, td = (_dev(x) for x in (r, v, nv, d))
    bad_mask = np.zeros((T, N), bool)
    for t, n in spots:
        bad_mask[t, n] = True
    # lambda = 0, with and without the mask
    for mask in (False, True):
        adv, tgt, ret = (x.cpu().numpy() for x in _ops().gae(tr, tv, tnv, td if mask else None, gamma=0.99, lam=0.0,
                                                              use_done_mask=mask))
        cut = (1 - d).astype(np.float32) if mask else np.ones_like(r)
        t32 = r + (np.float32(0.99) * nv) * cut
        ok = ~bad_mask
        leaked = int((adv[ok] != (t32 - v)[ok]).sum())
        assert leaked == 0, "lambda = 0: a non-finite delta leaked into %d other elements" % leaked
        assert np.array_equal(ret[ok], ((t32 - v) + v)[ok]) and np.array_equal(tgt[ok], t32[ok])
        assert not np.any(np.isfinite(adv[bad_mask]))
    # lambda > 0 with the done mask: steps at or before a done that lies before the bad step, and all later steps
    adv, _, ret = (x.cpu().numpy() for x in _ops().gae(tr, tv, tnv, td, gamma=0.99, lam=0.95, use_done_mask=True))
    a64, _, r64, S = _gae64(r, v, nv, d, 0.99, 0.95, True)
    sep = np.ones((T, N), bool)
    for t, n in spots:
        dn = np.nonzero(d[:t, n])[0]
        first = dn.max() + 1 if len(dn) else 0                  # the segment of the bad step starts here
        sep[first:t + 1, n] = False
    assert np.all(np.isfinite(a64[sep]))
    bound = (8 + 4 * 2) * EPS32 * S                             # k as in test_gae_vs_float64_formula, 2 chunks
    err = np.abs(adv - a64)
    assert np.all(err[sep] <= bound[sep]), "lambda > 0: %d elements behind a done differ from float64" % (
        (~(err <= bound) & sep).sum())
    assert np.all(np.abs(ret - r64)[sep] <= (bound + EPS32 * (S + np.abs(v)))[sep])


# ------------------------------------------------------------------------------------------------------------ adv_norm
ADV_N = [2, 3, 255, 256, 257, 1025, 261121, 524288, 528387, 4194305]


def _ulp(x):
    return np.spacing(np.float32(abs(x))).astype(np.float64)


@pytest.mark.parametrize("n", ADV_N)
@pytest.mark.parametrize("kind", ["randn", "offset", "const", "outlier"])
def test_adv_norm_vs_float64(n, kind):
    rs = np.random.RandomState(n % 100003)
    if kind == "randn":
        x = rs.randn(n)
    elif kind == "offset":
        x = rs.randn(n) * 1e-2 + 1e3
    elif kind == "const":
        x = np.full(n, -2.75)
    else:
        x = rs.randn(n)
        x[rs.randint(n)] = 1e6
    x = x.astype(np.float32)
    x64 = x.astype(np.float64)
    mean, std = x64.mean(), x64.std(ddof=1)
    t = _dev(x)
    _ops().adv_norm_(t)
    y = t.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(y))
    if kind == "const":
        assert np.all(y == 0.0)
        return
    ref = (x64 - mean) / (std + 1e-8)
    # kernel: fp32 mean (<= ulp(|mean|) / 2 off) and x - mean rounded (<= ulp(2 max|x|) / 2 = ulp(max|x|)): absolute
    # (ulp(|mean|) + ulp(max|x|)) / std; 1 / (fp32(sqrt(var)) + eps) and the product: <= 4 roundings of the result.
    # The double sums (m terms per thread + 2 x 8 tree levels, m = n / 65536 at the 256-block cap) put
    # (m + 20) * 2^-53 * sum(x^2) into n * var (relative error / 2 of std) and (m + 20) * 2^-53 * sum|x| / n into mean.
    m = -(-n // (256 * min(256, -(-n // 1024))))
    var_rel = (m + 20) * 2.0 ** -53 * (x64 * x64).sum() / ((n - 1) * std * std)
    tol = ((_ulp(mean) + _ulp(np.abs(x64).max()) + (m + 20) * 2.0 ** -53 * np.abs(x64).sum() / n) / std
           + (4 * EPS32 + var_rel) * np.abs(ref) + 1e-6)
    err = np.abs(y - ref)
    assert np.all(err <= tol), "worst %.3g x tol at %d" % ((err / tol).max(), np.argmax(err / tol))
    # torch's own fp32 expression (PPO.py:115) differs from float64 by its mean / std rounding (measured here in
    # float64) plus the same elementwise roundings as the kernel
    xt = _dev(x)
    m32, s32 = xt.mean(), xt.std()
    tref = ((xt - m32) / (s32 + 1e-8)).cpu().numpy().astype(np.float64)
    dm, ds = abs(float(m32) - mean), abs(float(s32) - std)
    tol_t = 2 * tol + dm / std + ds / std * np.abs(ref)
    assert np.all(np.abs(y - tref) <= tol_t)


# ------------------------------------------------------------------------------------------------------------ losses
CLIP, ENT = 0.1, 0.01


def _losses64(p, a, old, adv, value, target, clip=CLIP, ent=ENT):
    """float64 autograd of the torch formulation (Categorical(probs=p), PPO.py:124-133), with the fp32 clamp eps of
    the kernel's (float32) Categorical."""
    p = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    value = torch.tensor(value, dtype=torch.float64, requires_grad=True)
    q = p / p.sum(-1, keepdim=True)
    logits = torch.log(torch.clamp(q, EPS32, 1 - EPS32))
    H = -(q * logits).sum(-1)
    logp = logits.gather(1, torch.tensor(a, dtype=torch.int64).view(-1, 1)).view(-1)
    ratio = torch.exp(logp - torch.tensor(old, dtype=torch.float64))
    ad = torch.tensor(adv, dtype=torch.float64)
    s1, s2 = ratio * ad, torch.clamp(ratio, 1 - clip, 1 + clip) * ad
    per = -torch.min(s1, s2) - ent * H
    al = per.mean()
    vl = torch.nn.functional.smooth_l1_loss(value, torch.tensor(target, dtype=torch.float64))
    gp, = torch.autograd.grad(al, p)
    gv, = torch.autograd.grad(vl, value)
    d = dict(al=float(al), vl=float(vl), gp=gp.numpy(), gv=gv.numpy(), per=per.detach().numpy(),
             q=q.detach().numpy(), l=logits.detach().numpy(), logp=logp.detach().numpy(), ratio=ratio.detach().numpy(),
             S=p.detach().sum(-1).numpy())
    return d


def _loss_inputs(B, seed, A=5):
    rs = np.random.RandomState(seed)
    p = rs.gamma(0.8, size=(B, A))
    p *= (rs.uniform(0.3, 3.0, B) / p.sum(1))[:, None]             # rows sum anywhere in [0.3, 3]
    a = rs.randint(0, A, B)
    k = max(1, B // 16)
    p[:k, :] = np.where(np.arange(A)[None] == a[:k, None], 0.0, p[:k])          # q = 0 at the taken action
    one = slice(k, 2 * k)
    p[one] = 0.0
    p[one, a[one]] = rs.uniform(0.3, 3.0, len(p[one]))                         # q = 1 at the taken action
    p = p.astype(np.float32)
    q64 = p.astype(np.float64) / p.astype(np.float64).sum(1, keepdims=True)
    logp = np.log(np.clip(q64[np.arange(B), a], EPS32, 1 - EPS32))
    # ratio just inside / just outside 1 +- clip (1e-4 away: fp32 ratio is within 16 * 2^-23 < 2e-6 of float64)
    r = np.exp(rs.randn(B) * 0.15)
    sel = rs.randint(0, 5, B)
    r = np.where(sel == 1, 1 + CLIP - 1e-4, np.where(sel == 2, 1 + CLIP + 1e-4, np.where(
        sel == 3, 1 - CLIP + 1e-4, np.where(sel == 4, 1 - CLIP - 1e-4, r))))
    old = (logp - np.log(r)).astype(np.float32)
    adv = rs.randn(B).astype(np.float32)
    adv[rs.rand(B) < 0.1] = 0.0                                                 # adv = 0: s1 == s2 ties
    value = (rs.randn(B) * 2).astype(np.float32)
    target = rs.randn(B).astype(np.float32)
    return p, a.astype(np.int32), old, adv, value, target


def _run_losses(p, a, old, adv, value, target, n_valid=None):
    tp = _dev(p).requires_grad_(True)
    tv = _dev(value).view(-1, 1).requires_grad_(True)
    al, vl = _ops().ppo_losses(tp, tv, _dev(a), _dev(old), _dev(adv), _dev(target), clip=CLIP, ent_coef=ENT,
                               n_valid=n_valid)
    gp, gv = torch.autograd.grad(al + vl, (tp, tv))
    gp, gv = gp.cpu().numpy().astype(np.float64), gv.view(-1).cpu().numpy().astype(np.float64)
    return float(al.detach()), float(vl.detach()), gp, gv


@pytest.mark.parametrize("B", [1, 255, 257, 32769])
def test_losses_vs_float64_autograd(B):
    p, a, old, adv, value, target = _loss_inputs(B, B)
    al, vl, gp, gv = _run_losses(p, a, old, adv, value, target)
    R = _losses64(p, a, old, adv, value, target)
    nb = (B + 255) // 256
    # per-row relative error of logp and ratio: q (A + 1 roundings), logf, expf of a difference of magnitude
    # <= |logp| + |old|: rel <= 8 * 2^-23 * (1 + |logp| + |old|)
    rel = 8 * EPS32 * (1 + np.abs(R["logp"]) + np.abs(old))
    row_err = rel * np.abs(R["ratio"] * adv) + ENT * 8 * EPS32 * (np.abs(R["l"]) + 2).sum(1)
    # the sum: a 256-wide tree (8 levels) then the blocks in sequence, each <= 2^-24 of the partial magnitudes
    tol_al = (row_err.sum() + (8 + nb) * EPS32 * np.abs(R["per"]).sum()) / B + EPS32 * abs(R["al"])
    assert abs(al - R["al"]) <= tol_al, (al, R["al"], tol_al)
    d = np.abs(value.astype(np.float64) - target)
    # 0.5 d^2 or |d| - 0.5 (3 roundings each) summed like the action loss
    tol_vl = (8 + nb + 3) * EPS32 * np.where(d < 1, 0.5 * d * d, d - 0.5).sum() / B + EPS32 * vl
    assert abs(vl - R["vl"]) <= tol_vl
    # d/dvalue = clip(d, -1, 1) / B: d and the product, <= 3 roundings
    np.testing.assert_allclose(gv, R["gv"], rtol=3 * EPS32, atol=0)
    # d/dprobs = (gq_k - sum_j gq_j q_j) / S / B with gq = policy term (error rel above) + entropy terms (error
    # 8 eps each): bounded by 8 eps * the magnitudes |gq_k| + sum_j |gq_j q_j|, plus 4 roundings of the final quotient
    q, S = R["q"], R["S"]
    ratio_ad = np.abs(R["ratio"] * adv)
    inside = (q >= EPS32) & (q <= 1 - EPS32)
    gpol = np.zeros_like(q)
    ia = inside[np.arange(B), a]
    gpol[np.arange(B)[ia], a[ia]] = ratio_ad[ia] / q[np.arange(B)[ia], a[ia]]
    gent = ENT * (np.abs(R["l"]) + 1)
    mag = (rel[:, None] * gpol + 8 * EPS32 * gent)
    tol_gp = (mag + (mag * q).sum(1, keepdims=True)) / S[:, None] / B + 4 * EPS32 * np.abs(R["gp"])
    err = np.abs(gp - R["gp"])
    assert np.all(err <= tol_gp), "grad_probs: worst %.3g x tol at %s" % (
        (err / tol_gp).max(), np.unravel_index(np.argmax(err / tol_gp), err.shape))


@pytest.mark.parametrize("n_valid", [1, 256, 257])
def test_losses_padding_across_workgroups_equals_unpadded(n_valid):
    P = 300 + 211                                                # padding spans two or three more workgroups
    p, a, old, adv, value, target = _loss_inputs(n_valid + P, 1000 + n_valid)
    al, vl, gp, gv = _run_losses(p, a, old, adv, value, target, n_valid=n_valid)
    al2, vl2, gp2, gv2 = _run_losses(*(x[:n_valid] for x in (p, a, old, adv, value, target)))
    assert al == al2 and vl == vl2
    assert np.array_equal(gp[:n_valid], gp2) and np.array_equal(gv[:n_valid], gv2)
    assert not gp[n_valid:].any() and not gv[n_valid:].any()


# ------------------------------------------------------------------------------------------------------------ conv
# Inputs on coarse dyadic grids: every product and partial sum below is a multiple of a power of two far below 2^24
# times it, hence exact in fp32 whatever the order -- the float64 references must be matched bit for bit, so a lost
# block-cap remainder, grid-stride tail or sample-loop step shows up as an exact mismatch, not inside a tolerance.
def _dyadic(rs, shape, den, lim):
    return (rs.randint(-lim * den, lim * den + 1, size=shape) / den).astype(np.float32)


@pytest.mark.parametrize("C", [4, 16, 64, 256])
def test_bias_relu_grid_stride_vs_float64(C):
    c4 = C // 4
    n4 = 8192 * 256 * 3 // 2 + 37 * c4                           # > 8192 x 256 float4s: the capped grid strides
    npix = n4 // c4
    rs = np.random.RandomState(C)
    y = _dyadic(rs, (npix, C), 64, 4)
    b = _dyadic(rs, (C,), 64, 2)
    t, tb = _dev(y), _dev(b)
    _libmod().check(_libmod().lib().ppo_bias_relu_nhwc(_marshal().ptr(t), _marshal().ptr(tb), npix, C, _marshal().stream(t)),
                 "ppo_bias_relu_nhwc")
    ref = np.maximum(y.astype(np.float64) + b.astype(np.float64), 0.0)      # exact in fp32 (multiples of 1/64, < 8)
    assert np.array_equal(t.cpu().numpy().astype(np.float64), ref)


def _relu_bwd(gy, y, C):
    npix = gy.shape[0]
    lib = _libmod().lib()
    blocks = lib.ppo_relu_bwd_bias_grad_nhwc_blocks(npix, C)
    tg, ty = _dev(gy), _dev(y)
    gx = torch.empty_like(tg)
    part = torch.empty((max(blocks, 1), C), dtype=torch.float32, device=DEV)
    m = _marshal()
    _libmod().check(lib.ppo_relu_bwd_bias_grad_nhwc(m.ptr(tg), m.ptr(ty), m.ptr(gx), m.ptr(part), npix, C, m.stream(tg)),
                 "ppo_relu_bwd_bias_grad_nhwc")
    return blocks, gx, part


@pytest.mark.parametrize("npix,C", [(n, c) for n in (1, 511, 513, 70000) for c in (4, 12, 48, 256)] +
                         [(4096 * 512 + 1, 4), (4096 * 512 + 1, 16)])
def test_relu_bwd_bias_grad_vs_float64(npix, C):
    rs = np.random.RandomState(npix % 9973 + C)
    gy = _dyadic(rs, (npix, C), 4, 1)                              # |partial sums| <= npix < 2^22: exact in fp32
    y = _dyadic(rs, (npix, C), 4, 1)
    blocks, gx, part = _relu_bwd(gy, y, C)
    if npix > 4096 * 512:
        assert blocks == 4096                                    # past the block cap: > 512 pixels per block
    g64 = np.where(y > 0, gy, 0).astype(np.float64)
    assert np.array_equal(gx.cpu().numpy().astype(np.float64), g64)
    assert np.array_equal(part.sum(0).cpu().numpy().astype(np.float64), g64.sum(0))


def test_relu_bwd_bias_grad_rejects_more_than_256_channels():
    assert _libmod().lib().ppo_relu_bwd_bias_grad_nhwc_blocks(100, 260) < 0
    gy = np.zeros((8, 260), np.float32)
    with pytest.raises(_libmod().TwoarmyLibraryError):
        _relu_bwd(gy, gy, 260)


def _conv1_ref64(frames, w, b):
    B, F, _ = frames.shape
    x = torch.tensor(frames, dtype=torch.float64).view(B, F, 17, 17)
    up = torch.nn.functional.interpolate(x, scale_factor=4, mode="nearest")
    return torch.relu(torch.nn.functional.conv2d(up, torch.tensor(w, dtype=torch.float64),
                                                 torch.tensor(b, dtype=torch.float64), stride=2))


@pytest.mark.parametrize("F", [4, 8])
@pytest.mark.parametrize("B", [1, 256, 257, 1000])
def test_conv1_up4_fwd_bwd_vs_float64(F, B):
    """Forward and weight / bias gradients past 256 samples (the backward's groups walk several samples each)."""
    rs = np.random.RandomState(F * 10000 + B)
    frames = np.array([-1.0, -0.5, 0.5, 1.0], np.float32)[rs.randint(0, 4, (B, F, 289))]
    w = _dyadic(rs, (64, F, 4, 4), 64, 1)
    b = _dyadic(rs, (64,), 64, 1)
    # forward: 16 F products of multiples of 1/128 plus the bias, |.| <= 16 F + 1: exact in fp32 (folded weights too)
    ref = _conv1_ref64(frames, w, b)
    tw, tb = _dev(w).requires_grad_(True), _dev(b).requires_grad_(True)
    y = _ops().conv1_up4_bias_relu(_dev(frames), tw, tb)
    assert torch.equal(y.double().cpu(), ref)
    gy = _dyadic(rs, tuple(ref.shape), 4, 1)
    # gradients: products are multiples of 1/8 and |any partial sum| <= B * 1089 < 2^21: exact in fp32
    gw, gb = torch.autograd.grad(y, (tw, tb), _dev(gy).contiguous(memory_format=torch.channels_last))
    xr = torch.tensor(frames, dtype=torch.float64).view(B, F, 17, 17)
    wr = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    br = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    y64 = torch.relu(torch.nn.functional.conv2d(torch.nn.functional.interpolate(xr, scale_factor=4, mode="nearest"),
                                                wr, br, stride=2))
    gw64, gb64 = torch.autograd.grad(y64, (wr, br), torch.tensor(gy, dtype=torch.float64))
    assert torch.equal(gw.double().cpu(), gw64) and torch.equal(gb.double().cpu(), gb64)


def test_conv1_up4_infer_one_frame_sixteen_channels_vs_float64():
    """Net_Encoder's instantiation (F = 1, C_out = 16) past 256 samples."""
    B = 257
    rs = np.random.RandomState(16)
    frames = np.array([0.0, -1.0, -0.5, 1.0], np.float32)[rs.randint(0, 4, (B, 1, 289))]
    w = _dyadic(rs, (16, 1, 4, 4), 64, 1)
    b = _dyadic(rs, (16,), 64, 1)
    y = _ops().conv1_up4_bias_relu_infer(_dev(frames), _dev(w), _dev(b))    # exact: as in the F = 4 / 8 forward
    assert torch.equal(y.double().cpu(), _conv1_ref64(frames, w, b))


# ------------------------------------------------------------------------------------------------------------ rejections
# Every argument rule of these entry points violated alone, by a raw call past the front end: TW_E_ARG, and after a
# synchronise every output still holds its fill value -- nothing was launched.  The same call with the rule kept is
# accepted.  The shapes are the smallest at which each rule can still be misread.
def _fill(n, dtype=torch.float32, value=CANARY):
    """n elements of `value` with 4 spare ones behind them, so that the same buffer can be passed 4 bytes further on."""
    t = torch.full((n + 4,), value, dtype=dtype, device=DEV)
    assert t.data_ptr() % 16 == 0
    return t


def _each_rejected(fn, good, bad, outs, value=CANARY):
    """bad: (argument position, value) pairs, each put alone into the accepted argument list `good`."""
    canaries = [(t, value) for t in outs]
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert rejected(fn, args, canaries), (fn, i, getattr(v, "value", v))
    assert accepted(fn, good), fn
    assert not all(bool((t == value).all()) for t in outs), fn                  # the accepted call does write


def test_gae_rejections_launch_nothing():
    T, N = 5, 9
    r, v, nv = (_dev(np.ones((T, N), np.float32)) for _ in range(3))
    done = torch.zeros((T, N), dtype=torch.uint8, device=DEV)
    outs = [_fill(T * N) for _ in range(3)]
    good = [_P(r), _P(v), _P(nv), _P(done), 0.99, 0.95, 1, T, N] + [_P(o) for o in outs]
    bad = [(0, None), (1, None), (2, None), (3, None), (7, 0), (7, -1), (8, 0), (8, -1)]    # (3, None): mask without done
    _each_rejected("ppo_gae", good, bad, outs)


def test_adv_norm_rejections_launch_nothing():
    n = 9
    adv = _fill(n)
    ws = _fill(4096, torch.float64)
    good = [_P(adv), n, 1e-8, _P(ws)]
    _each_rejected("ppo_adv_norm", good, [(0, None), (1, 0), (1, -1), (3, None)], [adv, ws])


def test_loss_rejections_launch_nothing():
    B, A = 3, 5
    probs = torch.full((B, A), 0.2, device=DEV)
    action = torch.zeros(B, dtype=torch.int32, device=DEV)
    old, adv, value, target = (torch.full((B,), x, device=DEV) for x in (-1.6, 1.0, 0.5, 0.0))
    outs = [_fill(2), _fill(B * A), _fill(B), _fill(2)]                         # losses, grad_probs, grad_value, workspace
    good = [_P(x) for x in (probs, action, old, adv, value, target)] + [B, B, A, 0.1, 0.01] + [_P(o) for o in outs]
    bad = [(i, None) for i in (0, 1, 2, 3, 4, 5, 11, 12, 13, 14)]
    bad += [(8, a) for a in (2, 3, 4, 6, 7)] + [(7, 0), (7, B + 1)]
    _each_rejected("ppo_loss_fwd_bwd_masked", good, bad, outs)


def test_prior_loss_and_episode_summary_reject_unbuilt_action_counts():
    B = 3
    probs = torch.full((B, 8), 0.125, device=DEV)
    moves = torch.ones(B, dtype=torch.uint8, device=DEV)
    outs = [_fill(2), _fill(2, torch.int32, -7), _fill(B * 8), _fill(4)]        # out, counts, grad_probs, workspace
    good = [_P(probs), _P(moves), B, B, 5, 1.0] + [_P(o) for o in outs]
    for a in (1, 6, 8):
        args = list(good)
        args[4] = a
        assert rejected("ppo_prior_loss_fwd_bwd", args, [(outs[0], CANARY), (outs[1], -7), (outs[2], CANARY),
                                                         (outs[3], CANARY)]), a
    T, N = 5, 9
    ep_r = torch.ones((T, N), dtype=torch.float64, device=DEV)
    ep_l = torch.ones((T, N), dtype=torch.int32, device=DEV)
    term = torch.ones((T, N), dtype=torch.uint8, device=DEV)
    trunc = torch.zeros((T, N), dtype=torch.uint8, device=DEV)
    rew = torch.ones((T, N), device=DEV)
    act = torch.zeros((T, N), dtype=torch.int32, device=DEV)
    score, summary, ws = _fill(1, torch.float64), _fill(8, torch.float64), _fill(24, torch.float64)
    ah, rh = _fill(7, torch.int64, -7), _fill(6, torch.int64, -7)
    good = [_P(x) for x in (ep_r, ep_l, term, trunc, rew, act)] + [5, T, N, 0.99, 0.01] + [_P(x) for x in (score, summary, ah, rh, ws)]
    can = [(score, CANARY), (summary, CANARY), (ws, CANARY), (ah, -7), (rh, -7)]
    args = list(good)
    args[6] = 6
    assert rejected("ppo_episode_summary", args, can)
    assert accepted("ppo_episode_summary", good) and not bool((summary[:8] == CANARY).any())


def test_bias_relu_rejections_launch_nothing():
    npix, Cc = 2, 8
    y, bias = _fill(npix * Cc), _fill(Cc)
    good = [_P(y), _P(bias), npix, Cc]
    _each_rejected("ppo_bias_relu_nhwc", good, [(3, 6), (0, _P(y, 4)), (1, _P(bias, 4))], [y])


def test_relu_bwd_bias_grad_rejects_each_misaligned_pointer():
    npix, Cc = 2, 8
    gy, y = _fill(npix * Cc, value=1.0), _fill(npix * Cc, value=1.0)
    gx, part = _fill(npix * Cc), _fill(Cc)
    good = [_P(gy), _P(y), _P(gx), _P(part), npix, Cc]
    bad = [(i, _P(t, 4)) for i, t in enumerate((gy, y, gx, part))]
    _each_rejected("ppo_relu_bwd_bias_grad_nhwc", good, bad, [gx, part])


def test_conv1_up4_rejections_launch_nothing():
    B, F = 2, 4
    frames = torch.ones(B * 8 * 289, device=DEV)                                # room for F = 8 as well
    wf, bias, out = _fill(16 * 8 * 64, value=0.5), _fill(64, value=0.5), _fill(B * 1089 * 64)
    good = [_P(frames), B, F, 64, _P(wf), _P(bias), _P(out)]
    bad = [(4, _P(wf, 4)), (5, _P(bias, 4)), (6, _P(out, 4))]
    for f, c in ((4, 16), (1, 64), (2, 64)):                                    # two arguments make one rule here
        args = list(good)
        args[2], args[3] = f, c
        assert rejected("ppo_conv1_up4_bias_relu_c", args, [(out, CANARY)]), (f, c)
    _each_rejected("ppo_conv1_up4_bias_relu_c", good, bad, [out])
    gy, y = _fill(B * 1089 * 64, value=1.0), _fill(B * 1089 * 64, value=1.0)
    gw, gb = _fill(B * 16 * 8 * 64), _fill(B * 4 * 64)
    good = [_P(frames), B, F, _P(gy), _P(y), _P(gw), _P(gb)]
    bad = [(2, 1), (1, 0)] + [(i + 3, _P(t, 4)) for i, t in enumerate((gy, y, gw, gb))]
    _each_rejected("ppo_conv1_up4_bwd", good, bad, [gw, gb])
