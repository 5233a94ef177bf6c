"""The shortest-path prior on the device: mg_nav_optimal_moves (exact integers against prior_ref.py), the fused
set-valued imitation loss ppo_prior_loss_fwd_bwd (against float64 autograd under a rounding bound derived below), and the
trainer / CLI plumbing around them."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import nav_ref
import prior_ref
import visit_ref
from nav_util import dev, host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = nav_ref.UNREACHABLE
EPS32 = prior_ref.EPS32
SIDES = [(1, 1), (1, 7), (5, 9), (17, 17), (32, 32)]                  # (W, H)


def nav():
    from twoarmy_amd import minigrid_nav
    return minigrid_nav


def ops():
    from twoarmy_amd import ppo_ops
    return ppo_ops


# ------------------------------------------------------------------------------------------------ labels
_CASES = {}


def case(W, H, N):
    """N random worlds of one size with their BFS fields, computed once and never modified."""
    key = (W, H, N)
    if key not in _CASES:
        rng = np.random.default_rng(11 * W + 37 * H + 1000 * N)
        ty, st = np.zeros((N, W * H), np.uint8), np.zeros((N, W * H), np.uint8)
        for n in range(N):
            ty[n], st[n] = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[n % 3])
            ty[n][ty[n] == 8] = 1
            ty[n][rng.permutation(W * H)[:min((1, 3, 0)[n % 3] if N > 1 else 1, W * H)]] = 8
        dist = nav_ref.fields(ty, st, W, H)[0]
        for a in (ty, st, dist):
            a.setflags(write=False)
        _CASES[key] = dict(ty=ty, st=st, dist=dist, tables=[prior_ref.cell_moves(dist[n], W, H) for n in range(N)])
    return _CASES[key]


def positions(rng, T, N, W, H):
    """Every cell in turn (cell centres and corners), then the edge values of the cell rule."""
    k = np.arange(T * N)
    c = (k * 7 + k // (W * H)) % (W * H)
    pos = np.stack([c // W + rng.choice([0.0, 0.5, 0.999], T * N), c % W + rng.choice([0.0, 0.5, 0.999], T * N)], 1)
    pos = pos.astype(np.float32)
    special = [np.nan, np.inf, -np.inf, -0.0, W - 1, W, H - 1, H, -1, -0.5, np.float32(H) - np.float32(1e-6)]
    i = 0
    for a in special:
        for b in special:
            if i < T * N and T * N > 8:
                pos[(i * 3) % (T * N)] = (a, b)
            i += 1
    return pos.reshape(T, N, 2)


def on_sources_and_cut_off_cells(pos, dist, W):
    """Rows 2 and 3 of pos: every env on its first source / its first unreachable cell, where it has one."""
    for n in range(pos.shape[1]):
        for t, cells in ((2, np.flatnonzero(dist[n] == 0)), (3, np.flatnonzero(dist[n] == U))):
            if cells.size:
                pos[t, n] = (cells[0] // W + 0.5, cells[0] % W + 0.25)
    return pos


def run_moves(dist, pos, W, H, age=None, init_pos=None, off=0, want_dist=True, pad=0):
    """The kernel through the front end, outputs at byte / element offset `off` inside 0xA5-filled buffers and the
    field's rows padded by `pad`; checks that nothing but the outputs changed.  -> (moves, acting_dist) on the host."""
    T, N = pos.shape[:2]
    M = T * N
    mbuf = torch.full((16 + off + M + 37,), 0xA5, dtype=torch.uint8, device=DEV)
    dbuf = torch.full((16 + 2 * (off + M) + 38,), 0xA5, dtype=torch.uint8, device=DEV)
    mv = mbuf[16 + off:16 + off + M].view(T, N)
    dv = dbuf[16 + 2 * off:16 + 2 * (off + M)].view(torch.uint16).view(T, N)
    assert mbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0
    field = dev(np.concatenate([dist, np.full((N, pad), 0xA5A5, np.uint16)], axis=1))[:, :W * H]
    got = nav().optimal_moves(field, dev(pos), W, H, age=None if age is None else dev(age),
                              init_pos=None if init_pos is None else dev(init_pos), out=mv,
                              dist_out=dv if want_dist else False)
    assert got[0] is mv and (got[1] is dv if want_dist else got[1] is None)
    hm, hd = host(mbuf), host(dbuf)
    assert (hm[:16 + off] == 0xA5).all() and (hm[16 + off + M:] == 0xA5).all()
    assert (hd[:16 + 2 * off] == 0xA5).all() and (hd[16 + 2 * (off + M):] == 0xA5).all()
    if not want_dist:
        assert (hd == 0xA5).all()
    return host(mv), host(dv) if want_dist else None


@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("W,H", SIDES)
def test_moves_equal_the_reference(W, H, N):
    c = case(W, H, N)
    rng = np.random.default_rng(W * 100 + H + N)
    init = np.array([H - 1 + 0.5, 0.25], np.float32)
    for i, T in enumerate((1, 5, 64)):
        pos = positions(rng, T, N, W, H)
        if T >= 5:
            on_sources_and_cut_off_cells(pos, c["dist"], W)
        age = rng.integers(-1, 3, (T, N)).astype(np.int32)
        want = prior_ref.optimal_moves(c["dist"], pos, W, H, tables=c["tables"])
        want_age = prior_ref.optimal_moves(c["dist"], pos, W, H, age, init, c["tables"])
        for off in range(4):
            m, d = run_moves(c["dist"], pos, W, H, off=off, pad=(0, 1, 7, 2)[off])                 # age = NULL
            assert np.array_equal(m, want[0]) and np.array_equal(d, want[1]), (T, off)
        m, d = run_moves(c["dist"], pos, W, H, age, init, off=(i + 1) % 4)
        assert np.array_equal(m, want_age[0]) and np.array_equal(d, want_age[1]), T
        m, d = run_moves(c["dist"], pos, W, H, age, init, off=i, want_dist=False)                  # acting_dist = NULL
        assert np.array_equal(m, want_age[0]) and d is None
        if T >= 5 and T * N >= 64 and W * H > 1:                 # the cases are worth their name
            assert (want[0] == 0).any() and (age <= 0).any()
            if N > 1:
                assert (want[1] == U).any() and (want[1] != U).any() and not np.array_equal(want[0], want_age[0])
    if N == 65 and W * H >= 45:
        assert {bin(int(v)).count("1") for v in want[0].ravel()} >= {0, 1, 2} and (want[0] == prior_ref.STAY).any()


def test_more_than_one_workgroup_and_every_alignment():
    """4200 elements: three workgroups of 2048, each output at every offset of a 16-byte chunk."""
    W = H = 17
    N, T = 3, 1400
    c = case(W, H, N)
    rng = np.random.default_rng(5)
    pos = positions(rng, T, N, W, H)
    age = (rng.integers(0, 40, (T, N)) - 1).astype(np.int32)
    init = np.array([15.0, 3.0], np.float32)
    want = prior_ref.optimal_moves(c["dist"], pos, W, H, age, init, c["tables"])
    for off in (0, 1, 7, 8, 15):
        m, d = run_moves(c["dist"], pos, W, H, age, init, off=off)
        assert np.array_equal(m, want[0]) and np.array_equal(d, want[1]), off


@pytest.mark.parametrize("W,H", [(5, 9), (17, 17), (32, 32)])
def test_lowest_bit_is_the_field_kernels_expert_action(W, H):
    """Kernel to kernel: mg_nav_field's agent_action on a cell == the lowest set bit of mg_nav_optimal_moves there."""
    N, T = 65, 5
    c = case(W, H, N)
    rng = np.random.default_rng(W + H)
    ty, st = dev(c["ty"]), dev(c["st"])
    field = nav().distance_field(ty, st, W, H)[0]
    ax, ay = rng.integers(0, W, (T, N)).astype(np.int32), rng.integers(0, H, (T, N)).astype(np.int32)
    pos = np.stack([ay, ax], -1).astype(np.float32)
    moves, adist = nav().optimal_moves(field, dev(pos), W, H)
    moves, adist = host(moves), host(adist)
    for t in range(T):
        _, fd, fa, _ = nav().distance_field(ty, st, W, H, agent=(dev(ax[t]), dev(ay[t])), want_field=False)
        assert [prior_ref.lowest_action(v) for v in moves[t]] == host(fa).tolist()
        assert np.array_equal(adist[t].astype(np.int64), host(fd))
    assert {prior_ref.lowest_action(v) for v in moves.ravel()} >= {-1, 0, 1, 2, 3}


def test_moves_bad_arguments_launch_nothing():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    W, H, N, T = 5, 4, 3, 2
    dist = torch.zeros((N, W * H + 2), dtype=torch.int16, device=DEV)
    pos = torch.zeros((T + 1, N, 2), dtype=torch.float32, device=DEV)
    age = torch.ones((T + 1, N), dtype=torch.int32, device=DEV)
    init = torch.zeros(4, dtype=torch.float32, device=DEV)
    moves = torch.full((T * N + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    ad = torch.full((2 * T * N + 4,), 0xA5, dtype=torch.uint8, device=DEV)
    good = dict(dist=dist.data_ptr(), pitch=W * H + 2, n=N, W=W, H=H, pos=pos.data_ptr(), age=age.data_ptr(),
                init=init.data_ptr(), T=T, moves=moves.data_ptr(), ad=ad.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        v = lambda x: None if x is None else C.c_void_p(x)                              # noqa: E731
        return lib.mg_nav_optimal_moves(v(a["dist"]), a["pitch"], a["n"], a["W"], a["H"], v(a["pos"]), v(a["age"]),
                                        v(a["init"]), a["T"], v(a["moves"]), v(a["ad"]), None)
    bad = [dict(dist=None), dict(pos=None), dict(moves=None), dict(n=0), dict(n=-1), dict(T=-1), dict(W=0), dict(H=0),
           dict(W=33), dict(H=33), dict(pitch=W * H - 1), dict(pitch=-1), dict(dist=good["dist"] + 1),
           dict(ad=good["ad"] + 1), dict(pos=good["pos"] + 4), dict(age=good["age"] + 2), dict(init=good["init"] + 1),
           dict(init=None), dict(n=1 << 20, T=1 << 20)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(T=0) == 0
    torch.cuda.synchronize()
    assert (host(moves) == 0xA5).all() and (host(ad) == 0xA5).all()
    assert call() == 0 and call(age=None, init=None, ad=None, moves=good["moves"] + 1) == 0     # and the good calls launch
    torch.cuda.synchronize()
    assert (host(moves)[:T * N + 1] == prior_ref.STAY).all() and (host(moves)[T * N + 1:] == 0xA5).all()   # all-zero field
    assert (host(ad)[:2 * T * N] == 0).all() and (host(ad)[2 * T * N:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ loss
LOSS_A = (2, 3, 4, 5, 7)
LOSS_B = (1, 63, 65, 257, 1000)


def loss_inputs(B, A, seed):
    """Rows that sum anywhere in [0.3, 3]; masks over all 8 bits (bits >= A ignored), a share of them single-bit, full
    and empty; rows with m = 0 and m = 1; tie rows.  Conditions on the inputs, checked here on the CPU in float64:
    * a row whose clamp is not meant to act has 1e-3 / 4 <= m <= 1 - 1e-3 / 4 (every entry is at least 1e-3 of its row);
    * the two largest q of a row are exactly equal (tie rows: the lowest index wins) or more than 1e-3 apart, so the
      float32 arg-max is the float64 one."""
    rs = np.random.RandomState(seed)
    p = rs.gamma(0.8, size=(B, A)) + 0.02
    mask = rs.randint(0, 256, B).astype(np.uint8)
    kind = rs.randint(0, 10, B)
    a = rs.randint(0, A, B)
    mask = np.where(kind == 0, 1 << a, mask)                               # single-bit masks
    mask = np.where(kind == 1, 0xFF, mask)                                 # full masks (and bits >= A)
    mask = np.where(kind == 2, (1 << A) - 1, mask)                         # full, nothing above
    mask = np.where(kind == 3, 0xFF & ~((1 << A) - 1), mask).astype(np.uint8)      # only ignored bits: unlabelled
    bits = prior_ref.mask_bits(mask, A) > 0
    p = np.where((kind == 4)[:, None] & bits, 0.0, p)                      # m = 0 (or an all-zero row, mended below)
    p = np.where((kind == 5)[:, None] & ~bits, 0.0, p)                     # m = 1
    p[p.sum(1) == 0] = 1.0
    for _ in range(50):                                                    # separate the two largest entries
        srt = np.sort(p / p.sum(1, keepdims=True), 1)
        close = (srt[:, -1] - srt[:, -2] < 4e-3) if A > 1 else np.zeros(B, bool)
        if not close.any():
            break
        top = np.argmax(p, 1)
        p[close, top[close]] *= 1.5
    tie = kind == 6
    top = np.argmax(p, 1)
    other = (top + 1 + rs.randint(0, A - 1, B)) % A
    p[tie, other[tie]] = p[tie, top[tie]]
    p *= (rs.uniform(0.3, 3.0, B) / p.sum(1))[:, None]
    p = p.astype(np.float32)
    p[tie, other[tie]] = p[tie, top[tie]]                                  # equal as float32, hence as q
    p64 = p.astype(np.float64)
    q = p64 / p64.sum(1, keepdims=True)
    srt = np.sort(q, 1)
    gap = srt[:, -1] - srt[:, -2]
    assert ((gap == 0) | (gap > 1e-3)).all() and (gap[~tie] > 1e-3).all()
    m = (q * bits).sum(1)
    lab = bits.any(1)
    free = lab & (m > 0) & ((q * ~bits).sum(1) > 0)
    assert ((m[free] >= 2.5e-4) & (m[free] <= 1 - 2.5e-4)).all()
    return p, mask, np.argmax(q, 1)


def run_loss(p, mask, coef, n_valid=None):
    tp = dev(p).requires_grad_(True)
    loss, (out, counts) = ops().prior_loss(tp, dev(mask), coef, n_valid=n_valid)
    gp, = torch.autograd.grad(loss, tp)
    assert float(loss.detach()) == float(out[0])
    return host(out).astype(np.float64), host(counts), host(gp).astype(np.float64), out, counts, gp


def check_loss(p, mask, top, coef, n_valid=None):
    """Kernel against float64 under the rounding bound; -> the largest |err| / bound seen.
    Roundings, each counted as 2^-23 (twice the unit roundoff) of the magnitude it acts on:
      S = sum p: A - 1;  q = p / S: 1;  m = sum of the masked q: A - 1  -> m is relative-accurate to (2A - 1) eps (all
      terms are non-negative);  l = -logf(clamp(m)): the relative error of m as an absolute one, plus 2 eps |l| for logf
      -> row error (2A + 1) eps (1 + |l|).  Clamped rows hold the constants -log(eps) / -log(1 - eps): inside the same bound.
      The sum of n rows: a 256-wide tree (8 levels) then the nb blocks in sequence: (8 + nb) eps sum|l|; the division by
      the count, the product with coef and the final rounding: 3 eps |loss|.  The mean mass alike with (2A - 1) eps m.
      Gradient coef / n * (1 - [j in mask] / m) / S: 1 / m carries (2A - 1) + 1 roundings -> 2A eps / m absolute (one
      spare: 2A + 1) in the bracket, which cancels where m is near 1; the subtraction, S (A - 1), the division, coef / n
      and the product: A + 3 relative roundings of the result (one spare: A + 4)."""
    B, A = p.shape
    out, counts, gp, *_ = run_loss(p, mask, coef, n_valid)
    R = prior_ref.loss64(p, mask, coef, n_valid)
    lab, n = R["lab"], R["labelled"]
    nb = (B + 255) // 256
    bits = prior_ref.mask_bits(mask, A)
    assert counts.tolist() == [n, int((bits[np.arange(B), top] > 0)[lab].sum())]
    assert np.isfinite(out).all() and np.isfinite(gp).all()
    if n == 0:
        assert out.tolist() == [0.0, 0.0] and not gp.any()
        return 0.0
    l, m = R["l"][lab], R["m"][lab]
    tol_l = coef * (((2 * A + 1) * EPS32 * (1 + np.abs(l))).sum() + (8 + nb) * EPS32 * np.abs(l).sum()) / n \
        + 3 * EPS32 * abs(R["loss"])
    tol_m = ((2 * A - 1) * EPS32 * m).sum() / n + (8 + nb) * EPS32 * m.sum() / n + 2 * EPS32 * R["mass"]
    worst = max(abs(out[0] - R["loss"]) / tol_l, abs(out[1] - R["mass"]) / tol_m)
    assert abs(out[0] - R["loss"]) <= tol_l, (out[0], R["loss"], tol_l)
    assert abs(out[1] - R["mass"]) <= tol_m, (out[1], R["mass"], tol_m)
    inside = lab & (R["m"] >= EPS32) & (R["m"] <= 1 - EPS32)
    assert not gp[~inside].any()                                        # clamp active, unlabelled, padding: exactly 0
    assert not R["gp"][~inside].any()
    if inside.any():
        mi, Si = R["m"][inside][:, None], R["S"][inside][:, None]
        tol_g = coef / (n * Si) * (2 * A + 1) * EPS32 * bits[inside] / mi + (A + 4) * EPS32 * np.abs(R["gp"][inside])
        err = np.abs(gp[inside] - R["gp"][inside])
        assert np.all(err <= tol_g), "grad_probs: worst %.3g x bound" % (err / tol_g).max()
        worst = max(worst, (err / tol_g).max())
    return worst


@pytest.mark.parametrize("A", LOSS_A)
def test_loss_vs_float64_autograd(A):
    worst = 0.0
    for B in LOSS_B:
        p, mask, top = loss_inputs(B, A, 100 * A + B)
        worst = max(worst, check_loss(p, mask, top, 0.5))
        if B >= 257:
            R = prior_ref.loss64(p, mask, 0.5)
            clamped = R["lab"] & ((R["m"] < EPS32) | (R["m"] > 1 - EPS32))
            assert (R["m"][clamped] == 0).any() and (R["m"][clamped] > 0.5).any() and (~R["lab"]).any()
    print("A = %d: largest |err| / bound %.3f" % (A, worst))


@pytest.mark.parametrize("n_valid", [1, 256, 257])
def test_loss_padding_across_workgroups(n_valid):
    P = 300 + 211                                                # padding spans two or three more workgroups
    p, mask, top = loss_inputs(n_valid + P, 5, 7000 + n_valid)
    mask[0] |= 1                                                 # n_valid = 1 keeps a labelled row
    check_loss(p, mask, top, 1.25, n_valid)
    out, counts, gp, *_ = run_loss(p, mask, 1.25, n_valid)
    out2, counts2, gp2, *_ = run_loss(p[:n_valid], mask[:n_valid], 1.25)
    assert np.array_equal(out, out2) and np.array_equal(counts, counts2)
    assert np.array_equal(gp[:n_valid], gp2) and not gp[n_valid:].any()


def test_single_bit_masks_are_the_categorical_log_prob_and_no_labels_are_zeros():
    B, A, coef = 1000, 5, 0.3
    p, _, top = loss_inputs(B, A, 42)
    a = np.random.RandomState(1).randint(0, A, B)
    mask = (1 << a).astype(np.uint8)
    check_loss(p, mask, top, coef)
    out, counts, gp, *_ = run_loss(p, mask, coef)
    # torch's own float32 Categorical on the host (its clamp eps is that of the dtype, so float32 it is): the same
    # formula evaluated with other roundings, a few ulp per row and 10 tree levels of the mean
    want = float(-torch.distributions.Categorical(probs=torch.tensor(p)).log_prob(torch.tensor(a)).double().mean() * coef)
    assert abs(out[0] - want) <= 64 * EPS32 * abs(want) and counts[0] == B
    for none in (np.zeros(B, np.uint8), np.full(B, 0xE0, np.uint8)):
        out, counts, gp, *_ = run_loss(p, none, coef)
        assert out.tolist() == [0.0, 0.0] and counts.tolist() == [0, 0] and not gp.any()
    out, counts, gp, *_ = run_loss(p, mask, coef, n_valid=0)
    assert out.tolist() == [0.0, 0.0] and counts.tolist() == [0, 0] and not gp.any()


def test_two_calls_give_equal_bits_and_the_nodes_add():
    B, A = 1000, 5
    p, mask, _ = loss_inputs(B, A, 77)
    r1, r2 = run_loss(p, mask, 0.7), run_loss(p, mask, 0.7)
    assert torch.equal(r1[3], r2[3]) and torch.equal(r1[4], r2[4]) and torch.equal(r1[5], r2[5])
    rs = np.random.RandomState(3)
    tp = dev(p).requires_grad_(True)
    tv = dev(rs.randn(B, 1).astype(np.float32)).requires_grad_(True)
    act, old = dev(rs.randint(0, A, B).astype(np.int32)), dev((rs.randn(B) * 0.1 - 1.6).astype(np.float32))
    adv, tgt = dev(rs.randn(B).astype(np.float32)), dev(rs.randn(B).astype(np.float32))
    al, vl = ops().ppo_losses(tp, tv, act, old, adv, tgt)
    pl, _ = ops().prior_loss(tp, dev(mask), 0.7)
    g_al, = torch.autograd.grad(al, tp, retain_graph=True)
    g_pl, = torch.autograd.grad(pl, tp, retain_graph=True)
    (al + pl).backward()
    assert g_pl.abs().max() > 0 and torch.equal(tp.grad, g_al + g_pl)
    assert float((al + pl).detach()) == float(al.detach() + pl.detach())


def test_loss_bad_arguments():
    from twoarmy_amd import _lib
    lib = _lib.lib()
    B, A = 8, 5
    t = [torch.zeros(B * A, device=DEV), torch.zeros(B, dtype=torch.uint8, device=DEV), torch.zeros(2, device=DEV),
         torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(B * A, device=DEV), torch.zeros(4, device=DEV)]
    ptrs = [C.c_void_p(x.data_ptr()) for x in t]

    def call(B=B, n_valid=B, A=A, drop=None):
        a = [None if i == drop else q for i, q in enumerate(ptrs)]
        return lib.ppo_prior_loss_fwd_bwd(a[0], a[1], B, n_valid, A, 1.0, a[2], a[3], a[4], a[5], None)
    for kw in [dict(B=0), dict(n_valid=-1), dict(n_valid=B + 1), dict(A=1), dict(A=6), dict(A=8)] + \
            [dict(drop=i) for i in range(6)]:
        assert call(**kw) == -1, kw


# ------------------------------------------------------------------------------------------------ trainer, CLI
def _trainer(state=None):
    from twoarmy_amd.engine import TwoarmyEngine
    from twoarmy_amd.soa.agent.PPO import PPO
    from twoarmy_amd.soa.ppo_vec import VecPPOTrainer
    torch.manual_seed(5)
    eng = TwoarmyEngine(4, 8, 17, seed=9981)
    agent = PPO()
    agent.K_epochs = 1
    if state is not None:
        agent.actor.load_state_dict(state[0]); agent.critic.load_state_dict(state[1])
    agent.to(eng.device).use_nhwc()
    return VecPPOTrainer(agent, eng, rollout_steps=8, minibatch=32), eng


def _state(tr):
    return ({k: v.clone() for k, v in tr.agent.actor.state_dict().items()},
            {k: v.clone() for k, v in tr.agent.critic.state_dict().items()})


def test_trainer_labels_stats_and_update(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)      # scoped: two updates must agree bit for bit
    T, N = 8, 8
    plain, e0 = _trainer()
    state = _state(plain)
    prior, e1 = _trainer(state)
    twin, e2 = _trainer(state)
    with pytest.raises(RuntimeError):
        prior.prior_stats()
    prior.enable_prior(0.5, decay=0.5)
    assert plain.prior is None and plain.expert_moves is None and twin.expert_moves is None
    perms = [torch.randperm(T * N, generator=torch.Generator().manual_seed(u)) for u in range(2)]
    for u in range(2):
        for tr in (plain, prior, twin):
            tr.collect()
        if u == 0:
            assert torch.equal(prior.action, plain.action) and torch.equal(prior.pos, plain.pos)
        with pytest.raises(RuntimeError):
            prior.update(permutations=[perms[u]])                         # labels of this rollout are missing
        if u == 1:
            prior.account_distance()                                      # label_expert() reuses this rollout's field
        moves = prior.label_expert()
        assert moves is prior.expert_moves and moves.dtype == torch.uint8 and moves.shape == (T, N)
        # the labels against the host reference on the engine's planes and the acting positions
        ty = e1.get_state()[0]
        field = nav_ref.fields(ty, None, 17, 17, nav_ref.PASS_DEFAULT | (1 << 6))[0]
        assert np.array_equal(host(prior.nav_field).view(np.uint16), field)
        pos, age = host(prior.pos[3:3 + T]), host(prior.age[:-1])
        acting = prior_ref.acting_positions(pos, age, host(prior.init_pos))
        idx = torch.arange(T * N, device=DEV)
        p4 = prior._policy_x((idx // N).int(), (idx % N).int(), False)[1]
        assert np.array_equal(host(p4[:, 3]).reshape(T, N, 2), acting)
        want_m, want_d = prior_ref.optimal_moves(field, pos, 17, 17, age, host(prior.init_pos))
        assert np.array_equal(host(moves), want_m) and np.array_equal(host(prior.expert_dist).view(np.uint16), want_d)
        assert (u > 0 or (age <= 0).any()) and (want_m != 0).any()   # the first rollout starts at the reset position
        # the statistics against numpy
        ps = prior.prior_stats()
        act, probs = host(prior.action), host(prior.act_probs).astype(np.float64)
        bits = prior_ref.mask_bits(prior_ref.to_policy_mask(want_m, 5).ravel(), 5).reshape(T, N, 5)
        lab = bits.sum(-1) > 0
        hit = bits[np.arange(T)[:, None], np.arange(N)[None], act] > 0
        mass = (probs * bits).sum(-1) / probs.sum(-1)
        assert ps["labelled"] == int(lab.sum()) and ps["agree"] == (hit & lab).sum() / lab.sum()
        assert abs(ps["opt_mass"] - mass[lab].mean()) <= 1e-12 and ps["coef"] == 0.5 * 0.5 ** u
        assert np.allclose(probs.sum(-1), 1.0, atol=1e-5) and (probs > 0).all()
        # the updates: the critic does not see the prior, the actor does; plain trainers are what they were
        losses = [tr.update(permutations=[perms[u]]) for tr in (plain, prior, twin)]
        assert all(torch.equal(a, b) for a, b in zip(losses[0], losses[2]))
        for a, b in zip(list(plain.agent.actor.parameters()) + list(plain.agent.critic.parameters()),
                        list(twin.agent.actor.parameters()) + list(twin.agent.critic.parameters())):
            assert torch.equal(a, b)
        if u == 0:                                                        # one start, one rollout: only the actor's step differs
            assert torch.equal(losses[0][1], losses[1][1])                  # the value loss of the last minibatch
            for a, b in zip(plain.agent.critic.parameters(), prior.agent.critic.parameters()):
                assert torch.equal(a, b)
            assert any(not torch.equal(a, b)
                       for a, b in zip(plain.agent.actor.parameters(), prior.agent.actor.parameters()))
        logged = prior.agent.writer.scalars
        assert len(logged["loss/prior_loss_update"]) == 2 * (u + 1) and "loss/prior_loss_update" not in plain.agent.writer.scalars
        assert logged["loss/prior_loss_update"][-1][1] > 0
        for tr in (plain, prior, twin):
            tr.carry_over()
    for e in (e0, e1, e2):
        e.close()


ARGS = ["--env", "MiniGrid-twoarmy-17x17-v4", "--num_envs", "8", "--rollout_steps", "8", "--minibatch", "32",
        "--k_epochs", "1", "--updates", "1"]


def test_train_ppo_appends_the_expert_fields_only_when_asked(capsys):
    from twoarmy_amd.soa import train_ppo
    lines = lambda: [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]     # noqa: E731
    a = train_ppo.main(ARGS)
    none = lines()
    b = train_ppo.main(ARGS + ["--prior_coef", "0.1"])
    with_prior = lines()
    c = train_ppo.main(ARGS + ["--expert_agreement"])
    only_stats = lines()
    assert len(none) == len(with_prior) == len(only_stats) == 1
    assert a.prior is None and a.expert_moves is None and "expert" not in none[0]
    assert re.search(r" rewards \[[\d ]+\]$", none[0])                    # the line ends where it always did
    pat = r" expert agree (\d\.\d{3}) opt_mass (\d\.\d{3})$"
    m, s = re.search(pat, with_prior[0]), re.search(pat, only_stats[0])
    assert m and s and m.groups() == s.groups()                          # the first rollout precedes any update
    assert 0 < float(m.group(2)) < 1
    blank = lambda ln: re.sub(r"-?\d+(?:\.\d+)?|(?<=[ /])-(?=[ /])", "#", ln)       # noqa: E731
    assert blank(with_prior[0][:m.start()]) == blank(none[0])
    assert b.prior["coef"] == 0.1 and b.prior["updates"] == 1 and "loss/prior_loss_update" in b.agent.writer.scalars
    assert c.prior["coef"] == 0.0 and "loss/prior_loss_update" not in c.agent.writer.scalars      # no loss launch
