"""Host-side checks of the shortest-path prior: the test reference of the optimal-move sets (prior_ref.py) against
nav_ref's expert action, the float64 statement of the set-valued loss against torch's Categorical and against the
header's gradient formula, and the front end's constants and mask mapping.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import nav_ref
import prior_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = nav_ref.UNREACHABLE


@pytest.fixture(autouse=True)
def front_end():
    """The feature under test: both ABI functions are declared, bound and fronted."""
    import twoarmy_amd
    from twoarmy_amd import minigrid_nav as nav, ppo_ops
    syms = twoarmy_amd._lib.exported_symbols()
    assert "mg_nav_optimal_moves" in syms and "ppo_prior_loss_fwd_bwd" in syms
    assert callable(nav.optimal_moves) and callable(nav.to_policy_mask) and callable(ppo_ops.prior_loss)
    return nav


def _worlds():
    """About 100 random worlds up to 32 x 32: (W, H, type, state, goal or None)."""
    rng = np.random.default_rng(20240)
    sizes = [(1, 1), (1, 7), (7, 1), (5, 9), (9, 4), (17, 17), (31, 32), (32, 32)]
    out = []
    for i in range(100):
        W, H = sizes[i % len(sizes)]
        ty, st = nav_ref.random_world(rng, W, H, (0.0, 0.2, 0.45)[i % 3])
        for g in rng.integers(0, W * H, i % 4):
            ty[g] = 8
        goal = None if i % 2 == 0 else (int(rng.integers(0, W)), int(rng.integers(0, H)))
        out.append((W, H, ty, st, goal))
    return out


def test_lowest_bit_is_the_expert_action_on_every_cell(front_end):
    stay = front_end.MOVE_STAY
    assert stay == prior_ref.STAY
    seen = set()
    for W, H, ty, st, goal in _worlds():
        dist = nav_ref.field(ty, st, W, H, goal=goal)["dist"]
        moves = prior_ref.cell_moves(dist, W, H)
        assert moves[W * H] == 0
        d = dist.astype(np.int64)
        assert np.array_equal(moves[:W * H] == 0, d == U)              # empty exactly on unreachable cells
        assert np.array_equal(moves[:W * H] == stay, d == 0)           # the stay bit alone, exactly on sources
        assert not (moves[:W * H][d != 0] & stay).any()
        for y in range(H):
            for x in range(W):
                want = nav_ref.field(ty, st, W, H, goal=goal, agent=(x, y))["agent_action"] if W * H <= 81 else None
                got = prior_ref.lowest_action(moves[y * W + x])
                if want is None:                                       # large worlds: the tie-break restated, not a BFS per cell
                    want = -1
                    if d[y * W + x] == 0:
                        want = 6
                    elif d[y * W + x] != U:
                        for k, dx, dy in nav_ref.MOVES:
                            if 0 <= x + dx < W and 0 <= y + dy < H and d[(y + dy) * W + x + dx] == d[y * W + x] - 1:
                                want = k
                                break
                assert got == want, (W, H, x, y)
                seen.add(bin(int(moves[y * W + x])).count("1"))
    assert seen >= {0, 1, 2, 3}                                        # cells with several optimal moves exist


def test_policy_mask_mapping(front_end):
    moves = np.arange(32, dtype=np.uint8)
    for A in (2, 3, 4, 5, 7):
        got = front_end.to_policy_mask(torch.from_numpy(moves), A).numpy()
        assert np.array_equal(got, prior_ref.to_policy_mask(moves, A))
        assert got.max() < (1 << A)
    assert np.array_equal(prior_ref.to_policy_mask(moves, 5), moves)   # five actions: the identity
    assert prior_ref.to_policy_mask(np.array([0x10, 0x1F], np.uint8), 3).tolist() == [4, 7]


def _rows(B, A, seed):
    rs = np.random.RandomState(seed)
    p = rs.gamma(0.8, size=(B, A)) + 1e-3
    p *= (rs.uniform(0.3, 3.0, B) / p.sum(1))[:, None]
    return rs, p


@pytest.mark.parametrize("A", [2, 3, 4, 5, 7])
def test_single_bit_masks_are_the_categorical_log_prob(A):
    B, coef = 200, 0.37
    rs, p = _rows(B, A, A)
    a = rs.randint(0, A, B)
    R = prior_ref.loss64(p, (1 << a).astype(np.uint8), coef)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    want = -torch.distributions.Categorical(probs=tp).log_prob(torch.tensor(a)).mean() * coef
    gp, = torch.autograd.grad(want, tp)
    assert abs(R["loss"] - float(want)) <= 1e-12 * abs(float(want))
    np.testing.assert_allclose(R["gp"], gp.numpy(), rtol=1e-9, atol=1e-15)
    assert R["labelled"] == B


@pytest.mark.parametrize("A", [2, 3, 4, 5, 7])
def test_gradient_formula_equals_autograd(A):
    B, coef = 300, 1.7
    rs, p = _rows(B, A, 10 + A)
    mask = rs.randint(0, 256, B).astype(np.uint8)                      # bits >= A set and ignored, empty masks included
    p[:20] = np.where(prior_ref.mask_bits(mask[:20], A) > 0, 0.0, p[:20])          # m = 0 where the mask is not full
    p[20:40] = np.where(prior_ref.mask_bits(mask[20:40], A) > 0, p[20:40], 0.0)    # m = 1 where it is not empty
    p[:40] += (p[:40].sum(1) == 0)[:, None]                            # no all-zero row
    for n_valid in (B, 117, 1):
        R = prior_ref.loss64(p, mask, coef, n_valid)
        g = prior_ref.grad_formula(p, mask, coef, n_valid)
        np.testing.assert_allclose(g, R["gp"], rtol=1e-9, atol=1e-15)
        assert not g[n_valid:].any() and not g[~R["lab"]].any()
    R = prior_ref.loss64(p, mask, coef)
    clamped = R["lab"] & ((R["m"] < prior_ref.EPS32) | (R["m"] > 1 - prior_ref.EPS32))
    assert clamped.any() and not R["gp"][clamped].any() and R["gp"][R["lab"] & ~clamped].any()
    none = prior_ref.loss64(p, np.zeros(B, np.uint8), coef)
    assert none["loss"] == 0.0 and none["labelled"] == 0 and not none["gp"].any()


def test_headers_state_the_contract():
    nav_h = open(os.path.join(ROOT, "include", "minigrid_nav.h")).read()
    ppo_h = open(os.path.join(ROOT, "include", "twoarmy_ppo.h")).read()
    assert int(re.search(r"#define MG_NAV_MOVE_STAY_BIT\s+(\d+)", nav_h).group(1)) == 4 and prior_ref.STAY == 1 << 4
    assert "lowest set bit" in nav_h and "4 * ceil(B/256)" in ppo_h
