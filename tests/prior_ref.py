"""Host restatement of the shortest-path prior (include/minigrid_nav.h: mg_nav_optimal_moves; include/twoarmy_ppo.h:
ppo_prior_loss_fwd_bwd): the SET of optimal moves of a cell from a nav_ref BFS field, in plain loops, and the set-valued
imitation loss in float64 autograd with the fp32 clamp eps of the kernel's (float32) Categorical.  Test-side only."""
import numpy as np
import torch

import nav_ref
import visit_ref

UNREACHABLE = nav_ref.UNREACHABLE
STAY = 0x10
EPS32 = float(np.finfo(np.float32).eps)


def cell_moves(dist, W, H):
    """dist uint16[H*W] of one world -> uint8[H*W + 1]: bit k set iff the neighbour in direction k (nav_ref.MOVES: left,
    right, up, down) lies inside the world and is one move nearer; STAY alone on a source; 0 on an unreachable cell and
    in the extra slot H*W ("no cell")."""
    d = np.asarray(dist).astype(np.int64).reshape(H, W)
    out = np.zeros(H * W + 1, np.uint8)
    for y in range(H):
        for x in range(W):
            if d[y, x] == 0:
                out[y * W + x] = STAY
            elif d[y, x] != UNREACHABLE:
                for k, dx, dy in nav_ref.MOVES:
                    nx, ny = x + dx, y + dy
                    if 0 <= nx < W and 0 <= ny < H and d[ny, nx] == d[y, x] - 1:
                        out[y * W + x] |= 1 << k
    return out


def lowest_action(mask):
    """The action the lowest set bit stands for: 0..3, STAY -> 6, empty -> -1 (mg_nav_field's agent_action)."""
    mask = int(mask)
    if mask == 0:
        return -1
    k = (mask & -mask).bit_length() - 1
    return 6 if k == 4 else k


def acting_positions(pos, age=None, init_pos=None):
    """pos float32[T, N, 2], age int[T, N] -> the acting positions: init_pos where age <= 0."""
    pos = np.asarray(pos, np.float32)
    if age is None:
        return pos
    return np.where((np.asarray(age) <= 0)[..., None], np.asarray(init_pos, np.float32), pos).astype(np.float32)


def optimal_moves(dist, pos, W, H, age=None, init_pos=None, tables=None):
    """dist uint16[N, H*W], pos float32[T, N, 2] -> (moves uint8[T, N], acting_dist uint16[T, N]).  tables: the
    cell_moves() of every env, where the caller keeps them."""
    p = acting_positions(pos, age, init_pos)
    T, N = p.shape[:2]
    tables = [cell_moves(dist[n], W, H) for n in range(N)] if tables is None else tables
    ext = np.concatenate([np.asarray(dist), np.full((N, 1), UNREACHABLE, np.uint16)], axis=1)
    moves, ad = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint16)
    for t in range(T):
        for n in range(N):
            c = visit_ref.cell_of(p[t, n, 0], p[t, n, 1], W, H)
            moves[t, n], ad[t, n] = tables[n][c], ext[n, c]
    return moves, ad


def to_policy_mask(moves, A):
    """Bits 0 .. min(4, A - 1) - 1 stay, the stay bit moves to bit A - 1."""
    m = np.asarray(moves).astype(np.int64)
    return ((m & ((1 << min(4, A - 1)) - 1)) | (((m >> 4) & 1) << (A - 1))).astype(np.uint8)


def mask_bits(mask, A):
    """uint8[B] -> float64[B, A] of 0 / 1; bits >= A are dropped."""
    return ((np.asarray(mask).astype(np.int64)[:, None] >> np.arange(A)) & 1).astype(np.float64)


def loss64(p, mask, coef, n_valid=None):
    """float64 autograd of coef * mean over the labelled rows of -log(clamp(m, eps32, 1 - eps32)), m = the mass of
    Categorical(probs=p) on the mask -> dict(loss, mass, labelled, agree, gp, l, m, q, S, lab, top)."""
    p = torch.tensor(np.asarray(p), dtype=torch.float64, requires_grad=True)
    B, A = p.shape
    n_valid = B if n_valid is None else n_valid
    bits = torch.tensor(mask_bits(mask, A))
    lab = (bits.sum(1) > 0) & (torch.arange(B) < n_valid)
    S = p.sum(-1, keepdim=True)
    q = p / S
    m = (q * bits).sum(-1)
    l = -torch.log(torch.clamp(m, EPS32, 1 - EPS32))
    n = int(lab.sum())
    top = q.argmax(1)                                        # ties: checked by the caller, who knows where they are
    if n == 0:
        z = np.zeros(B)
        return dict(loss=0.0, mass=0.0, labelled=0, agree=0, gp=np.zeros((B, A)), l=z, m=z, q=q.detach().numpy(),
                    S=S.detach().view(-1).numpy(), lab=lab.numpy(), top=top.numpy())
    loss = coef * l[lab].sum() / n
    gp, = torch.autograd.grad(loss, p)
    return dict(loss=float(loss.detach()), mass=float(m[lab].sum().detach() / n), labelled=n, agree=None, gp=gp.numpy(),
                l=l.detach().numpy(), m=m.detach().numpy(), q=q.detach().numpy(), S=S.detach().view(-1).numpy(),
                lab=lab.numpy(), top=top.numpy())


def grad_formula(p, mask, coef, n_valid=None):
    """The analytic gradient of the header: coef / n_lab * (1 - [j in mask] / m) / sum(p) inside the clamp, else 0."""
    p = np.asarray(p, np.float64)
    B, A = p.shape
    n_valid = B if n_valid is None else n_valid
    bits = mask_bits(mask, A)
    lab = (bits.sum(1) > 0) & (np.arange(B) < n_valid)
    S = p.sum(1)
    m = (p / S[:, None] * bits).sum(1)
    inside = lab & (m >= EPS32) & (m <= 1 - EPS32)
    g = np.zeros((B, A))
    n = int(lab.sum())
    if n:
        with np.errstate(divide="ignore", invalid="ignore"):
            full = coef / n * (1 - bits / m[:, None]) / S[:, None]
        g[inside] = full[inside]
    return g
