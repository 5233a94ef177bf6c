"""torch front end of the PPO HIP kernels (include/twoarmy_ppo.h).  No CPU fallback: every op
needs device tensors and the HIP library."""
import ctypes as C

import torch

from ._marshal import call as _call, constant as _constant, ptr as _p, query as _query

_CL = torch.channels_last


def _pf(t):
    """Pointer to t detached, contiguous and checked to be fp32 (a parameter or a view goes in as it is)."""
    return _p(t.detach().contiguous(), torch.float32)


def _step_outputs(out, want_steps, T, N, dtypes, device):
    """The per-step output pair of a scan: the caller's `out`, fresh [T,N] tensors, or (None, None)."""
    if out is None:
        return tuple(torch.empty((T, N), dtype=d, device=device) if want_steps else None for d in dtypes)
    assert out[0].shape == (T, N) and out[1].shape == (T, N)
    return out


def sample(probs, uniforms=None, seed=0, offset=0, offset_dev=None):
    """Categorical(probs).sample() + log_prob (reference soa/agent/PPO.py:86-88) -> (int32[B], float[B]).
    offset_dev: int64[1] device tensor added to the Philox row counter at run time (graph-captured launches)."""
    B, A = probs.shape
    action = torch.empty(B, dtype=torch.int32, device=probs.device)
    logp = torch.empty(B, dtype=torch.float32, device=probs.device)
    _call("ppo_sample_dev", probs, _p(probs, torch.float32), B, A, _p(uniforms, torch.float32), seed, offset,
          _p(offset_dev, torch.int64), _p(action), _p(logp))
    return action, logp


def gae(reward, value, next_value, done=None, gamma=0.99, lam=0.0, use_done_mask=False, want_ret=True):
    """Returns (adv, target, ret) [T,N].  lam=0, use_done_mask=False is the reference (PPO.py:113-114)."""
    T, N = reward.shape
    adv = torch.empty_like(reward)
    target = torch.empty_like(reward)
    ret = torch.empty_like(reward) if want_ret else None
    _call("ppo_gae", reward, _p(reward, torch.float32), _p(value, torch.float32), _p(next_value, torch.float32),
          _p(done, torch.uint8), gamma, lam, int(bool(use_done_mask)), T, N, _p(adv), _p(target), _p(ret))
    return adv, target, ret


def run_ends(t, n, goal, done, broken=None):
    """Where the runs of a flat record array end (ppo_run_ends, include/twoarmy_ppo.h) -> uint8[H]: 1 unless the record
    behind continues the run (not done, same env, next step, same goal).  t, n int32[H], goal f32[H,2], done u8[H], e.g.
    the records of her_relabel.  broken: an int32[1] device tensor that gets ADDED the number of records that are not
    done and still end a run (out of pattern)."""
    H = t.numel()
    assert n.shape == (H,) and goal.shape == (H, 2) and done.shape == (H,) and (broken is None or broken.shape == (1,))
    run_end = torch.empty(H, dtype=torch.uint8, device=t.device)
    _call("ppo_run_ends", t, _p(t, torch.int32), _p(n, torch.int32), _p(goal, torch.float32), _p(done, torch.uint8), H,
          _p(run_end), _p(broken, torch.int32))
    return run_end


def gae_runs(reward, value, next_value, done, run_end, gamma, lam, use_done_mask, want_ret=True):
    """gae() along a flat record array, cut at the run ends instead of scanned per column (ppo_gae_runs,
    include/twoarmy_ppo.h) -> (adv, target, ret), each [H].  done may be None without the done mask."""
    H = reward.numel()
    assert reward.shape == (H,) and value.shape == (H,) and next_value.shape == (H,) and run_end.shape == (H,)
    assert done is None or done.shape == (H,)
    adv = torch.empty_like(reward)
    target = torch.empty_like(reward)
    ret = torch.empty_like(reward) if want_ret else None
    ws = torch.empty(_query("ppo_gae_runs_workspace", H), dtype=torch.float32, device=reward.device)
    _call("ppo_gae_runs", reward, _p(reward, torch.float32), _p(value, torch.float32), _p(next_value, torch.float32),
          _p(done, torch.uint8), _p(run_end, torch.uint8), gamma, lam, int(bool(use_done_mask)), H, _p(adv), _p(target),
          _p(ret), _p(ws))
    return adv, target, ret


def adv_norm_(adv, eps=1e-8):
    ws = torch.empty(4096, dtype=torch.float64, device=adv.device)
    _call("ppo_adv_norm", adv, _p(adv, torch.float32), adv.numel(), eps, _p(ws))
    return adv


class _AttachGrad(torch.autograd.Function):
    """Scalar loss whose gradient w.r.t. `x` was already produced by the fused HIP kernel."""

    @staticmethod
    def forward(ctx, x, loss, grad):
        ctx.save_for_backward(grad)
        ctx.xshape = x.shape
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g).view(ctx.xshape), None, None


UPDATE_STATS_WORDS = 16
# stats[i] of ppo_loss_fwd_bwd_stats (include/twoarmy_ppo.h); 13..15 are reserved
UPDATE_STATS = dict(rows=0, entropy_sum=1, logr_sum=2, k3_sum=3, clipped=4, ratio_dev_max=5, t_sum=6, t_sq_sum=7, e_sum=8,
                    e_sq_sum=9, saturated=10, top_mass_sum=11, calls=12)
_stats_workspaces = {}


def _stats_workspace(device, B):
    """The partial sums of ppo_loss_fwd_bwd_stats for B rows on `device`, made once per (device, B) and kept: written
    before it is read by every call, so calls that share it must be ordered on one stream (an update's are)."""
    k = (torch.device(device), int(B))
    if k not in _stats_workspaces:
        _stats_workspaces[k] = torch.empty(_query("ppo_loss_stats_workspace", int(B)), dtype=torch.float64, device=device)
    return _stats_workspaces[k]


def ppo_losses(probs, value, action, old_logp, adv, target_v, clip=0.1, ent_coef=0.01, n_valid=None, stats=None):
    """(action_loss, value_loss) of the reference (PPO.py:124-133).  One fused forward+backward launch;
    the two losses are separate autograd nodes so `action_loss.backward(); value_loss.backward()` works
    exactly like in the reference.  n_valid < B: rows n_valid.. are padding of a fixed-shape minibatch.
    stats: a float64[16] device tensor (or a row of a larger one) that the call ADDS this minibatch's diagnostics to
    (ppo_loss_fwd_bwd_stats, include/twoarmy_ppo.h; read with update_stats_read); the losses and gradients are the same
    bits.  None: ppo_loss_fwd_bwd_masked, nothing else launched."""
    B, A = probs.shape
    n_valid = B if n_valid is None else int(n_valid)
    with torch.no_grad():
        probs_c = probs.detach().contiguous()
        value_c = value.detach().contiguous().view(-1)
        losses = torch.empty(2, dtype=torch.float32, device=probs.device)
        gp = torch.empty_like(probs_c)
        gv = torch.empty_like(value_c)
        ws = torch.empty(2 * ((B + 255) // 256), dtype=torch.float32, device=probs.device)
        args = [_p(probs_c, torch.float32), _p(action.contiguous(), torch.int32), _p(old_logp.contiguous().view(-1)),
                _p(adv.contiguous().view(-1)), _p(value_c), _p(target_v.contiguous().view(-1)), B, n_valid, A, float(clip),
                float(ent_coef), _p(losses), _p(gp), _p(gv), _p(ws)]
        if stats is None:
            _call("ppo_loss_fwd_bwd_masked", probs, *args)
        else:
            assert stats.shape == (UPDATE_STATS_WORDS,) and stats.device == probs.device
            _call("ppo_loss_fwd_bwd_stats", probs, *args, _p(stats, torch.float64),
                  _p(_stats_workspace(probs.device, B), torch.float64))
    return _AttachGrad.apply(probs, losses[0], gp), _AttachGrad.apply(value, losses[1], gv)


def update_stats_read(stats):
    """The accumulators of ppo_losses(..., stats=) as numbers: float64[..., 16] on any device -> a dict of Python floats
    (one row) or numpy arrays over the leading dimensions.  rows, calls: counts.  entropy, top_mass (mean of max_k q):
    means over the rows.  approx_kl = k3_sum / rows, the non-negative estimator mean((r - 1) - log r);
    approx_kl_k1 = -logr_sum / rows.  clip_frac: the share of rows outside the clip range; saturated_frac: of rows whose
    acted action sits on the Categorical's clamp.  ratio_dev_max = max |r - 1|.  explained_variance = 1 - Var(e) / Var(t),
    e = target - value, population variances from the raw moments (include/twoarmy_ppo.h on their precision).  Where
    rows == 0 every mean is NaN; where Var(t) == 0 explained_variance is NaN.  This is the one host read."""
    import numpy as np
    s = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    assert s.dtype == np.float64 and s.shape[-1] == UPDATE_STATS_WORDS
    g = {k: s[..., i] for k, i in UPDATE_STATS.items()}
    n = np.where(g["rows"] > 0, g["rows"], np.nan)                       # NaN rows: every mean below is NaN
    with np.errstate(all="ignore"):                                      # NaN in, NaN out: nothing to warn about
        var_t = np.maximum(g["t_sq_sum"] / n - (g["t_sum"] / n) ** 2, 0.0)
        var_e = np.maximum(g["e_sq_sum"] / n - (g["e_sum"] / n) ** 2, 0.0)
        out = dict(rows=g["rows"], calls=g["calls"], entropy=g["entropy_sum"] / n, approx_kl=g["k3_sum"] / n,
                   approx_kl_k1=-g["logr_sum"] / n, clip_frac=g["clipped"] / n, ratio_dev_max=g["ratio_dev_max"],
                   explained_variance=1.0 - var_e / np.where(var_t > 0, var_t, np.nan),
                   saturated_frac=g["saturated"] / n, top_mass=g["top_mass_sum"] / n)
    return {k: float(v) if s.ndim == 1 else np.array(v) for k, v in out.items()}


def prior_loss(probs, moves, coef, n_valid=None):
    """Set-valued imitation term of the shortest-path prior (ppo_prior_loss_fwd_bwd, include/twoarmy_ppo.h):
    coef * mean over the labelled rows of -log(mass of Categorical(probs) on the optimal actions).  moves uint8[B]: a mask
    over policy indices (minigrid_nav.to_policy_mask); rows from n_valid on are padding.  -> (loss, (out, counts)): loss is
    an autograd node on probs like ppo_losses' (so `(action_loss + loss).backward()` works); out f32[2] = (loss, mean
    mass on the optimal actions) and counts i32[2] = (labelled rows, rows whose arg-max is optimal) stay on the device."""
    B, A = probs.shape
    n_valid = B if n_valid is None else int(n_valid)
    assert moves.shape == (B,) and moves.device == probs.device
    with torch.no_grad():
        probs_c = probs.detach().contiguous()
        out = torch.empty(2, dtype=torch.float32, device=probs.device)
        counts = torch.empty(2, dtype=torch.int32, device=probs.device)
        gp = torch.empty_like(probs_c)
        ws = torch.empty(4 * ((B + 255) // 256), dtype=torch.float32, device=probs.device)
        _call("ppo_prior_loss_fwd_bwd", probs, _p(probs_c, torch.float32), _p(moves, torch.uint8), B, n_valid, A, float(coef),
              _p(out), _p(counts), _p(gp), _p(ws))
    return _AttachGrad.apply(probs, out[0], gp), (out, counts)


def gather_stack(frames, pos_frames, k_idx, n_idx, age, init_frame, init_pos):
    """frames [K,N,pitch>=289] (may be a [..., :289] view of a 292-pitched buffer) -> ([B,4,289], [B,4,2]).
    uint8 frames are matrix codes (TW_F_MATRIX_CODE) and are expanded to fp32 on the fly."""
    K, N = frames.shape[:2]
    pitch = frames.stride(1)
    assert frames.stride(2) == 1 and frames.stride(0) == N * pitch
    B = k_idx.numel()
    out = torch.empty((B, 4, 289), dtype=torch.float32, device=frames.device)
    pos_out = torch.empty((B, 4, 2), dtype=torch.float32, device=frames.device) if pos_frames is not None else None
    assert frames.dtype in (torch.float32, torch.uint8)
    _call("ppo_gather_stack" if frames.dtype == torch.float32 else "ppo_gather_stack_u8", frames,
          C.c_void_p(frames.data_ptr()), pitch, _p(pos_frames, torch.float32), N, _p(k_idx, torch.int32),
          _p(n_idx, torch.int32), _p(age, torch.int32), _p(init_frame, torch.float32), _p(init_pos, torch.float32), B,
          _p(out), _p(pos_out))
    return out, pos_out


def age_scan(terminated, truncated, age0):
    T, N = terminated.shape
    age = torch.empty((T + 1, N), dtype=torch.int32, device=terminated.device)
    _call("ppo_age_scan", terminated, _p(terminated, torch.uint8), _p(truncated, torch.uint8), _p(age0, torch.int32),
          T, N, _p(age))
    return age


def episode_scan(reward, terminated, truncated, carry_return, carry_length, want_steps=True, out=None):
    """Per-episode return and length carried across calls (ppo_episode_scan, include/twoarmy_ppo.h; reference
    soa/train_ppo.py:124 `ep_reward += reward`).  reward / terminated / truncated [T,N]; carry_return f64[N] and
    carry_length i32[N] are updated IN PLACE.  Returns (ep_return f64[T,N], ep_length i32[T,N]), or (None, None) with
    want_steps=False; out = (ep_return, ep_length) reuses buffers of the caller."""
    T, N = reward.shape
    assert terminated.shape == (T, N) and truncated.shape == (T, N) and carry_return.shape == (N,) and carry_length.shape == (N,)
    ep_return, ep_length = _step_outputs(out, want_steps, T, N, (torch.float64, torch.int32), reward.device)
    _call("ppo_episode_scan", reward, _p(reward, torch.float32), _p(terminated, torch.uint8), _p(truncated, torch.uint8),
          T, N, _p(carry_return, torch.float64), _p(carry_length, torch.int32), _p(ep_return, torch.float64),
          _p(ep_length, torch.int32))
    return ep_return, ep_length


def episode_summary_workspace(T, N):
    return _query("ppo_episode_summary_workspace", int(T), int(N))


def episode_summary(ep_return, ep_length, terminated, truncated, reward, action=None, n_actions=5, keep=0.99, gain=0.01,
                    score=None, summary=None, action_hist=None, reward_hist=None, workspace=None):
    """What the episodes that finished in this rollout looked like, plus the reference's running score folded over them
    in row-major order (ppo_episode_summary, include/twoarmy_ppo.h; soa/train_ppo.py:140).  score f64[1] is updated IN
    PLACE (None: no fold).  Returns (summary f64[8], action_hist i64[A], reward_hist i64[6]); no host synchronisation."""
    T, N = reward.shape
    dev = reward.device
    summary = torch.empty(8, dtype=torch.float64, device=dev) if summary is None else summary
    action_hist = torch.empty(n_actions, dtype=torch.int64, device=dev) if action_hist is None else action_hist
    reward_hist = torch.empty(6, dtype=torch.int64, device=dev) if reward_hist is None else reward_hist
    need = episode_summary_workspace(T, N)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=dev)
    assert workspace.numel() >= need and summary.numel() == 8 and action_hist.numel() == n_actions and reward_hist.numel() == 6
    assert ep_return.shape == (T, N) and ep_length.shape == (T, N) and (action is None or action.shape == (T, N))
    _call("ppo_episode_summary", reward, _p(ep_return, torch.float64), _p(ep_length, torch.int32), _p(terminated, torch.uint8),
          _p(truncated, torch.uint8), _p(reward, torch.float32), _p(action, torch.int32), int(n_actions), T, N, float(keep),
          float(gain), _p(score, torch.float64), _p(summary, torch.float64), _p(action_hist, torch.int64),
          _p(reward_hist, torch.int64), _p(workspace, torch.float64))
    return summary, action_hist, reward_hist


def visit_carry_words(width, height, N):
    return _query("ppo_visit_carry_words", int(width), int(height), int(N))


def visit_scan(pos, terminated, truncated, carry, width=17, height=17, want_steps=True, out=None):
    """Which cells the running episode of every env has stood on, carried across calls (ppo_visit_scan,
    include/twoarmy_ppo.h).  pos f32[T,N,2] (y, x) after each step; terminated / truncated u8[T,N]; carry
    u32[visit_carry_words(width, height, N)] is updated IN PLACE (all-zero: nothing seen).  Returns (first_visit u8[T,N],
    ep_cells i32[T,N]), or (None, None) with want_steps=False; out = (first_visit, ep_cells) reuses the caller's buffers."""
    T, N = terminated.shape
    assert pos.shape == (T, N, 2) and truncated.shape == (T, N) and carry.numel() == visit_carry_words(width, height, N)
    first_visit, ep_cells = _step_outputs(out, want_steps, T, N, (torch.uint8, torch.int32), pos.device)
    _call("ppo_visit_scan", pos, _p(pos, torch.float32), _p(terminated, torch.uint8), _p(truncated, torch.uint8), T, N,
          int(width), int(height), _p(carry, torch.int32), _p(first_visit, torch.uint8), _p(ep_cells, torch.int32))
    return first_visit, ep_cells


def visit_hist(pos, counts, width=17, height=17, mask=None, t_idx=None, n_idx=None):
    """counts i64[width*height + 1] += visits per cell, last entry = positions outside the grid (ppo_visit_hist,
    include/twoarmy_ppo.h; the reference's values_matrix[y, x] += 1, soa/img_proccess/heatmap.py:63).  pos f32[T,N,2];
    dense over every (t, n) whose mask u8[T,N] is non-zero (mask None: all), or, with t_idx / n_idx i32[B], over those
    records (hindsight records; out-of-range ones count as outside).  Returns counts; no host synchronisation."""
    T, N = pos.shape[:2]
    assert pos.shape == (T, N, 2) and counts.numel() == int(width) * int(height) + 1
    assert (t_idx is None) == (n_idx is None) and (mask is None or mask.shape == (T, N))
    B = 0 if t_idx is None else t_idx.numel()
    assert t_idx is None or n_idx.numel() == B
    if t_idx is not None and B == 0:
        return counts
    _call("ppo_visit_hist", pos, _p(pos, torch.float32), T, N, _p(mask, torch.uint8), _p(t_idx, torch.int32),
          _p(n_idx, torch.int32), B, int(width), int(height), _p(counts, torch.int64))
    return counts


BONUS_KINDS = {"state": 1, "action": 2}
BONUS_SCOPES = {"env": 0, "shared": 1}


def bonus_table_words(kind, scope, width=17, height=17, n_actions=7, N=1):
    """32-bit words of one count table (kind "state" / "action", scope "env" / "shared"; ppo_bonus_table_words)."""
    return _query("ppo_bonus_table_words", BONUS_KINDS[kind], BONUS_SCOPES[scope], int(width), int(height),
                  int(n_actions), int(N))


def bonus_workspace_bytes(kind_mask, scope, T, width=17, height=17, n_actions=7):
    return _query("ppo_bonus_workspace_bytes", int(kind_mask), BONUS_SCOPES[scope], int(T), int(width), int(height),
                  int(n_actions))


def _bonus_args(pos, per_step, tables, dir, dir_ptr, words):
    """What the two bonus scans share -> (T, N, kind mask, (dir pointer, stride_t, stride_n)): pos is [T,N,2], every
    tensor of per_step [T,N] or None, and the (state, action) tables given have words(kind, N) words."""
    T, N = pos.shape[:2]
    assert pos.shape == (T, N, 2)
    for t in per_step:
        assert t is None or t.shape == (T, N)
    mask = (1 if tables[0] is not None else 0) | (2 if tables[1] is not None else 0)
    dp, st, sn = None, 0, 0
    if dir is not None:
        assert dir.shape in ((T, N), (N,))
        dp, st, sn = _p(dir, torch.int32), (N if dir.dim() == 2 else 0), 1
    elif dir_ptr is not None:
        dp, st, sn = C.c_void_p(int(dir_ptr[0])), int(dir_ptr[1]), int(dir_ptr[2])
    for kind, tab in zip(("state", "action"), tables):
        assert tab is None or tab.numel() == words(kind, N)
    return T, N, mask, (dp, st, sn)


def bonus_scan(pos, action, reward, state_table=None, action_table=None, scope="env", scale=1.0, width=17, height=17,
               n_actions=7, keep=None, dir=None, dir_ptr=None, bonus_state=None, bonus_action=None, reward_out=None,
               workspace=None):
    """Count-based exploration bonuses of one rollout (ppo_bonus_scan, include/twoarmy_ppo.h; the reference's StateBonus /
    ActionBonus, gym_minigrid/wrappers.py:34-102).  pos f32[T,N,2] (y, x) after each step, action i32[T,N], reward
    f32[T,N]; the tables given (i32 words, bonus_table_words; updated IN PLACE) select the kinds.  dir: i32[T,N] or [N]
    (one direction per env), or dir_ptr = (address, stride_t, stride_n) of directions that live elsewhere on the device
    (the engine's records); neither: direction 0.  keep u8[T,N]: steps whose reward passes through unshaped.  Writes the
    outputs given (bonus_state / bonus_action / reward_out f32[T,N]; reward_out may be reward); no host synchronisation."""
    T, N, mask, dirs = _bonus_args(pos, (action, reward, keep, bonus_state, bonus_action, reward_out),
                                   (state_table, action_table), dir, dir_ptr,
                                   lambda kind, N: bonus_table_words(kind, scope, width, height, n_actions, N))
    if BONUS_SCOPES[scope] == 1:
        need = bonus_workspace_bytes(mask, scope, T, width, height, n_actions)
        if workspace is None:
            workspace = torch.empty(max(1, need // 4), dtype=torch.int32, device=pos.device)
        assert workspace.numel() * 4 >= need
    _call("ppo_bonus_scan", pos, _p(pos, torch.float32), _p(action, torch.int32), *dirs, _p(reward, torch.float32),
          _p(keep, torch.uint8), T, N, int(width), int(height), int(n_actions), mask, BONUS_SCOPES[scope], float(scale),
          _p(state_table, torch.int32), _p(action_table, torch.int32), _p(bonus_state, torch.float32),
          _p(bonus_action, torch.float32), _p(reward_out, torch.float32), _p(workspace, torch.int32))
    return reward_out


BONUS_FORMS = {"sqrt": 0, "first": 1}
BONUS_EPISODE_COUNT_BITS = 24                           # include/twoarmy_ppo.h: word = stamp << 24 | count


def bonus_episode_words(kind, width=17, height=17, n_actions=7, N=1):
    """32-bit words of one episodic count table (kind "state" / "action"; ppo_bonus_episode_words): N spans of K stamped
    counts and N generation words."""
    return _query("ppo_bonus_episode_words", BONUS_KINDS[kind], int(width), int(height), int(n_actions), int(N))


def bonus_episode_counts(table, N):
    """The running episodes' counts of an episodic table as int64[N, K] on the table's device: a word counts while its
    stamp is its env's generation (include/twoarmy_ppo.h)."""
    K = table.numel() // N - 1
    w = table[:N * K].view(N, K).to(torch.int64) & 0xFFFFFFFF
    gen = table[N * K:].to(torch.int64).view(N, 1)
    return torch.where((w >> BONUS_EPISODE_COUNT_BITS) == gen, w & ((1 << BONUS_EPISODE_COUNT_BITS) - 1), 0)


def bonus_scan_episode(pos, action, reward, terminated, truncated, state_table=None, action_table=None, form="sqrt",
                       scale=1.0, width=17, height=17, n_actions=7, keep=None, dir=None, dir_ptr=None, bonus_state=None,
                       bonus_action=None, reward_out=None):
    """Count bonuses whose counts clear at each episode end (ppo_bonus_scan_episode, include/twoarmy_ppo.h): bonus_scan's
    env scope, cut where terminated | truncated u8[T,N] is set; the done step is counted and paid before the clear.  form
    "sqrt": scale / sqrt(count), "first": scale at a key's first visit of the episode, else 0.  The tables given (i32 words,
    bonus_episode_words; updated IN PLACE, they carry the running episodes between calls) select the kinds.  Every other
    argument as in bonus_scan; no host synchronisation."""
    T, N, mask, dirs = _bonus_args(pos, (action, reward, keep, terminated, truncated, bonus_state, bonus_action, reward_out),
                                   (state_table, action_table), dir, dir_ptr,
                                   lambda kind, N: bonus_episode_words(kind, width, height, n_actions, N))
    _call("ppo_bonus_scan_episode", pos, _p(pos, torch.float32), _p(action, torch.int32), *dirs,
          _p(reward, torch.float32), _p(keep, torch.uint8), _p(terminated, torch.uint8), _p(truncated, torch.uint8), T, N,
          int(width), int(height), int(n_actions), mask, BONUS_FORMS[form], float(scale), _p(state_table, torch.int32),
          _p(action_table, torch.int32), _p(bonus_state, torch.float32), _p(bonus_action, torch.float32),
          _p(reward_out, torch.float32))
    return reward_out


REWARD_NORM_STATS = dict(count=0, mean=1, m2=2, scale=3)     # stats[i] of ppo_reward_norm_update (include/twoarmy_ppo.h)


def reward_norm_workspace(N):
    return _query("ppo_reward_norm_workspace", int(N))


def reward_norm_update(reward, terminated, truncated, gamma, ret_carry, stats, workspace=None):
    """Advance the running moments of the discounted return by one rollout (ppo_reward_norm_update,
    include/twoarmy_ppo.h): reward f32[T,N], terminated / truncated u8[T,N]; ret_carry f64[N] (the envs' running returns)
    and stats f64[4] = (count, mean, M2, scale) are updated IN PLACE, all-zero = nothing seen.  workspace: f64 of
    reward_norm_workspace(N) elements, made here if None.  Returns stats; two launches, no host synchronisation.  An empty
    rollout (T == 0) returns at once and changes nothing."""
    T, N = reward.shape
    assert terminated.shape == (T, N) and truncated.shape == (T, N) and ret_carry.shape == (N,) and stats.shape == (4,)
    need = reward_norm_workspace(N)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=reward.device)
    assert workspace.numel() >= need
    if T == 0:
        return stats
    _call("ppo_reward_norm_update", reward, _p(reward, torch.float32), _p(terminated, torch.uint8), _p(truncated, torch.uint8),
          T, N, float(gamma), _p(ret_carry, torch.float64), _p(stats, torch.float64), _p(workspace, torch.float64))
    return stats


def reward_norm_apply(reward, stats, clip=0.0, out=None):
    """reward * (float)stats[3], clamped to [-clip, clip] where clip is positive and finite (ppo_reward_norm_apply):
    reward f32 of any shape, contiguous; the scale is read from stats f64[4] on the device when the launch runs.  out: a
    tensor of reward's shape, reward itself for in place, or None for a new one.  Returns out; one launch, no host
    synchronisation."""
    assert stats.shape == (4,)
    out = torch.empty_like(reward) if out is None else out
    assert out.shape == reward.shape
    if reward.numel():
        _call("ppo_reward_norm_apply", reward, _p(reward, torch.float32), reward.numel(), _p(stats, torch.float64),
              float(clip), _p(out, torch.float32))
    return out


def reward_norm_read(stats):
    """stats f64[4] as numbers: {"count", "mean", "var" = M2 / count, "std", "scale" = what reward_norm_apply multiplies
    by}; with nothing seen var and std are 0.0 and scale is 1.0.  One device-to-host copy."""
    count, mean, m2, scale = stats.detach().cpu().tolist()
    var = m2 / count if count else 0.0
    return dict(count=count, mean=mean, var=var, std=var ** 0.5, scale=scale if count else 1.0)


def her_relabel(pos, terminated, truncated, age0, reward, choices=None, seed=0, env_id0=0, step0=0, max_goals=4, skip=0):
    """Hindsight relabelling of a time-major rollout (ppo_her_relabel_window, include/twoarmy_ppo.h; reference
    Buffer_gridworld.her_func, soa/env_buffer.py:101-143; skip = 4: pre_her_func / pre_f_her_func on the 9-frame window
    records, :145-280).  Returns a dict of relabelled index records
    {t int32[H], n int32[H], goal f32[H,2], reward f32[H], done u8[H]} and the per-env counts."""
    T, N = terminated.shape
    dev = pos.device
    assert pos.shape == (T, N, 2) and pos.is_contiguous() and reward.shape == (T, N)
    if choices is not None:
        assert choices.shape == (T, N, 4) and choices.dtype == torch.int32 and choices.is_contiguous()
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    args = [_p(pos, torch.float32), _p(terminated.contiguous(), torch.uint8), _p(truncated.contiguous(), torch.uint8),
            _p(age0.contiguous(), torch.int32), _p(reward.contiguous(), torch.float32), _p(choices), int(seed),
            int(env_id0), int(step0), T, N, int(max_goals), int(skip)]
    _call("ppo_her_relabel_window", pos, *args, None, _p(counts), None, None, None, None, None)
    incl = torch.cumsum(counts.long(), 0)
    H = int(incl[-1])                                   # the one host sync: the record count sizes the outputs
    offsets = (incl - counts.long()).contiguous()
    out = dict(t=torch.empty(H, dtype=torch.int32, device=dev), n=torch.empty(H, dtype=torch.int32, device=dev),
               goal=torch.empty((H, 2), dtype=torch.float32, device=dev),
               reward=torch.empty(H, dtype=torch.float32, device=dev), done=torch.empty(H, dtype=torch.uint8, device=dev),
               counts=counts)
    if H:
        _call("ppo_her_relabel_window", pos, *args, _p(offsets), _p(counts), _p(out["t"]), _p(out["n"]), _p(out["goal"]),
              _p(out["reward"]), _p(out["done"]))
    return out


HER_RULES = {"late": 0, "key16": 1, "table": 2}          # PPO_HER_LATE / _KEY16 / _TABLE of include/twoarmy_ppo.h


def her_select(pos, terminated, truncated, age0, rule, key16=None, table=None, width=17, height=17, seed=0, env_id0=0,
               step0=0, max_goals=4, skip=0, choices=None, stats=None):
    """Which first visits of every episode become hindsight goals, by rule (ppo_her_select, include/twoarmy_ppo.h): the
    `choices` i32[T,N,4] that her_relabel takes.  rule "late" (or 0): the latest first visits; "key16" (1): the smallest
    key16 u16[T,N] (minigrid_nav.lookup's distances: nearest the goal); "table" (2): the smallest
    table i64[width*height + 1] entry of the candidate's cell (the lifetime visit counts: the rarest cells).  Ties fall by a
    Philox word of (seed, env_id0 + n, step0 + t1, rank).  Only the rows of handled episodes are written; a `choices` made
    here starts as -1 everywhere.  stats i64[6] is ADDED {episodes, candidates, picks, records the picks will emit, sum
    of the picked keys, picks with an unreachable key}; made (zero) here if None.  Returns (choices, stats); no host
    synchronisation.  An empty rollout (T == 0) returns at once: its tensors have no address to pass, so the entry is
    not called and none of its argument rules is applied to the other arguments."""
    T, N = terminated.shape
    dev = pos.device
    rule = HER_RULES.get(rule, rule)
    assert pos.shape == (T, N, 2) and truncated.shape == (T, N) and age0.shape == (N,)
    assert key16 is None or (key16.shape == (T, N) and key16.element_size() == 2)
    assert table is None or table.numel() == int(width) * int(height) + 1
    if choices is None:
        choices = torch.full((T, N, 4), -1, dtype=torch.int32, device=dev)
    if stats is None:
        stats = torch.zeros(6, dtype=torch.int64, device=dev)
    assert choices.shape == (T, N, 4) and stats.shape == (6,)
    if T == 0:
        return choices, stats
    _call("ppo_her_select", pos, _p(pos, torch.float32), _p(terminated, torch.uint8), _p(truncated, torch.uint8),
          _p(age0, torch.int32), T, N, int(max_goals), int(skip), int(rule), _p(key16), _p(table, torch.int64), int(width),
          int(height), int(seed), int(env_id0), int(step0), _p(choices, torch.int32), _p(stats, torch.int64))
    return choices, stats


class _ConvBiasReLU(torch.autograd.Function):
    """relu(conv2d(x, w) + b) on channels-last fp32 tensors: the conv (and its two backward GEMMs) in MIOpen, bias +
    ReLU and ReLU-backward + bias-gradient as ONE pass each (ppo_bias_relu_nhwc / ppo_relu_bwd_bias_grad_nhwc) instead
    of the add / clamp / threshold_backward / sum passes PyTorch runs around a Conv2d + ReLU pair."""

    @staticmethod
    def forward(ctx, x, w, b, stride):
        y = torch.ops.aten.convolution(x, w, None, list(stride), [0, 0], [1, 1], False, [0, 0], 1)
        assert y.is_contiguous(memory_format=torch.channels_last), "conv epilogue kernels need channels-last activations"
        B, Cc, H, W = y.shape
        _call("ppo_bias_relu_nhwc", y, _p(y, None, _CL), _pf(b), B * H * W, Cc)
        ctx.save_for_backward(x, w, y)
        ctx.stride = list(stride)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        gy = gy.contiguous(memory_format=torch.channels_last)
        B, Cc, H, W = y.shape
        npix = B * H * W
        blocks = _query("ppo_relu_bwd_bias_grad_nhwc_blocks", npix, Cc)
        g = torch.empty_like(y)                                   # channels-last like y
        partial = torch.empty((blocks, Cc), dtype=torch.float32, device=y.device)
        _call("ppo_relu_bwd_bias_grad_nhwc", y, _p(gy, None, _CL), _p(y, None, _CL), _p(g, None, _CL), _p(partial), npix, Cc)
        gx, gw, _ = torch.ops.aten.convolution_backward(g, x, w, None, ctx.stride, [0, 0], [1, 1], False, [0, 0], 1,
                                                        [bool(ctx.needs_input_grad[0]), True, False])
        return gx, gw, partial.sum(0), None


def conv_bias_relu(x, weight, bias, stride):
    """relu(conv2d(x, weight, bias, stride)) for channels-last fp32 device tensors (see _ConvBiasReLU)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    return _ConvBiasReLU.apply(x, weight, bias, tuple(stride))


def fold_conv1_weights(w):
    """Conv2d(F -> 64, k4, s2) weights [64, F, 4, 4] applied to a nearest-x4 upsampled image == parity-dependent 2x2-tap
    weights on the source image (include/twoarmy_ppo.h): -> float[2][2][2][2][F][64], contiguous."""
    O, F = w.shape[0], w.shape[1]
    w = w.detach().reshape(O, F, 4, 4).float()
    z = torch.zeros_like(w[:, :, 0:1, :])
    rows = torch.stack([torch.cat([w.sum(2, keepdim=True), z], 2),                       # parity 0: all four rows on tap 0
                        torch.cat([w[:, :, 0:2].sum(2, keepdim=True), w[:, :, 2:4].sum(2, keepdim=True)], 2)], 0)  # [py][O][F][ty][4]
    zc = torch.zeros_like(rows[..., 0:1])
    cols = torch.stack([torch.cat([rows.sum(-1, keepdim=True), zc], -1),
                        torch.cat([rows[..., 0:2].sum(-1, keepdim=True), rows[..., 2:4].sum(-1, keepdim=True)], -1)], 1)
    # cols: [py][px][O][F][ty][tx] -> [py][px][ty][tx][F][O]
    return cols.permute(0, 1, 4, 5, 3, 2).contiguous()


@torch.no_grad()
def conv1_up4_bias_relu_infer(frames, weight, bias):
    """Inference-only fused layer for any supported (F, C_out) (include/twoarmy_ppo.h: ppo_conv1_up4_bias_relu_c):
    frames [B, F, 289] -> relu(conv2d(upsample_x4(frames), weight, bias, stride 2)) as a channels-last [B, C, 33, 33]."""
    B, F, _ = frames.shape
    Cout = weight.shape[0]
    y = torch.empty((B, Cout, 33, 33), dtype=torch.float32, device=frames.device, memory_format=torch.channels_last)
    wf = fold_conv1_weights(weight)
    _call("ppo_conv1_up4_bias_relu_c", y, _pf(frames), B, F, Cout, _p(wf), _pf(bias), _p(y, None, _CL))
    return y


class _Conv1Up4(torch.autograd.Function):
    """relu(conv1(upsample_x4(frames)) + b) in one kernel (ppo_conv1_up4_bias_relu); backward in one kernel too
    (ppo_conv1_up4_bwd: ReLU mask, folded weight gradient and bias gradient from one read of gy and y; the frames
    themselves need no gradient)."""

    @staticmethod
    def forward(ctx, frames, w, b, wf):
        B, F, _ = frames.shape
        y = torch.empty((B, w.shape[0], 33, 33), dtype=torch.float32, device=frames.device,
                        memory_format=torch.channels_last)
        if wf is None:
            wf = fold_conv1_weights(w)
        fr = frames.contiguous()
        _call("ppo_conv1_up4_bias_relu", y, _p(fr, torch.float32), B, F, _p(wf), _pf(b), _p(y, None, _CL))
        ctx.save_for_backward(fr, w, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        fr, w, y = ctx.saved_tensors
        gy = gy.contiguous(memory_format=torch.channels_last)
        B, F = fr.shape[0], fr.shape[1]
        groups = _query("ppo_conv1_up4_bwd_groups", B)
        gw_part = torch.empty((groups, 2, 2, 2, 2, F, 64), dtype=torch.float32, device=y.device)
        gb_part = torch.empty((groups, 4, 64), dtype=torch.float32, device=y.device)
        _call("ppo_conv1_up4_bwd", y, _p(fr, torch.float32), B, F, _p(gy, None, _CL), _p(y, None, _CL), _p(gw_part),
              _p(gb_part))
        return None, unfold_conv1_grad(gw_part.sum(0)).to(w.dtype), gb_part.sum((0, 1)), None


def unfold_conv1_grad(gwf):
    """Gradient w.r.t. the folded weights [py][px][ty][tx][F][O] -> gradient w.r.t. W[O][F][4][4] (transpose of
    fold_conv1_weights: row r of W feeds tap 0 of parity 0 and tap r // 2 of parity 1; columns alike)."""
    ty = _constant("conv1_tap_of_row", [[0, 0, 0, 0], [0, 0, 1, 1]], torch.int64, gwf.device)   # [py][r]
    out = None
    for py in (0, 1):
        for px in (0, 1):
            g = gwf[py, px][ty[py]][:, ty[px]]                                        # [r][k][F][O]
            out = g if out is None else out + g
    return out.permute(3, 2, 0, 1).contiguous()


def conv1_up4_bias_relu(frames, weight, bias, folded=None):
    """frames [B, F, 289] (F = 4 or 8) -> relu(conv2d(upsample_x4(frames), weight, bias, stride 2)), channels-last.
    folded: fold_conv1_weights(weight) computed by the caller (e.g. once per rollout), or None."""
    assert frames.is_cuda and frames.dtype == torch.float32 and weight.shape[2:] == (4, 4) and weight.shape[0] == 64
    return _Conv1Up4.apply(frames, weight, bias, folded)


def fold_decoder_tail(w3):
    """ConvTranspose2d(16 -> 1, k4, s2) followed by AvgPool2d(4) (Net_Decoder, all_net.py:100-137) as ONE 3x3 / stride-2 /
    pad-1 convolution: pooled cell y averages image rows 4y..4y+3, row 4y+d of the transposed conv reads input row 2y+u
    through tap row d-2u, so input row 2y-1 contributes tap rows {2,3}, row 2y all four, row 2y+1 rows {0,1}."""
    m = _constant("decoder_tail_rows", [[0., 0., 1., 1.], [1., 1., 1., 1.], [1., 1., 0., 0.]], w3.dtype, w3.device)
    return torch.einsum("ur,crs,vs->cuv", m, w3[:, 0], m).mul_(1.0 / 16.0).contiguous()


def decoder_frames(z, w1, b1, w2, b2, w3, b3):
    """Net_Decoder (inference) in one fused pass per frame: z [n,64,4,4] -> predicted 17x17 frames [n,289]
    (ppo_decoder_frames, include/twoarmy_ppo.h); weights in ConvTranspose2d layout."""
    assert z.dim() == 4 and tuple(z.shape[1:]) == (64, 4, 4) and z.dtype == torch.float32
    z = z.contiguous()
    n = z.shape[0]
    out = torch.empty((n, 289), dtype=torch.float32, device=z.device)
    if n:
        _call("ppo_decoder_frames", z, _p(z), n, _pf(w1), _pf(b1), _pf(w2), _pf(b2), _p(fold_decoder_tail(w3.detach())), 0.0,
              _p(out))
        out += b3.detach().view(1, 1)            # the bias as a device-side add: no host synchronisation in the rollout
    return out


def lstm_cell_(gates, c, gates_b=None, bias=None):
    """LSTM cell pointwise ops in one pass (ppo_lstm_cell): pre-activations gates [B,4H] (i, f, g, o; None: zero) + gates_b (optional
    [B,4H] view whose rows may be strided, e.g. xin[:, t] of a [B,T,4H] tensor) + bias (optional [4H]); c [B,H] is
    updated IN PLACE; returns the new hidden state h [B,H]."""
    B, H = c.shape
    H4 = 4 * H
    assert c.dtype == torch.float32 and (gates is not None or gates_b is not None)
    assert gates is None or (gates.shape == (B, H4) and gates.dtype == torch.float32)
    pb, ldb = None, 0
    if gates_b is not None:
        assert gates_b.shape == (B, H4) and gates_b.stride(1) == 1 and gates_b.dtype == torch.float32 and gates_b.is_cuda
        pb, ldb = C.c_void_p(gates_b.data_ptr()), gates_b.stride(0) if B > 1 else H4
    h = torch.empty_like(c)
    _call("ppo_lstm_cell", c, _p(gates), pb, ldb, _p(bias), _p(c), _p(h), B, H)
    return h
