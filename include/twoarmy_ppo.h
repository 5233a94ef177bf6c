/*
 * twoarmy_ppo.h -- C ABI of the PPO math kernels (libtwoarmy_hip.so, <package>/csrc/ppo_kernels.hip).
 *
 * Replaces, for batches of B samples resident in HBM, the torch ops of the reference's
 * soa/agent/PPO.py (paths relative to the reference root):
 *   select_action  PPO.py:73-92    Categorical(probs).sample() / log_prob        -> ppo_sample
 *   update         PPO.py:112-115  target_v = r + g*V(s'), adv = target_v - V(s) -> ppo_gae (lambda = 0, no mask)
 *                  PPO.py:115      (commented) adv = (adv - mean) / (std + 1e-8) -> ppo_adv_norm
 *                  PPO.py:124-133  ratio-clip surrogate + entropy, SmoothL1      -> ppo_loss_fwd_bwd
 *   train_ppo.py:116-123  5-frame stack shift + store                            -> ppo_gather_stack
 *   train_ppo.py:124,136-141  ep_reward += reward; running_score fold per episode  -> ppo_episode_scan / _summary
 * GAE(gamma, lambda) with done masks has no reference counterpart: it collapses to the
 * reference formula at lambda = 0, use_done_mask = 0 and is otherwise pinned against a float64 statement of the
 * formula (tests/test_ppo_kernels_edges_gpu.py).
 *
 * Conventions as in twoarmy.h: device pointers, caller-owned, `stream` = hipStream_t as void*,
 * asynchronous, 0 = ok / negative = TW_E_*.  All tensors fp32 unless noted; time-major [T][N].
 */
#ifndef TWOARMY_PPO_H
#define TWOARMY_PPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* torch.distributions.Categorical(probs=p) semantics: q = p / sum(p); logits = log(clamp(q, eps, 1-eps)),
 * eps = FLT_EPSILON; log_prob(a) = logits[a].  Sampling is inverse-CDF on q with a supplied uniform
 * u in [0,1): a = min{k : cumsum(q)[k] > u}, cumsum in fp32; where the rounded cumsum ends at or below u,
 * a = the last k with q[k] > 0 (never an action of probability 0).  uniforms == NULL -> u from
 * Philox4x32-10(key = seed, counter = (lo32(row + offset), hi32(row + offset), 0, 'TWOS')),
 * u = (word0 >> 8) * 2^-24.
 *   probs float[B][A] (A in {2, 3, 4, 5, 7}; any other A returns TW_E_ARG), uniforms float[B]|NULL,
 *   action int32[B], logp float[B] */
int ppo_sample(const float *probs, int B, int A, const float *uniforms, uint64_t seed, uint64_t offset,
               int32_t *action, float *logp, void *stream);
/* The same with the Philox row counter = row + offset + *offset_dev: a launch recorded in a HIP graph (the whole
 * rollout of VecPPOTrainer is one) takes its position in the stream from device memory at replay time. */
int ppo_sample_dev(const float *probs, int B, int A, const float *uniforms, uint64_t seed, uint64_t offset,
                   const uint64_t *offset_dev, int32_t *action, float *logp, void *stream);

/* delta_t = r_t + gamma * nv_t * cut_t - v_t;  A_t = delta_t + gamma*lambda*cut_t*A_{t+1} (A_T = 0);
 * cut_t = use_done_mask ? 1 - done_t : 1.  Where gamma*lambda*cut_t = 0 (lambda = 0, or a done) A_t = delta_t
 * exactly: a non-finite delta of a later step does not reach it.  Outputs (each nullable): adv = A, target = r + gamma*nv*cut
 * (the reference's target_v), ret = A + v.  Segmented reverse scan: one wavefront scans 64 time steps of
 * one env with 6 shuffle steps over affine maps; [T][N] tiles are transposed through LDS.
 *   reward, value, next_value float[T][N]; done uint8[T][N] (nullable when !use_done_mask) */
int ppo_gae(const float *reward, const float *value, const float *next_value, const uint8_t *done,
            float gamma, float lambda, int use_done_mask, int T, int N, float *adv, float *target, float *ret,
            void *stream);

/* GAE(lambda) for the hindsight records of ppo_her_relabel, which form no [T][N] tile: a flat array of H records that
 * come as RUNS of consecutive steps of one env under one goal, each run ending with its own done record.
 *
 * ppo_run_ends: where the runs end, one launch.  For j < H - 1
 *   link_j = done_j == 0 && n_{j+1} == n_j && t_{j+1} == t_j + 1 && goal_{j+1}[0] == goal_j[0] && goal_{j+1}[1] == goal_j[1]
 * (float compares: a NaN never links, -0.0 links with +0.0), link_{H-1} = 0 and nothing at index H is read;
 * run_end_j = !link_j.  `broken` int32[1] | NULL, in/out, gets ADDED the number of j with done_j == 0 && !link_j: the
 * records that break the run pattern (external `choices`, a permuted array).  An integer atomic per wavefront: exact.
 *   t, n int32[H]; goal float[H][2]; done uint8[H]; run_end uint8[H]
 * TW_E_ARG, and nothing is launched: NULL t, n, goal, done or run_end; H <= 0 or H >= 2^40.
 *
 * ppo_gae_runs: ppo_gae's formula and rounding sequence along the array, cut at the run ends:
 *   cut_j = (use_done_mask && done_j) ? 0 : 1;   tv_j = r_j + (gamma * nv_j) * cut_j;   delta_j = tv_j - v_j
 *   c_j = (run_end_j || j == H - 1) ? 0 : gamma * lambda * cut_j;   A_j = c_j != 0 ? fma(c_j, A_{j+1}, delta_j) : delta_j
 *   adv = A, target = tv, ret = A + v   (each nullable)
 * The run ends cut the scan, not the done flags: without the done mask (the reference, PPO.py:113) a done record keeps
 * its bootstrap gamma * nv, and a record that breaks the pattern is a run of its own with A = delta.  Where c_j = 0,
 * A_j is delta_j exactly: a non-finite delta never leaves its run.  With lambda = 0, or every run_end set, adv, target
 * and ret are bit for bit what ppo_gae gives on the same arrays as [1][H].
 * Runs may have any length and start anywhere.  The scan is a tree, not a walk: a workgroup takes 2048 consecutive
 * records, its four wavefronts 8 chunks of 64 each (6 shuffle steps over affine maps, as ppo_gae, then a fold over the
 * chunks and the wavefronts), and writes its composite map to `workspace`; the composites are scanned the same way
 * (2048 per workgroup, a level more for every factor of 2048 in H), and an apply pass per level hands every workgroup
 * the value that enters it from behind.  Launches: 1 for H <= 2048, 3 up to 2048^2, 5 up to 2048^3, 7 beyond; the
 * serial depth is 8 chunks + 4 wavefronts per level, whatever H.  Every combine keeps the c != 0 guard.
 * `workspace`: ppo_gae_runs_workspace(H) floats = 2 * (n_1 + n_2 + ...) with n_0 = H, n_{l+1} = ceil(n_l / 2048) for as
 * long as n_l > 2048, at least 2; every entry is written before it is read (no initialisation needed).  All launches go
 * to `stream`, nothing is allocated or read back between them: the call may be captured into a graph and replayed.
 * Deterministic: two calls on equal inputs give equal bits.
 *   reward, value, next_value float[H]; done uint8[H] (nullable when !use_done_mask); run_end uint8[H]
 * TW_E_ARG, and nothing is launched: NULL reward, value, next_value, run_end or workspace; use_done_mask with a NULL
 * done; H <= 0 or H >= 2^40.  ppo_gae_runs_workspace: host only; TW_E_ARG for H <= 0 or H >= 2^40. */
int ppo_run_ends(const int32_t *t, const int32_t *n, const float *goal, const uint8_t *done, int64_t H,
                 uint8_t *run_end, int32_t *broken, void *stream);
int ppo_gae_runs(const float *reward, const float *value, const float *next_value, const uint8_t *done,
                 const uint8_t *run_end, float gamma, float lambda, int use_done_mask, int64_t H,
                 float *adv, float *target, float *ret, float *workspace, void *stream);
int ppo_gae_runs_workspace(int64_t H);

/* adv <- (adv - mean) / (std + eps), std unbiased (torch.Tensor.std default).  workspace: >= 4096 doubles. */
int ppo_adv_norm(float *adv, int64_t n, float eps, double *workspace, void *stream);

/* Fused forward + backward of the reference losses (PPO.py:124-133) for one minibatch:
 *   action_loss = mean(-min(ratio*adv, clamp(ratio, 1-clip, 1+clip)*adv) - ent_coef * H),
 *   value_loss  = smooth_l1(value, target_v)  (beta = 1, mean)
 * with ratio = exp(logp(a) - old_logp) and Categorical(probs) semantics as in ppo_sample.
 * Writes losses[0] = action_loss, losses[1] = value_loss, d(action_loss)/d(probs) float[B][A] and
 * d(value_loss)/d(value) float[B].  Deterministic (fixed-order two-stage reduction).
 * workspace: >= 2 * ceil(B/256) floats. */
int ppo_loss_fwd_bwd(const float *probs, const int32_t *action, const float *old_logp, const float *adv,
                     const float *value, const float *target_v, int B, int A, float clip, float ent_coef,
                     float *losses, float *grad_probs, float *grad_value, float *workspace, void *stream);
/* The same for a minibatch padded to a fixed shape: rows n_valid .. B-1 are padding (they carry no loss and get zero
 * gradients; the means run over the n_valid real rows).  Keeps every conv launch of an update at ONE batch size:
 * MIOpen searches kernels per shape, and an odd last minibatch costs a new multi-second search. */
int ppo_loss_fwd_bwd_masked(const float *probs, const int32_t *action, const float *old_logp, const float *adv,
                            const float *value, const float *target_v, int B, int n_valid, int A, float clip,
                            float ent_coef, float *losses, float *grad_probs, float *grad_value, float *workspace,
                            void *stream);

/* ppo_loss_fwd_bwd_masked plus the diagnostics of the update, accumulated on the device: losses, grad_probs and grad_value
 * are bit for bit what ppo_loss_fwd_bwd_masked writes for the same arguments (one row routine, two instantiations), and
 * `stats` double[16], in/out, gets ADDED what the rows b < n_valid contribute.  All-zero = nothing accumulated, so one fill
 * clears it.  With the row's float32 values as the loss computes them -- q = p / sum(p), l = log(clamp(q, eps, 1 - eps)),
 * H = -sum q l, lr = l[a] - old_logp[b] (the float32 difference that feeds expf), ratio = expf(lr), lo = 1 - clip,
 * hi = 1 + clip -- a row adds:
 *    0 rows            1
 *    1 entropy_sum     (double)H
 *    2 logr_sum        (double)lr                                   -logr_sum / rows = the k1 estimate of KL(old || new)
 *    3 k3_sum          ((double)ratio - 1.0) - (double)lr           the non-negative estimator (r - 1) - log r, evaluated in
 *                                                                   double from the two float32 values: exact near r = 1
 *    4 clipped         1 where ratio < lo or ratio > hi             the loss's own float compares
 *    5 ratio_dev_max   stats[5] = fmax(stats[5], |(double)ratio - 1|)          a maximum, not a sum
 *    6 t_sum           (double)target_v
 *    7 t_sq_sum        (double)target_v squared in double
 *    8 e_sum           e = target_v - value as ONE float32 subtraction, then (double)e
 *    9 e_sq_sum        (double)e squared in double
 *   10 saturated       1 where q[a] of the acted action lies outside [eps, 1 - eps]: the clamp is active there and the
 *                      row sends no policy gradient
 *   11 top_mass_sum    (double)max_k q[k]
 *   12 calls           1 per call
 *   13..15 reserved    never read or written
 * t_sq_sum and e_sq_sum are RAW second moments: a variance taken from them and the sums loses digits where |mean| is far
 * larger than the standard deviation.  Twoarmy's targets are of order 1.
 * Deterministic, no floating-point atomics: per-workgroup partials (12 doubles each: the 64 lanes of a wavefront as a
 * binary tree in lane order, then the four wavefronts in order) go into `stats_workspace`,
 * ppo_loss_stats_workspace(B) = 12 * ceil(B / 256) doubles, every one written before it is read (no initialisation needed);
 * the final pass, one wavefront, gives lane l the partials l, l + 64, ... folded in that order and combines the lanes by the
 * same tree.  Two calls from equal `stats` on equal inputs give equal bits.  Rows n_valid .. B-1 add exactly nothing (+0.0
 * and 0), and which partials meet where does not depend on the number of workgroups: a padded call and the unpadded call on
 * the first n_valid rows leave equal bits in all of `stats`.  Cutting one batch into several calls changes the sums by double
 * rounding only; counts and the maximum do not change.
 * Two launches, both on `stream`, nothing allocated or read back between them: the call may be captured into a graph and
 * replayed.
 * TW_E_ARG, and nothing is launched: the rules of ppo_loss_fwd_bwd_masked (every pointer set, B > 0, A == 5,
 * 0 < n_valid <= B), NULL stats or stats_workspace, either of the two off 8-byte alignment.
 * ppo_loss_stats_workspace: host only; TW_E_ARG for B <= 0. */
int ppo_loss_fwd_bwd_stats(const float *probs, const int32_t *action, const float *old_logp, const float *adv,
                           const float *value, const float *target_v, int B, int n_valid, int A, float clip,
                           float ent_coef, float *losses, float *grad_probs, float *grad_value, float *workspace,
                           double *stats, double *stats_workspace, void *stream);
int ppo_loss_stats_workspace(int B);

/* Shortest-path prior: a set-valued imitation term on the actor, forward + backward for one minibatch.  No reference
 * counterpart; the labels are the optimal-move sets of mg_nav_optimal_moves (minigrid_nav.h).
 *   probs float[B][A] (A as for ppo_sample); moves uint8[B]: a mask over POLICY indices, bit a set iff action a is optimal
 *   (bits >= A are ignored).  A row is labelled iff it lies below n_valid (0 <= n_valid <= B; the rest is padding) and its
 *   masked bits are non-zero.
 * With Categorical(probs) semantics as in ppo_sample: q = p / sum(p); m = sum of q[a] over the mask in ascending a;
 *   l = -log(clamp(m, eps, 1 - eps)), eps = FLT_EPSILON -- a single-bit mask gives -Categorical(probs=p).log_prob(a).
 *   out[0] = coef * mean of l over the labelled rows; out[1] = mean of m over them
 *   counts[0] = labelled rows; counts[1] = labelled rows whose arg-max of q (lowest index on ties) lies in the mask
 *   grad_probs[b][j] = coef / counts[0] * (1 - [j in mask] / m) / sum(p) = d out[0] / d probs[b][j] inside the clamp,
 *   eps <= m <= 1 - eps (torch.clamp passes the gradient on the closed interval); 0 where the clamp is active and for
 *   unlabelled and padding rows.  Whether the upper clamp is active is decided on the mass OUTSIDE the mask (< eps),
 *   which is accurate where m itself is within rounding of 1: a mask that holds all the mass, a full mask included,
 *   always has l = -log(1 - eps) and gradient 0.
 * With no labelled row out = {0, 0}, counts = {0, 0} and every gradient is 0.
 * Deterministic: per-workgroup partial sums (a 256-wide tree) in `workspace`, added in block order; two calls give equal
 * bits.  workspace: >= 4 * ceil(B/256) floats.  Two launches. */
int ppo_prior_loss_fwd_bwd(const float *probs, const uint8_t *moves, int B, int n_valid, int A, float coef, float *out,
                           int32_t *counts, float *grad_probs, float *workspace, void *stream);

/* Policy-input assembly from time-major frames (replaces the 5-deep np.delete/np.append stacks of
 * train_ppo.py:116-121 and the [0:4] / [1:5] slices of PPO.py:113-114,124).  For sample b with newest
 * frame index k_b (row of `frames`), env n_b and age_b = number of env steps taken in the current
 * episode when that newest frame was produced:
 *   out[b][j] = (age_b - (3 - j) <= 0) ? init_frame : frames[k_b - (3 - j)][n_b]      j = 0..3
 * i.e. the four newest frames, never crossing the episode start: older slots repeat the reset frame
 * exactly as np.tile does in Env_transact.reset (env_buffer.py:420-423).  Same for the (y,x) stacks.
 *   frames float[K][N][frame_pitch]; pos_frames float[K][N][2]; k_idx, n_idx, age int32[B];
 *   init_frame float[289]; init_pos float[2]; out float[B][4][289]; pos_out float[B][4][2] (nullable) */
int ppo_gather_stack(const float *frames, int frame_pitch, const float *pos_frames, int N,
                     const int32_t *k_idx, const int32_t *n_idx, const int32_t *age, const float *init_frame,
                     const float *init_pos, int B, float *out, float *pos_out, void *stream);

/* Same, for frames stored as uint8 codes (tw_step/tw_rollout with TW_F_MATRIX_CODE, twoarmy.h): frame_pitch in
 * bytes, each code expanded to its matrix_env value {0: 0.9, 1: -0.9, 2: -0.5, 3: 0.3}; init_frame stays float[289].
 * BASELINE config 5 ("reduced-precision frames"): the stored rollout is 4x smaller and the expansion is exact.
 * Only the codes 0..3 are defined; what a larger byte expands to is unspecified. */
int ppo_gather_stack_u8(const uint8_t *frames, int frame_pitch, const float *pos_frames, int N,
                        const int32_t *k_idx, const int32_t *n_idx, const int32_t *age, const float *init_frame,
                        const float *init_pos, int B, float *out, float *pos_out, void *stream);

/* Episode age before every step of a rollout: age[0][n] = age0[n]; age[t+1][n] = done[t][n] ? 0 : age[t][n]+1.
 *   done uint8[T][N] (terminated | truncated), age0 int32[N], age int32[T+1][N] */
int ppo_age_scan(const uint8_t *terminated, const uint8_t *truncated, const int32_t *age0, int T, int N,
                 int32_t *age, void *stream);

/* Episode accounting on the device (replaces the host bookkeeping of train_ppo.py:124 `ep_reward += reward` and
 * :136-141, where the finished episode's return is folded into running_score and reset).
 *
 * ppo_episode_scan: for every env n, in step order: acc = carry_return[n], len = carry_length[n]; for t = 0 .. T-1:
 *   acc += (double)reward[t][n]; len += 1; ep_return[t][n] = acc; ep_length[t][n] = len; and where
 *   terminated | truncated is set, acc = 0, len = 0 after the write.  The carries are written back at the end, so at
 * a done step ep_return / ep_length are the return and length of the episode that ends there, wherever it began.
 * The additions are float64, one per step, in step order: the result does not depend on how a rollout is cut into
 * launches (T = 128 once and 128 launches of T = 1 give the same bits).
 * After a done step the scan restarts from exactly +0.0 and 0: a NaN or inf reward never leaves its episode or its env.
 * Only the first T * N elements of ep_return / ep_length and the N elements of the carries are written.
 *   reward float[T][N]; terminated, truncated uint8[T][N]; carry_return double[N] in/out; carry_length int32[N] in/out;
 *   ep_return double[T][N] | NULL; ep_length int32[T][N] | NULL
 * Alignment: reward 4 bytes; carry_length, ep_length 4 bytes; carry_return, ep_return 8 bytes (NULL counts as aligned).
 * TW_E_ARG, and nothing is launched: NULL reward, terminated, truncated, carry_return or carry_length; T <= 0 or N <= 0;
 * T * N >= 2^40; a pointer off the alignment above. */
int ppo_episode_scan(const float *reward, const uint8_t *terminated, const uint8_t *truncated, int T, int N,
                     double *carry_return, int32_t *carry_length, double *ep_return, int32_t *ep_length, void *stream);

/* What the episodes that finished in one rollout looked like, and the reference's running score over them:
 *   summary double[8] = {episodes, successes (terminated), truncated-only, sum of returns, min return, max return,
 *       sum of lengths, max length} over the done steps; with no finished episode min = +inf, max = -inf, the rest 0
 *   action_hist int64[A] | NULL: steps with action == a (A in {2, 3, 4, 5, 7} as for ppo_sample; action == NULL: zeros)
 *   reward_hist int64[6]: steps whose reward equals, as float32, -0.01, -0.1, -0.9, 0.2, 0.9; last bucket: anything else
 *   score double[1] in/out | NULL: for every done step in row-major (t, then n) order
 *       score = score * keep + ep_return[t][n] * gain        (train_ppo.py:140 with keep = 0.99, gain = 0.01;
 *       the episodes of one time step are taken in ascending env index); not written when no episode finished.
 * Deterministic: a grid fixed by (T, N), per-block partial results in `workspace`
 * (ppo_episode_summary_workspace(T, N) doubles), one ordered final pass.  Counts, min and max are exact; the sums
 * and the fold are evaluated as a tree in row-major order, so they agree with a sequential evaluation up to rounding.
 * The grid, with M = T * N: nblocks = min(ceil(M / 2048), 256) workgroups of 256 threads; workgroup b takes the
 * per_block = ceil(M / nblocks) elements from b * per_block on, thread i of it the per_thread = ceil(per_block / 256)
 * elements from b * per_block + i * per_thread on, both cut at the end of the block's share and at M (a run may be empty).
 * The tree: a thread folds its run in order; the 64 lanes of a wavefront are combined as a binary tree (6 levels), the 4
 * wavefronts of a workgroup one after the other; the final pass gives each of 64 lanes per_lane = ceil(nblocks / 64)
 * consecutive partials, folded one after the other, and combines the lanes by the same 6-level tree.  The workspace
 * holds ppo_episode_summary_workspace(T, N) = 24 * nblocks doubles, every one written before it is read: it needs no
 * initialisation.  ep_return / ep_length are read at done steps only.
 * An action outside [0, A) is counted in no bin, and action_hist[k] for k >= A is not written.  A non-finite return leaves
 * episodes, successes, truncated, length_sum, max_length and both histograms as they would be without it; min and max ignore
 * a NaN (fmin / fmax); return_sum and score take the non-finite value.
 *   ep_return double[T][N], ep_length int32[T][N] (ppo_episode_scan's outputs); action int32[T][N] | NULL
 * Alignment: reward 4 bytes; ep_length, action 4 bytes; ep_return, score, summary, workspace 8 bytes; action_hist,
 * reward_hist 8 bytes (NULL counts as aligned).
 * TW_E_ARG, and nothing is launched: NULL ep_return, ep_length, terminated, truncated, reward, summary, reward_hist or
 * workspace; T <= 0 or N <= 0; T * N >= 2^40; an A outside {2, 3, 4, 5, 7}; a pointer off the alignment above.
 * ppo_episode_summary_workspace: host only; TW_E_ARG for T <= 0, N <= 0 or T * N >= 2^40. */
int ppo_episode_summary(const double *ep_return, const int32_t *ep_length, const uint8_t *terminated,
                        const uint8_t *truncated, const float *reward, const int32_t *action, int A, int T, int N,
                        double keep, double gain, double *score, double *summary, int64_t *action_hist,
                        int64_t *reward_hist, double *workspace, void *stream);
int ppo_episode_summary_workspace(int T, int N);

/* Visited cells on the device (<package>/csrc/visitation.hip): the visit-count matrix the reference builds for its heatmap
 * after every PPO.update (soa/agent/PPO.py:161 -> soa/img_proccess/heatmap.py:58-81, `values_matrix[y, x] += 1` over
 * the buffer's after-step positions) and the set of distinct cells an episode has stood on (the goal candidates of
 * her_func, soa/env_buffer.py:138).  The pictures are not drawn.
 *
 * Cell of a position (y, x) = (pos[..][0], pos[..][1]): valid iff 0 <= y < height and 0 <= x < width as float comparisons
 * (NaN and +-inf fail, -0.0 passes as 0); cell = (int)y * width + (int)x, row-major like values_matrix[y][x].  Every
 * invalid position is counted in ONE extra bin, other = width * height, and never addresses anything else.
 * 1 <= width, height <= 32.  pos and counts are 8-byte aligned.
 *
 * ppo_visit_scan: for every env n, in step order: seen = the set in `carry`; for t = 0 .. T-1:
 *   first_visit[t][n] = cell valid and not in seen; seen += cell; ep_cells[t][n] = |seen|; and where
 *   terminated | truncated is set, seen = {} after the write.  The carry is written back at the end.
 * The set is empty at an episode's first step (the reset cell is not in it: the reference's buffer holds after-step
 * positions only), so within one episode the steps with first_visit = 1 are the indices np.unique(episode_p, axis=0,
 * return_index=True) returns, and at a done step ep_cells is the episode's coverage wherever it began.  The result
 * does not depend on how the steps are cut into launches.
 *   pos float[T][N][2]; terminated, truncated uint8[T][N]; first_visit uint8[T][N] | NULL; ep_cells int32[T][N] | NULL
 *   carry uint32[ppo_visit_carry_words(width, height, N)] in/out, opaque, all-zero = nothing seen (bit c & 31 of word
 *   [c >> 5][n] = cell c of env n: word-major over envs, so a wavefront's accesses are contiguous).
 *
 * ppo_visit_hist: counts int64[width * height + 1] += number of records per cell (last entry: other).
 *   dense   (t_idx == NULL): every (t, n) with mask == NULL || mask[t][n] != 0;  mask uint8[T][N]
 *   indexed (t_idx, n_idx int32[B]): the records (t_idx[b], n_idx[b]), e.g. the hindsight records of ppo_her_relabel;
 *           a record outside [0, T) x [0, N) counts as other; B == 0 adds nothing.
 * Integer adds only: exact, whatever the scheduling.
 *
 * Both return TW_E_ARG and launch nothing on NULL pos / counts / carry / terminated / truncated, width or height outside
 * 1..32, negative T, N or B, one of t_idx / n_idx without the other; T * N == 0 returns 0 and launches nothing. */
int ppo_visit_scan(const float *pos, const uint8_t *terminated, const uint8_t *truncated, int T, int N, int width,
                   int height, uint32_t *carry, uint8_t *first_visit, int32_t *ep_cells, void *stream);
int ppo_visit_carry_words(int width, int height, int N);
int ppo_visit_hist(const float *pos, int T, int N, const uint8_t *mask, const int32_t *t_idx, const int32_t *n_idx, int B,
                   int width, int height, int64_t *counts, void *stream);

/* Count-based exploration bonuses on the device (<package>/csrc/exploration_bonus.hip): the reference's StateBonus and
 * ActionBonus wrappers (gym_minigrid/wrappers.py:69-102 and :34-66), `reward += 1 / math.sqrt(count)` with a count per
 * agent_pos / per (agent_pos, agent_dir, action) that outlives reset().
 *
 * Keys.  state (kind 1): the cell of the after-step position exactly as ppo_visit_scan takes it (same device function);
 * K = width * height + 1.  action (kind 2): (cell * 4 + dir) * n_actions + action with dir in 0..3 and action in
 * [0, n_actions), 1 <= n_actions <= 8; K = width * height * 4 * n_actions + 1.  A step with an invalid cell, dir or
 * action counts in the table's LAST slot (`other`), takes its bonus from that slot's count and addresses nothing else.
 *
 * Scopes.  env (0): one table per env = N independent copies of the wrapper; for every env in step order
 * c = ++count[n][key].  shared (1): one table for all envs, a time step being simultaneous:
 * c(t, n) = carry[key] + #{(t', n') : t' <= t, key(t', n') = key}, so all envs on one key in row t get the same bonus,
 * which already includes the whole row; at N = 1 this is the env scope.  Counts are never cleared by an episode end
 * (ppo_bonus_scan_episode below clears them).  In
 * both scopes the result does not depend on how the steps are cut into launches.
 *
 * Arithmetic, IEEE double, one rounding per operation: b = scale * (1.0 / sqrt((double)c)); bonus_*[t][n] = (float)b;
 * reward_out[t][n] = (float)(((double)reward[t][n] + b_state) + b_action)  (ActionBonus(StateBonus(env)); a kind that is
 * off contributes 0.0), except where keep[t][n] != 0: there the counts still advance and reward_out = reward (the
 * reference's Env_transact.step overwrites the reward of a terminated step above the wrappers, env_buffer.py:448-450).
 *
 * Tables, opaque except that all-zero = nothing counted; ppo_bonus_table_words(kind, scope, ...) 32-bit words each,
 * 8-byte aligned:
 *   env     uint32[N][K], env-major: an env's K counts are contiguous (1.2 KB state / 32 KB action for Twoarmy: 133 MB of
 *           action counts at 4096 envs), because the wavefront that owns the env gathers and stores within that one span
 *   shared  int64[K]
 * so count of (cell, dir, action) = table[(n *) K + key] as laid out above; the last entry of a (per-env) table is other.
 * env scope: one wavefront per env, the keys of up to 256 steps in LDS, a step's count = carried count + its rank among
 * the earlier equal keys of the chunk + 1, the chunk's last occurrence of a key stores the new count; no atomics.  An
 * env's column of the time-major pos / action / reward is read with stride N (adjacent envs share the cache lines).
 * shared scope: a histogram per row in `workspace` (uint32[T][K] per kind, ppo_bonus_workspace_bytes; 4 MB for Twoarmy's
 * action keys at T = 128), an inclusive scan over t per key that also updates the table, then a gather pass.
 *
 *   pos float[T][N][2] (8-byte aligned); action int32[T][N] (kind 2 only); dir int32, element (t, n) at
 *   dir[t * dir_stride_t + n * dir_stride_n] (NULL: direction 0; stride_t = 0: one value per env, e.g. the engine's records);
 *   reward float[T][N] | NULL (needed for reward_out); keep uint8[T][N] | NULL; kind_mask 1 state, 2 action, 3 both;
 *   bonus_state, bonus_action, reward_out float[T][N], each | NULL; reward_out may alias reward.
 * TW_E_ARG and nothing launched: NULL or misaligned pos, a missing table / action / workspace that the kinds and the scope
 * need, reward_out without reward, width or height outside 1..32, n_actions outside 1..8, kind_mask outside 1..3, scope
 * outside 0..1, negative T, N or dir strides, T * N >= 2^31.  T * N == 0 returns 0 and launches nothing. */
int ppo_bonus_table_words(int kind, int scope, int width, int height, int n_actions, int N);
int64_t ppo_bonus_workspace_bytes(int kind_mask, int scope, int T, int width, int height, int n_actions);
int ppo_bonus_scan(const float *pos, const int32_t *action, const int32_t *dir, long dir_stride_t, long dir_stride_n,
                   const float *reward, const uint8_t *keep, int T, int N, int width, int height, int n_actions,
                   int kind_mask, int scope, double scale, void *state_table, void *action_table, float *bonus_state,
                   float *bonus_action, float *reward_out, void *workspace, void *stream);

/* Episodic count bonuses: the env scope of ppo_bonus_scan with counts that clear at each episode end (the per-episode
 * counts of RIDE / NovelD / AGAC on MiniGrid).  Keys, K, the `other` slot, dir addressing, keep, the aliasing of
 * reward_out, kind_mask and the forming of bonus_* and reward_out are ppo_bonus_scan's.
 *
 * Rule.  For every env in step order, c = ++count[n][key] for each kind that is on, and the bonus of step t comes from c;
 * then, if terminated[t][n] | truncated[t][n], every count of env n becomes 0.  The done step itself is counted and paid
 * before the clear, the first step of the next episode counts from 0, and the position an env is reset to is no visit.
 *   form 0: b = scale * (1.0 / sqrt((double)c))     form 1, first visit: b = (c == 1) ? scale : 0.0
 * IEEE double, one rounding per operation.  The result does not depend on how the steps are cut into launches, a cut
 * directly behind a done step included, and neither do the bits of the tables.
 *
 * Tables carry the running episodes' counts between calls; all-zero = nothing counted.  One table per kind,
 * ppo_bonus_episode_words(kind, ...) = N * (K + 1) 32-bit words, 8-byte aligned:
 *   uint32 word[N][K]   env-major like the env scope;  word = stamp << 24 | count  (BONUS_EPISODE_COUNT_BITS = 24)
 *   uint32 gen[N]       the generation of env n's running episode, 0..255, behind the N spans
 * count of (n, key) = (word[n][key] >> 24 == gen[n]) ? word[n][key] & 0xFFFFFF : 0; a word with another stamp is left over
 * from an earlier episode and counts as 0.  An episode end is gen[n] += 1 and touches no count: filling an env's span
 * instead would write K words per end (32 KB of action counts for Twoarmy).  After generation 255 comes 0, and that one
 * end in 256 does fill env n's K words with zeros, so a stamp is never met again by a word older than the fill and the
 * wrap is exact.  Each table has its own gen[]; a call advances those of the kinds that are on.  A count stays at
 * 2^24 - 1 once it gets there (16.7 million steps onto one key within one episode); below that it is exact.
 * One wavefront per env, the keys of up to 256 steps in LDS, no atomics: a step's count = the carried count if no done
 * lies earlier in the chunk, else 0, + its rank among the earlier equal keys since the chunk's last earlier done + 1; the
 * chunk's last occurrence of a key stores its count under the stamp of its own episode.
 *
 *   terminated, truncated uint8[T][N]; every other argument, `stream` included, as in ppo_bonus_scan.
 * TW_E_ARG and nothing launched: everything ppo_bonus_scan refuses in the env scope, NULL terminated or truncated, form
 * outside 0..1.  T * N == 0 returns 0 and launches nothing.  ppo_bonus_episode_words returns -1 by the rules of
 * ppo_bonus_table_words. */
#define BONUS_EPISODE_COUNT_BITS 24
int ppo_bonus_episode_words(int kind, int width, int height, int n_actions, int N);
int ppo_bonus_scan_episode(const float *pos, const int32_t *action, const int32_t *dir, long dir_stride_t, long dir_stride_n,
                           const float *reward, const uint8_t *keep, const uint8_t *terminated, const uint8_t *truncated,
                           int T, int N, int width, int height, int n_actions, int kind_mask, int form, double scale,
                           void *state_table, void *action_table, float *bonus_state, float *bonus_action,
                           float *reward_out, void *stream);

/* Reward normalisation (<package>/csrc/reward_norm.hip): rewards divided by the running standard deviation of the
 * discounted return, gym's NormalizeReward / the baselines' VecNormalize for N envs at once.  No reference counterpart;
 * pinned bit for bit against the float64 restatement of the formulas below (tests/reward_norm_ref.py).
 *
 * stats double[4], in/out: {count, mean, M2, scale} of every return seen so far; variance = M2 / count.  All-zero = nothing
 * seen, so one fill clears it.  ret_carry double[N], in/out: the running return of every env, 0 at an episode's start.
 *
 * ppo_reward_norm_update, two launches.  All arithmetic is IEEE float64 with ONE rounding per operation; no product is
 * fused into a sum.
 * Scan: for every env n, G = ret_carry[n], (k, mean, M2) = (0, 0, 0), and for t = 0 .. T-1 in order
 *   p = gamma * G;  G = p + (double)reward[t][n]
 *   k = k + 1;  d = G - mean;  q = d / k;  mean = mean + q;  e = G - mean;  f = d * e;  M2 = M2 + f          (Welford)
 *   then, where terminated[t][n] | truncated[t][n] is set, G = 0: the done step's return is counted, then cleared (the
 *   order of gym's wrapper).
 * ret_carry[n] = G at the end; the env's triple goes to workspace[n], workspace[N + n], workspace[2 N + n].
 * Fold: the N triples are merged pairwise by Chan's rule, merge(a, b) with a the LEFT operand:
 *   n = na + nb;  d = mb - ma;  mean = ma + (d * nb) / n;  M2 = (M2a + M2b) + (((d * d) * na) * nb) / n
 *   nb == 0 returns a's three values, else na == 0 returns b's, bit for bit.
 * The order is the balanced tree over the env index: the triples are elements 0 .. N-1 of an array padded with empty
 * triples (0, 0, 0) to P = the next power of two; level l = 0, 1, ... replaces element 2^l * 2j by
 * merge(element 2^l * 2j, element 2^l * (2j + 1)) for every j, until element 0 holds the rollout's triple.  The lower
 * index is always the left operand.  One workgroup walks the tree, 64 elements per wavefront and pass (six shuffle
 * levels), in place in `workspace`: the result depends on N and the data alone.
 * Then stats[0..2] = merge(a = stats[0..2], b = the rollout's triple) and, of the merged values,
 *   stats[3] = 1.0 / sqrt(M2 / count + 1e-8)   (a quotient, a sum, a square root, a quotient);  1.0 where count == 0.
 * The result depends on how the steps are cut into calls only through the order of the merges (every call is one merge
 * into stats).  A non-finite reward makes the statistics non-finite for good.
 *   reward float[T][N]; terminated, truncated uint8[T][N]; workspace double[ppo_reward_norm_workspace(N) = 3 N], every
 *   entry written before it is read.
 * TW_E_ARG, and nothing is launched: NULL reward, terminated, truncated, ret_carry, stats or workspace; T < 0; N <= 0 or
 * 3 N >= 2^31; T * N >= 2^40; ret_carry, stats or workspace off 8-byte alignment; gamma outside [0, 1] (a NaN included).
 * T == 0 returns 0, launches nothing and leaves stats and ret_carry alone.  ppo_reward_norm_workspace: host only;
 * TW_E_ARG for N <= 0 or 3 N >= 2^31.
 *
 * ppo_reward_norm_apply, one launch, for the rollout's [T][N] rewards and for a flat array of hindsight records alike:
 *   s = stats[0] == 0 ? 1.0f : (float)stats[3];   x = reward[i] * s   (ONE float32 product)
 *   out[i] = (clip > 0 && clip < +inf) ? fminf(fmaxf(x, -clip), clip) : x
 * stats is read on the device: no host value enters the launch, and a captured launch scales by the statistics that are
 * current when it is replayed.  With all-zero stats and no clamp out[i] has the bits of reward[i].  out may alias reward
 * (wholly; a lane reads exactly the elements it writes).  16 bytes per lane by the aligned row store of row_store.h: any
 * n and any 4-byte alignment of reward and out; only out[0 .. n) is written.
 * TW_E_ARG, and nothing is launched: NULL reward, stats or out; n < 0 or n >= 2^40; reward or out off 4-byte alignment,
 * stats off 8; a NaN clip.  n == 0 returns 0 and launches nothing.
 * Neither call allocates or reads back: both may be captured into a graph and replayed.  No floating-point atomics: two
 * calls from equal state on equal inputs give equal bits. */
int ppo_reward_norm_workspace(int N);
int ppo_reward_norm_update(const float *reward, const uint8_t *terminated, const uint8_t *truncated, int T, int N,
                           double gamma, double *ret_carry, double *stats, double *workspace, void *stream);
int ppo_reward_norm_apply(const float *reward, int64_t n, const double *stats, float clip, float *out, void *stream);

/* Hindsight experience replay over one time-major rollout: replaces Buffer_gridworld.her_func
 * (soa/env_buffer.py:101-143, called from soa/train_ppo.py:128-134 at every episode end).  For every episode
 * [s0, t1] that starts (age0[n] == 0 or the step after a done) and ends (terminated | truncated) inside the
 * rollout and has <= 64 records:
 *   first_visit = np.unique(achieved (y,x) of its records, axis=0, return_index=True)   (lexicographic order)
 *   k = min(max_goals, len(first_visit)); picks = k entries of first_visit without replacement
 *   for index in picks (in pick order), skipping index == 0:  records 0..index are relabelled with
 *       goal := achieved(index), reward[index] := 0.9, done[index] := 1           (env_buffer.py:120-125)
 * The reference appends copies of those records to its ring buffer; here a relabelled record is the index tuple
 * (t, n, goal, reward, done) -- frames, positions, action and old log-prob are those of (t, n), which the
 * reference copies unchanged.  Output order: env-major, episodes in time order, picks in pick order, prefix in
 * time order (deterministic).
 *   choices int32[T][N][4] | NULL: row (t1, n) holds the picks of the episode ending at t1 as positions in the
 *       sorted unique array (entries outside [0, U) are ignored) -- replays any external RNG, e.g. the global
 *       np.random.choice stream of the reference.  NULL: partial Fisher-Yates with the words of
 *       Philox4x32-10(key = seed, counter = (env_id0 + n, step0 + t1, 0, 'TWOH')), pick j swaps perm[j] with
 *       perm[j + word_j % (U - j)]  (max_goals <= 4).
 * Two passes: offsets == NULL -> only counts[n] (records produced by env n) is written; then, with
 * offsets = exclusive prefix sum of counts (int64[N]), the records are written at offsets[n] ....
 *   pos float[T][N][2] (achieved (y,x) after each step), reward float[T][N], age0 int32[N] (episode age at t=0)
 * Positions must be finite (+0.0 and -0.0 are one position, as for np.unique); the records of an episode that holds a NaN
 * or an infinity are unspecified. */
int ppo_her_relabel(const float *pos, const uint8_t *terminated, const uint8_t *truncated, const int32_t *age0,
                    const float *reward, const int32_t *choices, uint64_t seed, uint32_t env_id0, uint32_t step0, int T,
                    int N, int max_goals, const int64_t *offsets, int32_t *counts, int32_t *out_t, int32_t *out_n,
                    float *out_goal, float *out_reward, uint8_t *out_done, void *stream);
/* The same relabelling for the 9-frame WINDOW records of the predictor / self-orientation entry points
 * (Buffer_gridworld.pre_her_func / pre_f_her_func, soa/env_buffer.py:145-280; windows stored from the fifth step on,
 * train_ppo_predictor.py:134).  Window record i carries the state after step i + 4 as its newest frame, so with
 * skip = 4 the first visits are taken among the states after steps skip, skip + 1, ... only, the first of those is
 * never a goal (`0 < index`), and a pick relabels transitions 0 .. index + skip -- the prefix records plus the four
 * sliding tail windows the reference appends.  skip = 0 is ppo_her_relabel. */
int ppo_her_relabel_window(const float *pos, const uint8_t *terminated, const uint8_t *truncated, const int32_t *age0,
                           const float *reward, const int32_t *choices, uint64_t seed, uint32_t env_id0, uint32_t step0,
                           int T, int N, int max_goals, int skip, const int64_t *offsets, int32_t *counts, int32_t *out_t,
                           int32_t *out_n, float *out_goal, float *out_reward, uint8_t *out_done, void *stream);

/* Which first visits become hindsight goals, by rule instead of the uniform draw: fills the `choices` that
 * ppo_her_relabel[_window] reads.  Same walk as there: one wavefront per env, one record per lane, and an episode is
 * handled iff it starts inside the arrays (age0[n] == 0 or the step after a done), ends inside them and has L <= 64
 * records.
 *
 * Candidates: the first visits among the records skip, skip + 1, ... (np.unique(axis=0) over (y, x), +0.0 and -0.0 one
 * position) EXCEPT the one at record `skip` itself, which the relabelling never uses (`0 < index`); C of them (C = 0 for
 * L <= skip + 1).  rank = a first visit's place in the lexicographically sorted unique array, the unit of `choices`; idx
 * = its record index inside the episode; s0, t1 = the episode's first and last row.
 *
 * Rules, the smallest key first:
 *   PPO_HER_LATE   key = 63 - idx                            the latest first visits, the longest prefixes
 *   PPO_HER_KEY16  key = key16[(s0 + idx) * N + n]           uint16[T][N], e.g. mg_nav_lookup's distances: the goals
 *                                                            nearest the real goal; 0xFFFF (unreachable) last by value
 *   PPO_HER_TABLE  key = table[cell(y, x)], signed int64     int64[width * height + 1], e.g. ppo_visit_hist's counts:
 *                                                            the rarest cells; cell by ppo_visit_scan's rule, a position
 *                                                            outside the world reads the extra bin width * height
 * Order: (key, word, rank) ascending, word = Philox4x32-10(key = seed, counter = (env_id0 + n, step0 + t1, rank,
 * 'TWOS' = 0x54574F53))[0].  Each lane counts the candidates before it; no atomics, no LDS.
 *
 * Written: with k' = min(max_goals, C), choices[t1][n][j] = rank of the candidate in place j for j < k', -1 for
 * k' <= j < 4, for the rows (t1, n) of handled episodes only; every other row of choices int32[T][N][4] is left as it
 * is, and ppo_her_relabel reads none of them.  The picks of a row are distinct.
 * stats int64[6] | NULL, each += (64-bit integer atomics: exact, whatever the scheduling): 0 handled episodes,
 * 1 candidates, 2 picks, 3 sum over the picks of idx + 1 = the records ppo_her_relabel emits from these choices,
 * 4 sum of the picked keys (LATE: 0; KEY16: the 0xFFFF keys left out), 5 picks with a 0xFFFF key (KEY16 only).
 *
 *   pos float[T][N][2] (8-byte aligned), terminated, truncated uint8[T][N], age0 int32[N]; key16, table, width and height
 *   are read by their rule only.  Positions must be finite, as for ppo_her_relabel.
 * TW_E_ARG, and nothing is launched or written: NULL pos, terminated, truncated, age0 or choices; T < 0 or N <= 0;
 * max_goals outside 1..4; skip outside 0..63; a rule other than the three; PPO_HER_KEY16 with a NULL key16; PPO_HER_TABLE
 * with a NULL table or width or height outside 1..32; T * N >= 2^40; pos off 8-byte alignment, choices off 4, key16 off
 * 2, table or stats off 8.  T == 0 returns 0 and launches nothing. */
#define PPO_HER_LATE 0
#define PPO_HER_KEY16 1
#define PPO_HER_TABLE 2
int ppo_her_select(const float *pos, const uint8_t *terminated, const uint8_t *truncated, const int32_t *age0, int T, int N,
                   int max_goals, int skip, int rule, const uint16_t *key16, const int64_t *table, int width, int height,
                   uint64_t seed, uint32_t env_id0, uint32_t step0, int32_t *choices, int64_t *stats, void *stream);

/* Epilogues of the conv layers of TINet (all_net.py:141-150: Conv2d + ReLU x 4) on channels-last activations
 * float[n_pixels][C] (n_pixels = B * H * W, C % 4 == 0, C <= 256); the conv GEMMs themselves run in MIOpen.
 *   ppo_bias_relu_nhwc               y <- relu(y + bias[c])  in place: what Conv2d's bias add + nn.ReLU compute, one pass.
 *   ppo_relu_bwd_bias_grad_nhwc      gx = gy * (y > 0)  (ReLU backward on the saved OUTPUT y) and the bias gradient as
 *                                    per-block partial sums partial[blocks][C] (the caller sums them: deterministic);
 *                                    blocks = ppo_relu_bwd_bias_grad_nhwc_blocks(n_pixels, C). */
int ppo_bias_relu_nhwc(float *y, const float *bias, int64_t n_pixels, int C, void *stream);
int ppo_relu_bwd_bias_grad_nhwc_blocks(int64_t n_pixels, int C);
int ppo_relu_bwd_bias_grad_nhwc(const float *gy, const float *y, float *gx, float *partial, int64_t n_pixels, int C,
                                void *stream);

/* First layer of TINet fused with its input upsampling (all_net.py:146,176-186):
 *   out = relu(conv2d(upsample_nearest_x4(frames), W, bias, stride 2))       frames float[B][F][17*17], F = 4 or 8
 * evaluated on the 17x17 frames with parity-folded 2x2-tap weights
 *   folded_w float[2][2][2][2][F][64] = [row parity][column parity][row tap][column tap][in channel][out channel]
 * (row parity 0: tap 0 = W rows 0+1+2+3, tap 1 = 0; parity 1: tap 0 = rows 0+1, tap 1 = rows 2+3; columns alike),
 * out float[B][33][33][64] (channels-last).  Same value as the literal layer up to the summation order. */
int ppo_conv1_up4_bias_relu(const float *frames, int B, int F, const float *folded_w, const float *bias, float *out,
                            void *stream);
/* The same layer shape with C_out output channels: (F, C_out) = (4, 64) / (8, 64) TINet, (1, 16) the world model's
 * Net_Encoder (all_net.py:7-50), whose eval-mode BatchNorm the caller folds into folded_w / bias.
 * folded_w float[2][2][2][2][F][C_out], out float[B][33][33][C_out]. */
int ppo_conv1_up4_bias_relu_c(const float *frames, int B, int F, int C_out, const float *folded_w, const float *bias,
                              float *out, void *stream);

/* Backward of ppo_conv1_up4_bias_relu w.r.t. the folded weights and the bias (the frames carry no gradient):
 *   g = gy * (y > 0);  gw_partial[group][2][2][2][2][F][64] / gb_partial[group][4][64] = per-block partial sums over the
 *   samples a group walks (groups = ppo_conv1_up4_bwd_groups(B); the caller adds groups -- and, for the bias, the four
 *   parities --, then maps the folded gradient back onto W[64][F][4][4]: dW[o][c][r][k] = sum over parities of
 *   gw[py][px][py ? r/2 : 0][px ? k/2 : 0][c][o]).  gy, y: float[B][33][33][64] channels-last, y = the layer's output. */
int ppo_conv1_up4_bwd_groups(int B);
int ppo_conv1_up4_bwd(const float *frames, int B, int F, const float *gy, const float *y, float *gw_partial,
                      float *gb_partial, void *stream);

/* Decoder of the frozen world model, inference only (Net_Decoder, all_net.py:100-137: three ConvTranspose2d with ReLUs
 * between them, then AvgPool2d(4)), one fused pass per frame:
 *   z float[n_frames][64][4][4] -> frames float[n_frames][289]   (the 17x17 predicted state matrix)
 *   w1 float[64][16][2][2], b1[16]; w2 float[16][16][5][5], b2[16]   (ConvTranspose2d layout [C_in][C_out][kH][kW])
 *   kfold float[16][3][3], b3: the last layer (16 -> 1, k4, s2) and the pooling are linear, hence one 3x3 / stride-2 /
 *   pad-1 convolution of the second activation: kfold[c][u][v] = 1/16 * sum of w3[c][0][rows R(u)][columns R(v)],
 *   R(0) = {2, 3}, R(1) = {0, 1, 2, 3}, R(2) = {0, 1}; b3 = the layer's bias.  The 68x68 image is never formed. */
int ppo_decoder_frames(const float *z, int n_frames, const float *w1, const float *b1, const float *w2, const float *b2,
                       const float *kfold, float b3, float *frames, void *stream);

/* Pointwise part of an LSTM cell (nn.LSTM gate order i, f, g, o; the world model's LSTM, all_net.py:52-98, inference):
 *   pre-activations = gates_a float[B][4H] (NULL: absent, e.g. the first step, whose hidden state is zero)  (+ gates_b: rows ldb floats apart, e.g. one time step of the input
 *   projections float[B][T][4H] -> ldb = T * 4H;  NULL: absent)  (+ bias float[4H]; NULL: absent)
 *   c float[B][H] updated in place;   h float[B][H] written
 *   c' = sigmoid(f) c + sigmoid(i) tanh(g),   h' = sigmoid(o) tanh(c').   H % 4 == 0, 16-byte aligned pointers. */
int ppo_lstm_cell(const float *gates_a, const float *gates_b, long long ldb, const float *bias, float *c, float *h, int B,
                  int H, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TWOARMY_PPO_H */
