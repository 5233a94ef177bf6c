// exploration_bonus.hip -- count-based exploration bonuses (C ABI in include/twoarmy_ppo.h).
//
// The reference's gym_minigrid/wrappers.py:34-102 keep a dict of visit counts and add 1/sqrt(count) to the reward:
// StateBonus keyed by agent_pos, ActionBonus by (agent_pos, agent_dir, action).  The bonus of a step depends on how often
// its key was seen BEFORE it, so the work is an ordered count, not a histogram:
//   env scope     ppo_bonus_env_kernel<false>: one wavefront per env; a chunk of steps has its keys in LDS, every step's rank
//                 among the earlier equal keys of the chunk is counted there, the carried counts are gathered with
//                 independent loads, and the last occurrence of a key stores the new count.  No atomics.
//   shared scope  ppo_bonus_row_hist_kernel (per-row histogram of keys), ppo_bonus_key_scan_kernel (inclusive scan over
//                 the rows per key, table += total), ppo_bonus_gather_kernel (count of (t, n) = table - total + prefix).
//   episode scope ppo_bonus_env_kernel<true>: the env scope's scan cut at the episode ends; every count carries the stamp
//                 of its episode, so a done clears an env's counts by stepping one generation word.
// Only integer adds reach the tables: the counts are exact whatever the scheduling, and the bonus is a pure function
// of the count.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "twoarmy.h"
#include "twoarmy_ppo.h"
#include "visit_cell.h"

namespace {

constexpr int BONUS_CHUNK = 256;                  // steps whose keys sit in LDS at once (env scope)
constexpr int BONUS_PER_LANE = BONUS_CHUNK / 64;
constexpr int BONUS_SLICE = 8192;                 // keys per LDS row histogram (shared scope); Twoarmy's 8093 fit in one
constexpr int BONUS_THREADS = 256;
constexpr int BONUS_MAX_ACTIONS = 8;

struct BonusIn {
    const float2 *pos;
    const int32_t *action;
    const int32_t *dir;
    long dir_stride_t, dir_stride_n;
    int T, N, width, height, n_actions;
};

__device__ __forceinline__ int bonus_keys(const BonusIn &in, int kind) {
    const int cells = in.width * in.height;
    return kind == 1 ? cells + 1 : cells * 4 * in.n_actions + 1;
}

// key of step (t, n): kind 1 = the cell, kind 2 = (cell * 4 + dir) * n_actions + action; anything invalid is the
// table's last slot
template <int KIND>
__device__ __forceinline__ int bonus_key(const BonusIn &in, int t, int n) {
    const size_t i = (size_t)t * in.N + n;
    const float2 p = in.pos[i];
    const int cells = in.width * in.height;
    const int cell = visit_cell(p.x, p.y, in.width, in.height);
    if (KIND == 1) return cell;
    const int d = in.dir ? in.dir[(size_t)t * in.dir_stride_t + (size_t)n * in.dir_stride_n] : 0;
    const int a = in.action[i];
    const bool ok = cell < cells && d >= 0 && d < 4 && a >= 0 && a < in.n_actions;
    return ok ? (cell * 4 + d) * in.n_actions + a : cells * 4 * in.n_actions;
}

// scale * (1 / sqrt(c)) in IEEE double, one rounding per operation (the product must not fuse into a later add)
template <typename C>
__device__ __forceinline__ double bonus_value(C count, double scale) {
#pragma clang fp contract(off)
    const double inv = 1.0 / sqrt((double)count);
    return scale * inv;
}

__device__ __forceinline__ void bonus_write(size_t i, double bs, double ba, const float *reward, const uint8_t *keep,
                                            float *bonus_state, float *bonus_action, float *reward_out) {
#pragma clang fp contract(off)
    if (bonus_state) bonus_state[i] = (float)bs;
    if (bonus_action) bonus_action[i] = (float)ba;
    if (reward_out) {
        const float r = reward[i];
        const double shaped = ((double)r + bs) + ba;              // ActionBonus(StateBonus(env)): state first
        reward_out[i] = (keep && keep[i]) ? r : (float)shaped;
    }
}

// -------------------------------------------------------------------------------------- env scope and episode scope
// One scan, bonus_chunk, in two instantiations: EPISODIC = false is the env scope, whose table word is the lifetime count;
// EPISODIC = true cuts it at the episode ends (ppo_bonus_scan_episode).  There a table word is stamp << 24 | count; it
// counts only while its stamp equals the env's generation word, so an episode end clears the env's K counts by adding 1
// to that one word.  The generation that follows 255 is 0, and the step onto it fills the env's span with zeros: no word
// older than 256 episode ends survives, and a stamp can only be met again by a word of the running episode.
constexpr uint32_t EP_COUNT_MASK = (1u << BONUS_EPISODE_COUNT_BITS) - 1u;
constexpr uint32_t EP_GEN_MASK = (1u << (32 - BONUS_EPISODE_COUNT_BITS)) - 1u;

// The done flags of one chunk as ballots: bit l of done[j] = step j * 64 + l ends an episode.  Wave-uniform.
struct EpisodeCuts {
    unsigned long long done[BONUS_PER_LANE];
    int total;                                                     // episode ends in the chunk
};

__device__ __forceinline__ EpisodeCuts episode_cuts(const uint8_t *terminated, const uint8_t *truncated, int n, int N,
                                                    int c0, int len) {
    EpisodeCuts cuts;
    cuts.total = 0;
#pragma unroll
    for (int j = 0; j < BONUS_PER_LANE; ++j) {
        const int u = j * 64 + (int)threadIdx.x;
        bool d = false;
        if (u < len) {
            const size_t i = (size_t)(c0 + u) * N + n;
            d = (terminated[i] | truncated[i]) != 0;
        }
        cuts.done[j] = __ballot(d);
        cuts.total += __popcll(cuts.done[j]);
    }
    return cuts;
}

// One chunk of one env for one kind.  Lane l owns the steps u = j * 64 + l of the chunk.  b[j] receives the bonus.
// Every step's rank among the earlier equal keys of the chunk is added to the carried count, and the chunk's last
// occurrence of a key stores the new count.  EPISODIC (cuts, gen = the env's generation before the chunk, K and form are
// read in no other case): a step counts from the carried count only if no done lies earlier in the chunk, and among the
// earlier equal keys only those behind the chunk's last earlier done.  The count is stored with the stamp of its own
// episode: what a table holds does not depend on where the chunks are cut.
template <int KIND, bool EPISODIC>
__device__ __forceinline__ void bonus_chunk(const BonusIn &in, int n, int c0, int len, const EpisodeCuts &cuts, uint32_t gen,
                                            uint32_t *table, int K, int form, double scale, int32_t *keys,
                                            double (&b)[BONUS_PER_LANE]) {
    const int lane = threadIdx.x;
    int k[BONUS_PER_LANE], since[BONUS_PER_LANE], ends[BONUS_PER_LANE];
    uint32_t carry[BONUS_PER_LANE];
    int before = 0, last = -1;                                     // of the rows j' < j: episode ends, and the last one
#pragma unroll
    for (int j = 0; j < BONUS_PER_LANE; ++j) {
        const int u = j * 64 + lane;
        if constexpr (EPISODIC) {
            const unsigned long long mine = cuts.done[j] & ((1ull << lane) - 1ull);   // the dones before u in its row
            ends[j] = before + __popcll(mine);
            since[j] = mine ? j * 64 + 63 - __clzll((long long)mine) : last;
            before += __popcll(cuts.done[j]);
            if (cuts.done[j]) last = j * 64 + 63 - __clzll((long long)cuts.done[j]);
        }
        k[j] = -1;
        carry[j] = 0u;
        if (u < len) {
            k[j] = bonus_key<KIND>(in, c0 + u, n);
            keys[u] = k[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BONUS_PER_LANE; ++j)                       // independent gathers: nothing waits on them yet
        if (j * 64 + lane < len) carry[j] = table[k[j]];
    int earlier[BONUS_PER_LANE] = {};
    bool later[BONUS_PER_LANE] = {};
    for (int v = 0; v < len; ++v) {
        const int kv = keys[v];                                    // one address for the wavefront: a broadcast read
#pragma unroll
        for (int j = 0; j < BONUS_PER_LANE; ++j) {
            const int u = j * 64 + lane;
            const bool same = kv == k[j];
            bool counted = same && v < u;
            if constexpr (EPISODIC) counted = counted && v > since[j];
            earlier[j] += counted ? 1 : 0;
            later[j] = later[j] || (same && v > u);
        }
    }
    int wrap = 0;
    bool wraps = false;
    if constexpr (EPISODIC) {
        // the done that steps from the last generation onto 0 is number 255 - gen of the chunk (from 0); it clears for real
        wrap = (int)(EP_GEN_MASK - gen);
        wraps = wrap < cuts.total;
        if (wraps) {
            __syncthreads();                                       // the gathers have landed before their words are zeroed
            for (int c = lane; c < K; c += 64) table[c] = 0u;
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < BONUS_PER_LANE; ++j) {
        if (j * 64 + lane < len) {
            if constexpr (EPISODIC) {
                const bool fresh = ends[j] == 0 && (carry[j] >> BONUS_EPISODE_COUNT_BITS) == gen;
                const uint32_t sum = (fresh ? carry[j] & EP_COUNT_MASK : 0u) + (uint32_t)earlier[j] + 1u;
                const uint32_t count = min(sum, EP_COUNT_MASK);    // at most 2^24 - 1 + 256: no 32-bit wrap
                const uint32_t stamp = (gen + (uint32_t)ends[j]) & EP_GEN_MASK;
                // a key last seen at or before the real clear stays zero
                if (!later[j] && !(wraps && ends[j] <= wrap)) table[k[j]] = stamp << BONUS_EPISODE_COUNT_BITS | count;
                b[j] = form == 0 ? bonus_value(count, scale) : (count == 1u ? scale : 0.0);
            } else {
                const uint32_t count = carry[j] + (uint32_t)earlier[j] + 1u;
                if (!later[j]) table[k[j]] = count;                // the chunk's last occurrence of the key
                b[j] = bonus_value(count, scale);
            }
        }
    }
    __syncthreads();                                               // keys[] is reused; the next chunk gathers what was stored
}

// The episode ends, an argument of the episodic kernel only: the env scope's has nothing there to read, and the empty
// array keeps it at no bytes, so that kernel's argument block and code are what they were without it.
template <bool EPISODIC>
struct EpisodeFlags {
    char none[0];
};
template <>
struct EpisodeFlags<true> {
    const uint8_t *terminated, *truncated;
};

// One wavefront per env.  EPISODIC: the kernel also owns the env's generation words, which follow the N spans of counts.
template <bool EPISODIC>
__global__ __launch_bounds__(64) void ppo_bonus_env_kernel(BonusIn in, const float *reward, const uint8_t *keep,
                                                           EpisodeFlags<EPISODIC> flags, int kind_mask, int form,
                                                           double scale, uint32_t *state_table, uint32_t *action_table,
                                                           float *bonus_state, float *bonus_action, float *reward_out) {
    __shared__ int32_t keys[BONUS_CHUNK];
    const int lane = threadIdx.x;
    const int n = blockIdx.x;
    const int ks = bonus_keys(in, 1), ka = bonus_keys(in, 2);
    uint32_t *gen_state = nullptr, *gen_action = nullptr;
    uint32_t gs = 0u, ga = 0u;
    if constexpr (EPISODIC) {
        if (kind_mask & 1) gen_state = state_table + (size_t)in.N * ks + n;
        if (kind_mask & 2) gen_action = action_table + (size_t)in.N * ka + n;
        gs = gen_state ? *gen_state & EP_GEN_MASK : 0u;
        ga = gen_action ? *gen_action & EP_GEN_MASK : 0u;
    }
    for (int c0 = 0; c0 < in.T; c0 += BONUS_CHUNK) {
        const int len = min(BONUS_CHUNK, in.T - c0);
        EpisodeCuts cuts = {};
        if constexpr (EPISODIC) cuts = episode_cuts(flags.terminated, flags.truncated, n, in.N, c0, len);
        double bs[BONUS_PER_LANE] = {}, ba[BONUS_PER_LANE] = {};
        if (kind_mask & 1)
            bonus_chunk<1, EPISODIC>(in, n, c0, len, cuts, gs, state_table + (size_t)n * ks, ks, form, scale, keys, bs);
        if (kind_mask & 2)
            bonus_chunk<2, EPISODIC>(in, n, c0, len, cuts, ga, action_table + (size_t)n * ka, ka, form, scale, keys, ba);
        if constexpr (EPISODIC) {
            gs = (gs + (uint32_t)cuts.total) & EP_GEN_MASK;
            ga = (ga + (uint32_t)cuts.total) & EP_GEN_MASK;
        }
#pragma unroll
        for (int j = 0; j < BONUS_PER_LANE; ++j) {
            const int u = j * 64 + lane;
            if (u < len)
                bonus_write((size_t)(c0 + u) * in.N + n, bs[j], ba[j], reward, keep, bonus_state, bonus_action, reward_out);
        }
    }
    if constexpr (EPISODIC) {
        if (lane == 0) {
            if (gen_state) *gen_state = gs;
            if (gen_action) *gen_action = ga;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- shared scope
// hist[t][k0 .. k0 + BONUS_SLICE) of row t = blockIdx.x and key slice blockIdx.y: the block owns that part of the row,
// so it is written with plain stores and needs no clearing beforehand.
template <int KIND>
__global__ __launch_bounds__(BONUS_THREADS) void ppo_bonus_row_hist_kernel(BonusIn in, uint32_t *__restrict__ hist) {
    __shared__ uint32_t part[BONUS_SLICE];
    const int K = bonus_keys(in, KIND);
    const int t = blockIdx.x;
    const int k0 = blockIdx.y * BONUS_SLICE;
    const int kn = min(BONUS_SLICE, K - k0);
    for (int c = threadIdx.x; c < kn; c += BONUS_THREADS) part[c] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // every lane of a wavefront runs the same number of rounds (visit_grouped_add's ballots need all of them)
    for (int base = threadIdx.x - lane; base < in.N; base += BONUS_THREADS) {
        const int n = base + lane;
        bool pending = n < in.N;
        int c = 0;
        if (pending) {
            c = bonus_key<KIND>(in, t, n) - k0;
            pending = c >= 0 && c < kn;
        }
        visit_grouped_add(part, c, pending, lane);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < kn; c += BONUS_THREADS) hist[(size_t)t * K + k0 + c] = part[c];
}

// hist[t][k] <- hist[0][k] + ... + hist[t][k]; table[k] += hist[T-1][k].  One thread per key, coalesced rows.
__global__ __launch_bounds__(BONUS_THREADS) void ppo_bonus_key_scan_kernel(uint32_t *__restrict__ hist, int T, int K,
                                                                           int64_t *__restrict__ table) {
    const int k = blockIdx.x * BONUS_THREADS + threadIdx.x;
    if (k >= K) return;
    uint32_t run = 0u;
    for (int t = 0; t < T; ++t) {
        run += hist[(size_t)t * K + k];
        hist[(size_t)t * K + k] = run;
    }
    table[k] += (int64_t)run;
}

template <int KIND>
__device__ __forceinline__ double bonus_shared_value(const BonusIn &in, int t, int n, const uint32_t *hist,
                                                     const int64_t *table, double scale) {
    const int K = bonus_keys(in, KIND);
    const int k = bonus_key<KIND>(in, t, n);
    // table already holds this launch's total: count = carry + rows 0 .. t
    const int64_t count = table[k] - (int64_t)hist[(size_t)(in.T - 1) * K + k] + (int64_t)hist[(size_t)t * K + k];
    return bonus_value(count, scale);
}

__global__ __launch_bounds__(BONUS_THREADS) void ppo_bonus_gather_kernel(BonusIn in, const float *reward,
                                                                         const uint8_t *keep, int kind_mask, double scale,
                                                                         const int64_t *state_table,
                                                                         const int64_t *action_table,
                                                                         const uint32_t *hist_state,
                                                                         const uint32_t *hist_action, float *bonus_state,
                                                                         float *bonus_action, float *reward_out) {
    const int64_t i = (int64_t)blockIdx.x * BONUS_THREADS + threadIdx.x;
    if (i >= (int64_t)in.T * in.N) return;
    const int t = (int)(i / in.N), n = (int)(i % in.N);
    const double bs = (kind_mask & 1) ? bonus_shared_value<1>(in, t, n, hist_state, state_table, scale) : 0.0;
    const double ba = (kind_mask & 2) ? bonus_shared_value<2>(in, t, n, hist_action, action_table, scale) : 0.0;
    bonus_write((size_t)i, bs, ba, reward, keep, bonus_state, bonus_action, reward_out);
}

int64_t bonus_keys_host(int kind, int width, int height, int n_actions) {
    const int64_t cells = (int64_t)width * height;
    return kind == 1 ? cells + 1 : cells * 4 * n_actions + 1;
}

bool bonus_geom_ok(int width, int height, int n_actions) {
    return visit_grid_ok(width, height) && n_actions >= 1 && n_actions <= BONUS_MAX_ACTIONS;
}

// Words of one table that holds (K + extra) * times words for the K keys of `kind`; TW_E_ARG where there is no such
// table or it has 2^31 words or more.
int bonus_words(int kind, int width, int height, int n_actions, int extra, int64_t times) {
    if ((kind != 1 && kind != 2) || !bonus_geom_ok(width, height, n_actions) || times < 0) return TW_E_ARG;
    const int64_t words = (bonus_keys_host(kind, width, height, n_actions) + extra) * times;
    return words < ((int64_t)1 << 31) ? (int)words : TW_E_ARG;
}

BonusIn bonus_in(const float *pos, const int32_t *action, const int32_t *dir, long dir_stride_t, long dir_stride_n, int T,
                 int N, int width, int height, int n_actions) {
    return {reinterpret_cast<const float2 *>(pos), action, dir, dir_stride_t, dir_stride_n, T, N, width, height, n_actions};
}

// What both scan entries refuse.  words(kind): the entry's own table-size query, asked for the kinds in the mask.
template <typename Words>
bool bonus_scan_ok(const BonusIn &in, const float *reward, int kind_mask, const void *state_table, const void *action_table,
                   const float *reward_out, Words words) {
    if (!in.pos || ((uintptr_t)in.pos & 7u) || in.T < 0 || in.N < 0 || !bonus_geom_ok(in.width, in.height, in.n_actions))
        return false;
    if (kind_mask < 1 || kind_mask > 3) return false;
    if ((kind_mask & 1) && (!state_table || ((uintptr_t)state_table & 7u))) return false;
    if ((kind_mask & 2) && (!action_table || ((uintptr_t)action_table & 7u) || !in.action)) return false;
    if (in.dir && (in.dir_stride_t < 0 || in.dir_stride_n < 0)) return false;
    if (reward_out && !reward) return false;
    if ((int64_t)in.T * in.N >= ((int64_t)1 << 31)) return false;         // a row histogram's 32-bit prefix cannot wrap
    for (int kind = 1; kind <= 2; ++kind)
        if ((kind_mask & kind) && words(kind) < 0) return false;
    return true;
}

}  // namespace

extern "C" {

int ppo_bonus_table_words(int kind, int scope, int width, int height, int n_actions, int N) {
    if ((scope != 0 && scope != 1) || N < 0) return TW_E_ARG;
    return bonus_words(kind, width, height, n_actions, 0, scope == 0 ? N : 2);        // a span per env, or one of int64
}

int64_t ppo_bonus_workspace_bytes(int kind_mask, int scope, int T, int width, int height, int n_actions) {
    if (kind_mask < 1 || kind_mask > 3 || (scope != 0 && scope != 1) || !bonus_geom_ok(width, height, n_actions) || T < 0)
        return TW_E_ARG;
    if (scope == 0) return 0;
    int64_t K = 0;
    if (kind_mask & 1) K += bonus_keys_host(1, width, height, n_actions);
    if (kind_mask & 2) K += bonus_keys_host(2, width, height, n_actions);
    return 4 * K * (int64_t)T;
}

int ppo_bonus_scan(const float *pos, const int32_t *action, const int32_t *dir, long dir_stride_t, long dir_stride_n,
                   const float *reward, const uint8_t *keep, int T, int N, int width, int height, int n_actions,
                   int kind_mask, int scope, double scale, void *state_table, void *action_table, float *bonus_state,
                   float *bonus_action, float *reward_out, void *workspace, void *stream) {
    const BonusIn in = bonus_in(pos, action, dir, dir_stride_t, dir_stride_n, T, N, width, height, n_actions);
    const auto words = [&](int kind) { return ppo_bonus_table_words(kind, scope, width, height, n_actions, N); };
    if (!bonus_scan_ok(in, reward, kind_mask, state_table, action_table, reward_out, words)) return TW_E_ARG;
    if ((scope != 0 && scope != 1) || (scope == 1 && (!workspace || ((uintptr_t)workspace & 3u)))) return TW_E_ARG;
    if (T == 0 || N == 0) return TW_OK;
    const hipStream_t s = (hipStream_t)stream;
    if (scope == 0) {
        hipLaunchKernelGGL(ppo_bonus_env_kernel<false>, dim3(N), dim3(64), 0, s, in, reward, keep, EpisodeFlags<false>{},
                           kind_mask, 0, scale, (uint32_t *)state_table, (uint32_t *)action_table, bonus_state, bonus_action,
                           reward_out);
        return tw_launched(__func__);
    }
    const int Ks = (int)bonus_keys_host(1, width, height, n_actions), Ka = (int)bonus_keys_host(2, width, height, n_actions);
    uint32_t *hist_state = (uint32_t *)workspace;
    uint32_t *hist_action = hist_state + ((kind_mask & 1) ? (size_t)T * Ks : 0);
    if (kind_mask & 1) {
        hipLaunchKernelGGL(ppo_bonus_row_hist_kernel<1>, dim3(T, (Ks + BONUS_SLICE - 1) / BONUS_SLICE), dim3(BONUS_THREADS),
                           0, s, in, hist_state);
        hipLaunchKernelGGL(ppo_bonus_key_scan_kernel, dim3((Ks + BONUS_THREADS - 1) / BONUS_THREADS), dim3(BONUS_THREADS), 0,
                           s, hist_state, T, Ks, (int64_t *)state_table);
    }
    if (kind_mask & 2) {
        hipLaunchKernelGGL(ppo_bonus_row_hist_kernel<2>, dim3(T, (Ka + BONUS_SLICE - 1) / BONUS_SLICE), dim3(BONUS_THREADS),
                           0, s, in, hist_action);
        hipLaunchKernelGGL(ppo_bonus_key_scan_kernel, dim3((Ka + BONUS_THREADS - 1) / BONUS_THREADS), dim3(BONUS_THREADS), 0,
                           s, hist_action, T, Ka, (int64_t *)action_table);
    }
    if (bonus_state || bonus_action || reward_out) {
        const int64_t blocks = ((int64_t)T * N + BONUS_THREADS - 1) / BONUS_THREADS;
        hipLaunchKernelGGL(ppo_bonus_gather_kernel, dim3((unsigned)blocks), dim3(BONUS_THREADS), 0, s, in, reward, keep,
                           kind_mask, scale, (const int64_t *)state_table, (const int64_t *)action_table, hist_state,
                           hist_action, bonus_state, bonus_action, reward_out);
    }
    return tw_launched(__func__);
}

int ppo_bonus_episode_words(int kind, int width, int height, int n_actions, int N) {
    return bonus_words(kind, width, height, n_actions, 1, N);                              // K counts and a generation per env
}

int ppo_bonus_scan_episode(const float *pos, const int32_t *action, const int32_t *dir, long dir_stride_t, long dir_stride_n,
                           const float *reward, const uint8_t *keep, const uint8_t *terminated, const uint8_t *truncated,
                           int T, int N, int width, int height, int n_actions, int kind_mask, int form, double scale,
                           void *state_table, void *action_table, float *bonus_state, float *bonus_action,
                           float *reward_out, void *stream) {
    const BonusIn in = bonus_in(pos, action, dir, dir_stride_t, dir_stride_n, T, N, width, height, n_actions);
    const auto words = [&](int kind) { return ppo_bonus_episode_words(kind, width, height, n_actions, N); };
    if (!bonus_scan_ok(in, reward, kind_mask, state_table, action_table, reward_out, words)) return TW_E_ARG;
    if ((form != 0 && form != 1) || !terminated || !truncated) return TW_E_ARG;
    if (T == 0 || N == 0) return TW_OK;
    hipLaunchKernelGGL(ppo_bonus_env_kernel<true>, dim3(N), dim3(64), 0, (hipStream_t)stream, in, reward, keep,
                       EpisodeFlags<true>{terminated, truncated}, kind_mask, form, scale, (uint32_t *)state_table,
                       (uint32_t *)action_table, bonus_state, bonus_action, reward_out);
    return tw_launched(__func__);
}

}  // extern "C"
