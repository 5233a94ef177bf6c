// reward_norm.hip -- running return normalisation of rewards (C ABI in include/twoarmy_ppo.h, "Reward normalisation").
//
// gym's NormalizeReward / the baselines' VecNormalize for N envs at once: the rewards are divided by the running standard
// deviation of the discounted return.  Three kernels:
//   ppo_reward_norm_scan_kernel   one lane per env over coalesced rows, ppo_episode_scan's shape: the return G and the
//                                 env's own Welford moments (count, mean, M2) of the rollout, a float64 chain of T steps
//                                 with the rows loaded RN_ROWS ahead of it; the triple goes to the workspace
//   ppo_reward_norm_fold_kernel   ONE workgroup merges the N triples by Chan's rule along the balanced tree over the env
//                                 index, 64 elements per wavefront and pass (6 shuffle levels, left operand = lower index),
//                                 in place at stride 64^pass; thread 0 then merges the rollout into the running triple and
//                                 writes the scale.  The tree is fixed by N alone: no atomics, no dependence on the grid
//   ppo_reward_norm_apply_kernel  out = clamp(r * (float)scale): 16 bytes per lane through row_store.h, stats read on the
//                                 device
// Every float64 formula is written one operation per statement under fp contract(off): hipcc would otherwise fuse a
// product into the sum behind it, and the header promises one rounding per operation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "launch.h"
#include "row_store.h"
#include "twoarmy.h"
#include "twoarmy_ppo.h"

namespace {

constexpr int RN_ROWS = 8;                        // rows in flight ahead of the chain, as EP_ROWS of ppo_episode_scan
constexpr int RN_FOLD_THREADS = 1024;             // 16 wavefronts: 4 chunks of 64 envs each at 4096 envs
constexpr int RN_APPLY_THREADS = 256;

struct Moments {
    double n, mean, m2;
};

// One step of an env: the return, then Welford.  The caller clears G behind a done step.
__device__ __forceinline__ void rn_step(double gamma, float r, double &G, Moments &m) {
#pragma clang fp contract(off)
    const double p = gamma * G;
    G = p + (double)r;
    m.n = m.n + 1.0;
    const double d = G - m.mean;
    const double q = d / m.n;
    m.mean = m.mean + q;
    const double e = G - m.mean;
    const double f = d * e;
    m.m2 = m.m2 + f;
}

// Chan's rule, a = left, b = right; an empty operand hands back the other's bits.  Branch-free: the lanes of a tree
// level that hold no pair compute it too and drop the result.
__device__ __forceinline__ Moments rn_merge(const Moments &a, const Moments &b) {
#pragma clang fp contract(off)
    const double n = a.n + b.n;
    const double d = b.mean - a.mean;
    const double dn = d * b.n;
    const double shift = dn / n;
    const double mean = a.mean + shift;
    const double dd = d * d;
    const double dda = dd * a.n;
    const double ddab = dda * b.n;
    const double between = ddab / n;
    const double within = a.m2 + b.m2;
    const double m2 = within + between;
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    return {n, mean, m2};
}

__device__ __forceinline__ double rn_scale(const Moments &m) {
#pragma clang fp contract(off)
    if (m.n == 0.0) return 1.0;
    const double var = m.m2 / m.n;
    const double v = var + 1e-8;
    const double s = sqrt(v);
    return 1.0 / s;
}

__global__ __launch_bounds__(64) void ppo_reward_norm_scan_kernel(const float *__restrict__ reward,
                                                                  const uint8_t *__restrict__ terminated,
                                                                  const uint8_t *__restrict__ truncated, int T, int N,
                                                                  double gamma, double *__restrict__ ret_carry,
                                                                  double *__restrict__ workspace) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    double G = ret_carry[n];
    Moments m = {0.0, 0.0, 0.0};
    float r[RN_ROWS], rn[RN_ROWS];
    uint32_t d[RN_ROWS], dn[RN_ROWS];
#pragma unroll
    for (int j = 0; j < RN_ROWS; ++j) {
        const size_t i = (size_t)j * N + n;
        r[j] = j < T ? reward[i] : 0.f;
        d[j] = j < T ? (uint32_t)(terminated[i] | truncated[i]) : 0u;
    }
    for (int t0 = 0; t0 < T; t0 += RN_ROWS) {
#pragma unroll
        for (int j = 0; j < RN_ROWS; ++j) {                         // next batch: loads only, nothing waits on them yet
            const int t = t0 + RN_ROWS + j;
            const size_t i = (size_t)t * N + n;
            rn[j] = t < T ? reward[i] : 0.f;
            dn[j] = t < T ? (uint32_t)(terminated[i] | truncated[i]) : 0u;
        }
#pragma unroll
        for (int j = 0; j < RN_ROWS; ++j) {
            if (t0 + j < T) {
                rn_step(gamma, r[j], G, m);
                if (d[j]) G = 0.0;                                  // the done step's return is counted, then cleared
            }
        }
#pragma unroll
        for (int j = 0; j < RN_ROWS; ++j) { r[j] = rn[j]; d[j] = dn[j]; }
    }
    ret_carry[n] = G;
    workspace[n] = m.n;                                             // three planes of N: coalesced here and in the fold
    workspace[(size_t)N + n] = m.mean;
    workspace[2 * (size_t)N + n] = m.m2;
}

// Six levels of the tree over the 64 elements a wavefront holds, one per lane: at level l the lanes whose low l + 1 bits
// are zero merge their own element (left) with the one 2^l lanes up (right).  Lane 0 ends with the chunk's triple.
__device__ __forceinline__ Moments rn_wave_tree(Moments m, int lane) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        const Moments right = {__shfl_down(m.n, w, 64), __shfl_down(m.mean, w, 64), __shfl_down(m.m2, w, 64)};
        const Moments both = rn_merge(m, right);
        if ((lane & (2 * w - 1)) == 0) m = both;
    }
    return m;
}

// The whole tree, in place: pass p merges the elements alive at stride 64^p, 64 of them per wavefront, and leaves each
// chunk's triple in the chunk's first slot.  An element at or beyond N is empty and is never read.  Six levels per pass
// are the levels 6p .. 6p + 5 of the tree padded to the next power of two; the levels beyond it meet empty operands only.
__global__ __launch_bounds__(RN_FOLD_THREADS) void ppo_reward_norm_fold_kernel(double *workspace, int N, double *stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t plane = (size_t)N;
    Moments m = {0.0, 0.0, 0.0};
    int64_t count = N, stride = 1;
    for (;;) {
        const int64_t chunks = (count + 63) / 64;
        for (int64_t c = wave; c < chunks; c += RN_FOLD_THREADS / 64) {
            const int64_t i = c * 64 + lane;
            const size_t e = (size_t)(i * stride);
            m = Moments{0.0, 0.0, 0.0};
            if (i < count) m = Moments{workspace[e], workspace[plane + e], workspace[2 * plane + e]};
            m = rn_wave_tree(m, lane);
            if (lane == 0) {
                workspace[e] = m.n;
                workspace[plane + e] = m.mean;
                workspace[2 * plane + e] = m.m2;
            }
        }
        if (chunks == 1) break;                                     // wavefront 0 took that chunk: its lane 0 holds the rollout
        count = chunks;
        stride *= 64;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const Moments running = {stats[0], stats[1], stats[2]};
        const Moments all = rn_merge(running, m);
        stats[0] = all.n;
        stats[1] = all.mean;
        stats[2] = all.m2;
        stats[3] = rn_scale(all);
    }
}

__device__ __forceinline__ float rn_scaled(float r, float scale, float clip, bool clamp) {
#pragma clang fp contract(off)
    const float x = r * scale;
    return clamp ? fminf(fmaxf(x, -clip), clip) : x;
}

// reward and out may be one array: a lane reads the elements it stores and no others.
__global__ __launch_bounds__(RN_APPLY_THREADS) void ppo_reward_norm_apply_kernel(const float *reward, int64_t n,
                                                                                 const double *__restrict__ stats, float clip,
                                                                                 float *out, int64_t chunks) {
    const int64_t c = (int64_t)blockIdx.x * RN_APPLY_THREADS + threadIdx.x;
    if (c >= chunks) return;
    const float scale = stats[0] == 0.0 ? 1.0f : (float)stats[3];
    const bool clamp = clip > 0.0f && clip < INFINITY;
    mg_row_store(out, n, c, [&](int64_t q) -> float { return rn_scaled(reward[q], scale, clip, clamp); });
}

bool rn_aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
constexpr int64_t RN_MAX_ELEMS = (int64_t)1 << 40;

}  // namespace

extern "C" {

int ppo_reward_norm_workspace(int N) {
    if (N <= 0 || 3 * (int64_t)N >= ((int64_t)1 << 31)) return TW_E_ARG;
    return 3 * N;
}

int ppo_reward_norm_update(const float *reward, const uint8_t *terminated, const uint8_t *truncated, int T, int N,
                           double gamma, double *ret_carry, double *stats, double *workspace, void *stream) {
    if (!reward || !terminated || !truncated || !ret_carry || !stats || !workspace) return TW_E_ARG;
    if (T < 0 || ppo_reward_norm_workspace(N) < 0 || (int64_t)T * N >= RN_MAX_ELEMS) return TW_E_ARG;
    if (!rn_aligned(ret_carry, 8) || !rn_aligned(stats, 8) || !rn_aligned(workspace, 8)) return TW_E_ARG;
    if (!(gamma >= 0.0 && gamma <= 1.0)) return TW_E_ARG;             // a NaN fails both compares
    if (T == 0) return TW_OK;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ppo_reward_norm_scan_kernel, dim3((N + 63) / 64), dim3(64), 0, s, reward, terminated, truncated, T, N,
                       gamma, ret_carry, workspace);
    hipLaunchKernelGGL(ppo_reward_norm_fold_kernel, dim3(1), dim3(RN_FOLD_THREADS), 0, s, workspace, N, stats);
    return tw_launched(__func__);
}

int ppo_reward_norm_apply(const float *reward, int64_t n, const double *stats, float clip, float *out, void *stream) {
    if (!reward || !stats || !out || n < 0 || n >= RN_MAX_ELEMS) return TW_E_ARG;
    if (!rn_aligned(reward, 4) || !rn_aligned(out, 4) || !rn_aligned(stats, 8) || clip != clip) return TW_E_ARG;
    if (n == 0) return TW_OK;
    const int64_t chunks = mg_row_chunks(n, 4);
    const int64_t blocks = (chunks + RN_APPLY_THREADS - 1) / RN_APPLY_THREADS;
    hipLaunchKernelGGL(ppo_reward_norm_apply_kernel, dim3((unsigned)blocks), dim3(RN_APPLY_THREADS), 0, (hipStream_t)stream,
                       reward, n, stats, clip, out, chunks);
    return tw_launched(__func__);
}

}  // extern "C"
