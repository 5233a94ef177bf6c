// visitation.hip -- which grid cells the agents stood on (C ABI in include/twoarmy_ppo.h).
//
// The reference draws a visit-count heatmap after every PPO.update (soa/agent/PPO.py:161): soa/img_proccess/heatmap.py:58-81
// walks the buffer's after-step positions and does values_matrix[y, x] += 1.  Two kernels restate the matrix and add the
// per-episode set of visited cells (the goal candidates of her_func, soa/env_buffer.py:138):
//   ppo_visit_scan   one lane per env, the episode's cell set as a bitmap in LDS, carried across launches
//   ppo_visit_hist   int64 counts per cell: equal cells grouped within a wavefront, one LDS add per group, per-block
//                    partial histograms, one 64-bit atomic per non-empty bin and block at the end
// Only integer adds and ORs: the results are exact and do not depend on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "twoarmy.h"
#include "twoarmy_ppo.h"
#include "visit_cell.h"

namespace {

constexpr int VISIT_MAX_WORDS = VISIT_MAX_SIDE * VISIT_MAX_SIDE / 32;        // bitmap words of the largest grid
constexpr int VISIT_ROWS = 8;                                               // rows loaded ahead of the dependent chain

// One lane per env over coalesced rows, like ppo_episode_scan.  The bitmap is indexed by a run-time cell number, so it
// lives in LDS and not in registers (a register array indexed at run time becomes scratch): word w of lane l sits at
// bits[w * 64 + l], which puts lane l on bank l whatever w is -- no bank conflict, and no barrier, since a lane only
// ever touches its own column.  The carry is word-major over envs (carry[w * N + n]) so that a wavefront's loads and
// stores of one word are contiguous.
__global__ __launch_bounds__(64) void ppo_visit_scan_kernel(const float2 *__restrict__ pos,
                                                            const uint8_t *__restrict__ terminated,
                                                            const uint8_t *__restrict__ truncated, int T, int N, int width,
                                                            int height, uint32_t *__restrict__ carry,
                                                            uint8_t *__restrict__ first_visit,
                                                            int32_t *__restrict__ ep_cells) {
    __shared__ uint32_t bits[VISIT_MAX_WORDS * 64];
    const int lane = threadIdx.x;
    const int n = blockIdx.x * 64 + lane;
    if (n >= N) return;
    const int cells = width * height;
    const int words = (cells + 31) >> 5;
    int seen = 0;
    for (int w = 0; w < words; ++w) {
        const uint32_t v = carry[(size_t)w * N + n];
        bits[w * 64 + lane] = v;
        seen += __popc(v);
    }
    float2 p[VISIT_ROWS], pn[VISIT_ROWS];
    uint32_t d[VISIT_ROWS], dn[VISIT_ROWS];
#pragma unroll
    for (int j = 0; j < VISIT_ROWS; ++j) {
        const size_t i = (size_t)j * N + n;
        p[j] = j < T ? pos[i] : make_float2(0.f, 0.f);
        d[j] = j < T ? (uint32_t)(terminated[i] | truncated[i]) : 0u;
    }
    for (int t0 = 0; t0 < T; t0 += VISIT_ROWS) {
#pragma unroll
        for (int j = 0; j < VISIT_ROWS; ++j) {                      // next batch: loads only, nothing waits on them yet
            const int t = t0 + VISIT_ROWS + j;
            const size_t i = (size_t)t * N + n;
            pn[j] = t < T ? pos[i] : make_float2(0.f, 0.f);
            dn[j] = t < T ? (uint32_t)(terminated[i] | truncated[i]) : 0u;
        }
#pragma unroll
        for (int j = 0; j < VISIT_ROWS; ++j) {
            const int t = t0 + j;
            if (t < T) {
                const size_t i = (size_t)t * N + n;
                const int c = visit_cell(p[j].x, p[j].y, width, height);
                uint32_t fresh = 0u;
                if (c < cells) {
                    const uint32_t bit = 1u << (c & 31);
                    const uint32_t old = bits[(c >> 5) * 64 + lane];
                    fresh = (old & bit) ? 0u : 1u;
                    bits[(c >> 5) * 64 + lane] = old | bit;
                }
                seen += (int)fresh;
                if (first_visit) first_visit[i] = (uint8_t)fresh;
                if (ep_cells) ep_cells[i] = seen;
                if (d[j]) {
                    for (int w = 0; w < words; ++w) bits[w * 64 + lane] = 0u;
                    seen = 0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < VISIT_ROWS; ++j) { p[j] = pn[j]; d[j] = dn[j]; }
    }
    for (int w = 0; w < words; ++w) carry[(size_t)w * N + n] = bits[w * 64 + lane];
}

// Positions are concentrated: on the step after a reset every env stands next to the same start cell, and a plain LDS
// histogram would have 64 lanes adding to one address.  So a wavefront first groups equal cells (visit_grouped_add,
// visit_cell.h).  Blocks keep 32-bit partial histograms (a block sees < 2^31 elements)
// and add their non-empty bins to the int64 counts at the end.
constexpr int VISIT_HIST_THREADS = 256;
constexpr int VISIT_HIST_PER_THREAD = 8;
constexpr int VISIT_HIST_MAX_BLOCKS = 512;

__global__ __launch_bounds__(VISIT_HIST_THREADS) void ppo_visit_hist_kernel(
    const float2 *__restrict__ pos, int T, int N, const uint8_t *__restrict__ mask, const int32_t *__restrict__ t_idx,
    const int32_t *__restrict__ n_idx, int64_t M, int width, int height, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t hist[VISIT_MAX_SIDE * VISIT_MAX_SIDE + 1];
    const int cells = width * height;
    for (int c = threadIdx.x; c <= cells; c += VISIT_HIST_THREADS) hist[c] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * VISIT_HIST_THREADS;
    // every lane of a wavefront runs the same number of rounds (the ballots below need all of them)
    for (int64_t base = (int64_t)blockIdx.x * VISIT_HIST_THREADS + (threadIdx.x - lane); base < M; base += stride) {
        const int64_t i = base + lane;
        bool pending = i < M;
        int c = cells;
        if (pending) {
            if (t_idx) {
                const int t = t_idx[i], n = n_idx[i];
                if (t >= 0 && t < T && n >= 0 && n < N) {
                    const float2 p = pos[(size_t)t * N + n];
                    c = visit_cell(p.x, p.y, width, height);
                }
            } else if (mask && mask[i] == 0) {
                pending = false;
            } else {
                const float2 p = pos[i];
                c = visit_cell(p.x, p.y, width, height);
            }
        }
        visit_grouped_add(hist, c, pending, lane);
    }
    __syncthreads();
    for (int c = threadIdx.x; c <= cells; c += VISIT_HIST_THREADS) {
        const uint32_t v = hist[c];
        if (v) atomicAdd(&counts[c], (unsigned long long)v);
    }
}

}  // namespace

extern "C" {

int ppo_visit_carry_words(int width, int height, int N) {
    if (!visit_grid_ok(width, height) || N < 0) return TW_E_ARG;
    const int64_t words = (int64_t)((width * height + 31) / 32) * N;
    return words < ((int64_t)1 << 31) ? (int)words : TW_E_ARG;
}

int ppo_visit_scan(const float *pos, const uint8_t *terminated, const uint8_t *truncated, int T, int N, int width,
                   int height, uint32_t *carry, uint8_t *first_visit, int32_t *ep_cells, void *stream) {
    if (!pos || !terminated || !truncated || !carry || !visit_grid_ok(width, height) || T < 0 || N < 0) return TW_E_ARG;
    if (ppo_visit_carry_words(width, height, N) < 0 || ((uintptr_t)pos & 7u)) return TW_E_ARG;
    if (T == 0 || N == 0) return TW_OK;
    hipLaunchKernelGGL(ppo_visit_scan_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2 *>(pos), terminated, truncated, T, N, width, height, carry,
                       first_visit, ep_cells);
    return tw_launched(__func__);
}

int ppo_visit_hist(const float *pos, int T, int N, const uint8_t *mask, const int32_t *t_idx, const int32_t *n_idx, int B,
                   int width, int height, int64_t *counts, void *stream) {
    if (!pos || !counts || !visit_grid_ok(width, height) || T < 0 || N < 0 || B < 0) return TW_E_ARG;
    if ((t_idx == nullptr) != (n_idx == nullptr) || ((uintptr_t)pos & 7u) || ((uintptr_t)counts & 7u)) return TW_E_ARG;
    if ((int64_t)T * N > ((int64_t)1 << 40)) return TW_E_ARG;              // a block's 32-bit partial counts cannot wrap
    if (T == 0 || N == 0) return TW_OK;
    const int64_t M = t_idx ? (int64_t)B : (int64_t)T * N;
    if (M == 0) return TW_OK;
    const int64_t per_block = (int64_t)VISIT_HIST_THREADS * VISIT_HIST_PER_THREAD;
    const int64_t want = (M + per_block - 1) / per_block;
    const int blocks = (int)(want < VISIT_HIST_MAX_BLOCKS ? want : VISIT_HIST_MAX_BLOCKS);
    hipLaunchKernelGGL(ppo_visit_hist_kernel, dim3(blocks), dim3(VISIT_HIST_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2 *>(pos), T, N, mask, t_idx, n_idx, M, width, height,
                       reinterpret_cast<unsigned long long *>(counts));
    return tw_launched(__func__);
}

}  // extern "C"
