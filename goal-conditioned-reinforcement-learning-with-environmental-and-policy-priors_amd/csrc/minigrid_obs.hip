/*
 * minigrid_obs.hip -- the observation wrappers of gym_minigrid/wrappers.py on the device (C ABI: include/minigrid_obs.h).
 *
 *   mg_obs_onehot_kernel     one lane per 16-byte chunk of the output.  A chunk spans at most two cells (21 bytes
 *                            each): the lane folds the two cells' index bits into one 42-bit mask, shifts it to the
 *                            chunk's first byte and spreads 4 bits -> 4 bytes with one multiply.  7 bytes leave per
 *                            byte read: a store stream.
 *   mg_obs_full_kernel       the plane -> x-major transposition goes through LDS: a workgroup resolves the cells of its
 *                            span of the output (empty rule, agent stamp) into LDS, then stores whole 16-byte chunks.
 *   mg_obs_symbolic_kernel,  one lane per 16-byte chunk (four int32 / float32 values), generated in registers.
 *   mg_obs_flat_kernel
 *   mg_obs_goal_index_kernel one wave per env: ballot over 64 cells at a time, first set bit.
 *   mg_obs_goal_direction_kernel   one lane per env; the slope is one IEEE double division, the angle a table entry.
 *
 * Every chunked kernel stores its rows (the whole array for the dense symbolic grid) by the rule of row_store.h:
 * aligned 16-byte chunks inside the row, the elements of its first and last chunk one by one.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "minigrid_obs.h"
#include "row_store.h"
#include "twoarmy.h"

#define MG_OBS_THREADS 256
#define MG_OBS_FULL_CHUNKS 256                              /* 16-byte chunks per workgroup of mg_obs_full_kernel */
#define MG_OBS_FULL_CELLS (MG_OBS_FULL_CHUNKS * 16 / 3 + 3) /* cells a span of 4096 bytes can touch (1367), + 1 */

/* ------------------------------------------------------------------------------------------------ one-hot */
/* bits 0..3 of b -> bytes 0..3 of the result (bit i lands at 8 * i: the four partial products do not overlap) */
__device__ static inline uint32_t mg_obs_spread4(uint32_t b)
{
    return ((b & 15u) * 0x00204081u) & 0x01010101u;
}

/* out[i, j, type] = out[i, j, 12 + colour] = out[i, j, 18 + state] = 1 as a 21-bit mask; an index >= 21 sets *bad */
__device__ static inline uint32_t mg_obs_cell_mask(const uint8_t *__restrict__ img, int cell, int n_cells, int *bad)
{
    if (cell >= n_cells) return 0;
    const uint32_t t = img[3 * cell], c = img[3 * cell + 1], s = img[3 * cell + 2];
    uint32_t m = 0;
    if (t < MG_OBS_ONEHOT_BITS) m |= 1u << t; else *bad = 1;
    if (MG_OBS_TYPE_BITS + c < MG_OBS_ONEHOT_BITS) m |= 1u << (MG_OBS_TYPE_BITS + c); else *bad = 1;
    if (MG_OBS_TYPE_BITS + MG_OBS_COLOUR_BITS + s < MG_OBS_ONEHOT_BITS) m |= 1u << (MG_OBS_TYPE_BITS + MG_OBS_COLOUR_BITS + s);
    else *bad = 1;
    return m;
}

__global__ __launch_bounds__(MG_OBS_THREADS) void mg_obs_onehot_kernel(const uint8_t *__restrict__ image, int64_t ipitch,
                                                                       int N, int n_cells, uint8_t *__restrict__ out,
                                                                       int64_t opitch, int32_t *__restrict__ error, int cpr)
{
    const int64_t g = (int64_t)blockIdx.x * MG_OBS_THREADS + threadIdx.x;
    if (g >= (int64_t)N * cpr) return;
    const int e = (int)(g / cpr), c = (int)(g - (int64_t)e * cpr);
    uint8_t *ob = out + (int64_t)e * opitch;
    const int F = n_cells * MG_OBS_ONEHOT_BITS, lo = mg_row_chunk(mg_row_misalign(ob, 16), F, c, 16).lo;
    if (lo >= F) return;
    const uint8_t *img = image + (int64_t)e * ipitch;
    const int cell0 = lo / MG_OBS_ONEHOT_BITS, k0 = lo - cell0 * MG_OBS_ONEHOT_BITS;
    int bad = 0;
    uint64_t m = (uint64_t)mg_obs_cell_mask(img, cell0, n_cells, &bad) |
                 (uint64_t)mg_obs_cell_mask(img, cell0 + 1, n_cells, &bad) << MG_OBS_ONEHOT_BITS;
    m >>= k0;                                               /* bit j = byte lo + j; k0 + 16 <= 37 < 42 */
    mg_row_store(ob, F, c, [&](int) {
        const uint32_t w = (uint32_t)m;
        return make_uint4(mg_obs_spread4(w), mg_obs_spread4(w >> 4), mg_obs_spread4(w >> 8), mg_obs_spread4(w >> 12));
    }, [&](int q) { return (uint8_t)((m >> (q - lo)) & 1u); });
    if (bad && error) error[e] = 1;                         /* zeroed on the stream before the launch */
}

/* ------------------------------------------------------------------------------------------------ full grid */
__global__ __launch_bounds__(MG_OBS_THREADS) void mg_obs_full_kernel(
    const uint8_t *__restrict__ type, const uint8_t *__restrict__ colour, const uint8_t *__restrict__ state, int N, int W,
    int H, const int32_t *__restrict__ agent_x, const int32_t *__restrict__ agent_y, const int32_t *__restrict__ agent_dir,
    int astride, uint8_t *__restrict__ out, int64_t pitch, int32_t *__restrict__ error, int bpe)
{
    __shared__ __attribute__((aligned(16))) uint8_t cells[MG_OBS_FULL_CELLS * 3];
    const int tid = threadIdx.x;
    const int e = blockIdx.x / bpe, b = blockIdx.x - e * bpe;
    uint8_t *ob = out + (int64_t)e * pitch;
    const int HW = W * H, F = HW * 3;
    const mg_row_span_t<int> g = mg_row_span(mg_row_misalign(ob, 16), F, b, MG_OBS_FULL_CHUNKS, 16);
    if (g.c0 >= g.c1) return;                               /* uniform per workgroup; workgroup 0 always has chunks */
    const int cell_lo = g.p_lo / 3, cell_hi = (g.p_hi - 1) / 3;                   /* x-major cells x * H + y, inclusive */
    const int ax = agent_x[(int64_t)e * astride], ay = agent_y[(int64_t)e * astride], ad = agent_dir[(int64_t)e * astride];
    const bool inside = ax >= 0 && ax < W && ay >= 0 && ay < H;
    const int acell = inside ? ax * H + ay : -1;
    const uint8_t *ty = type + (int64_t)e * HW, *co = colour + (int64_t)e * HW;
    const uint8_t *st = state ? state + (int64_t)e * HW : nullptr;
    for (int t = tid; t <= cell_hi - cell_lo; t += MG_OBS_THREADS) {
        const int c = cell_lo + t, x = c / H, y = c - x * H, src = y * W + x;
        uint8_t v0 = ty[src], v1 = 0, v2 = 0;
        if (v0 <= 1) v0 = 1;                                /* empty: (1, 0, 0) */
        else { v1 = co[src]; v2 = st ? st[src] : 0; }
        if (c == acell) { v0 = 10; v1 = 0; v2 = (uint8_t)ad; }
        cells[3 * t] = v0; cells[3 * t + 1] = v1; cells[3 * t + 2] = v2;
    }
    if (b == 0 && tid == 0 && error) error[e] = inside ? 0 : 2;
    __syncthreads();
    const int off = -3 * cell_lo;                           /* cells[off + p] = output byte p, p_lo <= p < p_hi */
    for (int c = g.c0 + tid; c < g.c1; c += MG_OBS_THREADS)
        mg_row_store(ob, F, c, [&](int p) {
            uint32_t w[4];
#pragma unroll
            for (int d = 0; d < 4; d++)
                w[d] = (uint32_t)cells[off + p + 4 * d] | (uint32_t)cells[off + p + 4 * d + 1] << 8 |
                       (uint32_t)cells[off + p + 4 * d + 2] << 16 | (uint32_t)cells[off + p + 4 * d + 3] << 24;
            return make_uint4(w[0], w[1], w[2], w[3]);
        }, [&](int q) { return cells[off + q]; });
}

/* ------------------------------------------------------------------------------------------------ symbolic, flat */
__global__ __launch_bounds__(MG_OBS_THREADS) void mg_obs_symbolic_kernel(const uint8_t *__restrict__ type, int W, int H,
                                                                         int32_t *__restrict__ out, int64_t total,
                                                                         int64_t chunks)
{
    const int64_t c = (int64_t)blockIdx.x * MG_OBS_THREADS + threadIdx.x;
    if (c >= chunks) return;
    const int HW = W * H, R = HW * 3;
    mg_row_store(out, total, c, [&](int64_t i) -> int32_t {
        const int64_t e = i / R;
        const int r = (int)(i - e * R), f = r / 3, k = r - 3 * f;
        if (k == 0) return f / H;
        if (k == 1) return f % H;
        const int t = type[e * HW + f];                     /* objects.reshape(1, w, h)[0][x][y] = flat cell x * h + y */
        return t <= 1 ? -1 : t;
    });
}

__global__ __launch_bounds__(MG_OBS_THREADS) void mg_obs_flat_kernel(const uint8_t *__restrict__ image, int64_t ipitch,
                                                                     int N, int n_img, const float *__restrict__ tail,
                                                                     int n_tail, float *__restrict__ out, int64_t opitch,
                                                                     int cpr)
{
    const int64_t g = (int64_t)blockIdx.x * MG_OBS_THREADS + threadIdx.x;
    if (g >= (int64_t)N * cpr) return;
    const int e = (int)(g / cpr), c = (int)(g - (int64_t)e * cpr);
    const uint8_t *img = image + (int64_t)e * ipitch;
    mg_row_store(out + (int64_t)e * opitch, (int64_t)n_img + n_tail, (int64_t)c, [&](int64_t i) -> float {
        return i < n_img ? (float)img[i] : tail[i - n_img];
    });
}

/* ------------------------------------------------------------------------------------------------ goal direction */
__global__ __launch_bounds__(MG_OBS_THREADS) void mg_obs_goal_index_kernel(const uint8_t *__restrict__ type, int N, int HW,
                                                                           int32_t *__restrict__ goal_index)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (MG_OBS_THREADS / 64) + (threadIdx.x >> 6);
    if (e >= N) return;                                     /* uniform per wave */
    const uint8_t *ty = type + e * HW;
    int found = -1;
    for (int base = 0; base < HW; base += 64) {             /* uniform per wave */
        const int k = base + lane;
        const unsigned long long hit = __ballot(k < HW && ty[k] == 8);
        if (hit) { found = base + __ffsll((long long)hit) - 1; break; }
    }
    if (lane == 0) goal_index[e] = found;
}

__global__ __launch_bounds__(MG_OBS_THREADS) void mg_obs_goal_direction_kernel(
    const int32_t *__restrict__ goal_index, int N, int W, int H, const int32_t *__restrict__ agent_x,
    const int32_t *__restrict__ agent_y, int astride, int mode, const double *__restrict__ table, double *__restrict__ out,
    int32_t *__restrict__ error)
{
    const int64_t e = (int64_t)blockIdx.x * MG_OBS_THREADS + threadIdx.x;
    if (e >= N) return;
    const int k = goal_index[e], ax = agent_x[e * astride], ay = agent_y[e * astride];
    int err = 0;
    double v = __longlong_as_double(0x7FF8000000000000LL);
    if (k < 0 || k >= W * H) err = 1;
    else if (ax < 0 || ax >= W || ay < 0 || ay >= H) err = 2;
    else {
        const int p = k % W - ay, q = k / H - ax;           /* goal_position = (k // height, k % width) */
        v = mode == MG_OBS_ANGLE ? table[(p + H - 1) * (2 * W - 1) + (q + W - 1)] : (double)p / (double)q;
    }
    out[e] = v;
    if (error) error[e] = err;
}

/* ------------------------------------------------------------------------------------------------ C ABI */
static inline bool mg_obs_grid_ok(int64_t threads, unsigned *blocks)
{
    const int64_t b = (threads + MG_OBS_THREADS - 1) / MG_OBS_THREADS;
    if (b <= 0 || b >= ((int64_t)1 << 31)) return false;
    *blocks = (unsigned)b;
    return true;
}

extern "C" int mg_obs_onehot(const uint8_t *image, int64_t image_pitch, int n_envs, int n_cells, uint8_t *out,
                             int64_t out_pitch, int32_t *error, void *stream)
{
    if (!image || !out || n_envs <= 0 || n_cells <= 0) return TW_E_ARG;
    const int64_t in_row = (int64_t)n_cells * 3, row = (int64_t)n_cells * MG_OBS_ONEHOT_BITS;
    if (row >= ((int64_t)1 << 31) - 64) return TW_E_ARG;
    if ((image_pitch != 0 && image_pitch < in_row) || (out_pitch != 0 && out_pitch < row)) return TW_E_ARG;
    const int64_t cpr = mg_row_chunks(row, 16);
    unsigned blocks;
    if (!mg_obs_grid_ok(cpr * n_envs, &blocks)) return TW_E_ARG;
    if (error && hipMemsetAsync(error, 0, sizeof(int32_t) * (size_t)n_envs, (hipStream_t)stream) != hipSuccess) return TW_E_HIP;
    hipLaunchKernelGGL(mg_obs_onehot_kernel, dim3(blocks), dim3(MG_OBS_THREADS), 0, (hipStream_t)stream, image,
                       image_pitch ? image_pitch : in_row, n_envs, n_cells, out, out_pitch ? out_pitch : row, error, (int)cpr);
    return tw_launched(__func__);
}

extern "C" int mg_obs_full(const uint8_t *type, const uint8_t *colour, const uint8_t *state, int n_envs, int width,
                           int height, const int32_t *agent_x, const int32_t *agent_y, const int32_t *agent_dir,
                           int agent_stride, uint8_t *out, int64_t out_pitch, int32_t *error, void *stream)
{
    if (!type || !colour || !agent_x || !agent_y || !agent_dir || !out) return TW_E_ARG;
    if (n_envs <= 0 || width <= 0 || height <= 0 || agent_stride <= 0) return TW_E_ARG;
    const int64_t row = (int64_t)width * height * 3;
    if (row >= ((int64_t)1 << 31) - 64) return TW_E_ARG;
    if (out_pitch != 0 && out_pitch < row) return TW_E_ARG;
    const int64_t bpe = (mg_row_chunks(row, 16) + MG_OBS_FULL_CHUNKS - 1) / MG_OBS_FULL_CHUNKS;
    if (bpe * n_envs >= ((int64_t)1 << 31)) return TW_E_ARG;
    hipLaunchKernelGGL(mg_obs_full_kernel, dim3((unsigned)(bpe * n_envs)), dim3(MG_OBS_THREADS), 0, (hipStream_t)stream,
                       type, colour, state, n_envs, width, height, agent_x, agent_y, agent_dir, agent_stride, out,
                       out_pitch ? out_pitch : row, error, (int)bpe);
    return tw_launched(__func__);
}

extern "C" int mg_obs_symbolic(const uint8_t *type, int n_envs, int width, int height, int32_t *out, void *stream)
{
    if (!type || !out || n_envs <= 0 || width <= 0 || height <= 0 || ((uintptr_t)out & 3)) return TW_E_ARG;
    const int64_t total = (int64_t)n_envs * width * height * 3;
    if ((int64_t)width * height * 3 >= ((int64_t)1 << 31) || total >= ((int64_t)1 << 31)) return TW_E_ARG;
    const int64_t chunks = mg_row_chunks(total, 4);
    unsigned blocks;
    if (!mg_obs_grid_ok(chunks, &blocks)) return TW_E_ARG;
    hipLaunchKernelGGL(mg_obs_symbolic_kernel, dim3(blocks), dim3(MG_OBS_THREADS), 0, (hipStream_t)stream, type, width,
                       height, out, total, chunks);
    return tw_launched(__func__);
}

extern "C" int mg_obs_flat(const uint8_t *image, int64_t image_pitch, int n_envs, int n_img, const float *tail, int n_tail,
                           float *out, int64_t out_pitch, void *stream)
{
    if (!image || !out || n_envs <= 0 || n_img <= 0 || n_tail < 0 || (n_tail > 0 && !tail)) return TW_E_ARG;
    if ((uintptr_t)out & 3) return TW_E_ARG;
    const int64_t row = (int64_t)n_img + n_tail;
    if (row >= ((int64_t)1 << 29)) return TW_E_ARG;
    if ((image_pitch != 0 && image_pitch < n_img) || (out_pitch != 0 && out_pitch < row)) return TW_E_ARG;
    const int64_t cpr = mg_row_chunks(row, 4);
    unsigned blocks;
    if (!mg_obs_grid_ok(cpr * n_envs, &blocks)) return TW_E_ARG;
    hipLaunchKernelGGL(mg_obs_flat_kernel, dim3(blocks), dim3(MG_OBS_THREADS), 0, (hipStream_t)stream, image,
                       image_pitch ? image_pitch : (int64_t)n_img, n_envs, n_img, tail, n_tail, out,
                       out_pitch ? out_pitch : row, (int)cpr);
    return tw_launched(__func__);
}

extern "C" int mg_obs_goal_index(const uint8_t *type, int n_envs, int width, int height, int32_t *goal_index, void *stream)
{
    if (!type || !goal_index || n_envs <= 0 || width <= 0 || height <= 0) return TW_E_ARG;
    if ((int64_t)width * height >= ((int64_t)1 << 31) - 64) return TW_E_ARG;
    unsigned blocks;
    if (!mg_obs_grid_ok((int64_t)n_envs * 64, &blocks)) return TW_E_ARG;
    hipLaunchKernelGGL(mg_obs_goal_index_kernel, dim3(blocks), dim3(MG_OBS_THREADS), 0, (hipStream_t)stream, type, n_envs,
                       width * height, goal_index);
    return tw_launched(__func__);
}

extern "C" int mg_obs_angle_table_size(int width, int height)
{
    if (width <= 0 || height <= 0) return TW_E_ARG;
    const int64_t n = ((int64_t)width + height - 1) * (2 * (int64_t)width - 1);
    return n >= ((int64_t)1 << 31) ? TW_E_ARG : (int)n;
}

extern "C" int mg_obs_goal_direction(const int32_t *goal_index, int n_envs, int width, int height, const int32_t *agent_x,
                                     const int32_t *agent_y, int agent_stride, int mode, const double *angle_table,
                                     double *out, int32_t *error, void *stream)
{
    if (!goal_index || !agent_x || !agent_y || !out) return TW_E_ARG;
    if (n_envs <= 0 || width <= 0 || height <= 0 || agent_stride <= 0) return TW_E_ARG;
    if (mode != MG_OBS_SLOPE && mode != MG_OBS_ANGLE) return TW_E_ARG;
    if (mode == MG_OBS_ANGLE && !angle_table) return TW_E_ARG;
    if ((int64_t)width * height >= ((int64_t)1 << 31) || mg_obs_angle_table_size(width, height) < 0) return TW_E_ARG;
    unsigned blocks;
    if (!mg_obs_grid_ok(n_envs, &blocks)) return TW_E_ARG;
    hipLaunchKernelGGL(mg_obs_goal_direction_kernel, dim3(blocks), dim3(MG_OBS_THREADS), 0, (hipStream_t)stream,
                       goal_index, n_envs, width, height, agent_x, agent_y, agent_stride, mode, angle_table, out, error);
    return tw_launched(__func__);
}
